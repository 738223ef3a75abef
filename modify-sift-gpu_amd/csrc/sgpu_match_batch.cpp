// sgpu_match_batch.cpp -- host side of the grouped pair matcher (sgpu_match_batch*,
// sgpu_match_images*), over the shared path of sgpu_pairs.cpp.
#include <cstring>

#include "sgpu_ctx.h"

using namespace sgh;

// The guided form's matrices: host [npairs][9] or null (a missing one: the identity, threshold
// 1e20, SiftMatch.cpp:667-675).
struct BatchGeometry {
    const float* H = nullptr;
    const float* F = nullptr;
    float hdistmax = 0.f, fdistmax = 0.f;
};

// The grouped pair matcher over the sets of src; their s8 / sums forms are the batch's where the
// sets are the last extract's, else derived here in one launch.  One table upload, six launches,
// two device->host copies and two synchronisations, whatever npairs is.
// Guided (geo.H or geo.F set): the work items run k_match_pairs_guided over the sets' device
// locations; the pairs' matrices follow the plan's tables in the same upload.  Nothing else
// changes.
static int match_batch_impl(sgpu_ctx* ctx, const SetSource& src, const int64_t* off, int nsets,
                            const int* set_pairs, int npairs, float distmax, float ratiomax, int mbm,
                            int max_match, int* out_pairs, int64_t cap, int* out_counts,
                            const BatchGeometry& geo = BatchGeometry{}) {
    const bool guided = geo.H || geo.F;
    const int need = SET_DESC | (guided ? SET_LOC : 0);
    hipStream_t st = ctx->stream;
    DeviceSets sets;
    if (src.images) {
        // the last extract's sets come first: its refusals precede the pair list's, and a
        // quantisation it has to make is queued whatever the list holds
        if (const int rc = resolve_sets(ctx, src, 0, need, sets)) return rc;
    } else if (!src.device && npairs > 0) {
        // host input is read whenever there are rows: validated offsets before any size is taken
        // from them
        if (probe_offsets(off, nsets) != sgplan::kPlanOk) return ctx->fail(SGPU_EINVAL, "bad set offsets");
        if (off[nsets] > 0 && !src.desc) return ctx->fail(SGPU_EINVAL, "null descriptors");
        if (off[nsets] > 0 && guided && !src.loc)
            return ctx->fail(SGPU_EINVAL, "guided match needs locations");
    }
    sgplan::Plan& plan = ctx->b_hplan;
    const int prc = sgplan::build_plan(off, nsets, set_pairs, npairs, mbm != 0, max_match, plan);
    ctx->b_planned = prc == sgplan::kPlanOk;
    if (prc == sgplan::kPlanBadArgument)
        return ctx->fail(SGPU_EINVAL, "bad set offsets or pair indices");
    if (prc != sgplan::kPlanOk) return ctx->fail(SGPU_ERANGE, "match batch too large");
    if (npairs == 0) return 0;
    if (!out_counts) return ctx->fail(SGPU_EINVAL, "null out_counts");
    if (cap < 0) cap = 0;
    if (cap > 0 && !out_pairs) return ctx->fail(SGPU_EINVAL, "null out_pairs");
    const int64_t total_rows = off[nsets];
    if (plan.items.empty()) {   // every pair has an empty set
        for (int p = 0; p < npairs; p++) out_counts[p] = 0;
        ctx->timing[T_MATCH] = 0.f;
        return 0;
    }
    // the pair list is checked: a caller's sets, uploaded if they are the host's (there are rows,
    // so the host's pointers have been checked above)
    if (!src.images)
        if (const int rc = resolve_sets(ctx, src, total_rows, need, sets)) return rc;
    if (!sets.u8) return ctx->fail(SGPU_EINVAL, "null descriptors");
    if (guided && !sets.loc) return ctx->fail(SGPU_EINVAL, "guided match needs locations");
    if (const int rc = ensure_dist_table(ctx)) return rc;
    // the tables in one buffer, one upload (guided: then the geometry of every pair)
    const sgplan::TableLayout lay = sgplan::table_layout(plan);
    ctx->b_tables.resize(lay.bytes + (guided ? (size_t)npairs * sizeof(sgk::GuidedParams) : 0));
    unsigned char* tb = ctx->b_tables.data();
    sgplan::pack_tables(plan, tb);
    if (guided) {
        static const float kIdentity[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        auto* g = reinterpret_cast<sgk::GuidedParams*>(tb + lay.bytes);
        for (int p = 0; p < npairs; p++) {
            memcpy(g[p].H, geo.H ? geo.H + 9 * (size_t)p : kIdentity, sizeof(g[p].H));
            memcpy(g[p].F, geo.F ? geo.F + 9 * (size_t)p : kIdentity, sizeof(g[p].F));
            g[p].hdistmax = geo.H ? geo.hdistmax : 1.0e+20f;
            g[p].fdistmax = geo.F ? geo.fdistmax : 1.0e+20f;
        }
    }
    const int64_t out_rows = std::min<int64_t>(cap, plan.out_bound);
    if (const int rc = ensure_pair_buffers(ctx, plan, ctx->b_tables.size(), out_rows, npairs,
                                           sets.s8 && sets.sums ? 0 : total_rows))
        return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->b_plan.p, tb, ctx->b_tables.size(), hipMemcpyHostToDevice, st));
    const unsigned char* dt = ctx->b_plan.as<unsigned char>();
    long long* d_offs = ctx->b_cnt.as<long long>();
    int* d_counts = reinterpret_cast<int*>(d_offs + npairs + 1);
    if (!sets.timing_started) HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    if (const int rc = derive_s8(ctx, sets, total_rows)) return rc;
    MatchPass pass{sets.s8, sets.sums, plan, sgplan::view_tables(lay, dt), distmax, ratiomax,
                   max_match, out_rows, d_counts, d_offs, ctx->b_out.as<int>()};
    if (guided) {
        pass.loc = sets.loc;
        pass.loc_stride = sets.loc_stride;
        pass.d_geom = reinterpret_cast<const sgk::GuidedParams*>(dt + lay.bytes);
    }
    if (const int rc = queue_match_pass(ctx, pass)) return rc;
    HIPCHK(ctx, hipEventRecord(ctx->ev[2], st));
    HIPCHK(ctx, hipMemcpyAsync(out_counts, d_counts, (size_t)npairs * sizeof(int),
                               hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&ctx->timing[T_MATCH], ctx->ev[1], ctx->ev[2]);
    return download_fitting(ctx, out_counts, npairs, ctx->b_out.as<int>(), out_pairs, cap);
}

// the argument checks and sources of the two call families
static int match_sets(sgpu_ctx* ctx, const uint8_t* desc, const float* loc, const int64_t* set_offsets,
                      int nsets, const int* set_pairs, int npairs, float distmax, float ratiomax,
                      int mbm, int max_match, int* out_pairs, int64_t cap, int* out_counts, int flags,
                      const BatchGeometry& geo) {
    if (!ctx) return SGPU_EINVAL;
    if (nsets < 0 || npairs < 0 || !set_offsets) return ctx->fail(SGPU_EINVAL, "bad match batch arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    SetSource src;
    src.device = (flags & SGPU_INPUT_DEVICE) != 0;
    src.desc = desc;
    src.loc = loc;
    return match_batch_impl(ctx, src, set_offsets, nsets, set_pairs, npairs, distmax, ratiomax, mbm,
                            max_match, out_pairs, cap, out_counts, geo);
}
static int match_batch_images(sgpu_ctx* ctx, const int* image_pairs, int npairs, float distmax,
                              float ratiomax, int mbm, int max_match, int* out_pairs, int64_t cap,
                              int* out_counts, const BatchGeometry& geo) {
    if (!ctx) return SGPU_EINVAL;
    if (npairs < 0) return ctx->fail(SGPU_EINVAL, "bad match arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    SetSource src;
    src.images = true;
    return match_batch_impl(ctx, src, ctx->img_off.data(), ctx->batch, image_pairs, npairs, distmax,
                            ratiomax, mbm, max_match, out_pairs, cap, out_counts, geo);
}

extern "C" {

int sgpu_match_batch(sgpu_ctx* ctx, const uint8_t* desc, const int64_t* set_offsets, int nsets,
                     const int* set_pairs, int npairs, float distmax, float ratiomax,
                     int mutual_best_match, int max_match, int* out_pairs, int64_t cap,
                     int* out_counts, int flags) {
    return match_sets(ctx, desc, nullptr, set_offsets, nsets, set_pairs, npairs, distmax, ratiomax,
                      mutual_best_match, max_match, out_pairs, cap, out_counts, flags, BatchGeometry{});
}

int sgpu_match_images(sgpu_ctx* ctx, const int* image_pairs, int npairs, float distmax,
                      float ratiomax, int mutual_best_match, int max_match, int* out_pairs,
                      int64_t cap, int* out_counts) {
    return match_batch_images(ctx, image_pairs, npairs, distmax, ratiomax, mutual_best_match,
                              max_match, out_pairs, cap, out_counts, BatchGeometry{});
}

// the guided forms; without a matrix they are the plain calls
int sgpu_match_batch_guided(sgpu_ctx* ctx, const uint8_t* desc, const float* loc,
                            const int64_t* set_offsets, int nsets, const int* set_pairs,
                            int npairs, const float* H, const float* F, float distmax,
                            float ratiomax, float hdistmax, float fdistmax, int mutual_best_match,
                            int max_match, int* out_pairs, int64_t cap, int* out_counts, int flags) {
    if (!H && !F)
        return sgpu_match_batch(ctx, desc, set_offsets, nsets, set_pairs, npairs, distmax, ratiomax,
                                mutual_best_match, max_match, out_pairs, cap, out_counts, flags);
    return match_sets(ctx, desc, loc, set_offsets, nsets, set_pairs, npairs, distmax, ratiomax,
                      mutual_best_match, max_match, out_pairs, cap, out_counts, flags,
                      BatchGeometry{H, F, hdistmax, fdistmax});
}

int sgpu_match_images_guided(sgpu_ctx* ctx, const int* image_pairs, int npairs, const float* H,
                             const float* F, float distmax, float ratiomax, float hdistmax,
                             float fdistmax, int mutual_best_match, int max_match, int* out_pairs,
                             int64_t cap, int* out_counts) {
    if (!H && !F)
        return sgpu_match_images(ctx, image_pairs, npairs, distmax, ratiomax, mutual_best_match,
                                 max_match, out_pairs, cap, out_counts);
    return match_batch_images(ctx, image_pairs, npairs, distmax, ratiomax, mutual_best_match,
                              max_match, out_pairs, cap, out_counts,
                              BatchGeometry{H, F, hdistmax, fdistmax});
}

}  // extern "C"
