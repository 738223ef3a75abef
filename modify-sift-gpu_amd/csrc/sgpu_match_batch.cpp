// sgpu_match_batch.cpp -- host side of the grouped pair matcher (sgpu_match_batch*,
// sgpu_match_images*) and of the geometry estimator over its matches (sgpu_estimate_*).
#include <cstring>

#include "sgpu_ctx.h"

using namespace sgh;

extern "C" {

// The grouped pair matcher over device-resident sets: u8 = the sets' descriptors, s8 / sums =
// their matcher forms when the caller has them (sgpu_match_images), else derived here in one
// launch.  One table upload, six launches, two device->host copies and two
// synchronisations, whatever npairs is.
// Guided (geo.H or geo.F set): the work items run k_match_pairs_guided over the device locations
// geo.loc; the pairs' matrices (a missing one: the identity, threshold 1e20, SiftMatch.cpp:
// 667-675) follow the plan's tables in the same upload.  Nothing else changes.
struct BatchGeometry {
    const float* loc = nullptr;   // device: x, y of row r at loc[r * stride]
    int stride = 2;
    const float* H = nullptr;     // host [npairs][9] or null
    const float* F = nullptr;
    float hdistmax = 0.f, fdistmax = 0.f;
};
static int match_batch_impl(sgpu_ctx* ctx, const uint8_t* u8, const uint8_t* s8, const int* sums,
                            const int64_t* off, int nsets, const int* set_pairs, int npairs,
                            float distmax, float ratiomax, int mbm, int max_match, int* out_pairs,
                            int64_t cap, int* out_counts, bool timing_started = false,
                            const BatchGeometry& geo = BatchGeometry{}) {
    const bool guided = geo.H || geo.F;
    hipStream_t st = ctx->stream;
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
    if (!u8) return ctx->fail(SGPU_EINVAL, "null descriptors");
    if (guided && !geo.loc) return ctx->fail(SGPU_EINVAL, "guided match needs locations");
    if (const int rc = ensure_dist_table(ctx)) return rc;
    // the tables in one buffer, one upload: [items][sides][finish panels][pairs]
    // (guided: [geometry of every pair])
    const size_t b_items = plan.items.size() * sizeof(sgplan::Item);
    const size_t b_sides = plan.sides.size() * sizeof(sgplan::Side);
    const size_t b_fp = plan.fpanels.size() * sizeof(sgplan::FinishPanel);
    const size_t b_pairs = plan.pairs.size() * sizeof(sgplan::PairRec);
    const size_t b_geom = guided ? (size_t)npairs * sizeof(sgk::GuidedParams) : 0;
    ctx->b_tables.resize(b_items + b_sides + b_fp + b_pairs + b_geom);
    unsigned char* tb = ctx->b_tables.data();
    memcpy(tb, plan.items.data(), b_items);
    memcpy(tb + b_items, plan.sides.data(), b_sides);
    memcpy(tb + b_items + b_sides, plan.fpanels.data(), b_fp);
    memcpy(tb + b_items + b_sides + b_fp, plan.pairs.data(), b_pairs);
    if (guided) {
        static const float kIdentity[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        auto* g = reinterpret_cast<sgk::GuidedParams*>(tb + b_items + b_sides + b_fp + b_pairs);
        for (int p = 0; p < npairs; p++) {
            memcpy(g[p].H, geo.H ? geo.H + 9 * (size_t)p : kIdentity, sizeof(g[p].H));
            memcpy(g[p].F, geo.F ? geo.F + 9 * (size_t)p : kIdentity, sizeof(g[p].F));
            g[p].hdistmax = geo.H ? geo.hdistmax : 1.0e+20f;
            g[p].fdistmax = geo.F ? geo.fdistmax : 1.0e+20f;
        }
    }
    const int64_t out_rows = std::min<int64_t>(cap, plan.out_bound);
    ALLOCCHK(ctx, ctx->b_plan.ensure(ctx->b_tables.size()));
    ALLOCCHK(ctx, ctx->b_part.ensure((size_t)plan.part_total * sizeof(sgk::Top2)));
    ALLOCCHK(ctx, ctx->b_dec.ensure((size_t)plan.dec_total * sizeof(int)));
    // [offsets npairs + 1 (64-bit)][counts npairs]
    ALLOCCHK(ctx, ctx->b_cnt.ensure((size_t)(npairs + 1) * sizeof(long long) + (size_t)npairs * sizeof(int)));
    ALLOCCHK(ctx, ctx->b_out.ensure((size_t)std::max<int64_t>(out_rows, 1) * 2 * sizeof(int)));
    if (!s8 || !sums) {
        ALLOCCHK(ctx, ctx->b_s8.ensure((size_t)total_rows * 128));
        ALLOCCHK(ctx, ctx->b_sums.ensure((size_t)total_rows * sizeof(int)));
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->b_plan.p, tb, ctx->b_tables.size(), hipMemcpyHostToDevice, st));
    const unsigned char* dt = ctx->b_plan.as<unsigned char>();
    const auto* d_items = reinterpret_cast<const sgplan::Item*>(dt);
    const auto* d_sides = reinterpret_cast<const sgplan::Side*>(dt + b_items);
    const auto* d_fp = reinterpret_cast<const sgplan::FinishPanel*>(dt + b_items + b_sides);
    const auto* d_pairs = reinterpret_cast<const sgplan::PairRec*>(dt + b_items + b_sides + b_fp);
    const auto* d_geom =
        reinterpret_cast<const sgk::GuidedParams*>(dt + b_items + b_sides + b_fp + b_pairs);
    long long* d_offs = ctx->b_cnt.as<long long>();
    int* d_counts = reinterpret_cast<int*>(d_offs + npairs + 1);
    if (!timing_started) HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    if (!s8 || !sums) {
        sgk::PrepSet prep{u8, (int)total_rows, ctx->b_s8.as<uint8_t>()};
        prep.sums = ctx->b_sums.as<int>();
        HIPCHK(ctx, sgk::launch_prep_set(prep, st));
        s8 = ctx->b_s8.as<uint8_t>();
        sums = ctx->b_sums.as<int>();
    }
    if (guided)
        HIPCHK(ctx, sgk::launch_match_pairs_guided(s8, d_items, (int)plan.items.size(),
                                                   ctx->b_part.as<sgk::Top2>(), geo.loc, geo.stride,
                                                   d_geom, st));
    else
        HIPCHK(ctx, sgk::launch_match_pairs(s8, d_items, (int)plan.items.size(),
                                            ctx->b_part.as<sgk::Top2>(), st));
    HIPCHK(ctx, sgk::launch_match_pairs_finish(ctx->b_part.as<sgk::Top2>(), d_sides, d_fp,
                                               (int)plan.fpanels.size(), sums,
                                               ctx->m_dist.as<float>(), distmax, ratiomax,
                                               ctx->b_dec.as<int>(), st));
    HIPCHK(ctx, sgk::launch_match_pairs_compact(ctx->b_dec.as<int>(), d_pairs, npairs, max_match,
                                                out_rows, d_counts, d_offs, ctx->b_out.as<int>(), st));
    HIPCHK(ctx, hipEventRecord(ctx->ev[2], st));
    HIPCHK(ctx, hipMemcpyAsync(out_counts, d_counts, (size_t)npairs * sizeof(int),
                               hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&ctx->timing[T_MATCH], ctx->ev[1], ctx->ev[2]);
    // the pairs that fit form a prefix (the offsets only grow): copy their matches
    int64_t total = 0, fit = 0;
    bool fits = true;
    for (int p = 0; p < npairs; p++) {
        total += out_counts[p];
        fits = fits && total <= cap;
        if (fits) fit = total;
    }
    if (fit > 0) {
        HIPCHK(ctx, hipMemcpyAsync(out_pairs, ctx->b_out.p, (size_t)fit * 2 * sizeof(int),
                                   hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
    }
    if (total > cap) return ctx->fail(SGPU_ERANGE, "matches exceed cap (counts are complete)");
    if (total > INT_MAX) return ctx->fail(SGPU_ERANGE, "match total exceeds the return type");
    return (int)total;
}

int sgpu_match_batch(sgpu_ctx* ctx, const uint8_t* desc, const int64_t* set_offsets, int nsets,
                     const int* set_pairs, int npairs, float distmax, float ratiomax,
                     int mutual_best_match, int max_match, int* out_pairs, int64_t cap,
                     int* out_counts, int flags) {
    if (!ctx) return SGPU_EINVAL;
    if (nsets < 0 || npairs < 0 || !set_offsets) return ctx->fail(SGPU_EINVAL, "bad match batch arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint8_t* u8 = desc;
    if (!(flags & SGPU_INPUT_DEVICE) && npairs > 0) {
        // validated offsets before any size is taken from them
        sgplan::Plan probe;
        if (sgplan::build_plan(set_offsets, nsets, nullptr, 0, false, 0, probe) != sgplan::kPlanOk)
            return ctx->fail(SGPU_EINVAL, "bad set offsets");
        const int64_t total_rows = set_offsets[nsets];
        if (total_rows > 0) {
            if (!desc) return ctx->fail(SGPU_EINVAL, "null descriptors");
            ALLOCCHK(ctx, ctx->b_desc.ensure((size_t)total_rows * 128));
            HIPCHK(ctx, hipMemcpyAsync(ctx->b_desc.p, desc, (size_t)total_rows * 128,
                                       hipMemcpyHostToDevice, ctx->stream));
            u8 = ctx->b_desc.as<uint8_t>();
        }
    }
    return match_batch_impl(ctx, u8, nullptr, nullptr, set_offsets, nsets, set_pairs, npairs, distmax,
                            ratiomax, mutual_best_match, max_match, out_pairs, cap, out_counts);
}

int sgpu_match_images(sgpu_ctx* ctx, const int* image_pairs, int npairs, float distmax,
                      float ratiomax, int mutual_best_match, int max_match, int* out_pairs,
                      int64_t cap, int* out_counts) {
    if (!ctx) return SGPU_EINVAL;
    if (npairs < 0) return ctx->fail(SGPU_EINVAL, "bad match arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // a quantisation this call has to make counts into its device time (times[8]); it is queued
    // on the matcher's stream, with no wait in between
    const bool quantises = !ctx->f_ready;
    if (quantises) HIPCHK(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    const int rc = feature_u8(ctx);
    if (rc != SGPU_OK) return rc;
    return match_batch_impl(ctx, ctx->f_u8.as<uint8_t>(), ctx->f_s8.as<uint8_t>(),
                            ctx->f_sums.as<int>(), ctx->img_off.data(), ctx->batch, image_pairs,
                            npairs, distmax, ratiomax, mutual_best_match, max_match, out_pairs, cap,
                            out_counts, quantises);
}

int sgpu_match_batch_guided(sgpu_ctx* ctx, const uint8_t* desc, const float* loc,
                            const int64_t* set_offsets, int nsets, const int* set_pairs,
                            int npairs, const float* H, const float* F, float distmax,
                            float ratiomax, float hdistmax, float fdistmax, int mutual_best_match,
                            int max_match, int* out_pairs, int64_t cap, int* out_counts, int flags) {
    if (!H && !F)
        return sgpu_match_batch(ctx, desc, set_offsets, nsets, set_pairs, npairs, distmax, ratiomax,
                                mutual_best_match, max_match, out_pairs, cap, out_counts, flags);
    if (!ctx) return SGPU_EINVAL;
    if (nsets < 0 || npairs < 0 || !set_offsets) return ctx->fail(SGPU_EINVAL, "bad match batch arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint8_t* u8 = desc;
    BatchGeometry geo;
    geo.loc = loc;
    geo.H = H;
    geo.F = F;
    geo.hdistmax = hdistmax;
    geo.fdistmax = fdistmax;
    if (!(flags & SGPU_INPUT_DEVICE) && npairs > 0) {
        // validated offsets before any size is taken from them
        sgplan::Plan probe;
        if (sgplan::build_plan(set_offsets, nsets, nullptr, 0, false, 0, probe) != sgplan::kPlanOk)
            return ctx->fail(SGPU_EINVAL, "bad set offsets");
        const int64_t total_rows = set_offsets[nsets];
        if (total_rows > 0) {
            if (!desc) return ctx->fail(SGPU_EINVAL, "null descriptors");
            if (!loc) return ctx->fail(SGPU_EINVAL, "guided match needs locations");
            ALLOCCHK(ctx, ctx->b_desc.ensure((size_t)total_rows * 128));
            ALLOCCHK(ctx, ctx->b_loc.ensure((size_t)total_rows * 2 * sizeof(float)));
            HIPCHK(ctx, hipMemcpyAsync(ctx->b_desc.p, desc, (size_t)total_rows * 128,
                                       hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipMemcpyAsync(ctx->b_loc.p, loc, (size_t)total_rows * 2 * sizeof(float),
                                       hipMemcpyHostToDevice, ctx->stream));
            u8 = ctx->b_desc.as<uint8_t>();
            geo.loc = ctx->b_loc.as<float>();
        }
    }
    return match_batch_impl(ctx, u8, nullptr, nullptr, set_offsets, nsets, set_pairs, npairs, distmax,
                            ratiomax, mutual_best_match, max_match, out_pairs, cap, out_counts, false,
                            geo);
}

int sgpu_match_images_guided(sgpu_ctx* ctx, const int* image_pairs, int npairs, const float* H,
                             const float* F, float distmax, float ratiomax, float hdistmax,
                             float fdistmax, int mutual_best_match, int max_match, int* out_pairs,
                             int64_t cap, int* out_counts) {
    if (!H && !F)
        return sgpu_match_images(ctx, image_pairs, npairs, distmax, ratiomax, mutual_best_match,
                                 max_match, out_pairs, cap, out_counts);
    if (!ctx) return SGPU_EINVAL;
    if (npairs < 0) return ctx->fail(SGPU_EINVAL, "bad match arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool quantises = !ctx->f_ready;
    if (quantises) HIPCHK(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    int rc = feature_u8(ctx);
    if (rc != SGPU_OK) return rc;
    // the batch's device keys [x, y, scale, orientation]: the locations are their first two floats
    BatchGeometry geo;
    rc = sgpu_device_features(ctx, &geo.loc, nullptr, nullptr);
    if (rc != SGPU_OK) return rc;
    geo.stride = 4;
    geo.H = H;
    geo.F = F;
    geo.hdistmax = hdistmax;
    geo.fdistmax = fdistmax;
    return match_batch_impl(ctx, ctx->f_u8.as<uint8_t>(), ctx->f_s8.as<uint8_t>(),
                            ctx->f_sums.as<int>(), ctx->img_off.data(), ctx->batch, image_pairs,
                            npairs, distmax, ratiomax, mutual_best_match, max_match, out_pairs, cap,
                            out_counts, quantises, geo);
}

// H / F of every pair of a pair list (sift_geom.h is the contract, sift_geom.hip the kernels).
// loc: device locations (x, y of buffer row r at loc[r * stride]), or host_loc: packed host
// locations uploaded here, after every argument has been checked.  One table upload
// ([pairs][items][matches]), one memset, three launches, two device->host copies and one
// synchronisation, whatever npairs is.  rounds > 0 (the _refined calls): one more launch, the
// local refinement of every pair's winner, and its accepted rounds in the same result copy.
static int estimate_impl(sgpu_ctx* ctx, const float* loc, int stride, const float* host_loc,
                         const int64_t* off, int nsets, const int* set_pairs, int npairs,
                         const int* matches, const int* counts, int model, float threshold,
                         int iterations, uint32_t seed, float* out_models, int* out_inliers,
                         uint8_t* out_mask, int rounds, int* out_rounds) {
    hipStream_t st = ctx->stream;
    sgeo::Plan& plan = ctx->e_hplan;
    const int prc = sgeo::build_plan(off, nsets, set_pairs, npairs, counts, model, iterations, plan);
    if (prc == sgeo::kPlanBadArgument)
        return ctx->fail(SGPU_EINVAL, "bad offsets, pair indices, counts, model or iterations");
    if (prc != sgeo::kPlanOk) return ctx->fail(SGPU_ERANGE, "estimate batch too large");
    ctx->timing[T_ESTIMATE] = 0.f;
    if (npairs == 0) return SGPU_OK;
    if (!out_models || !out_inliers) return ctx->fail(SGPU_EINVAL, "null outputs");
    const long long total = plan.total;
    if (total > 0 && !matches) return ctx->fail(SGPU_EINVAL, "null matches");
    if (!sgeo::check_matches(off, set_pairs, npairs, matches, counts))
        return ctx->fail(SGPU_EINVAL, "a match index lies outside its set");
    if (total > 0 && !loc && !host_loc) return ctx->fail(SGPU_EINVAL, "null locations");
    if (host_loc && total > 0) {
        const size_t bytes = (size_t)off[nsets] * 2 * sizeof(float);
        ALLOCCHK(ctx, ctx->e_loc.ensure(bytes));
        HIPCHK(ctx, hipMemcpyAsync(ctx->e_loc.p, host_loc, bytes, hipMemcpyHostToDevice, st));
        loc = ctx->e_loc.as<float>();
        stride = 2;
    }
    const size_t b_pairs = plan.pairs.size() * sizeof(sgeo::PairRec);
    const size_t b_items = plan.items.size() * sizeof(sgeo::Item);
    const size_t b_matches = (size_t)total * 2 * sizeof(int);
    static_assert(sizeof(sgeo::PairRec) % 8 == 0 && sizeof(sgeo::Item) == 8, "the matches stay 8-byte aligned");
    ctx->e_tables.resize(b_pairs + b_items + b_matches);
    unsigned char* tb = ctx->e_tables.data();
    memcpy(tb, plan.pairs.data(), b_pairs);
    if (b_items) memcpy(tb + b_pairs, plan.items.data(), b_items);
    if (b_matches) memcpy(tb + b_pairs + b_items, matches, b_matches);
    // [models npairs x 9 floats][inliers npairs][error flag][accepted rounds npairs, if refined]
    const size_t b_models = (size_t)npairs * 9 * sizeof(float);
    const size_t b_plain = b_models + (size_t)(npairs + 1) * sizeof(int);
    const size_t b_result = b_plain + (rounds > 0 ? (size_t)npairs * sizeof(int) : 0);
    const size_t b_slots = (size_t)npairs * sizeof(unsigned long long);
    ALLOCCHK(ctx, ctx->e_plan.ensure(ctx->e_tables.size()));
    ALLOCCHK(ctx, ctx->e_pts.ensure((size_t)std::max<long long>(total, 1) * sizeof(float4)));
    ALLOCCHK(ctx, ctx->e_slots.ensure(b_slots));
    ALLOCCHK(ctx, ctx->e_out.ensure(b_result));
    if (out_mask) ALLOCCHK(ctx, ctx->e_mask.ensure((size_t)std::max<long long>(total, 1)));
    ctx->e_result.resize(b_result);
    HIPCHK(ctx, hipMemcpyAsync(ctx->e_plan.p, tb, ctx->e_tables.size(), hipMemcpyHostToDevice, st));
    const unsigned char* dt = ctx->e_plan.as<unsigned char>();
    const auto* d_pairs = reinterpret_cast<const sgeo::PairRec*>(dt);
    const auto* d_items = reinterpret_cast<const sgeo::Item*>(dt + b_pairs);
    const auto* d_matches = reinterpret_cast<const int*>(dt + b_pairs + b_items);
    auto* d_slots = ctx->e_slots.as<unsigned long long>();
    float* d_models = ctx->e_out.as<float>();
    int* d_inliers = reinterpret_cast<int*>(ctx->e_out.as<unsigned char>() + b_models);
    int* d_err = d_inliers + npairs;
    int* d_rounds = d_err + 1;
    float4* d_pts = ctx->e_pts.as<float4>();
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipMemsetAsync(d_slots, 0, b_slots, st));
    HIPCHK(ctx, hipMemsetAsync(d_err, 0, sizeof(int), st));
    HIPCHK(ctx, sgk::launch_estimate_gather(loc, stride, d_pairs, npairs, d_matches, total, d_pts, st));
    HIPCHK(ctx, sgk::launch_estimate_pairs(d_pts, d_pairs, d_items, (int)plan.items.size(), model,
                                           threshold, iterations, seed, d_slots, st));
    HIPCHK(ctx, sgk::launch_estimate_finish(d_pts, d_pairs, npairs, model, threshold, seed, d_slots,
                                            d_models, d_inliers,
                                            out_mask ? ctx->e_mask.as<uint8_t>() : nullptr, d_err, st));
    HIPCHK(ctx, sgk::launch_estimate_refine(d_pts, d_pairs, npairs, model, threshold, rounds, d_models,
                                            d_inliers, out_mask ? ctx->e_mask.as<uint8_t>() : nullptr,
                                            d_rounds, st));
    HIPCHK(ctx, hipEventRecord(ctx->ev[2], st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->e_result.data(), ctx->e_out.p, b_result, hipMemcpyDeviceToHost, st));
    if (out_mask && total > 0)
        HIPCHK(ctx, hipMemcpyAsync(out_mask, ctx->e_mask.p, (size_t)total, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&ctx->timing[T_ESTIMATE], ctx->ev[1], ctx->ev[2]);
    memcpy(out_models, ctx->e_result.data(), b_models);
    memcpy(out_inliers, ctx->e_result.data() + b_models, (size_t)npairs * sizeof(int));
    if (out_rounds) {
        if (rounds > 0) memcpy(out_rounds, ctx->e_result.data() + b_plain, (size_t)npairs * sizeof(int));
        else memset(out_rounds, 0, (size_t)npairs * sizeof(int));
    }
    int err = 0;
    memcpy(&err, ctx->e_result.data() + b_models + (size_t)npairs * sizeof(int), sizeof(int));
    if (err) return ctx->fail(SGPU_ENODEV, "estimate: a regenerated winner's inlier count differs from its score");
    return SGPU_OK;
}

int sgpu_estimate_batch_refined(sgpu_ctx* ctx, const float* loc, const int64_t* set_offsets,
                                int nsets, const int* set_pairs, int npairs, const int* matches,
                                const int* match_counts, int model, float threshold,
                                int iterations, uint32_t seed, int refine_rounds, float* out_models,
                                int* out_inliers, uint8_t* out_mask, int* out_rounds, int flags) {
    if (!ctx) return SGPU_EINVAL;
    if (nsets < 0 || npairs < 0 || !set_offsets) return ctx->fail(SGPU_EINVAL, "bad estimate batch arguments");
    if (refine_rounds < 0 || refine_rounds > sgeo::kMaxRefineRounds)
        return ctx->fail(SGPU_EINVAL, "refine_rounds outside [0, 16]");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool dev = (flags & SGPU_INPUT_DEVICE) != 0;
    return estimate_impl(ctx, dev ? loc : nullptr, 2, dev ? nullptr : loc, set_offsets, nsets,
                         set_pairs, npairs, matches, match_counts, model, threshold, iterations, seed,
                         out_models, out_inliers, out_mask, refine_rounds, out_rounds);
}

int sgpu_estimate_images_refined(sgpu_ctx* ctx, const int* image_pairs, int npairs,
                                 const int* matches, const int* match_counts, int model,
                                 float threshold, int iterations, uint32_t seed, int refine_rounds,
                                 float* out_models, int* out_inliers, uint8_t* out_mask,
                                 int* out_rounds) {
    if (!ctx) return SGPU_EINVAL;
    if (npairs < 0) return ctx->fail(SGPU_EINVAL, "bad estimate arguments");
    if (refine_rounds < 0 || refine_rounds > sgeo::kMaxRefineRounds)
        return ctx->fail(SGPU_EINVAL, "refine_rounds outside [0, 16]");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the states sgpu_match_images_guided refuses (feature_u8), without its quantisation
    if (ctx->batch <= 0 || ctx->img_off.empty())
        return ctx->fail(SGPU_EINVAL, "no extracted batch to estimate on");
    if (!ctx->opt.descriptors) return ctx->fail(SGPU_EINVAL, "descriptors disabled (-sd)");
    const float* keys = nullptr;
    const int rc = sgpu_device_features(ctx, &keys, nullptr, nullptr);   // (gathers a multi-part batch)
    if (rc != SGPU_OK) return rc;
    return estimate_impl(ctx, keys, 4, nullptr, ctx->img_off.data(), ctx->batch, image_pairs, npairs,
                         matches, match_counts, model, threshold, iterations, seed, out_models,
                         out_inliers, out_mask, refine_rounds, out_rounds);
}

// the unrefined forms: no round, no launch added
int sgpu_estimate_batch(sgpu_ctx* ctx, const float* loc, const int64_t* set_offsets, int nsets,
                        const int* set_pairs, int npairs, const int* matches,
                        const int* match_counts, int model, float threshold, int iterations,
                        uint32_t seed, float* out_models, int* out_inliers, uint8_t* out_mask,
                        int flags) {
    return sgpu_estimate_batch_refined(ctx, loc, set_offsets, nsets, set_pairs, npairs, matches,
                                       match_counts, model, threshold, iterations, seed, 0, out_models,
                                       out_inliers, out_mask, nullptr, flags);
}

int sgpu_estimate_images(sgpu_ctx* ctx, const int* image_pairs, int npairs, const int* matches,
                         const int* match_counts, int model, float threshold, int iterations,
                         uint32_t seed, float* out_models, int* out_inliers, uint8_t* out_mask) {
    return sgpu_estimate_images_refined(ctx, image_pairs, npairs, matches, match_counts, model,
                                        threshold, iterations, seed, 0, out_models, out_inliers,
                                        out_mask, nullptr);
}

}  // extern "C"
