// sgpu_prematch.cpp -- host side of preemptive matching (sgpu_select_top_scale_*, sgpu_prematch_*;
// DESIGN.md 4.18): every set's top rows by scale are selected and gathered on the device
// (sift_select.hip) and the grouped pair matcher of sgpu_match_batch.cpp runs over the gathered
// subsets.  The host knows the subsets' offsets from the set offsets and `top` alone, so it plans
// without a device round trip; one table block goes up, the counts (and the matches) come down.
#include <cstring>

#include "sgpu_ctx.h"

using namespace sgh;

namespace {

// offsets that sgpu_match_batch would accept, before any size is taken from them
int check_offsets(sgpu_ctx* ctx, const int64_t* off, int nsets) {
    const int prc = probe_offsets(off, nsets);
    if (prc == sgplan::kPlanBadArgument) return ctx->fail(SGPU_EINVAL, "bad set offsets");
    if (prc != sgplan::kPlanOk) return ctx->fail(SGPU_ERANGE, "too many rows");
    return SGPU_OK;
}

// [set offsets nsets + 1 (64-bit)][subset offsets nsets + 1 (int), padded to 8 bytes] at tb
size_t offset_tables(unsigned char* tb, const int64_t* off, const std::vector<int64_t>& sub, int nsets) {
    auto* so = reinterpret_cast<long long*>(tb);
    auto* su = reinterpret_cast<int*>(tb + ((size_t)nsets + 1) * sizeof(long long));
    for (int s = 0; s <= nsets; s++) {
        so[s] = off[s];
        su[s] = (int)sub[s];
    }
    return ((size_t)nsets + 1) * sizeof(long long) + round8(((size_t)nsets + 1) * sizeof(int));
}

// The selection alone.  One table upload, one launch, one download, one synchronisation.
int select_impl(sgpu_ctx* ctx, const SetSource& in, const int64_t* off, int nsets, int top,
                int* out_index, int64_t* out_offsets) {
    if (top < 1) return ctx->fail(SGPU_EINVAL, "top < 1");
    if (in.scale_stride < 1) return ctx->fail(SGPU_EINVAL, "scale_stride < 1");
    if (!out_index || !out_offsets) return ctx->fail(SGPU_EINVAL, "null outputs");
    if (const int rc = check_offsets(ctx, off, nsets)) return rc;
    const int64_t total_rows = nsets > 0 ? off[nsets] : 0;
    if (!in.images && total_rows > 0 && !in.scale) return ctx->fail(SGPU_EINVAL, "null scales");
    std::vector<int64_t>& sub = ctx->p_sub;
    sgsel::subset_offsets(off, nsets, top, sub);
    const int64_t total_sub = sub[nsets];
    if (total_sub > 0) {
        hipStream_t st = ctx->stream;
        DeviceSets sets;
        if (const int rc = resolve_sets(ctx, in, total_rows, SET_SCALE, sets)) return rc;
        ctx->b_tables.resize(((size_t)nsets + 1) * 16);
        const size_t b_tab = offset_tables(ctx->b_tables.data(), off, sub, nsets);
        ALLOCCHK(ctx, ctx->b_plan.ensure(b_tab));
        ALLOCCHK(ctx, ctx->p_index.ensure((size_t)total_sub * sizeof(int)));
        HIPCHK(ctx, hipMemcpyAsync(ctx->b_plan.p, ctx->b_tables.data(), b_tab, hipMemcpyHostToDevice, st));
        const auto* d_setoff = ctx->b_plan.as<long long>();
        const auto* d_suboff = reinterpret_cast<const int*>(d_setoff + nsets + 1);
        HIPCHK(ctx, sgk::launch_select_top_scale(sets.scale, sets.scale_stride, d_setoff, d_suboff,
                                                 nsets, top, ctx->p_index.as<int>(), st));
        HIPCHK(ctx, hipMemcpyAsync(out_index, ctx->p_index.p, (size_t)total_sub * sizeof(int),
                                   hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
    }
    memcpy(out_offsets, sub.data(), ((size_t)nsets + 1) * sizeof(int64_t));
    return SGPU_OK;
}

// The whole pre-pass.  Queue order on ctx->stream: k_select_top_scale -> k_gather_rows -> [prep of
// the gathered u8 rows, a caller's descriptors only] -> k_match_pairs, finish, count / scan / write
// over the subsets -> [k_remap_matches, only when matches are wanted].  One table upload, the
// counts' download and at most one of matches, two synchronisations, whatever nsets and npairs are.
int prematch_impl(sgpu_ctx* ctx, const SetSource& in, const int64_t* off, int nsets, const int* set_pairs,
                  int npairs, int top, float distmax, float ratiomax, int mbm, int* out_counts,
                  int* out_pairs, int64_t cap) {
    if (top < 1) return ctx->fail(SGPU_EINVAL, "top < 1");
    if (in.scale_stride < 1) return ctx->fail(SGPU_EINVAL, "scale_stride < 1");
    if (!out_counts) return ctx->fail(SGPU_EINVAL, "null out_counts");
    if (const int rc = check_offsets(ctx, off, nsets)) return rc;
    const int64_t total_rows = off[nsets];
    if (!in.images && total_rows > 0 && (!in.desc || !in.scale))
        return ctx->fail(SGPU_EINVAL, "null descriptors or scales");
    if (!set_pairs) {   // all pairs a < b, in lexicographic order
        if ((int64_t)npairs != (int64_t)nsets * (nsets - 1) / 2)
            return ctx->fail(SGPU_EINVAL, "npairs is not nsets (nsets - 1) / 2 for the all-pairs list");
        ctx->p_pairs.clear();
        ctx->p_pairs.reserve((size_t)npairs * 2);
        for (int a = 0; a < nsets; a++)
            for (int b = a + 1; b < nsets; b++) {
                ctx->p_pairs.push_back(a);
                ctx->p_pairs.push_back(b);
            }
        set_pairs = ctx->p_pairs.data();
    }
    hipStream_t st = ctx->stream;
    std::vector<int64_t>& sub = ctx->p_sub;
    sgsel::subset_offsets(off, nsets, top, sub);
    // the matcher's plan over the subsets, with max_match = top
    sgplan::Plan& plan = ctx->p_hplan;
    const int prc = sgplan::build_plan(sub.data(), nsets, set_pairs, npairs, mbm != 0, top, plan);
    if (prc == sgplan::kPlanBadArgument) return ctx->fail(SGPU_EINVAL, "bad pair indices");
    if (prc != sgplan::kPlanOk) return ctx->fail(SGPU_ERANGE, "match batch too large");
    ctx->timing[T_PREMATCH] = 0.f;
    if (npairs == 0) return 0;
    const bool want_matches = out_pairs != nullptr;
    cap = want_matches ? std::max<int64_t>(cap, 0) : 0;
    const int64_t total_sub = sub[nsets];
    if (plan.items.empty()) {   // every pair has an empty set
        memset(out_counts, 0, (size_t)npairs * sizeof(int));
        return 0;
    }

    // ---- everything is checked: the inputs.  The gather reads the batch's s8 form and sums, or a
    // caller's u8 rows
    DeviceSets sets;
    if (const int rc = resolve_sets(ctx, in, total_rows, SET_DESC | SET_SCALE, sets)) return rc;
    if (const int rc = ensure_dist_table(ctx)) return rc;

    // ---- the tables in one buffer, one upload: the matcher's [items][sides][finish panels][pairs],
    // then [set offsets][subset offsets][the two subsets' offsets of every pair]
    const sgplan::TableLayout lay = sgplan::table_layout(plan);
    const size_t o_off = lay.bytes;
    const size_t b_off = ((size_t)nsets + 1) * sizeof(long long) + round8(((size_t)nsets + 1) * sizeof(int));
    const size_t o_psub = o_off + b_off;
    ctx->b_tables.resize(o_psub + (size_t)npairs * 2 * sizeof(int));
    unsigned char* tb = ctx->b_tables.data();
    sgplan::pack_tables(plan, tb);
    offset_tables(tb + o_off, off, sub, nsets);
    auto* h_psub = reinterpret_cast<int*>(tb + o_psub);
    for (int p = 0; p < npairs; p++) {
        h_psub[2 * p] = (int)sub[set_pairs[2 * p]];
        h_psub[2 * p + 1] = (int)sub[set_pairs[2 * p + 1]];
    }
    const int64_t out_rows = std::min<int64_t>(cap, plan.out_bound);
    // b_s8 / b_sums hold the gathered subsets' forms
    if (const int rc = ensure_pair_buffers(ctx, plan, ctx->b_tables.size(), out_rows, npairs, total_sub))
        return rc;
    ALLOCCHK(ctx, ctx->p_index.ensure((size_t)total_sub * sizeof(int)));
    if (!in.images) ALLOCCHK(ctx, ctx->p_u8.ensure((size_t)total_sub * 128));
    HIPCHK(ctx, hipMemcpyAsync(ctx->b_plan.p, tb, ctx->b_tables.size(), hipMemcpyHostToDevice, st));
    const unsigned char* dt = ctx->b_plan.as<unsigned char>();
    const auto* d_setoff = reinterpret_cast<const long long*>(dt + o_off);
    const auto* d_suboff = reinterpret_cast<const int*>(d_setoff + nsets + 1);
    const auto* d_psub = reinterpret_cast<const int*>(dt + o_psub);
    long long* d_offs = ctx->b_cnt.as<long long>();
    int* d_counts = reinterpret_cast<int*>(d_offs + npairs + 1);
    int* d_index = ctx->p_index.as<int>();

    // ---- the queue
    if (!sets.timing_started) HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, sgk::launch_select_top_scale(sets.scale, sets.scale_stride, d_setoff, d_suboff, nsets,
                                             top, d_index, st));
    DeviceSets subs;   // the gathered subsets
    if (in.images) {
        // the matcher's forms exist: gather them, no prep
        HIPCHK(ctx, sgk::launch_gather_rows(sets.s8, sets.sums, d_setoff, d_suboff, d_index, nsets,
                                            ctx->b_s8.as<uint8_t>(), ctx->b_sums.as<int>(), st));
        subs.s8 = ctx->b_s8.as<uint8_t>();
        subs.sums = ctx->b_sums.as<int>();
    } else {
        HIPCHK(ctx, sgk::launch_gather_rows(sets.u8, nullptr, d_setoff, d_suboff, d_index, nsets,
                                            ctx->p_u8.as<uint8_t>(), nullptr, st));
        subs.u8 = ctx->p_u8.as<uint8_t>();
        if (const int rc = derive_s8(ctx, subs, total_sub)) return rc;
    }
    const MatchPass pass{subs.s8, subs.sums, plan, sgplan::view_tables(lay, dt), distmax, ratiomax,
                         top, out_rows, d_counts, d_offs, ctx->b_out.as<int>()};
    if (const int rc = queue_match_pass(ctx, pass)) return rc;
    if (want_matches && out_rows > 0)
        HIPCHK(ctx, sgk::launch_remap_matches(d_counts, d_offs, d_psub, d_index, npairs, out_rows,
                                              ctx->b_out.as<int>(), st));
    HIPCHK(ctx, hipEventRecord(ctx->ev[2], st));
    HIPCHK(ctx, hipMemcpyAsync(out_counts, d_counts, (size_t)npairs * sizeof(int),
                               hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&ctx->timing[T_PREMATCH], ctx->ev[1], ctx->ev[2]);
    return download_fitting(ctx, out_counts, npairs, ctx->b_out.as<int>(), out_pairs, cap, want_matches);
}

}  // namespace

extern "C" {

int sgpu_select_top_scale_batch(sgpu_ctx* ctx, const float* scale, int scale_stride,
                                const int64_t* set_offsets, int nsets, int top, int* out_index,
                                int64_t* out_offsets, int flags) {
    if (!ctx) return SGPU_EINVAL;
    if (nsets < 0 || !set_offsets) return ctx->fail(SGPU_EINVAL, "bad select arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    SetSource in;
    in.device = (flags & SGPU_INPUT_DEVICE) != 0;
    in.scale = scale;
    in.scale_stride = scale_stride;
    return select_impl(ctx, in, set_offsets, nsets, top, out_index, out_offsets);
}

int sgpu_select_top_scale_images(sgpu_ctx* ctx, int top, int* out_index, int64_t* out_offsets) {
    if (!ctx) return SGPU_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = check_batch(ctx, "select from")) return rc;
    SetSource in;
    in.images = true;
    return select_impl(ctx, in, ctx->img_off.data(), ctx->batch, top, out_index, out_offsets);
}

int sgpu_prematch_batch(sgpu_ctx* ctx, const uint8_t* desc, const float* scale, int scale_stride,
                        const int64_t* set_offsets, int nsets, const int* set_pairs, int npairs,
                        int top, float distmax, float ratiomax, int mutual_best_match,
                        int* out_counts, int* out_pairs, int64_t cap, int flags) {
    if (!ctx) return SGPU_EINVAL;
    if (nsets < 0 || npairs < 0 || !set_offsets) return ctx->fail(SGPU_EINVAL, "bad prematch arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    SetSource in;
    in.device = (flags & SGPU_INPUT_DEVICE) != 0;
    in.desc = desc;
    in.scale = scale;
    in.scale_stride = scale_stride;
    return prematch_impl(ctx, in, set_offsets, nsets, set_pairs, npairs, top, distmax, ratiomax,
                         mutual_best_match, out_counts, out_pairs, cap);
}

int sgpu_prematch_images(sgpu_ctx* ctx, const int* image_pairs, int npairs, int top, float distmax,
                         float ratiomax, int mutual_best_match, int* out_counts, int* out_pairs,
                         int64_t cap) {
    if (!ctx) return SGPU_EINVAL;
    if (npairs < 0) return ctx->fail(SGPU_EINVAL, "bad prematch arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = check_batch(ctx, "select from")) return rc;
    SetSource in;
    in.images = true;
    return prematch_impl(ctx, in, ctx->img_off.data(), ctx->batch, image_pairs, npairs, top, distmax,
                         ratiomax, mutual_best_match, out_counts, out_pairs, cap);
}

}  // extern "C"
