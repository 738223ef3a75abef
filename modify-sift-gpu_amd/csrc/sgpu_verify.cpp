// sgpu_verify.cpp -- host side of the verify chain (sgpu_verify_batch, sgpu_verify_images;
// DESIGN.md 4.17): the grouped pair matcher, the refined estimator of H and / or F and the guided
// pair matcher of sgpu_match_batch.cpp queued back to back on the context's stream.  What the
// stages hand each other -- the putative matches, their counts and offsets, the matrices -- stays
// in device memory; the host validates and plans once, uploads one table block and downloads one
// result block.
#include <cstring>

#include "sgpu_ctx.h"

using namespace sgh;

namespace {

struct VerifyOutput {
    float* H;
    int* inliers_H;
    float* F;
    int* inliers_F;
    int* putative;
    int* pairs;
    int64_t cap;
    int* counts;
};

// The whole call.  Queue order on ctx->stream: [prep] k_match_pairs, finish, compact (cap = the
// plan's bound) -> k_verify_pair_recs -> k_verify_gather -> per model: k_estimate_pairs (guarded),
// k_estimate_finish, k_estimate_refine -> k_verify_guided_params -> k_match_pairs_guided, finish,
// compact (the caller's cap, its own counts / offsets).  Two memsets (all slots, all error
// flags), one table upload, one result download, two synchronisations, whatever npairs and
// refine_rounds are.
int verify_impl(sgpu_ctx* ctx, const SetSource& in, const int64_t* off, int nsets,
                const int* set_pairs, int npairs, const sgpu_verify_params* vp,
                const VerifyOutput& out) {
    if (!vp) return ctx->fail(SGPU_EINVAL, "null verify params");
    if (vp->iterations < 1 || vp->iterations > sgeo::kMaxIterations)
        return ctx->fail(SGPU_EINVAL, "iterations outside [1, 65536]");
    if (vp->refine_rounds < 0 || vp->refine_rounds > sgeo::kMaxRefineRounds)
        return ctx->fail(SGPU_EINVAL, "refine_rounds outside [0, 16]");
    if (!out.H && !out.F) return ctx->fail(SGPU_EINVAL, "no model requested (out_H and out_F are null)");
    hipStream_t st = ctx->stream;
    // one plan for both matching passes: the same sets, pairs, mutual and max_match
    sgplan::Plan& plan = ctx->b_hplan;
    const int prc = sgplan::build_plan(off, nsets, set_pairs, npairs, vp->mutual_best_match != 0,
                                       vp->max_match, plan);
    ctx->b_planned = prc == sgplan::kPlanOk;
    if (prc == sgplan::kPlanBadArgument)
        return ctx->fail(SGPU_EINVAL, "bad set offsets or pair indices");
    if (prc != sgplan::kPlanOk) return ctx->fail(SGPU_ERANGE, "match batch too large");
    if (npairs == 0) return 0;
    if (!out.counts) return ctx->fail(SGPU_EINVAL, "null out_counts");
    const int64_t cap = std::max<int64_t>(out.cap, 0);
    if (cap > 0 && !out.pairs) return ctx->fail(SGPU_EINVAL, "null out_pairs");
    // the estimator's work items: every (pair, block) -- the host does not know the counts
    const int blocks = (vp->iterations + sgeo::kBlockHyp - 1) / sgeo::kBlockHyp;
    if ((int64_t)npairs * blocks > INT_MAX) return ctx->fail(SGPU_ERANGE, "estimate batch too large");
    const int nitems = npairs * blocks;
    const int nm = (out.H ? 1 : 0) + (out.F ? 1 : 0);
    const size_t n = (size_t)npairs;
    // host input is read whenever there are rows, as the separate calls upload it
    if (!in.images && !in.device && off[nsets] > 0 && !in.desc)
        return ctx->fail(SGPU_EINVAL, "null descriptors");
    if (!in.images && !in.device && off[nsets] > 0 && !in.loc)
        return ctx->fail(SGPU_EINVAL, "verify needs locations");
    if (plan.items.empty()) {   // every pair has an empty set: no match, no model
        memset(out.counts, 0, n * sizeof(int));
        if (out.putative) memset(out.putative, 0, n * sizeof(int));
        if (out.H) memset(out.H, 0, n * 9 * sizeof(float));
        if (out.F) memset(out.F, 0, n * 9 * sizeof(float));
        if (out.inliers_H) memset(out.inliers_H, 0, n * sizeof(int));
        if (out.inliers_F) memset(out.inliers_F, 0, n * sizeof(int));
        ctx->timing[T_VERIFY] = 0.f;
        return 0;
    }
    const int64_t total_rows = off[nsets];
    if (!in.images && !in.desc) return ctx->fail(SGPU_EINVAL, "null descriptors");
    if (!in.images && !in.loc) return ctx->fail(SGPU_EINVAL, "verify needs locations");

    // ---- everything is checked: the inputs
    DeviceSets sets;
    if (const int rc = resolve_sets(ctx, in, total_rows, SET_DESC | SET_LOC, sets)) return rc;
    if (const int rc = ensure_dist_table(ctx)) return rc;

    // ---- the tables in one buffer, one upload: the matcher's [items][sides][finish panels]
    // [pairs], then the estimator's [pairs][items]; the estimator's pairs carry their sets' first
    // rows, k_verify_pair_recs fills moff / m on the device
    const sgplan::TableLayout lay = sgplan::table_layout(plan);
    const size_t o_epairs = lay.bytes, o_eitems = o_epairs + n * sizeof(sgeo::PairRec);
    ctx->b_tables.resize(o_eitems + (size_t)nitems * sizeof(sgeo::Item));
    unsigned char* tb = ctx->b_tables.data();
    sgplan::pack_tables(plan, tb);
    auto* h_epairs = reinterpret_cast<sgeo::PairRec*>(tb + o_epairs);
    auto* h_eitems = reinterpret_cast<sgeo::Item*>(tb + o_eitems);
    for (int p = 0; p < npairs; p++) {
        h_epairs[p] = sgeo::PairRec{0, (int)off[set_pairs[2 * p]], (int)off[set_pairs[2 * p + 1]], 0, 0};
        for (int b = 0; b < blocks; b++) h_eitems[(size_t)p * blocks + b] = sgeo::Item{p, b};
    }

    // ---- the device block the stages share (v_buf):
    //   [putative offsets npairs + 1 (64-bit)][final offsets npairs + 1][slots nm x npairs (64-bit)]
    //   [result: final counts npairs | putative counts npairs | models nm x npairs x 9 |
    //            inliers nm x npairs | error flags nm]     <- the one download
    //   [accepted rounds nm x npairs][guided params npairs]
    const size_t b_offs = (n + 1) * sizeof(long long);
    const size_t b_slots = (size_t)nm * n * sizeof(unsigned long long);
    const size_t o_result = 2 * b_offs + b_slots;
    const size_t r_put = n * sizeof(int), r_models = 2 * n * sizeof(int);
    const size_t r_inliers = r_models + (size_t)nm * n * 9 * sizeof(float);
    const size_t r_err = r_inliers + (size_t)nm * n * sizeof(int);
    const size_t b_result = r_err + (size_t)nm * sizeof(int);
    const size_t o_rounds = o_result + b_result;
    const size_t o_geom = round8(o_rounds + (size_t)nm * n * sizeof(int));
    const size_t b_vbuf = o_geom + n * sizeof(sgk::GuidedParams);
    const int64_t bound = plan.out_bound;   // the putative pass has no user cap
    const int64_t out_rows = std::min<int64_t>(cap, bound);
    // b_out by the plan's bound, not the cap; the counts and offsets of both passes are v_buf's
    if (const int rc = ensure_pair_buffers(ctx, plan, ctx->b_tables.size(), bound, 0,
                                           sets.s8 && sets.sums ? 0 : total_rows))
        return rc;
    ALLOCCHK(ctx, ctx->e_pts.ensure((size_t)std::max<int64_t>(bound, 1) * sizeof(float4)));
    ALLOCCHK(ctx, ctx->v_buf.ensure(b_vbuf));
    ctx->v_result.resize(b_result);
    HIPCHK(ctx, hipMemcpyAsync(ctx->b_plan.p, tb, ctx->b_tables.size(), hipMemcpyHostToDevice, st));
    unsigned char* dt = ctx->b_plan.as<unsigned char>();
    auto* d_epairs = reinterpret_cast<sgeo::PairRec*>(dt + o_epairs);
    const auto* d_eitems = reinterpret_cast<const sgeo::Item*>(dt + o_eitems);
    unsigned char* dv = ctx->v_buf.as<unsigned char>();
    long long* d_offs1 = reinterpret_cast<long long*>(dv);
    long long* d_offs2 = reinterpret_cast<long long*>(dv + b_offs);
    auto* d_slots = reinterpret_cast<unsigned long long*>(dv + 2 * b_offs);
    int* d_counts2 = reinterpret_cast<int*>(dv + o_result);
    int* d_counts1 = reinterpret_cast<int*>(dv + o_result + r_put);
    float* d_models = reinterpret_cast<float*>(dv + o_result + r_models);
    int* d_inliers = reinterpret_cast<int*>(dv + o_result + r_inliers);
    int* d_err = reinterpret_cast<int*>(dv + o_result + r_err);
    int* d_rounds = reinterpret_cast<int*>(dv + o_rounds);
    auto* d_geom = reinterpret_cast<sgk::GuidedParams*>(dv + o_geom);
    int* d_out = ctx->b_out.as<int>();
    float4* d_pts = ctx->e_pts.as<float4>();

    // ---- the queue
    if (!sets.timing_started) HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    if (const int rc = derive_s8(ctx, sets, total_rows)) return rc;
    HIPCHK(ctx, hipMemsetAsync(d_slots, 0, b_slots, st));
    HIPCHK(ctx, hipMemsetAsync(d_err, 0, (size_t)nm * sizeof(int), st));
    // pass 1: the putative matches, all of them, in b_out
    MatchPass pass{sets.s8, sets.sums, plan, sgplan::view_tables(lay, dt), vp->distmax, vp->ratiomax,
                   vp->max_match, bound, d_counts1, d_offs1, d_out};
    if (const int rc = queue_match_pass(ctx, pass)) return rc;
    // the estimator's view of them
    HIPCHK(ctx, sgk::launch_verify_pair_recs(d_offs1, d_counts1, npairs, d_epairs, st));
    HIPCHK(ctx, sgk::launch_verify_gather(sets.loc, sets.loc_stride, d_epairs, npairs, d_out,
                                          d_offs1 + npairs, bound, d_pts, st));
    const float* d_H = nullptr;
    const float* d_F = nullptr;
    for (int k = 0; k < nm; k++) {
        const int model = (k == 0 && out.H) ? sgeo::kModelH : sgeo::kModelF;
        const float thr = model == sgeo::kModelH ? vp->h_threshold : vp->f_threshold;
        float* mk = d_models + (size_t)k * n * 9;
        int* ik = d_inliers + (size_t)k * n;
        (model == sgeo::kModelH ? d_H : d_F) = mk;
        HIPCHK(ctx, sgk::launch_verify_estimate_pairs(d_pts, d_epairs, d_eitems, nitems, model, thr,
                                                      vp->iterations, vp->seed,
                                                      d_slots + (size_t)k * n, st));
        HIPCHK(ctx, sgk::launch_estimate_finish(d_pts, d_epairs, npairs, model, thr, vp->seed,
                                                d_slots + (size_t)k * n, mk, ik, nullptr,
                                                d_err + k, st));
        HIPCHK(ctx, sgk::launch_estimate_refine(d_pts, d_epairs, npairs, model, thr,
                                                vp->refine_rounds, mk, ik, nullptr,
                                                d_rounds + (size_t)k * n, st));
    }
    // pass 2 under the device's matrices: b_part / b_dec again, and b_out, which the gather has
    // consumed; its own counts and offsets, so that the putative counts survive
    HIPCHK(ctx, sgk::launch_verify_guided_params(d_H, d_F, vp->hdistmax, vp->fdistmax, npairs, d_geom, st));
    pass.out_rows = out_rows;
    pass.d_counts = d_counts2;
    pass.d_offs = d_offs2;
    pass.loc = sets.loc;
    pass.loc_stride = sets.loc_stride;
    pass.d_geom = d_geom;
    if (const int rc = queue_match_pass(ctx, pass)) return rc;
    HIPCHK(ctx, hipEventRecord(ctx->ev[2], st));
    // ---- nothing has come down or been waited for so far: the one result block
    unsigned char* hr = ctx->v_result.data();
    HIPCHK(ctx, hipMemcpyAsync(hr, dv + o_result, b_result, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&ctx->timing[T_VERIFY], ctx->ev[1], ctx->ev[2]);
    memcpy(out.counts, hr, n * sizeof(int));
    if (out.putative) memcpy(out.putative, hr + r_put, n * sizeof(int));
    for (int k = 0; k < nm; k++) {
        const bool is_h = k == 0 && out.H;
        memcpy(is_h ? out.H : out.F, hr + r_models + (size_t)k * n * 9 * sizeof(float), n * 9 * sizeof(float));
        int* oi = is_h ? out.inliers_H : out.inliers_F;
        if (oi) memcpy(oi, hr + r_inliers + (size_t)k * n * sizeof(int), n * sizeof(int));
    }
    int err = 0;
    for (int k = 0; k < nm; k++) {
        int e = 0;
        memcpy(&e, hr + r_err + (size_t)k * sizeof(int), sizeof(int));
        err |= e;
    }
    if (err) return ctx->fail(SGPU_ENODEV, "estimate: a regenerated winner's inlier count differs from its score");
    return download_fitting(ctx, out.counts, npairs, d_out, out.pairs, cap);
}

}  // namespace

extern "C" {

void sgpu_default_verify_params(sgpu_verify_params* p) {
    if (!p) return;
    p->distmax = 0.7f;
    p->ratiomax = 0.8f;
    p->mutual_best_match = 1;
    p->max_match = 4096;
    p->h_threshold = 2.0f;
    p->f_threshold = 4.0f;
    p->hdistmax = 2.0f;
    p->fdistmax = 4.0f;
    p->iterations = 512;
    p->seed = 0;
    p->refine_rounds = 3;
}

int sgpu_verify_batch(sgpu_ctx* ctx, const uint8_t* desc, const float* loc,
                      const int64_t* set_offsets, int nsets, const int* set_pairs, int npairs,
                      const sgpu_verify_params* params, float* out_H, int* out_inliers_H,
                      float* out_F, int* out_inliers_F, int* out_putative, int* out_pairs,
                      int64_t cap, int* out_counts, int flags) {
    if (!ctx) return SGPU_EINVAL;
    if (nsets < 0 || npairs < 0 || !set_offsets) return ctx->fail(SGPU_EINVAL, "bad verify batch arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    SetSource in;
    in.device = (flags & SGPU_INPUT_DEVICE) != 0;
    in.desc = desc;
    in.loc = loc;
    return verify_impl(ctx, in, set_offsets, nsets, set_pairs, npairs, params,
                       VerifyOutput{out_H, out_inliers_H, out_F, out_inliers_F, out_putative,
                                    out_pairs, cap, out_counts});
}

int sgpu_verify_images(sgpu_ctx* ctx, const int* image_pairs, int npairs,
                       const sgpu_verify_params* params, float* out_H, int* out_inliers_H,
                       float* out_F, int* out_inliers_F, int* out_putative, int* out_pairs,
                       int64_t cap, int* out_counts) {
    if (!ctx) return SGPU_EINVAL;
    if (npairs < 0) return ctx->fail(SGPU_EINVAL, "bad verify arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the states sgpu_match_images_guided refuses (feature_u8), before anything is queued
    if (const int rc = check_batch(ctx, "verify on")) return rc;
    SetSource in;
    in.images = true;
    return verify_impl(ctx, in, ctx->img_off.data(), ctx->batch, image_pairs, npairs, params,
                       VerifyOutput{out_H, out_inliers_H, out_F, out_inliers_F, out_putative,
                                    out_pairs, cap, out_counts});
}

}  // extern "C"
