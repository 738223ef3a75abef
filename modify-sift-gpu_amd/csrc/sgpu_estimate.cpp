// sgpu_estimate.cpp -- host side of the geometry estimator over the grouped pair matcher's matches
// (sgpu_estimate_batch*, sgpu_estimate_images*).
#include <cstring>

#include "sgpu_ctx.h"

using namespace sgh;

extern "C" {

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
    if (const int rc = check_batch(ctx, "estimate on")) return rc;
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
