// sgpu_pose.cpp -- host side of the relative pose of verified pairs (sgpu_pose_batch,
// sgpu_pose_images): sift_pose.h is the rule, sift_pose.hip the kernel.
#include <cstring>

#include "sgpu_ctx.h"
#include "sift_pose.h"

using namespace sgh;

namespace {

// loc: device locations (x, y of buffer row r at loc[r * stride]), or host_loc: packed host
// locations uploaded here, after every argument has been checked.  One table upload ([pairs]
// [matches][set pairs][F][intrinsics]), one memset of the result block, two launches (the
// estimator's gather, k_pose), one download ([R][t][counts][points][mask]) and one
// synchronisation, whatever npairs is.
int pose_impl(sgpu_ctx* ctx, const float* loc, int stride, const float* host_loc, const int64_t* off,
              int nsets, const float* intrinsics, const int* set_pairs, int npairs, const int* matches,
              const int* counts, const float* F, float f_threshold, float min_angle, float* out_R,
              float* out_t, int* out_counts, uint8_t* out_mask, float* out_points) {
    hipStream_t st = ctx->stream;
    sgeo::Plan& plan = ctx->e_hplan;
    const char* why = "";
    const int arc = spose::check_args(off, nsets, intrinsics, set_pairs, npairs, matches, counts, F,
                                      f_threshold, min_angle, out_R, out_t, out_counts, plan, &why);
    if (arc == spose::kArgsTooLarge) return ctx->fail(SGPU_ERANGE, why);
    if (arc != spose::kArgsOk) return ctx->fail(SGPU_EINVAL, why);
    const long long total = plan.total;
    if (total > 0 && !loc && !host_loc) return ctx->fail(SGPU_EINVAL, "null locations");
    ctx->timing[T_POSE] = 0.f;
    if (npairs == 0) return SGPU_OK;
    if (host_loc && total > 0) {
        const size_t bytes = (size_t)off[nsets] * 2 * sizeof(float);
        ALLOCCHK(ctx, ctx->e_loc.ensure(bytes));
        HIPCHK(ctx, hipMemcpyAsync(ctx->e_loc.p, host_loc, bytes, hipMemcpyHostToDevice, st));
        loc = ctx->e_loc.as<float>();
        stride = 2;
    }
    // ---- the tables, one block
    const size_t b_pairs = (size_t)npairs * sizeof(sgeo::PairRec);
    const size_t b_matches = (size_t)total * 2 * sizeof(int);
    const size_t b_sets = (size_t)npairs * 2 * sizeof(int);
    const size_t b_F = (size_t)npairs * 9 * sizeof(float);
    const size_t b_K = (size_t)nsets * 4 * sizeof(float);
    static_assert(sizeof(sgeo::PairRec) % 8 == 0, "the matches stay 8-byte aligned");
    ctx->o_tables.resize(b_pairs + b_matches + b_sets + b_F + b_K);
    unsigned char* tb = ctx->o_tables.data();
    memcpy(tb, plan.pairs.data(), b_pairs);
    if (b_matches) memcpy(tb + b_pairs, matches, b_matches);
    memcpy(tb + b_pairs + b_matches, set_pairs, b_sets);
    memcpy(tb + b_pairs + b_matches + b_sets, F, b_F);
    memcpy(tb + b_pairs + b_matches + b_sets + b_F, intrinsics, b_K);
    // ---- the results, one block: [R][t][counts][points, if asked for][mask, if asked for]
    const size_t b_R = (size_t)npairs * 9 * sizeof(float), b_t = (size_t)npairs * 3 * sizeof(float);
    const size_t b_counts = (size_t)npairs * 3 * sizeof(int);
    const size_t b_points = out_points ? (size_t)total * 3 * sizeof(float) : 0;
    const size_t b_mask = out_mask ? (size_t)total : 0;
    const size_t b_result = b_R + b_t + b_counts + b_points + b_mask;
    ALLOCCHK(ctx, ctx->o_tab.ensure(ctx->o_tables.size()));
    ALLOCCHK(ctx, ctx->e_pts.ensure((size_t)std::max<long long>(total, 1) * sizeof(float4)));
    ALLOCCHK(ctx, ctx->o_out.ensure(b_result));
    ctx->o_result.resize(b_result);
    HIPCHK(ctx, hipMemcpyAsync(ctx->o_tab.p, tb, ctx->o_tables.size(), hipMemcpyHostToDevice, st));
    const unsigned char* dt = ctx->o_tab.as<unsigned char>();
    unsigned char* dr = ctx->o_out.as<unsigned char>();
    const int* d_matches = reinterpret_cast<const int*>(dt + b_pairs);
    sgk::PoseArgs a;
    a.pts = ctx->e_pts.as<float4>();
    a.pairs = reinterpret_cast<const sgeo::PairRec*>(dt);
    a.set_pairs = reinterpret_cast<const int*>(dt + b_pairs + b_matches);
    a.F = reinterpret_cast<const float*>(dt + b_pairs + b_matches + b_sets);
    a.intrinsics = reinterpret_cast<const float*>(dt + b_pairs + b_matches + b_sets + b_F);
    a.R = reinterpret_cast<float*>(dr);
    a.t = reinterpret_cast<float*>(dr + b_R);
    a.counts = reinterpret_cast<int*>(dr + b_R + b_t);
    a.points = out_points ? reinterpret_cast<float*>(dr + b_R + b_t + b_counts) : nullptr;
    a.mask = out_mask ? dr + b_R + b_t + b_counts + b_points : nullptr;
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipMemsetAsync(dr, 0, b_result, st));
    HIPCHK(ctx, sgk::launch_estimate_gather(loc, stride, a.pairs, npairs, d_matches, total,
                                            ctx->e_pts.as<float4>(), st));
    HIPCHK(ctx, sgk::launch_pose(a, npairs, f_threshold, spose::cos_min_angle(min_angle), st));
    HIPCHK(ctx, hipEventRecord(ctx->ev[2], st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->o_result.data(), dr, b_result, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&ctx->timing[T_POSE], ctx->ev[1], ctx->ev[2]);
    const unsigned char* hr = ctx->o_result.data();
    memcpy(out_R, hr, b_R);
    memcpy(out_t, hr + b_R, b_t);
    memcpy(out_counts, hr + b_R + b_t, b_counts);
    if (b_points) memcpy(out_points, hr + b_R + b_t + b_counts, b_points);
    if (b_mask) memcpy(out_mask, hr + b_R + b_t + b_counts + b_points, b_mask);
    return SGPU_OK;
}

}  // namespace

extern "C" {

int sgpu_pose_batch(sgpu_ctx* ctx, const float* loc, const int64_t* set_offsets, int nsets,
                    const float* intrinsics, const int* set_pairs, int npairs, const int* matches,
                    const int* match_counts, const float* F, float f_threshold, float min_angle,
                    float* out_R, float* out_t, int* out_counts, uint8_t* out_mask,
                    float* out_points, int flags) {
    if (!ctx) return SGPU_EINVAL;
    if (nsets < 0 || npairs < 0 || !set_offsets) return ctx->fail(SGPU_EINVAL, "bad pose batch arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool dev = (flags & SGPU_INPUT_DEVICE) != 0;
    return pose_impl(ctx, dev ? loc : nullptr, 2, dev ? nullptr : loc, set_offsets, nsets, intrinsics,
                     set_pairs, npairs, matches, match_counts, F, f_threshold, min_angle, out_R, out_t,
                     out_counts, out_mask, out_points);
}

int sgpu_pose_images(sgpu_ctx* ctx, const float* intrinsics, const int* image_pairs, int npairs,
                     const int* matches, const int* match_counts, const float* F, float f_threshold,
                     float min_angle, float* out_R, float* out_t, int* out_counts, uint8_t* out_mask,
                     float* out_points) {
    if (!ctx) return SGPU_EINVAL;
    if (npairs < 0) return ctx->fail(SGPU_EINVAL, "bad pose arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = check_batch(ctx, "take poses on")) return rc;
    const float* keys = nullptr;
    const int rc = sgpu_device_features(ctx, &keys, nullptr, nullptr);   // (gathers a multi-part batch)
    if (rc != SGPU_OK) return rc;
    return pose_impl(ctx, keys, 4, nullptr, ctx->img_off.data(), ctx->batch, intrinsics, image_pairs,
                     npairs, matches, match_counts, F, f_threshold, min_angle, out_R, out_t,
                     out_counts, out_mask, out_points);
}

}  // extern "C"
