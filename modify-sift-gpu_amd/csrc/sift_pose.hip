// sift_pose.hip -- relative pose and triangulation of verified pairs on the device
// (sgpu_pose_batch).  The contract and every arithmetic step live in sift_pose.h,
// shared with the host loop spose::pose_host; this file is the kernel:
//   k_pose   one wave per pair, a grid-stride over the pair list; the pair's matches are the float4
//            rows (x1, y1, x2, y2) that k_estimate_gather (sift_geom.hip) made.
//            Every lane decomposes the pair's E itself: the 3 x 3 Jacobi is unrolled over
//            compile-time indices, so its state is a handful of named doubles, the same in every
//            lane; no LDS, no array indexed at run time.
//            Pass one: lane l walks matches l, l + 64, ..., tests participation (the guided
//            matcher's float test) and counts, per candidate, the participants in front; a xor
//            butterfly sums the five counters over the wave.
//            Pass two, under the winner: the float test again (cheaper than keeping a bit per
//            match for an unbounded m), the midpoint, mask and point of the in-front matches, the
//            wide count.
// The outputs are zero before the launch (one memset by the host): a pair without matches leaves at
// once, a pair without a pose after its participant count, and pass two stores the in-front
// matches only.
#include "sift_kernels.h"
#include "sift_pose.h"

namespace sgk {
namespace {

constexpr int kPoseWaves = 4;            // waves (pairs in flight) per workgroup
constexpr int kPoseMaxBlocks = 2048;     // 256 CUs x 8 workgroups: the rest by the grid-stride

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(64 * kPoseWaves) void k_pose(PoseArgs a, int npairs, float f_threshold,
                                                         double cos_min) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int stride = (int)gridDim.x * kPoseWaves;
    for (int p = (int)blockIdx.x * kPoseWaves + wave; p < npairs; p += stride) {
        const sgeo::PairRec pr = a.pairs[p];
        const int m = pr.m;
        if (m == 0) continue;
        float F[9], Ka[4], Kb[4];
#pragma unroll
        for (int i = 0; i < 9; i++) F[i] = a.F[9 * (size_t)p + i];
        const int sa = a.set_pairs[2 * p], sb = a.set_pairs[2 * p + 1];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            Ka[i] = a.intrinsics[4 * (size_t)sa + i];
            Kb[i] = a.intrinsics[4 * (size_t)sb + i];
        }
        spose::Pose P;
        spose::Cams cam;
        const bool ok = spose::decompose(F, Ka, Kb, P);
        spose::cameras(Ka, Kb, cam);
        const float4* __restrict__ q = a.pts + pr.moff;

        int n = 0, front[4] = {0, 0, 0, 0};
        for (int k = lane; k < m; k += 64) {
            const float4 v = q[k];
            const bool part = sgeo::inlier(sgeo::kModelF, F, v.x, v.y, v.z, v.w, f_threshold);
            n += part;
            if (part && ok) {
                const int bits = spose::front_bits(cam, P, v.x, v.y, v.z, v.w);
#pragma unroll
                for (int c = 0; c < 4; c++) front[c] += (bits >> c) & 1;
            }
        }
        n = wave_sum(n);
#pragma unroll
        for (int c = 0; c < 4; c++) front[c] = wave_sum(front[c]);
        if (lane == 0) a.counts[3 * (size_t)p] = n;
        int most = 0;
        const int w = spose::winner(front, &most);
        if (!ok || most == 0) continue;   // the same in every lane: the sums are the wave's

        double R[9], t[3];
        spose::candidate(P, w, R, t);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 9; i++) a.R[9 * (size_t)p + i] = (float)R[i];
#pragma unroll
            for (int i = 0; i < 3; i++) a.t[3 * (size_t)p + i] = (float)t[i];
        }
        int nf = 0, nw = 0;
        for (int k = lane; k < m; k += 64) {
            const float4 v = q[k];
            if (!sgeo::inlier(sgeo::kModelF, F, v.x, v.y, v.z, v.w, f_threshold)) continue;
            float X[3];
            bool wd = false;
            if (!spose::resolve(cam, R, t, cos_min, v.x, v.y, v.z, v.w, X, &wd)) continue;
            nf++;
            nw += wd;
            const size_t at = (size_t)pr.moff + (size_t)k;
            if (a.mask) a.mask[at] = 1;
            if (a.points) {
                a.points[3 * at] = X[0];
                a.points[3 * at + 1] = X[1];
                a.points[3 * at + 2] = X[2];
            }
        }
        nf = wave_sum(nf);
        nw = wave_sum(nw);
        if (lane == 0) {
            a.counts[3 * (size_t)p + 1] = nf;
            a.counts[3 * (size_t)p + 2] = nw;
        }
    }
}

}  // namespace

hipError_t launch_pose(const PoseArgs& a, int npairs, float f_threshold, double cos_min,
                       hipStream_t stream) {
    if (npairs <= 0) return hipSuccess;
    const int blocks = std::min((npairs + kPoseWaves - 1) / kPoseWaves, kPoseMaxBlocks);
    hipLaunchKernelGGL(k_pose, dim3(blocks), dim3(64 * kPoseWaves), 0, stream, a, npairs, f_threshold,
                       cos_min);
    return hipGetLastError();
}

}  // namespace sgk
