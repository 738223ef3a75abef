// sift_geom.hip -- H / F estimation of many matched pairs in one call (sgpu_estimate_batch,
// DESIGN.md 4.14).  A fixed budget of RANSAC hypotheses per pair; sampler, solvers and the inlier
// test are sift_geom.h's, the same functions the host loop sgeo::estimate_host runs, so the
// results are its bits.
//
//   k_estimate_gather   a thread per match: the two locations of match k as one float4 row, so
//                       that the scoring kernel reads coalesced rows instead of gathering again
//                       in every workgroup
//   k_estimate_pairs    a workgroup per (pair, block of 256 hypotheses), a lane per hypothesis:
//                       the lane samples, solves in double and keeps its float[9] in registers;
//                       the pair's rows pass through LDS in tiles and every lane tests the same
//                       row at the same time (one broadcast LDS address), counting its own
//                       inliers.  The block's best (count, lowest t) goes to the pair's 64-bit
//                       slot by one atomic max; no model is stored per hypothesis.
//   k_estimate_finish   a workgroup per pair: regenerates the winner from its t, writes the
//                       model, the mask and the count; a count that differs from the slot's is
//                       reported through *err (a library error, never a device assert).
#include "sift_kernels.h"
#include "sift_geom.h"

namespace sgk {
namespace {

constexpr int kThreads = sgeo::kBlockHyp;
static_assert(kThreads == 256 && sgeo::kMatchTile % kThreads == 0, "a lane per hypothesis");

__global__ __launch_bounds__(256) void k_estimate_gather(const float* __restrict__ loc,
                                                         int loc_stride,
                                                         const sgeo::PairRec* __restrict__ pairs,
                                                         int npairs,
                                                         const int* __restrict__ matches,
                                                         long long total,
                                                         float4* __restrict__ pts) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= total) return;
    // the last pair whose first match is <= k (pairs without matches share their successor's)
    int lo = 0, hi = npairs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pairs[mid].moff <= k) lo = mid;
        else hi = mid - 1;
    }
    const sgeo::PairRec pr = pairs[lo];
    const int2 ij = reinterpret_cast<const int2*>(matches)[k];
    const float2 a = *reinterpret_cast<const float2*>(loc + (size_t)(pr.a_off + ij.x) * loc_stride);
    const float2 b = *reinterpret_cast<const float2*>(loc + (size_t)(pr.b_off + ij.y) * loc_stride);
    pts[k] = make_float4(a.x, a.y, b.x, b.y);
}

template <int MODEL>
__global__ __launch_bounds__(256) void k_estimate_pairs(const float4* __restrict__ pts,
                                                        const sgeo::PairRec* __restrict__ pairs,
                                                        const sgeo::Item* __restrict__ items,
                                                        float threshold, int iterations,
                                                        uint32_t seed,
                                                        unsigned long long* __restrict__ slots) {
    __shared__ float4 s_pts[sgeo::kMatchTile];
    __shared__ unsigned long long s_best[kThreads / 64];
    const sgeo::Item it = items[blockIdx.x];
    const sgeo::PairRec pr = pairs[it.pair];
    const float4* __restrict__ P = pts + pr.moff;
    const int m = pr.m;
    const uint32_t t = (uint32_t)it.block * kThreads + threadIdx.x;
    float M[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool valid = false;
    if (t < (uint32_t)iterations)
        valid = sgeo::hypothesis<MODEL>(reinterpret_cast<const float*>(P), m, seed,
                                        (uint32_t)it.pair, t, M);
    // (an invalid lane scores its zero matrix, which passes nothing, and takes part in the
    // barriers)
    int count = 0;
    for (int base = 0; base < m; base += sgeo::kMatchTile) {
        const int n = min(sgeo::kMatchTile, m - base);
        for (int i = threadIdx.x; i < n; i += kThreads) s_pts[i] = P[base + i];
        __syncthreads();
        for (int k = 0; k < n; k++) {
            const float4 q = s_pts[k];
            count += sgeo::inlier(MODEL, M, q.x, q.y, q.z, q.w, threshold) ? 1 : 0;
        }
        __syncthreads();
    }
    unsigned long long key = valid ? sgeo::hyp_key(count, t) : 0ull;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(key, d, 64);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kThreads / 64; w++) key = s_best[w] > key ? s_best[w] : key;
        if (key != 0ull) atomicMax(&slots[it.pair], key);
    }
}

template <int MODEL>
__global__ __launch_bounds__(256) void k_estimate_finish(const float4* __restrict__ pts,
                                                         const sgeo::PairRec* __restrict__ pairs,
                                                         float threshold, uint32_t seed,
                                                         const unsigned long long* __restrict__ slots,
                                                         float* __restrict__ models,
                                                         int* __restrict__ inliers,
                                                         uint8_t* __restrict__ mask,
                                                         int* __restrict__ err) {
    __shared__ float s_M[9];
    __shared__ int s_ok, s_count;
    const int p = blockIdx.x;
    const sgeo::PairRec pr = pairs[p];
    const float4* __restrict__ P = pts + pr.moff;
    const unsigned long long slot = slots[p];
    if (threadIdx.x == 0) {
        float M[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        bool ok = false;
        if (slot != 0ull)
            ok = sgeo::hypothesis<MODEL>(reinterpret_cast<const float*>(P), pr.m, seed, (uint32_t)p,
                                         0xFFFFFFFFu - (uint32_t)slot, M);
#pragma unroll
        for (int i = 0; i < 9; i++) s_M[i] = M[i];
        s_ok = ok ? 1 : 0;
        s_count = 0;
    }
    __syncthreads();
    float M[9];
#pragma unroll
    for (int i = 0; i < 9; i++) M[i] = s_M[i];
    const bool ok = s_ok != 0;
    int count = 0;
    for (int k = threadIdx.x; k < pr.m; k += kThreads) {
        const float4 q = P[k];
        const bool in = ok && sgeo::inlier(MODEL, M, q.x, q.y, q.z, q.w, threshold);
        if (mask) mask[pr.moff + k] = in ? 1 : 0;
        count += in ? 1 : 0;
    }
    if (count) atomicAdd(&s_count, count);
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 9; i++) models[9 * (size_t)p + i] = M[i];
        inliers[p] = s_count;
        // the winner regenerated here must be the hypothesis that was scored
        if ((slot != 0ull && !ok) || s_count != (int)(slot >> 32)) *err = 1;
    }
}

}  // namespace

hipError_t launch_estimate_gather(const float* loc, int loc_stride, const sgeo::PairRec* pairs,
                                  int npairs, const int* matches, long long total, float4* pts,
                                  hipStream_t stream) {
    if (total <= 0 || npairs <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((total + 255) / 256);
    hipLaunchKernelGGL(k_estimate_gather, dim3(grid), dim3(256), 0, stream, loc, loc_stride, pairs,
                       npairs, matches, total, pts);
    return hipGetLastError();
}

hipError_t launch_estimate_pairs(const float4* pts, const sgeo::PairRec* pairs,
                                 const sgeo::Item* items, int nitems, int model, float threshold,
                                 int iterations, uint32_t seed, unsigned long long* slots,
                                 hipStream_t stream) {
    if (nitems <= 0) return hipSuccess;
    if (model == sgeo::kModelF)
        hipLaunchKernelGGL(k_estimate_pairs<sgeo::kModelF>, dim3(nitems), dim3(kThreads), 0, stream,
                           pts, pairs, items, threshold, iterations, seed, slots);
    else
        hipLaunchKernelGGL(k_estimate_pairs<sgeo::kModelH>, dim3(nitems), dim3(kThreads), 0, stream,
                           pts, pairs, items, threshold, iterations, seed, slots);
    return hipGetLastError();
}

hipError_t launch_estimate_finish(const float4* pts, const sgeo::PairRec* pairs, int npairs,
                                  int model, float threshold, uint32_t seed,
                                  const unsigned long long* slots, float* models, int* inliers,
                                  uint8_t* mask, int* err, hipStream_t stream) {
    if (npairs <= 0) return hipSuccess;
    if (model == sgeo::kModelF)
        hipLaunchKernelGGL(k_estimate_finish<sgeo::kModelF>, dim3(npairs), dim3(kThreads), 0, stream,
                           pts, pairs, threshold, seed, slots, models, inliers, mask, err);
    else
        hipLaunchKernelGGL(k_estimate_finish<sgeo::kModelH>, dim3(npairs), dim3(kThreads), 0, stream,
                           pts, pairs, threshold, seed, slots, models, inliers, mask, err);
    return hipGetLastError();
}

}  // namespace sgk
