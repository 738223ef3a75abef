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
//   k_estimate_refine   (sgpu_estimate_*_refined, rounds > 0) a 64-lane workgroup per pair: the
//                       contract's round loop -- least-squares refit on the inliers, rescoring,
//                       acceptance -- inside one launch, whatever the number of rounds.
// The verify chain (sgpu_verify_batch) feeds these from the matcher's device
// output: k_verify_pair_recs, k_verify_gather, k_estimate_pairs<MODEL, true> and
// k_verify_guided_params, at the end of this file's kernels.
#include "sift_kernels.h"
#include "sift_geom.h"

namespace sgk {
namespace {

constexpr int kThreads = sgeo::kBlockHyp;
static_assert(kThreads == 256 && sgeo::kMatchTile % kThreads == 0, "a lane per hypothesis");

// match k of the concatenated list -> its float4 row
__device__ __forceinline__ void gather_row(const float* __restrict__ loc, int loc_stride,
                                           const sgeo::PairRec* __restrict__ pairs, int npairs,
                                           const int* __restrict__ matches, long long k,
                                           float4* __restrict__ pts) {
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

__global__ __launch_bounds__(256) void k_estimate_gather(const float* __restrict__ loc,
                                                         int loc_stride,
                                                         const sgeo::PairRec* __restrict__ pairs,
                                                         int npairs,
                                                         const int* __restrict__ matches,
                                                         long long total,
                                                         float4* __restrict__ pts) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= total) return;
    gather_row(loc, loc_stride, pairs, npairs, matches, k, pts);
}

// GUARD (the verify chain, whose items the host makes for every pair): a work item of a pair
// below the minimal sample ends here, the whole workgroup at once (pr is the workgroup's), before
// any barrier and before sample() could draw from fewer than S matches; its slot stays 0.
template <int MODEL, bool GUARD = false>
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
    if (GUARD && pr.m < (MODEL == sgeo::kModelF ? 8 : 4)) return;
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

// a sum over the wave's 64 lanes, in every lane: lane l < stride gets v[l] + v[l + stride], as
// sgeo::fold_lanes adds (the other lanes add the same two values the other way round)
__device__ inline double fold_wave(double v) {
#pragma unroll
    for (int d = sgeo::kRefineLanes / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ inline int sum_wave(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// Local refinement (sift_geom.h, "local refinement"): one wave per pair runs the whole round loop.
// Lane l takes the pair's rows l, l + 64, ..: the partial sums of the contract.  The normal matrix
// and the eigenvectors live in LDS, row k the work of lane k < 9, so that the Jacobi rotations
// index them at run time without a per-lane array; everything else is wave-uniform registers.
// __syncthreads() in a one-wave workgroup is an LDS fence, no hardware barrier.
template <int MODEL>
__global__ __launch_bounds__(64) void k_estimate_refine(const float4* __restrict__ pts,
                                                        const sgeo::PairRec* __restrict__ pairs,
                                                        float threshold, int rounds,
                                                        float* __restrict__ models,
                                                        int* __restrict__ inliers,
                                                        uint8_t* __restrict__ mask,
                                                        int* __restrict__ out_rounds) {
    constexpr int S = MODEL == sgeo::kModelF ? 8 : 4;
    __shared__ double s_A[81], s_V[81];
    const int p = blockIdx.x, lane = threadIdx.x;
    const sgeo::PairRec pr = pairs[p];
    const float4* __restrict__ P = pts + pr.moff;
    const int m = pr.m;
    float M[9];
#pragma unroll
    for (int i = 0; i < 9; i++) M[i] = models[9 * (size_t)p + i];
    int c = inliers[p];
    int done = 0;
    for (int r = 0; r < rounds && c >= S; r++) {
        // the two centroids, then the two mean deviations, over the inliers of M
        double sum[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = lane; k < m; k += 64) {
            const float4 q = P[k];
            if (sgeo::inlier(MODEL, M, q.x, q.y, q.z, q.w, threshold)) {
                sum[0] += (double)q.x;
                sum[1] += (double)q.y;
                sum[2] += (double)q.z;
                sum[3] += (double)q.w;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; e++) sum[e] = fold_wave(sum[e]);
        sgeo::RefitNorm nm;
        sgeo::refit_centroids(sum, c, nm);
        double dev1 = 0.0, dev2 = 0.0;
        for (int k = lane; k < m; k += 64) {
            const float4 q = P[k];
            if (sgeo::inlier(MODEL, M, q.x, q.y, q.z, q.w, threshold)) {
                double t1, t2;
                sgeo::refit_deviation(nm, (double)q.x, (double)q.y, (double)q.z, (double)q.w, t1, t2);
                dev1 += t1;
                dev2 += t2;
            }
        }
        dev1 = fold_wave(dev1);
        dev2 = fold_wave(dev2);
        if (!sgeo::refit_scales(dev1, dev2, c, nm)) break;
        // the normal matrix
        double N[sgeo::kNormalEntries];
#pragma unroll
        for (int e = 0; e < sgeo::kNormalEntries; e++) N[e] = 0.0;
        for (int k = lane; k < m; k += 64) {
            const float4 q = P[k];
            if (sgeo::inlier(MODEL, M, q.x, q.y, q.z, q.w, threshold))
                sgeo::refit_accumulate<MODEL>(nm, (double)q.x, (double)q.y, (double)q.z, (double)q.w, N);
        }
#pragma unroll
        for (int e = 0; e < sgeo::kNormalEntries; e++) N[e] = fold_wave(N[e]);
        // every lane holds all of N: lane 0 spreads it over both triangles of A
        __syncthreads();   // (the reads of the round before are done)
        if (lane == 0) {
            int e = 0;
#pragma unroll
            for (int i = 0; i < 9; i++) {
#pragma unroll
                for (int j = i; j < 9; j++) {
                    s_A[9 * i + j] = N[e];
                    s_A[9 * j + i] = N[e];
                    e++;
                }
            }
        }
        for (int i = lane; i < 81; i += 64) s_V[i] = (i % 10 == 0) ? 1.0 : 0.0;
        __syncthreads();
        // cyclic Jacobi, sgeo::jacobi_sweep_host with its loop over k spread over lanes 0 .. 8
        const int k = lane < 9 ? lane : 8;
        for (int sweep = 0; sweep < sgeo::kJacobiSweeps; sweep++) {
            for (int jp = 0; jp < 8; jp++) {
                for (int jq = jp + 1; jq < 9; jq++) {
                    const double app = s_A[10 * jp], aqq = s_A[10 * jq], apq = s_A[9 * jp + jq];
                    const double akp = s_A[9 * k + jp], akq = s_A[9 * k + jq];
                    const double vkp = s_V[9 * k + jp], vkq = s_V[9 * k + jq];
                    __syncthreads();
                    if (apq != 0.0 && lane < 9) {
                        const sgeo::JacobiRot rot = sgeo::jacobi_rotation(app, aqq, apq);
                        double x, y;
                        sgeo::jacobi_apply(rot, vkp, vkq, x, y);
                        s_V[9 * k + jp] = x;
                        s_V[9 * k + jq] = y;
                        if (k == jp) {
                            s_A[10 * jp] = sgeo::jacobi_app(rot, app, apq);
                            s_A[9 * jp + jq] = 0.0;
                        } else if (k == jq) {
                            s_A[10 * jq] = sgeo::jacobi_aqq(rot, aqq, apq);
                            s_A[9 * jq + jp] = 0.0;
                        } else {
                            sgeo::jacobi_apply(rot, akp, akq, x, y);
                            s_A[9 * k + jp] = x;
                            s_A[9 * jp + k] = x;
                            s_A[9 * k + jq] = y;
                            s_A[9 * jq + k] = y;
                        }
                    }
                    __syncthreads();
                }
            }
        }
        const int col = sgeo::jacobi_min_index(s_A);
        double g[9], D[9];
#pragma unroll
        for (int i = 0; i < 9; i++) g[i] = s_V[9 * i + col];
        if (!sgeo::refit_denormalise<MODEL>(nm, g, D)) break;
        float M2[9];
#pragma unroll
        for (int i = 0; i < 9; i++) M2[i] = (float)D[i];
        // score M', and whether any match changed side
        int c2 = 0;
        bool changed = false;
        for (int kk = lane; kk < m; kk += 64) {
            const float4 q = P[kk];
            const bool a = sgeo::inlier(MODEL, M, q.x, q.y, q.z, q.w, threshold);
            const bool b = sgeo::inlier(MODEL, M2, q.x, q.y, q.z, q.w, threshold);
            c2 += b ? 1 : 0;
            changed |= a != b;
        }
        c2 = sum_wave(c2);
        if (c2 < c) break;
#pragma unroll
        for (int i = 0; i < 9; i++) M[i] = M2[i];
        c = c2;
        done++;
        if (__ballot(changed) == 0ull) break;
    }
    if (lane == 0) out_rounds[p] = done;
    if (done == 0) return;
    // accepted: the model, its count and its mask replace the winner's
    if (lane < 9) {
        float v = M[0];
#pragma unroll
        for (int i = 1; i < 9; i++) v = lane == i ? M[i] : v;
        models[9 * (size_t)p + lane] = v;
    }
    if (lane == 0) inliers[p] = c;
    if (mask)
        for (int k = lane; k < m; k += 64) {
            const float4 q = P[k];
            mask[pr.moff + k] = sgeo::inlier(MODEL, M, q.x, q.y, q.z, q.w, threshold) ? 1 : 0;
        }
}

// ---- the verify chain's glue: the matcher's device output -> the estimator's tables -> the
// guided matcher's matrices, nothing through the host

__global__ __launch_bounds__(256) void k_verify_pair_recs(const long long* __restrict__ offs,
                                                          const int* __restrict__ counts, int npairs,
                                                          sgeo::PairRec* __restrict__ recs) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npairs) return;
    recs[p].moff = offs[p];
    recs[p].m = counts[p];
}

// k_estimate_gather under a total that only the device knows: the grid covers the host's bound
__global__ __launch_bounds__(256) void k_verify_gather(const float* __restrict__ loc, int loc_stride,
                                                       const sgeo::PairRec* __restrict__ pairs,
                                                       int npairs, const int* __restrict__ matches,
                                                       const long long* __restrict__ total,
                                                       float4* __restrict__ pts) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= *total) return;
    gather_row(loc, loc_stride, pairs, npairs, matches, k, pts);
}

__global__ __launch_bounds__(256) void k_verify_guided_params(const float* __restrict__ H,
                                                              const float* __restrict__ F,
                                                              float hdistmax, float fdistmax,
                                                              int npairs,
                                                              GuidedParams* __restrict__ geom) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npairs) return;
    GuidedParams g;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const float id = i % 4 == 0 ? 1.f : 0.f;
        g.H[i] = H ? H[9 * (size_t)p + i] : id;
        g.F[i] = F ? F[9 * (size_t)p + i] : id;
    }
    g.hdistmax = H ? hdistmax : 1.0e+20f;
    g.fdistmax = F ? fdistmax : 1.0e+20f;
    geom[p] = g;
}

}  // namespace

hipError_t launch_verify_pair_recs(const long long* offs, const int* counts, int npairs,
                                   sgeo::PairRec* recs, hipStream_t stream) {
    if (npairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_verify_pair_recs, dim3((npairs + 255) / 256), dim3(256), 0, stream, offs,
                       counts, npairs, recs);
    return hipGetLastError();
}

hipError_t launch_verify_gather(const float* loc, int loc_stride, const sgeo::PairRec* pairs,
                                int npairs, const int* matches, const long long* total,
                                long long bound, float4* pts, hipStream_t stream) {
    if (bound <= 0 || npairs <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((bound + 255) / 256);
    hipLaunchKernelGGL(k_verify_gather, dim3(grid), dim3(256), 0, stream, loc, loc_stride, pairs,
                       npairs, matches, total, pts);
    return hipGetLastError();
}

hipError_t launch_verify_estimate_pairs(const float4* pts, const sgeo::PairRec* pairs,
                                        const sgeo::Item* items, int nitems, int model,
                                        float threshold, int iterations, uint32_t seed,
                                        unsigned long long* slots, hipStream_t stream) {
    if (nitems <= 0) return hipSuccess;
    if (model == sgeo::kModelF)
        hipLaunchKernelGGL((k_estimate_pairs<sgeo::kModelF, true>), dim3(nitems), dim3(kThreads), 0,
                           stream, pts, pairs, items, threshold, iterations, seed, slots);
    else
        hipLaunchKernelGGL((k_estimate_pairs<sgeo::kModelH, true>), dim3(nitems), dim3(kThreads), 0,
                           stream, pts, pairs, items, threshold, iterations, seed, slots);
    return hipGetLastError();
}

hipError_t launch_verify_guided_params(const float* H, const float* F, float hdistmax,
                                       float fdistmax, int npairs, GuidedParams* geom,
                                       hipStream_t stream) {
    if (npairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_verify_guided_params, dim3((npairs + 255) / 256), dim3(256), 0, stream, H,
                       F, hdistmax, fdistmax, npairs, geom);
    return hipGetLastError();
}

hipError_t launch_estimate_refine(const float4* pts, const sgeo::PairRec* pairs, int npairs,
                                  int model, float threshold, int rounds, float* models,
                                  int* inliers, uint8_t* mask, int* out_rounds, hipStream_t stream) {
    if (npairs <= 0 || rounds <= 0) return hipSuccess;
    if (model == sgeo::kModelF)
        hipLaunchKernelGGL(k_estimate_refine<sgeo::kModelF>, dim3(npairs), dim3(64), 0, stream, pts,
                           pairs, threshold, rounds, models, inliers, mask, out_rounds);
    else
        hipLaunchKernelGGL(k_estimate_refine<sgeo::kModelH>, dim3(npairs), dim3(64), 0, stream, pts,
                           pairs, threshold, rounds, models, inliers, mask, out_rounds);
    return hipGetLastError();
}

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
