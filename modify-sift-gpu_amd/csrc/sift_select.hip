// sift_select.hip -- preemptive matching's device steps (sgpu_select_top_scale_*, sgpu_prematch_*;
// DESIGN.md 4.18): the top rows of every set by scale (the rule of sift_select.h), the gather of
// those rows into compact buffers the grouped pair matcher runs over, and the rewrite of its
// matches from subset positions to the sets' own row indices.
//
// k_select_top_scale  one workgroup per set: a most-significant-byte-first radix select over
//                     order_key (four passes, a 256-bin LDS histogram each) finds the cut (T, quota)
//                     exactly; one ordered sweep (ballots within a wave, an LDS prefix over the
//                     waves, as k_pairs_write) writes the selected indices in ascending order.
//                     The histogram adds are integer adds, whose sum does not depend on their
//                     order; no winner is decided by an atomic, so the result is a pure function
//                     of the input.
// k_gather_rows       one workgroup per set, 8 lanes per 128-byte row, 16 bytes per lane.
// k_remap_matches     one workgroup per pair: {i, j} -> {index[sub_a + i], index[sub_b + j]}.
// No kernel waits on another workgroup; every loop is bounded by its set's (or pair's) size.
#include "sift_kernels.h"
#include "sift_select.h"

namespace sgk {
namespace {

constexpr int kSelThreads = 256, kSelWaves = kSelThreads / 64;

__device__ __forceinline__ uint32_t load_key(const float* __restrict__ scale, int stride, long long row) {
    return sgsel::order_key(__float_as_uint(scale[row * stride]));
}

// index[sub_off[s] + k] = the k-th selected row of set s (set-local, ascending), k < min(n_s, top)
__global__ __launch_bounds__(kSelThreads) void k_select_top_scale(const float* __restrict__ scale,
                                                                  int stride,
                                                                  const long long* __restrict__ set_off,
                                                                  const int* __restrict__ sub_off,
                                                                  int top, int* __restrict__ index) {
    __shared__ int s_hist[256];
    __shared__ int s_w[2][kSelWaves];
    __shared__ int s_bin, s_above;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long base = set_off[blockIdx.x];
    const int n = (int)(set_off[blockIdx.x + 1] - base);
    int* __restrict__ out = index + sub_off[blockIdx.x];
    if (n <= top) {   // the identity (nothing for an empty set)
        for (int i = tid; i < n; i += kSelThreads) out[i] = i;
        return;
    }
    // ---- the cut: T = the top-th largest key, quota = rows with key == T that are taken
    uint32_t prefix = 0, mask = 0;
    int want = top;   // the rank looked for among the rows that match the prefix (1 = largest)
    for (int shift = 24; shift >= 0; shift -= 8) {
        s_hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += kSelThreads) {
            const uint32_t k = load_key(scale, stride, base + i);
            if ((k & mask) == prefix) atomicAdd(&s_hist[(k >> shift) & 255], 1);
        }
        __syncthreads();
        // thread b: the rows in the bins above b (a suffix sum over the 256 bins)
        const int h = s_hist[tid];
        int incl = h;   // bins [tid, end of this wave's 64]
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_down(incl, o, 64);
            if (lane + o < 64) incl += u;
        }
        if (lane == 0) s_w[0][wave] = incl;
        __syncthreads();
        int above = incl - h;
#pragma unroll
        for (int w = 1; w < kSelWaves; w++) above += w > wave ? s_w[0][w] : 0;
        // exactly one bin holds the rank: above < want <= above + h
        if (above < want && want <= above + h) {
            s_bin = tid;
            s_above = above;
        }
        __syncthreads();
        prefix |= (uint32_t)s_bin << shift;
        mask |= 255u << shift;
        want -= s_above;
        __syncthreads();   // s_hist, s_w, s_bin are rewritten by the next pass
    }
    const sgsel::Cut cut{prefix, want};
    // ---- the ordered sweep: 256 rows per step
    int eq_done = 0, sel_done = 0;   // uniform: rows with key == T / selected rows before this step
    for (int i0 = 0; i0 < n; i0 += kSelThreads) {
        const int i = i0 + tid;
        const bool in = i < n;
        const uint32_t k = in ? load_key(scale, stride, base + i) : 0u;
        const bool eq = in && k == cut.T;
        const unsigned long long beq = __ballot(eq);
        if (lane == 0) s_w[0][wave] = __popcll(beq);
        __syncthreads();
        int eq_before = eq_done + __popcll(beq & ((1ull << lane) - 1)), eq_tot = 0;
#pragma unroll
        for (int w = 0; w < kSelWaves; w++) {
            const int c = s_w[0][w];
            eq_before += w < wave ? c : 0;
            eq_tot += c;
        }
        const bool sel = in && sgsel::takes(cut, k, eq_before);
        const unsigned long long bsel = __ballot(sel);
        if (lane == 0) s_w[1][wave] = __popcll(bsel);
        __syncthreads();
        int pos = sel_done + __popcll(bsel & ((1ull << lane) - 1)), sel_tot = 0;
#pragma unroll
        for (int w = 0; w < kSelWaves; w++) {
            const int c = s_w[1][w];
            pos += w < wave ? c : 0;
            sel_tot += c;
        }
        if (sel && pos < top) out[pos] = i;   // (pos < top by the rule: g + quota = top)
        eq_done += eq_tot;
        sel_done += sel_tot;
        __syncthreads();   // s_w is rewritten by the next step
    }
}

// dst row sub_off[s] + k = src row set_off[s] + index[sub_off[s] + k] (128 bytes each), and the
// same for the rows' int terms when both term pointers are set
__global__ __launch_bounds__(256) void k_gather_rows(const uint4* __restrict__ src,
                                                     const int* __restrict__ src_terms,
                                                     const long long* __restrict__ set_off,
                                                     const int* __restrict__ sub_off,
                                                     const int* __restrict__ index,
                                                     uint4* __restrict__ dst,
                                                     int* __restrict__ dst_terms) {
    const long long base = set_off[blockIdx.x];
    const int o = sub_off[blockIdx.x], m = sub_off[blockIdx.x + 1] - o;
    const int part = threadIdx.x & 7;
    for (int k = threadIdx.x >> 3; k < m; k += 32) {
        const long long row = base + index[o + k];
        dst[(size_t)(o + k) * 8 + part] = src[(size_t)row * 8 + part];
        if (src_terms && part == 0) dst_terms[o + k] = src_terms[row];
    }
}

// pair p's matches out[offs[p] .. offs[p] + counts[p]) from subset positions to set rows; a pair
// that k_pairs_write did not write (it does not fit below cap as a whole) is left alone
__global__ __launch_bounds__(256) void k_remap_matches(const int* __restrict__ counts,
                                                       const long long* __restrict__ offs,
                                                       const int2* __restrict__ pair_sub,
                                                       const int* __restrict__ index,
                                                       long long cap, int* __restrict__ out) {
    const int cnt = counts[blockIdx.x];
    const long long base = offs[blockIdx.x];
    if (cnt <= 0 || base + cnt > cap) return;
    const int2 sub = pair_sub[blockIdx.x];
    int2* __restrict__ m = reinterpret_cast<int2*>(out) + base;
    for (int k = threadIdx.x; k < cnt; k += 256) {
        const int2 v = m[k];
        m[k] = make_int2(index[sub.x + v.x], index[sub.y + v.y]);
    }
}

}  // namespace

hipError_t launch_select_top_scale(const float* scale, int stride, const long long* set_off,
                                   const int* sub_off, int nsets, int top, int* index,
                                   hipStream_t stream) {
    if (nsets <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_select_top_scale, dim3(nsets), dim3(kSelThreads), 0, stream, scale, stride,
                       set_off, sub_off, top, index);
    return hipGetLastError();
}

hipError_t launch_gather_rows(const uint8_t* src, const int* src_terms, const long long* set_off,
                              const int* sub_off, const int* index, int nsets, uint8_t* dst,
                              int* dst_terms, hipStream_t stream) {
    if (nsets <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_gather_rows, dim3(nsets), dim3(256), 0, stream,
                       reinterpret_cast<const uint4*>(src), dst_terms ? src_terms : nullptr, set_off,
                       sub_off, index, reinterpret_cast<uint4*>(dst), dst_terms);
    return hipGetLastError();
}

hipError_t launch_remap_matches(const int* counts, const long long* offs, const int* pair_sub,
                                const int* index, int npairs, long long cap, int* out,
                                hipStream_t stream) {
    if (npairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_remap_matches, dim3(npairs), dim3(256), 0, stream, counts, offs,
                       reinterpret_cast<const int2*>(pair_sub), index, cap, out);
    return hipGetLastError();
}

}  // namespace sgk
