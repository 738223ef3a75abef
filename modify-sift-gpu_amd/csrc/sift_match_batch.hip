// sift_match_batch.hip -- the grouped pair matcher (sgpu_match_batch / sgpu_match_images) and the
// device quantiser of float descriptors.
//
// One call matches a list of set pairs of one descriptor buffer.  The host plans work items
// (sift_match_plan.h): item = (pair, direction, 128-row panel of A, column chunk of B).
// k_match_pairs runs one workgroup per item: it keeps the panel as i8 MFMA fragments, streams its
// columns of B through LDS in 128-column tiles and folds every 16x16 accumulator tile into
// per-row running (max, argmax, second) state -- the keyed fold of k_match_rows (sift_match.hip),
// re-implemented here so that the tuned single-pair kernels stay as they are.
// k_match_pairs_finish merges the chunks of every (side, panel), adds the row term and applies the
// distance / ratio test; k_pairs_count, k_pairs_scan and k_pairs_write do the mutual check and the
// ordered compaction.  The number of launches does not depend on the number of pairs.
//
// Exactness (as k_match_rows): u8 descriptors are mapped to s8 by s = u - 128 (xor 0x80) so the
// signed i8 MFMA (v_mfma_i32_16x16x64_i8) applies; dot(u1, u2) = dot(s1, s2) + 128*sum(u1) +
// 128*sum(u2) - 2^21, all in int32.  The column term enters the key, the row term is added once
// per row in the finish.  Every value is folded as the key ((acc + column term) << 7) | low, whose
// 7 low bits order equal dots as the reference does (direction 0: lowest column mod 32, then
// lowest, RowMatch_Kernel; direction 1: lowest column, i.e. ColMatch_Kernel's lowest row of set
// 1), so the results are exact for every ratiomax.
//
// Set boundaries: the sets lie back to back in one buffer, so the bytes after set B's last row are
// the next set's.  A column past the item's chunk is never computed from loaded bytes: its staged
// bytes are zero and its column term is kNegCol (it can neither win nor raise a second maximum);
// the staging load itself is clamped to the set's last row, so no load leaves the set either.
#include <algorithm>
#include <type_traits>

#include "sift_kernels.h"
#include "sift_match_plan.h"

namespace sgk {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int kPanel = 128;      // A rows per workgroup (4 waves x 32)
constexpr int kTile = 128;       // B columns per LDS tile
constexpr int kLdsRow = 144;     // bytes per staged B row (padding against bank conflicts)
static_assert(kPanel == sgplan::kPanelRows && kTile == sgplan::kTileCols, "the planner's geometry");
// Running maxima hold keys (acc << 7) | low, acc = dot - row term in [-2^23 - 2^22, 2^23]: every
// key fits in int32 and INT_MIN is below all of them.
constexpr int kNeg = INT_MIN;
// Column term of a missing column: its acc stays <= 0 (a staged zero column adds nothing), so with
// the row term >= 0 added in the finish it can neither win nor raise a second maximum, and
// (acc << 7) does not overflow.
constexpr int kNegCol = -(1 << 22);

// the median of three as min / max, which LLVM selects as one v_med3_i32 (compiler-visible, so
// the hazard recognizer sees the MFMA result it reads): with s <= m, med3(s, m, v) is the new
// second maximum after seeing v
__device__ __forceinline__ int med3i(int a, int b, int c) {
    return max(min(a, b), min(max(a, b), c));
}

// Equal-dot order of the two directions: does column a come before column b (-1 = none)?
__device__ __forceinline__ bool tie_before(bool tie32, int a, int b) {
    if (a < 0) return false;
    if (b < 0) return true;
    if (tie32 && (a & 31) != (b & 31)) return (a & 31) < (b & 31);
    return a < b;
}

// float descriptors [n][128] -> u8 (the host rule of sgpu_quantize_descriptors:
// (uint8_t)(int)(512 * d + 0.5), the product in float -- exact, a power of two -- and the add in
// double; a float add rounds (0.5 - 2^-25) + 0.5 up to 1), and in the same pass what the matcher
// needs of a set: the s8 form (xor 0x80) and the row sums 128 * sum(u8).  A thread per 16 output
// bytes, a descriptor per 8 consecutive lanes (the grid stride keeps the groups whole).  Any of
// the three outputs may be null.
__global__ __launch_bounds__(256) void k_quantize_desc(const float4* __restrict__ src, size_t n16,
                                                       uint4* __restrict__ u8, uint4* __restrict__ s8,
                                                       int* __restrict__ sums) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride) {
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float4 f = src[i * 4 + q];
            const float e[4] = {f.x, f.y, f.z, f.w};
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int b = (int)((double)(512.0f * e[k]) + 0.5);
                v |= ((uint32_t)b & 0xffu) << (8 * k);
            }
            w[q] = v;
        }
        int t = __builtin_amdgcn_udot4(w[0], 0x01010101u, 0, false);
        t = __builtin_amdgcn_udot4(w[1], 0x01010101u, t, false);
        t = __builtin_amdgcn_udot4(w[2], 0x01010101u, t, false);
        t = __builtin_amdgcn_udot4(w[3], 0x01010101u, t, false);
        if (u8) u8[i] = make_uint4(w[0], w[1], w[2], w[3]);
        if (s8)
            s8[i] = make_uint4(w[0] ^ 0x80808080u, w[1] ^ 0x80808080u, w[2] ^ 0x80808080u,
                               w[3] ^ 0x80808080u);
        t += __shfl_xor(t, 1, 64);
        t += __shfl_xor(t, 2, 64);
        t += __shfl_xor(t, 4, 64);
        if (sums && (i & 7) == 0) sums[i >> 3] = 128 * t;
    }
}

// One work item: a 128-row panel of set A against columns [c_begin, c_end) of set B, both sets of
// the s8 buffer S.  part[part_base + row] = the running top-2 of the row over those columns (dot
// without the row term).  Fragment layout, staging, keys and the tile bookkeeping are
// k_match_rows's plain keyed path; the tie order is the item's (tie32 = direction 0).
__global__ __launch_bounds__(256) void k_match_pairs(const uint8_t* __restrict__ S,
                                                     const sgplan::Item* __restrict__ items,
                                                     Top2* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) uint8_t s_b[2][kTile * kLdsRow];
    __shared__ int s_ct[2][kTile];   // column terms of the staged tile (from its bytes)
    const sgplan::Item it = items[blockIdx.x];
    const uint8_t* __restrict__ A = S + (size_t)it.a_off * 128;
    const uint8_t* __restrict__ B = S + (size_t)it.b_off * 128;
    const int nA = it.a_n, nB = it.b_n, panel = it.panel;
    const int c_begin = it.c_begin, c_end = min(it.c_end, nB);
    const bool tie32 = it.dir == 0;
    if (nA <= 0 || c_begin >= c_end) return;   // (the planner emits no such item)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int quad = lane >> 4, l16 = lane & 15;

    // A fragments: rows wave*32 + rb*16 + l16, bytes kh*64 + quad*16 .. +16
    v4i afrag[2][2];
#pragma unroll
    for (int rb = 0; rb < 2; rb++) {
        const int row = panel * kPanel + wave * 32 + rb * 16 + l16;
#pragma unroll
        for (int kh = 0; kh < 2; kh++) {
            if (row < nA)
                afrag[rb][kh] = *reinterpret_cast<const v4i*>(A + (size_t)row * 128 + kh * 64 + quad * 16);
            else
                afrag[rb][kh] = v4i{0, 0, 0, 0};
        }
    }
    // running state for this lane's 8 output rows: (rb, i) -> row wave*32 + rb*16 + quad*4 + i:
    // max key, second key, tile of the winner and the winner's key when it was taken
    int M[2][4], S2[2][4], I[2][4], W[2][4];
#pragma unroll
    for (int rb = 0; rb < 2; rb++)
#pragma unroll
        for (int i = 0; i < 4; i++) { M[rb][i] = kNeg; S2[rb][i] = kNeg; I[rb][i] = -1; W[rb][i] = 0; }
    const uint32_t prefix = tie32 ? 4u : 128u;   // keys differing below this bit tie

    // staging: thread t copies 64 bytes: column t>>1, half (t&1).  The loads are unconditional
    // and clamped to the set's last row (never the next set's bytes, never past the buffer);
    // stage_store zeroes the columns past the chunk.
    auto stage_load = [&](int tbase, uint4* r) {
        const int col = min(tbase + (tid >> 1), nB - 1);
        const uint8_t* src = B + (size_t)col * 128 + (tid & 1) * 64;
#pragma unroll
        for (int q = 0; q < 4; q++) r[q] = reinterpret_cast<const uint4*>(src)[q];
    };
    // the column term 128 * sum(u8 B[col]) - 2^21 from the staged s8 bytes (sum(u) = sum(s) +
    // 128 * 128; v_dot4_i32_i8, the two half-columns joined by one shuffle)
    auto stage_store = [&](int buf, const uint4* r, int tbase) {
        uint8_t* dst = &s_b[buf][(tid >> 1) * kLdsRow + (tid & 1) * 64];
        const bool in_chunk = tbase + (tid >> 1) < c_end;
        int sum = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint4 v = in_chunk ? r[q] : make_uint4(0, 0, 0, 0);
            sum = __builtin_amdgcn_sdot4((int)v.x, 0x01010101, sum, false);
            sum = __builtin_amdgcn_sdot4((int)v.y, 0x01010101, sum, false);
            sum = __builtin_amdgcn_sdot4((int)v.z, 0x01010101, sum, false);
            sum = __builtin_amdgcn_sdot4((int)v.w, 0x01010101, sum, false);
            reinterpret_cast<uint4*>(dst)[q] = v;
        }
        sum += __shfl_xor(sum, 1, 64);
        if (!(tid & 1)) s_ct[buf][tid >> 1] = in_chunk ? 128 * (sum + 16384) - 2097152 : kNegCol;
    };

    // the key's low 7 bits per column block: a larger value = an earlier column in the
    // direction's tie order (tie32: (31 - col % 32) << 2 | (3 - col / 32 in the tile); else
    // 127 - col in the tile)
    int low[8];
#pragma unroll
    for (int cb = 0; cb < 8; cb++)
        low[cb] = tie32 ? ((31 - ((cb & 1) * 16 + l16)) << 2) | (3 - (cb >> 1))
                        : 127 - (cb * 16 + l16);

    // tile j is computed from LDS buffer j & 1; tile j + 1 is loaded and stored within tile j
    uint4 stg[4];
    stage_load(c_begin, stg);
    stage_store(0, stg, c_begin);
    __syncthreads();
    auto tile = [&](auto par, int tb) {
        constexpr int buf = decltype(par)::value;
        const bool has_next = tb + kTile < c_end;
        stage_load(tb + kTile, stg);
        int mt[2][4], st[2][4];
#pragma unroll
        for (int rb = 0; rb < 2; rb++)
#pragma unroll
            for (int i = 0; i < 4; i++) { mt[rb][i] = M[rb][i]; st[rb][i] = S2[rb][i]; }
        // the accumulators start at 0 and the column term enters the key,
        // key = (acc << 7) + ((ct << 7) | low) = ((acc + ct) << 7) | low
        v4i acc[2][8];
        int ctlow[8];
#pragma unroll
        for (int cb = 0; cb < 8; cb++) {
            ctlow[cb] = (s_ct[buf][cb * 16 + l16] << 7) | low[cb];
            acc[0][cb] = v4i{0, 0, 0, 0};
            acc[1][cb] = acc[0][cb];
        }
        const uint8_t* sb = s_b[buf];
#pragma unroll
        for (int cb = 0; cb < 8; cb++) {
#pragma unroll
            for (int kh = 0; kh < 2; kh++) {
                const v4i bfrag = *reinterpret_cast<const v4i*>(
                    sb + (cb * 16 + l16) * kLdsRow + kh * 64 + quad * 16);
                acc[0][cb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(afrag[0][kh], bfrag, acc[0][cb], 0, 0, 0);
                acc[1][cb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(afrag[1][kh], bfrag, acc[1][cb], 0, 0, 0);
            }
        }
        // epilogue: fold the 2x8 tiles into the running top-2 (C layout: col = l16, row =
        // quad*4 + i within the 16-row block): one v_lshl_add, one v_max and one v_med3 per
        // value.  Column blocks 0..3 of every row first (their MFMAs finished earliest), then
        // 4..7: each row still folds its keys in column order.
#pragma unroll
        for (int half = 0; half < 2; half++)
#pragma unroll
            for (int rb = 0; rb < 2; rb++)
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int cb = 4 * half; cb < 4 * half + 4; cb++) {
                        const int key = (acc[rb][cb][i] << 7) + ctlow[cb];
                        st[rb][i] = med3i(st[rb][i], mt[rb][i], key);
                        mt[rb][i] = max(mt[rb][i], key);
                    }
        // a later tile takes over only when the key's tie-relevant prefix grows (the dot; tie32:
        // the dot and col % 32); the key is recorded with its tile at that moment
#pragma unroll
        for (int rb = 0; rb < 2; rb++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int m = mt[rb][i];
                const bool took = (uint32_t)(m ^ M[rb][i]) >= prefix;
                I[rb][i] = took ? tb : I[rb][i];
                W[rb][i] = took ? m : W[rb][i];
                M[rb][i] = m;
                S2[rb][i] = st[rb][i];
            }
        // one barrier per tile: the stores below go to the buffer of tile t - 1, which every wave
        // finished reading before the barrier that ended iteration t - 1
        if (has_next) stage_store(buf ^ 1, stg, tb + kTile);
        __syncthreads();
    };
    for (int tb = c_begin; tb < c_end; tb += 2 * kTile) {
        tile(std::integral_constant<int, 0>{}, tb);
        if (tb + kTile < c_end) tile(std::integral_constant<int, 1>{}, tb + kTile);
    }
    // keys -> (acc + column term, column)
#pragma unroll
    for (int rb = 0; rb < 2; rb++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int k = W[rb][i] & 127;
            const int in_tile = tie32 ? (3 - (k & 3)) * 32 + (31 - (k >> 2)) : 127 - k;
            I[rb][i] = I[rb][i] < 0 ? -1 : I[rb][i] + in_tile;
            M[rb][i] >>= 7;
            S2[rb][i] >>= 7;
        }
    // merge the 16 lanes that share a row (same quad): xor 1, 2, 4, 8; equal dots resolve in the
    // direction's tie order
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
#pragma unroll
        for (int rb = 0; rb < 2; rb++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int m2 = __shfl_xor(M[rb][i], off, 64);
                const int s2 = __shfl_xor(S2[rb][i], off, 64);
                const int i2 = __shfl_xor(I[rb][i], off, 64);
                const int m1 = M[rb][i], s1 = S2[rb][i], i1 = I[rb][i];
                M[rb][i] = max(m1, m2);
                S2[rb][i] = max(min(m1, m2), max(s1, s2));
                I[rb][i] = (m2 > m1 || (m2 == m1 && tie_before(tie32, i2, i1))) ? i2 : i1;
            }
    }
    if (l16 == 0) {
#pragma unroll
        for (int rb = 0; rb < 2; rb++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int row = panel * kPanel + wave * 32 + rb * 16 + quad * 4 + i;
                if (row < nA) part[(size_t)it.part_base + row] = Top2{M[rb][i], I[rb][i], S2[rb][i]};
            }
    }
}

// One workgroup per (side, panel), a thread per row: merge the side's column chunks (equal maxima
// in the direction's tie order; that choice is associative), add the row term 128 * sum(u8 row),
// clamp as the reference's running state from (0, -1, 0) and apply the distance / ratio test
// (RowMatch_Kernel / ColMatch_Kernel decision, as k_match_finish): dec[dec_off + row] = the
// matched column or -1.
__global__ __launch_bounds__(kPanel) void k_match_pairs_finish(const Top2* __restrict__ part,
                                                               const sgplan::Side* __restrict__ sides,
                                                               const sgplan::FinishPanel* __restrict__ fpanels,
                                                               const int* __restrict__ sums,
                                                               const float* __restrict__ dist,
                                                               float distmax, float ratiomax,
                                                               int* __restrict__ dec) {
    const sgplan::FinishPanel fp = fpanels[blockIdx.x];
    const sgplan::Side sd = sides[fp.side];
    const int r = fp.panel * kPanel + threadIdx.x;
    if (r >= sd.a_n) return;
    const bool tie32 = sd.tie32 != 0;
    Top2 t{INT_MIN, -1, INT_MIN};
    for (int c = 0; c < sd.chunks; c++) {
        const Top2 u = part[(size_t)sd.part_off + (size_t)c * sd.a_n + r];
        const int s = max(min(t.max, u.max), max(t.second, u.second));
        const bool later = u.max > t.max || (u.max == t.max && tie_before(tie32, u.idx, t.idx));
        t = Top2{max(t.max, u.max), later ? u.idx : t.idx, s};
    }
    const int rt = sums[(size_t)sd.a_off + r];
    int mx = t.max + rt, sc = t.second + rt, idx = t.idx;
    if (mx <= 0) { mx = 0; idx = -1; }
    if (sc < 0) sc = 0;
    const float d1 = dist[min(mx, kDistTable - 1)], d2 = dist[min(sc, kDistTable - 1)];
    const bool ok = (d1 < distmax) && (d1 < d2 * ratiomax);
    dec[(size_t)sd.dec_off + r] = ok && idx >= 0 ? idx : -1;
}

// the pair's match test of row i (SiftMatchCU.cpp:166-176): its decision j, kept when the other
// direction decided i for j (mutual) -- j < n_b by construction (a column of the pair's set b)
__device__ __forceinline__ int pair_match(const int* __restrict__ dec, const sgplan::PairRec& pr, int i) {
    if (i >= pr.n_a) return -1;
    const int j = dec[(size_t)pr.dec0 + i];
    if (j < 0) return -1;
    return (pr.dec1 < 0 || dec[(size_t)pr.dec1 + j] == i) ? j : -1;
}

// counts[p] = min(matches of pair p, max_match); one workgroup per pair
__global__ __launch_bounds__(256) void k_pairs_count(const int* __restrict__ dec,
                                                     const sgplan::PairRec* __restrict__ pairs,
                                                     int max_match, int* __restrict__ counts) {
    __shared__ int s_w[4];
    const sgplan::PairRec pr = pairs[blockIdx.x];
    int c = 0;
    for (int i = threadIdx.x; i < pr.n_a; i += 256) c += pair_match(dec, pr, i) >= 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = min(s_w[0] + s_w[1] + s_w[2] + s_w[3], max(max_match, 0));
}

// offs[0 .. n] = exclusive scan of counts[0 .. n): one workgroup, a contiguous slice per thread
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void k_pairs_scan(const int* __restrict__ counts, int n,
                                                             long long* __restrict__ offs) {
    __shared__ long long s_sum[kScanThreads];
    const int per = (n + kScanThreads - 1) / kScanThreads;
    const int b = min(n, (int)threadIdx.x * per), e = min(n, b + per);
    long long t = 0;
    for (int i = b; i < e; i++) t += counts[i];
    s_sum[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int k = 0; k < kScanThreads; k++) {
            const long long v = s_sum[k];
            s_sum[k] = run;
            run += v;
        }
        offs[n] = run;
    }
    __syncthreads();
    long long run = s_sum[threadIdx.x];
    for (int i = b; i < e; i++) {
        offs[i] = run;
        run += counts[i];
    }
}

// Pair p's matches {i, j} in ascending i at out[offs[p] ..), the first counts[p] of them; a pair
// that does not fit below cap as a whole writes nothing.  One workgroup per pair: 256 rows per
// step, slots by ballot within a wave and an LDS prefix over the 4 waves.
__global__ __launch_bounds__(256) void k_pairs_write(const int* __restrict__ dec,
                                                     const sgplan::PairRec* __restrict__ pairs,
                                                     const int* __restrict__ counts,
                                                     const long long* __restrict__ offs,
                                                     long long cap, int* __restrict__ out) {
    __shared__ int s_w[4];
    const sgplan::PairRec pr = pairs[blockIdx.x];
    const int cnt = counts[blockIdx.x];
    const long long base = offs[blockIdx.x];
    if (cnt <= 0 || base + cnt > cap) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int done = 0;   // uniform: matches of the rows before this step
    for (int i0 = 0; i0 < pr.n_a && done < cnt; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const int j = pair_match(dec, pr, i);
        const unsigned long long bal = __ballot(j >= 0);
        if (lane == 0) s_w[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const int c = s_w[w];
            before += w < wave ? c : 0;
            tot += c;
        }
        const int pos = done + before + __popcll(bal & ((1ull << lane) - 1));
        if (j >= 0 && pos < cnt) {
            out[2 * (base + pos)] = i;
            out[2 * (base + pos) + 1] = j;
        }
        done += tot;
        __syncthreads();   // s_w is rewritten by the next step
    }
}

}  // namespace

hipError_t launch_quantize_desc(const float* d, size_t n, uint8_t* u8, uint8_t* s8, int* sums,
                                hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const size_t n16 = n * 8;   // 128 bytes = 8 uint4 per descriptor
    const unsigned grid = (unsigned)std::min<size_t>((n16 + 255) / 256, 8192);
    hipLaunchKernelGGL(k_quantize_desc, dim3(grid), dim3(256), 0, stream,
                       reinterpret_cast<const float4*>(d), n16, reinterpret_cast<uint4*>(u8),
                       reinterpret_cast<uint4*>(s8), sums);
    return hipGetLastError();
}

hipError_t launch_match_pairs(const uint8_t* s8, const sgplan::Item* items, int nitems, Top2* part,
                              hipStream_t stream) {
    if (nitems <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_match_pairs, dim3(nitems), dim3(256), 0, stream, s8, items, part);
    return hipGetLastError();
}

hipError_t launch_match_pairs_finish(const Top2* part, const sgplan::Side* sides,
                                     const sgplan::FinishPanel* fpanels, int nfpanels,
                                     const int* sums, const float* dist, float distmax,
                                     float ratiomax, int* dec, hipStream_t stream) {
    if (nfpanels <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_match_pairs_finish, dim3(nfpanels), dim3(kPanel), 0, stream, part, sides,
                       fpanels, sums, dist, distmax, ratiomax, dec);
    return hipGetLastError();
}

hipError_t launch_match_pairs_compact(const int* dec, const sgplan::PairRec* pairs, int npairs,
                                      int max_match, long long cap, int* counts, long long* offs,
                                      int* out, hipStream_t stream) {
    if (npairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pairs_count, dim3(npairs), dim3(256), 0, stream, dec, pairs, max_match, counts);
    hipLaunchKernelGGL(k_pairs_scan, dim3(1), dim3(kScanThreads), 0, stream, counts, npairs, offs);
    hipLaunchKernelGGL(k_pairs_write, dim3(npairs), dim3(256), 0, stream, dec, pairs, counts, offs,
                       cap, out);
    return hipGetLastError();
}

}  // namespace sgk
