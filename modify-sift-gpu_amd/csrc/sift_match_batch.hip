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
// 7 low bits order equal dots as the reference does (direction 0: lowest rank of the column mod 32
// (row_tie_rank), then lowest, RowMatch_Kernel; direction 1: lowest column, i.e. ColMatch_Kernel's lowest row of set
// 1), so the results are exact for every ratiomax.
//
// Set boundaries: the sets lie back to back in one buffer, so the bytes after set B's last row are
// the next set's.  A column past the item's chunk is never computed from loaded bytes: its staged
// bytes are zero and its column term is kNegCol (it can neither win nor raise a second maximum);
// the staging load itself is clamped to the set's last row, so no load leaves the set either.
//
// Guided form (sgpu_match_batch_guided / sgpu_match_images_guided): k_match_pairs_guided is the
// same work item with the geometric test of MultiplyDescriptorG_Kernel fused in.  Every tile the
// workgroup evaluates the test for its own 128 x 128 point pairs into an LDS bit matrix
// (guided_words, the booleans of oracle::guided_pass and k_guided_mask) under its pair's
// matrices geom[Item::pair], and the accumulators start at the column term minus the geometric
// bias, as k_match_rows<GUIDED> does -- no mask is stored in device memory.
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
// Guided form: a value's accumulator starts at the column term minus 2^18 * fail + 2^23 * !good
// (sift_match.hip, k_match_rows), so acc = dot - row term - bias with dot in [0, 128 * 255^2]
// (< 2^23), the row term in [0, 128 * 128 * 255] (< 2^22) and the bias in {0, 2^18, 2^23,
// 2^23 + 2^18}: acc lies in [-2^22 - 2^23 - 2^18, 2^23) = [-12845056, 8388608).  Every partial
// sum of the MFMA chain obeys the same bounds (|dot of s8 forms| <= 2^21, the column term in
// [-2^21, 2^21), a missing column's kNegCol with zero bytes), so |acc| < 2^24 and (acc << 7)
// plus the 7 tie bits fits int32 with INT_MIN still below every key.
constexpr int kBiasFail = 1 << 18, kBiasNoGood = 1 << 23;
constexpr int kPassPitch = 5;    // words per LDS bit row (4 + 1 against bank conflicts)

// the median of three as min / max, which LLVM selects as one v_med3_i32 (compiler-visible, so
// the hazard recognizer sees the MFMA result it reads): with s <= m, med3(s, m, v) is the new
// second maximum after seeing v
__device__ __forceinline__ int med3i(int a, int b, int c) {
    return max(min(a, b), min(max(a, b), c));
}

// RowMatch_Kernel's rank of a column among equal maxima, lower wins: the 5 bits of col % 32
// reversed (its tree reduction merges two threads at their lowest differing bit and keeps the
// one with that bit clear; k_match_rows, sift_match.hip).
__device__ __forceinline__ int row_tie_rank(int col) { return (int)(__brev((unsigned)col) >> 27); }

// Equal-dot order of the two directions: does column a come before column b (-1 = none)?
__device__ __forceinline__ bool tie_before(bool tie32, int a, int b) {
    if (a < 0) return false;
    if (b < 0) return true;
    if (tie32 && (a & 31) != (b & 31)) return row_tie_rank(a) < row_tie_rank(b);
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

// The geometric test of one set-1 point (x1, y1) -- this thread's -- against 64 points of set 2,
// shared by both directions: bit k of w[q] = the pair passes with set-2 point base2 + q * 32 + k
// (MultiplyDescriptorG_Kernel, ProgramCU.cu:1648-1681, in the operation order of
// oracle::guided_pass and k_guided_mask: explicit fmaf's, a * (1 / b) for the divisions, the
// Sampson error only where the homography test passed; |a - b| = |b - a| exactly).  Direction 0:
// set 1 = the panel's rows, set 2 = the tile's columns; direction 1 (A = set b): set 1 = the
// tile's columns, set 2 = the panel's rows.  set2 = the locations of set 2 (its row 0), n2 its
// size and lim2 the first point that takes no part (the chunk's or the set's end): a load past
// the set is clamped to its last point and its bit is cleared.  base2 is uniform over the wave,
// so the set-2 loads are scalar loads (one per point and wave, none through LDS).
__device__ __forceinline__ void guided_words(const GuidedParams& gp, float x1, float y1, bool valid1,
                                             const float* __restrict__ set2, int loc_stride,
                                             int n2, int lim2, int base2, uint32_t w[2]) {
    const float* H = gp.H;
    const float* F = gp.F;
    const float h0 = __builtin_fmaf(H[0], x1, __builtin_fmaf(H[1], y1, H[2]));
    const float h1 = __builtin_fmaf(H[3], x1, __builtin_fmaf(H[4], y1, H[5]));
    const float h2 = __builtin_fmaf(H[6], x1, __builtin_fmaf(H[7], y1, H[8]));
    const float rh = 1.0f / h2;
    const float u = h0 * rh, v = h1 * rh;
    auto point2 = [&](int j) {
        return *reinterpret_cast<const float2*>(set2 + (size_t)min(j, n2 - 1) * loc_stride);
    };
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int j0 = base2 + q * 32;
        uint32_t bits = 0;
        // branch-free: a short-circuit '&&' compiles to a branch per pair.  All 64 points
        // unrolled: their scalar loads are issued together (some scalar registers spill to
        // lanes); batches of 16 points spill none but expose each batch's load latency and
        // measured 16 % slower on the shard's pairs.
#pragma unroll
        for (int k = 0; k < 32; k++) {
            const float2 p2 = point2(j0 + k);
            const bool ok = (__builtin_fabsf(u - p2.x) < gp.hdistmax) &
                            (__builtin_fabsf(v - p2.y) < gp.hdistmax);
            bits |= (uint32_t)ok << k;
        }
        const int nvalid = min(max(lim2 - j0, 0), 32);
        w[q] = valid1 ? bits & (nvalid == 32 ? 0xffffffffu : ((1u << nvalid) - 1u)) : 0u;
    }
    if (w[0] | w[1]) {
        const float f0 = __builtin_fmaf(F[0], x1, __builtin_fmaf(F[1], y1, F[2]));
        const float f1 = __builtin_fmaf(F[3], x1, __builtin_fmaf(F[4], y1, F[5]));
        const float f2 = __builtin_fmaf(F[6], x1, __builtin_fmaf(F[7], y1, F[8]));
        const float d0 = __builtin_fmaf(f1, f1, f0 * f0);
#pragma unroll
        for (int q = 0; q < 2; q++) {
            for (uint32_t rest = w[q]; rest; rest &= rest - 1) {
                const int jj = __builtin_ctz(rest);
                const float2 p2 = point2(base2 + q * 32 + jj);
                const float t0 = __builtin_fmaf(F[0], p2.x, __builtin_fmaf(F[3], p2.y, F[6]));
                const float t1 = __builtin_fmaf(F[1], p2.x, __builtin_fmaf(F[4], p2.y, F[7]));
                const float x2fx1 = __builtin_fmaf(p2.x, f0, __builtin_fmaf(p2.y, f1, f2));
                const float den = __builtin_fmaf(t1, t1, __builtin_fmaf(t0, t0, d0));
                const float se = (x2fx1 * x2fx1) * (1.0f / den);
                if (!(se < gp.fdistmax)) w[q] &= ~(1u << jj);
            }
        }
    }
}

// One work item: a 128-row panel of set A against columns [c_begin, c_end) of set B, both sets of
// the s8 buffer S.  part[part_base + row] = the running top-2 of the row over those columns (dot
// without the row term).  Fragment layout, staging, keys and the tile bookkeeping are
// k_match_rows's plain keyed path; the tie order is the item's (tie32 = direction 0).
//
// GUIDED: loc = the sets' locations (x, y of row r at loc[r * loc_stride]), geom = the pairs'
// matrices and thresholds, s_pass / s_good = the tile's bit matrices (see guided_words).
template <bool GUIDED>
__device__ __forceinline__ void match_pairs_item(const uint8_t* __restrict__ S,
                                                 const sgplan::Item* __restrict__ items,
                                                 Top2* __restrict__ part,
                                                 const float* __restrict__ loc, int loc_stride,
                                                 const GuidedParams* __restrict__ geom,
                                                 uint32_t* s_pass, uint32_t* s_good) {
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

    // guided: of the tile's 128 x 128 point pairs, thread t tests set-1 point t & 127 against the
    // 64 set-2 points of half t >> 7 (uniform over a wave).  Direction 0: set 1 = the panel's rows
    // (one location per thread and item); direction 1: set 1 = the tile's columns (the next
    // tile's location is loaded with its bytes, clamped to the set like them).
    const int p1 = tid & 127;
    const int half2 = GUIDED ? __builtin_amdgcn_readfirstlane(tid >> 7) * 64 : 0;
    const float* __restrict__ locA = GUIDED ? loc + (size_t)it.a_off * loc_stride : nullptr;
    const float* __restrict__ locB = GUIDED ? loc + (size_t)it.b_off * loc_stride : nullptr;
    const GuidedParams* __restrict__ gp = GUIDED ? geom + it.pair : nullptr;
    float2 l1row = make_float2(0.f, 0.f), l1next = l1row;
    if constexpr (GUIDED) {
        if (tie32)
            l1row = *reinterpret_cast<const float2*>(locA + (size_t)min(panel * kPanel + p1, nA - 1) * loc_stride);
    }

    // staging: thread t copies 64 bytes: column t>>1, half (t&1).  The loads are unconditional
    // and clamped to the set's last row (never the next set's bytes, never past the buffer);
    // stage_store zeroes the columns past the chunk.
    auto stage_load = [&](int tbase, uint4* r) {
        const int col = min(tbase + (tid >> 1), nB - 1);
        const uint8_t* src = B + (size_t)col * 128 + (tid & 1) * 64;
#pragma unroll
        for (int q = 0; q < 4; q++) r[q] = reinterpret_cast<const uint4*>(src)[q];
        if constexpr (GUIDED) {
            if (!tie32)
                l1next = *reinterpret_cast<const float2*>(locB + (size_t)min(tbase + p1, nB - 1) * loc_stride);
        }
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
    // direction's tie order (tie32: (31 - rank of col % 32) << 2 | (3 - col / 32 in the tile);
    // else 127 - col in the tile)
    int low[8];
#pragma unroll
    for (int cb = 0; cb < 8; cb++)
        low[cb] = tie32 ? ((31 - row_tie_rank((cb & 1) * 16 + l16)) << 2) | (3 - (cb >> 1))
                        : 127 - (cb * 16 + l16);

    // tile j is computed from LDS buffer j & 1; tile j + 1 is loaded and stored within tile j
    uint4 stg[4];
    stage_load(c_begin, stg);
    stage_store(0, stg, c_begin);
    __syncthreads();
    auto tile = [&](auto par, int tb) {
        constexpr int buf = decltype(par)::value;
        const bool has_next = tb + kTile < c_end;
        const float2 l1 = tie32 ? l1row : l1next;   // (guided: this tile's set-1 location)
        stage_load(tb + kTile, stg);
        // guided: this tile's geometric test.  s_pass[set-1 point][word of set-2 points] as
        // k_guided_mask's; s_good[8-point block of set 1][word] = some point of the block
        // passes (good_count > 0: the blocks count from the set's first row -- panels, chunks and
        // tiles all start at multiples of 128 -- and a set-1 point past the set does not pass).
        // rec = this lane's 16-byte record of k_match_rows<GUIDED>: byte rb * 8 + cb covers rows
        // wave*32 + rb*16 + quad*4 + i and column cb*16 + l16; bit i = the pair fails, bit 4 + i =
        // no point of its set-1 block passes.  The writes of the next tile wait for this tile's
        // closing barrier, so every read of this tile's bits is over by then.
        uint32_t rec[4] = {0, 0, 0, 0};
        if constexpr (GUIDED) {
            uint32_t w[2];
            guided_words(*gp, l1.x, l1.y, tie32 ? panel * kPanel + p1 < nA : tb + p1 < c_end,
                         tie32 ? locB : locA, loc_stride, tie32 ? nB : nA, tie32 ? c_end : nA,
                         (tie32 ? tb : panel * kPanel) + half2, w);
            s_pass[p1 * kPassPitch + (half2 >> 5)] = w[0];
            s_pass[p1 * kPassPitch + (half2 >> 5) + 1] = w[1];
            __syncthreads();
            if (tid < 64) {
                const int blk = tid >> 2, wd = tid & 3;
                uint32_t g = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) g |= s_pass[(blk * 8 + k) * kPassPitch + wd];
                s_good[blk * kPassPitch + wd] = g;
            }
            __syncthreads();
            if (tie32) {
                // set 1 = the rows, set 2 = the columns
#pragma unroll
                for (int rb = 0; rb < 2; rb++) {
                    const int row0 = wave * 32 + rb * 16 + quad * 4;
#pragma unroll
                    for (int cb = 0; cb < 8; cb++) {
                        const int col = cb * 16 + l16, wd = col >> 5, bit = col & 31;
                        uint32_t byte = ((s_good[(row0 >> 3) * kPassPitch + wd] >> bit) & 1u) ? 0u : 0xf0u;
#pragma unroll
                        for (int i = 0; i < 4; i++)
                            byte |= (((s_pass[(row0 + i) * kPassPitch + wd] >> bit) & 1u) ^ 1u) << i;
                        rec[rb * 2 + (cb >> 2)] |= byte << ((cb & 3) * 8);
                    }
                }
            } else {
                // set 1 = the columns, set 2 = the rows (word `wave` holds this wave's 32 rows)
#pragma unroll
                for (int cb = 0; cb < 8; cb++) {
                    const int c = cb * 16 + l16;
                    const uint32_t pw = s_pass[c * kPassPitch + wave];
                    const uint32_t gw = s_good[(c >> 3) * kPassPitch + wave];
#pragma unroll
                    for (int rb = 0; rb < 2; rb++) {
                        const int sh = rb * 16 + quad * 4;
                        const uint32_t byte = (~(pw >> sh) & 0xfu) | ((~(gw >> sh) & 0xfu) << 4);
                        rec[rb * 2 + (cb >> 2)] |= byte << ((cb & 3) * 8);
                    }
                }
            }
        }
        int mt[2][4], st[2][4];
#pragma unroll
        for (int rb = 0; rb < 2; rb++)
#pragma unroll
            for (int i = 0; i < 4; i++) { mt[rb][i] = M[rb][i]; st[rb][i] = S2[rb][i]; }
        // the accumulators start at 0 and the column term enters the key,
        // key = (acc << 7) + ((ct << 7) | low) = ((acc + ct) << 7) | low;
        // guided: they start at the column term minus the geometric bias and the key adds only
        // the tie bits (the range of acc: kBiasFail above)
        v4i acc[2][8];
        int ctlow[8];
#pragma unroll
        for (int cb = 0; cb < 8; cb++) {
            if constexpr (!GUIDED) {
                ctlow[cb] = (s_ct[buf][cb * 16 + l16] << 7) | low[cb];
                acc[0][cb] = v4i{0, 0, 0, 0};
                acc[1][cb] = acc[0][cb];
            } else {
                const int ct = s_ct[buf][cb * 16 + l16];
                ctlow[cb] = low[cb];
#pragma unroll
                for (int rb = 0; rb < 2; rb++) {
                    const int mb = (int)(rec[rb * 2 + (cb >> 2)] >> ((cb & 3) * 8));
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        acc[rb][cb][i] = ct - ((mb >> i) & 1) * kBiasFail - ((mb >> (4 + i)) & 1) * kBiasNoGood;
                }
            }
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
        // the dot and the rank of col % 32); the key is recorded with its tile at that moment
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
            const int in_tile = tie32 ? (3 - (k & 3)) * 32 + row_tie_rank(31 - (k >> 2)) : 127 - k;
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

__global__ __launch_bounds__(256) void k_match_pairs(const uint8_t* __restrict__ S,
                                                     const sgplan::Item* __restrict__ items,
                                                     Top2* __restrict__ part) {
    match_pairs_item<false>(S, items, part, nullptr, 0, nullptr, nullptr, nullptr);
}

// The guided work item: the pair's matrices are geom[Item::pair] (a missing matrix is the
// identity with its threshold at 1e20, filled in by the host).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void k_match_pairs_guided(const uint8_t* __restrict__ S,
                                                            const sgplan::Item* __restrict__ items,
                                                            Top2* __restrict__ part,
                                                            const float* __restrict__ loc,
                                                            int loc_stride,
                                                            const GuidedParams* __restrict__ geom) {
    __shared__ uint32_t s_pass[kPanel * kPassPitch];      // [set-1 point][word of set-2 points]
    __shared__ uint32_t s_good[kPanel / 8 * kPassPitch];  // [8-point block of set 1][word]
    match_pairs_item<true>(S, items, part, loc, loc_stride, geom, s_pass, s_good);
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

hipError_t launch_match_pairs_guided(const uint8_t* s8, const sgplan::Item* items, int nitems,
                                     Top2* part, const float* loc, int loc_stride,
                                     const GuidedParams* geom, hipStream_t stream) {
    if (nitems <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_match_pairs_guided, dim3(nitems), dim3(256), 0, stream, s8, items, part,
                       loc, loc_stride, geom);
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
