// sift_detect.hip -- keypoint detection (gfx950 / MI355X): DoG extrema, the scans that give
// every keypoint its slot, and the feature-count limits.
//
// Reference semantics: SiftGPU/ProgramCU.cu (ComputeKEY_Kernel) and SiftGPU/PyramidCU.cpp.
// MI355X-first, not a translation (sift_kernels.h):
//   * DoG images are never stored: the extremum kernel forms the 5 DoG planes of an octave in
//     LDS from the 6 Gaussian planes;
//   * keypoint compaction is a 1-bit-per-pixel mask written with wave ballots plus per-row
//     counts; one exclusive scan over rows gives every keypoint its slot in the reference's
//     (image, octave, level, row, column) order -- no histogram pyramid, no host round trips.
#include <algorithm>

#include "sift_device.h"
#include "sift_keys.h"
#include "sift_top_level.h"

// Build-time tuning knobs (tests/build_variant.sh passes -D overrides; the values here ship).
#ifndef SGK_EXT2_WAVES
#define SGK_EXT2_WAVES 1      // second argument of k_extrema_wave2's __launch_bounds__
#endif
#ifndef SGK_EXT_XCD
#define SGK_EXT_XCD 2         // workgroup order: 0 launch order, 1 xcd_block, 2 xcd_group<SGK_EXT_XCDG>
#endif
#ifndef SGK_EXT_XCDG
#define SGK_EXT_XCDG 4
#endif
#ifndef SGK_EXT_CPL
#define SGK_EXT_CPL 2         // columns per lane of k_extrema_wave2 where the planes allow pairs
#endif
#ifndef SGK_EXT_WAVES
#define SGK_EXT_WAVES 32768   // waves an octave is cut into (launch_extrema)
#endif
#ifndef SGK_EXT_MINROWS
#define SGK_EXT_MINROWS 16    // fewest rows of a batch's strip segment
#endif
#ifndef SGK_EXT_SEG_MIN
#define SGK_EXT_SEG_MIN 32    // fewest rows of a segment in a batch's upper octaves
#endif

namespace sgk {
namespace {

// (ComputeKEY_Kernel's state machine key_test, the keypoint locate() / key_at(): sift_keys.h,
// shared with the test-hook library's candidate dump)

// ------------------------------------------------------------------------------------------
// Extremum detection, wave-streaming form.  Each WAVE owns a strip segment of one image/octave
// and walks it row by row on its own -- no workgroup barriers, so every wave keeps its loads in
// flight independently (a workgroup-synchronised tile walk reached ~3.9 TB/s, the same read
// pattern without barriers ~5.9 TB/s, tests/microbench).
//   * the d+3 Gaussian planes' rows are loaded into registers two rows ahead, turned into the
//     d+2 DoG rows (D_m = G_m - G_{m-1}) and written to a wave-private 4-row LDS ring;
//   * the 3-wide row max/min of each DoG row is computed once and kept in registers for the
//     three output rows it borders; a branch-free 3x3x3 max/min pre-filter selects candidates,
//     which are compacted per wave (ballot + mbcnt) and given the exact ComputeKEY test
//     (key_test) from the ring;
//   * accepted pixels set their bit in the zeroed mask (atomicOr) and count in their row.
struct ExtremaWaveGrid {
    int wave0[kMaxOctaves + 1];        // first global wave of octave o
    int seg_rows[kMaxOctaves];         // rows per strip segment
    int nseg[kMaxOctaves];             // segments per strip column
};

// Layout of the loop (k_extrema_wave2):
//   * A wave covers 62 output columns with 64 lanes: lane l holds column x0 - 1 + l, lanes 0
//     and 63 only feed their neighbours, so no lane issues a separate halo load (halo loads
//     behind a lane branch made the compiler's wait counting assume they were missing and wait
//     for every load in flight).
//   * Two register row sets alternate (the loop is unrolled by two and both halves always run;
//     the second half of the last pair tests no pixel).
//   * The octave's fields are read as scalars before the loop: read inside the candidate branch
//     they were vector loads whose vmcnt(0) waited for the rows in flight.
// Round 2: 1.94 -> 1.72 ms per 128 x 1080p against the one-row form.
// CPL = columns per lane.  CPL = 2: lane l holds the column pair x0 - 1 + 2l, x0 + 2l (one 8-byte
// load per plane and row instead of two 4-byte ones: the texture-address unit, ~88 % busy with
// 4-byte loads, handles a load per lane whatever its width), 126 tested columns per wave;
// x0 = 126 sx + 1 keeps the pairs 8-byte aligned.
// LAZY: the octave's last Gaussian level was not filtered.  The wave fetches planes
// 0 .. nlev-2 and forms ND - 1 DoG rows; DoG levels j < d-1 are decided as always; for j = d-1 the
// pre-filter runs over the 18 values of the two planes it has (a superset of the 27-value one:
// a maximum over fewer values is no larger), ComputeKEY runs up to its last previous-plane row
// (key_test<true>), and a pixel it has not rejected by then gets its mask bit without a row count:
// k_extrema_top decides it.
template <int ND, int CPL, bool LAZY = false>   // ND = number of DoG planes = d + 2
__global__ __launch_bounds__(256, SGK_EXT2_WAVES) void k_extrema_wave2(const float* __restrict__ pyr,
                                                       uint32_t* __restrict__ mask,
                                                       uint32_t* __restrict__ row_count,
                                                       const FeatureParams fp,
                                                       const ExtremaWaveGrid eg) {
    static_assert(CPL == 1 || CPL == 2, "one or two columns per lane");
    constexpr int TW = 64 * CPL - 2;                // tested columns per wave
    constexpr int RW = 64 * CPL + 2 * CPL + 2;      // ring row: column index i at i + CPL (+pad)
    constexpr int NJ = ND - 2;
    constexpr int NR = LAZY ? ND - 1 : ND;          // DoG rows formed (NR + 1 Gaussian planes read)
    __shared__ __attribute__((aligned(8))) float s_ring[4][NR][4][RW];   // [wave][plane][row & 3][col]
    __shared__ uint16_t s_list[4][NJ * 64 * CPL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // Workgroup order.  Two neighbouring 128-column windows (126 columns apart, not line-aligned)
    // share a cache line of every row; the 4 waves of a workgroup are 4 neighbouring strips, so
    // the lines at workgroup boundaries were fetched twice whenever the neighbour ran on another
    // XCD (another L2).  SGK_EXT_XCD = 2 (shipped): xcd_group<4>, 4 consecutive workgroups -- an
    // octave-0 segment row of 16 strips -- on one XCD, dispatched together: detect 1.55-1.56 vs
    // 1.60-1.63 ms (alternating processes, tests/diag/r04l.sh; groups of 2 / 8 / 16 workgroups:
    // 1.59 / 1.56 / 1.58).  SGK_EXT_XCD = 1, xcd_block's partition of the grid into 8 contiguous
    // ranges, measured 1.90 vs 1.67 ms: the ranges hold different octaves, whose waves differ in
    // work, so XCDs went idle.
    const int gw = (SGK_EXT_XCD == 1 ? xcd_block(blockIdx.x, gridDim.x)
                    : SGK_EXT_XCD == 2 ? xcd_group<SGK_EXT_XCDG>(blockIdx.x, gridDim.x)
                                       : (int)blockIdx.x) * 4 + wave;
    if (gw >= eg.wave0[fp.n_octaves]) return;       // uniform per wave
    int o = 0;
    while (o + 1 < fp.n_octaves && gw >= eg.wave0[o + 1]) o++;
    // o is wave-uniform: said so, the octave's fields are scalar loads (lgkmcnt) instead of
    // vector loads from the argument block inside the candidate branch, whose vmcnt(0) would
    // wait for the rows in flight
    o = __builtin_amdgcn_readfirstlane(o);
    const OctaveDesc& od = fp.oct[o];
    const long long mask_off = od.mask_off, mask_lstride = od.mask_level_stride;
    const int nwords = od.nwords;
    const long long rc_base = fp.row_off[o];
    const int W = od.wa, H = od.h;
    const int strips_x = (W + TW - 1) / TW;
    const int id = gw - eg.wave0[o];
    const int sx = id % strips_x, rest = id / strips_x;
    const int sg = rest % eg.nseg[o], b = rest / eg.nseg[o];
    const int x0 = sx * TW + (CPL - 1);
    const int ys = sg * eg.seg_rows[o], ye = min(H, ys + eg.seg_rows[o]);
    const long long lstride = od.level_stride;
    const float* g0 = pyr + od.gauss_off + (long long)b * W * H;
    float(*ring)[4][RW] = s_ring[wave];
    uint16_t* list = s_list[wave];

    // this lane's columns x0 - 1 + CPL * lane + k; CPL = 2 loads the pair from column gx
    // (even; clamped to W - 2, W is even)
    const int xl = x0 - 1 + CPL * lane;
    const int gx = CPL == 1 ? clampi(xl, 0, W - 1) : min(xl, W - 2);
    bool out_col[CPL];
#pragma unroll
    for (int k = 0; k < CPL; k++) {
        const int i = CPL * lane + k, x = xl + k;
        out_col[k] = i >= 1 && i <= TW && x > 0 && x < W - 1;
    }
    struct Row { float m[NR + 1][CPL]; };
    Row rA, rB;
    auto fetch = [&](Row& r, int y) {   // G row y (clamped) into registers
        const float* q = g0 + (long long)clampi(y, 0, H - 1) * W + gx;
#pragma unroll
        for (int m = 0; m <= NR; m++) {
            if constexpr (CPL == 1) {
                r.m[m][0] = q[m * lstride];
            } else {
                const float2 v = *reinterpret_cast<const float2*>(q + m * lstride);
                r.m[m][0] = v.x;
                r.m[m][1] = v.y;
            }
        }
    };
    // Lanes exchange values through the wave-private ring and list.  LDS accesses of one wave
    // complete in issue order, but the compiler sees only per-lane addresses (a lane writes
    // its columns and reads its neighbours') and may reorder them: the empty asm statements keep
    // every write before the reads that follow it.
    // DoG row y into the ring (read by key_test for the rare candidates) and into dog[] (the
    // row max/min below take the neighbours' values by DPP wave shifts, not from LDS)
    float dog[NR][CPL];
    auto put = [&](const Row& r, int y) {
        float* rr = &ring[0][y & 3][CPL * lane + CPL];
#pragma unroll
        for (int m = 0; m < NR; m++) {
#pragma unroll
            for (int k = 0; k < CPL; k++) dog[m][k] = r.m[m + 1][k] - r.m[m][k];
            if constexpr (CPL == 1)
                rr[m * 4 * RW] = dog[m][0];
            else
                *reinterpret_cast<float2*>(&rr[m * 4 * RW]) = make_float2(dog[m][0], dog[m][1]);
        }
        asm volatile("" ::: "memory");
    };
    // rolling 3-wide row max/min of DoG rows y-1 and y (per plane), refreshed per step; the
    // wave's first and last columns get a neighbour from outside the wave (0) and are never
    // tested
    float hx0[NR][CPL], hn0[NR][CPL], hx1[NR][CPL], hn1[NR][CPL], cvx[NR][CPL];
    auto rowmm = [&](float (*mx)[CPL], float (*mn)[CPL], float (*cv)[CPL]) {   // of dog[]
#pragma unroll
        for (int m = 0; m < NR; m++) {
            float v[CPL + 2];   // columns left of, in and right of this lane's
#pragma unroll
            for (int k = 0; k < CPL; k++) v[k + 1] = dog[m][k];
            v[0] = __int_as_float(__builtin_amdgcn_update_dpp(
                0, __float_as_int(dog[m][CPL - 1]), 0x138, 0xf, 0xf, false));   // wave_shr:1
            v[CPL + 1] = __int_as_float(__builtin_amdgcn_update_dpp(
                0, __float_as_int(dog[m][0]), 0x130, 0xf, 0xf, false));         // wave_shl:1
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                mx[m][k] = fmax_(fmax_(v[k], v[k + 1]), v[k + 2]);
                mn[m][k] = fmin_(fmin_(v[k], v[k + 1]), v[k + 2]);
                if (cv) cv[m][k] = v[k + 1];
            }
        }
    };
    auto body = [&](int y) {   // test row y: DoG rows y-1, y are rolled, y+1 is in dog[]
        float hx2[NR][CPL], hn2[NR][CPL], cnx[NR][CPL];
        rowmm(hx2, hn2, cnx);
        const bool row_ok = y < ye && y > 0 && y < H - 1;
        int ncand = 0;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const float v = cvx[j + 1][k];
                float mx = hx0[j][k], mn = hn0[j][k];
#pragma unroll
                for (int m = j; m < j + 3 && m < NR; m++) {
                    mx = fmax_(mx, fmax_(fmax_(hx0[m][k], hx1[m][k]), hx2[m][k]));
                    mn = fmin_(mn, fmin_(fmin_(hn0[m][k], hn1[m][k]), hn2[m][k]));
                }
                // (stated as the negation of ComputeKEY's exits: a NaN v takes none of them and is
                // a candidate in the reference, and mx / mn include v, so they are never NaN for
                // another v)
                const bool cand = row_ok && out_col[k] && !(fabs_(v) <= fp.t0) && !(v < mx && v > mn);
                const unsigned long long bal = __ballot(cand);
                if (cand) {
                    const int pos = ncand + __builtin_amdgcn_mbcnt_hi(
                                                (uint32_t)(bal >> 32),
                                                __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                    list[pos] = (uint16_t)((j << 7) | (CPL * lane + k));
                }
                ncand += __popcll(bal);
            }
        }
        asm volatile("" ::: "memory");
        for (int c0 = 0; c0 < ncand; c0 += 64) {
            if (c0 + lane < ncand) {
                const int code = list[c0 + lane];
                const int j = code >> 7, cl = code & 127;
                auto get = [&](int m, int r, int c) {
                    return ring[j + m][(y + r - 1) & 3][cl + c - 1 + CPL];
                };
                const int xx = x0 - 1 + cl;
                uint32_t* mrow = mask + mask_off + j * mask_lstride + ((long long)b * H + y) * nwords;
                if (LAZY && j == NJ - 1) {
                    // pending: the bit alone (no list, no counter; k_extrema_top walks the mask)
                    if (key_test<true>(get, fp.t0, fp.t, fp.edge, fp.subpixel).result != 0.f)
                        atomicOr(&mrow[xx >> 5], 1u << (xx & 31));
                } else if (key_test(get, fp.t0, fp.t, fp.edge, fp.subpixel).result != 0.f) {
                    atomicOr(&mrow[xx >> 5], 1u << (xx & 31));
                    atomicAdd(&row_count[(long long)b * fp.rows_per_image + rc_base + j * H + y],
                              1u);
                }
            }
        }
#pragma unroll
        for (int m = 0; m < NR; m++)
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                hx0[m][k] = hx1[m][k]; hn0[m][k] = hn1[m][k];
                hx1[m][k] = hx2[m][k]; hn1[m][k] = hn2[m][k];
                cvx[m][k] = cnx[m][k];
            }
        asm volatile("" ::: "memory");   // this row's list and ring reads before the next writes
    };
    fetch(rA, ys - 1);
    put(rA, ys - 1);
    rowmm(hx0, hn0, nullptr);
    fetch(rA, ys);
    put(rA, ys);
    rowmm(hx1, hn1, cvx);
    // rows past ye (the row below the segment's last tested row) feed no test: they are
    // fetched clamped to ye, a row already read (cache hit, no HBM bytes).  Round 3 read 2 more
    // rows per segment from HBM (1.19x the algorithmic bytes with 17-row segments).
    fetch(rA, min(ys + 1, ye));
    fetch(rB, min(ys + 2, ye));
    // each set is refetched after the row test that follows its put: the test's atomics (a
    // data-dependent number of them) then come before, not after, the loads that the next wait
    // must leave in flight
    for (int y = ys; y < ye; y += 2) {
        put(rA, y + 1);
        body(y);
        fetch(rA, min(y + 3, ye));
        put(rB, y + 2);
        body(y + 1);
        fetch(rB, min(y + 4, ye));
    }
}

// ------------------------------------------------------------------------------------------
// Extremum detection in 2-D tiles, for cache-resident pyramids (one image: C2).  The wave kernel's
// walk of a strip segment is a chain of row loads; a single 1080p image gives it ~2,700 waves
// that each wait for ~5 dependent row fetches (29 us, profiles/r06a).  Here a workgroup owns 64
// tested columns x 16 rows of one octave and image for all d levels: it issues the loads of the
// d + 3 Gaussian planes' window (18 rows x 72 columns, aligned quads) at once, stores the d + 2
// DoG planes D_m = G_{m+1} - G_m into LDS, and each wave tests 4 rows (a lane per column): the
// same branch-free 3x3x3 pre-filter superset as k_extrema_wave2, then ComputeKEY's exact state
// machine (key_test) on the LDS values for every candidate.  The tested pixels (1 .. W-2 x
// 1 .. H-2 per octave), the mask bits and the row counts are the wave kernel's; only the order of
// the commutative atomics differs.
struct ExtremaTileGrid {
    int tile0[kMaxOctaves + 1];   // first workgroup of octave o
    int tx[kMaxOctaves];          // tiles per row of octave o
    int ty[kMaxOctaves];          // tiles per column
};
constexpr int kEtW = 64, kEtH = 16, kEtLW = 72;   // tile columns / rows, LDS row (18 quads)

template <int ND>
__global__ __launch_bounds__(256) void k_extrema_tile(const float* __restrict__ pyr,
                                                      uint32_t* __restrict__ mask,
                                                      uint32_t* __restrict__ row_count,
                                                      const FeatureParams fp,
                                                      const ExtremaTileGrid eg) {
    constexpr int NJ = ND - 2, R = kEtH + 2, NQ = kEtLW / 4, NIT = R * NQ;
    constexpr int LITEMS = (NIT + 255) / 256;
    __shared__ __attribute__((aligned(16))) float s_d[ND][R][kEtLW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bid = blockIdx.x;
    int o = 0;
    while (o + 1 < fp.n_octaves && bid >= eg.tile0[o + 1]) o++;
    o = __builtin_amdgcn_readfirstlane(o);
    const OctaveDesc& od = fp.oct[o];
    const int W = od.wa, H = od.h;
    const int id = bid - eg.tile0[o];
    const int sx = id % eg.tx[o], rest = id / eg.tx[o];
    const int sy = rest % eg.ty[o], b = rest / eg.ty[o];
    const int x0 = sx * kEtW, y0 = sy * kEtH;
    const long long lstride = od.level_stride;
    const float* g0 = pyr + od.gauss_off + (long long)b * W * H;
    // the window: rows y0 - 1 .. y0 + 16 (clamped), columns x0 - 4 .. x0 + 67 as aligned quads
    // (clamped: the tested columns' neighbours x0 - 1 .. x0 + 64 are inside the plane wherever a
    // tested column exists)
    float4 gq[LITEMS][ND + 1];
#pragma unroll
    for (int i = 0; i < LITEMS; i++) {
        const int it = min(tid + 256 * i, NIT - 1);
        const int rr = it / NQ, q = it - rr * NQ;
        const int y = clampi(y0 - 1 + rr, 0, H - 1);
        const int xq = clampi(x0 - 4 + 4 * q, 0, W - 4);
        const float* p = g0 + (long long)y * W + xq;
#pragma unroll
        for (int m = 0; m <= ND; m++) gq[i][m] = *reinterpret_cast<const float4*>(p + m * lstride);
    }
#pragma unroll
    for (int i = 0; i < LITEMS; i++) {
        const int it = tid + 256 * i;
        if (NIT % 256 != 0 && it >= NIT) break;
        const int rr = it / NQ, q = it - rr * NQ;
#pragma unroll
        for (int m = 0; m < ND; m++) {
            const float4 a = gq[i][m], c = gq[i][m + 1];
            *reinterpret_cast<float4*>(&s_d[m][rr][4 * q]) =
                make_float4(c.x - a.x, c.y - a.y, c.z - a.z, c.w - a.w);
        }
    }
    __syncthreads();
    // wave w: tile rows 4 w .. 4 w + 3 (LDS rows 4 w + 1 .. 4 w + 4), lane = column x0 + lane
    // (LDS column lane + 4)
    const int x = x0 + lane;
    const bool col_ok = x > 0 && x < W - 1;
    const int lc = lane + 4;
    float hx[ND][6], hn[ND][6];   // 3-wide row max / min of LDS rows 4 w .. 4 w + 5
#pragma unroll
    for (int m = 0; m < ND; m++)
#pragma unroll
        for (int r = 0; r < 6; r++) {
            const float* row = &s_d[m][4 * wave + r][lc];
            const float a = row[-1], c = row[0], e = row[1];
            hx[m][r] = fmax_(fmax_(a, c), e);
            hn[m][r] = fmin_(fmin_(a, c), e);
        }
    uint32_t pend = 0;   // bit i * NJ + j: row i, level j passed the pre-filter
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int y = y0 + 4 * wave + i;
        const bool row_ok = y > 0 && y < H - 1;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const float v = s_d[j + 1][4 * wave + 1 + i][lc];
            float mx = hx[j][i], mn = hn[j][i];
#pragma unroll
            for (int m = j; m < j + 3; m++) {
                mx = fmax_(mx, fmax_(fmax_(hx[m][i], hx[m][i + 1]), hx[m][i + 2]));
                mn = fmin_(mn, fmin_(fmin_(hn[m][i], hn[m][i + 1]), hn[m][i + 2]));
            }
            // (the negation of ComputeKEY's exits, which a NaN v does not take: k_extrema_wave2)
            if (row_ok && col_ok && !(fabs_(v) <= fp.t0) && !(v < mx && v > mn)) pend |= 1u << (i * NJ + j);
        }
    }
    // every lane works through its candidates one per iteration (the wave loops while any lane
    // has one left): ComputeKEY on the LDS values, accepted pixels set their mask bit and count
    while (__ballot(pend != 0)) {
        if (pend) {
            const int bit = __ffs(pend) - 1;
            pend &= pend - 1;
            const int i = bit / NJ, j = bit - i * NJ;
            const int lr = 4 * wave + 1 + i;
            auto get = [&](int m, int r, int c) { return s_d[j + m][lr + r - 1][lc + c - 1]; };
            if (key_test(get, fp.t0, fp.t, fp.edge, fp.subpixel).result != 0.f) {
                const int y = y0 + 4 * wave + i;
                uint32_t* mrow = mask + od.mask_off + j * od.mask_level_stride +
                                 ((long long)b * H + y) * od.nwords;
                atomicOr(&mrow[x >> 5], 1u << (x & 31));
                atomicAdd(&row_count[(long long)b * fp.rows_per_image + fp.row_off[o] + j * H + y], 1u);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// The pending pixels of the lazy extremum pass.  A unit is kTopRows consecutive
// rows of DoG level d-1's mask region of one octave (rows ordered image, row); waves take units
// by a static grid stride.  A wave loads its unit's mask words at once (a lane per word and row),
// then in rounds: every lane hands in the lowest set bit of each of its words, compacted into a
// wave-private list (ballot + mbcnt), and the wave works through the list with all 64 lanes per
// pixel.  Per pixel: the (fw+2)^2 window of level nlev-2 and the 3 x 3 of planes nlev-4 .. nlev-2
// are loaded one pixel ahead (the loads of pixel i+1 are in flight while pixel i is computed: the
// windows come from HBM, ~2 us away); top_level_eval gives level nlev-1 at the nine points, which
// are stored into the level's plane (neighbouring pending pixels store equal bits to shared
// points; nobody reads the plane in this kernel); lane 0 runs the exact ComputeKEY test with the
// last DoG plane formed from the fresh values in LDS.  Accepted: the row count; rejected: the bit
// is cleared.  A mask word belongs to one wave, bits and counts do not depend on the order, so
// mask, counts and everything after them are the dense path's.
constexpr int kTopRows = 8;
struct ExtremaTopGrid {
    int unit0[kMaxOctaves + 1];   // first unit of octave o
};

template <int FW>
__global__ __launch_bounds__(256) void k_extrema_top(float* __restrict__ pyr,
                                                     uint32_t* __restrict__ mask,
                                                     uint32_t* __restrict__ row_count,
                                                     const FeatureParams fp, const ExtremaTopGrid tg,
                                                     const TopLevelFilter tf) {
    using G = TopGeom<FW>;
    __shared__ TopLds s_all[4];
    __shared__ uint16_t s_list[4][kTopRows * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    TopLds& s = s_all[wave];
    uint16_t* list = s_list[wave];
    const int jt = fp.d - 1, top = fp.d + 2;   // top = nlev - 1
    const int nwaves = gridDim.x * 4;
    const int gm = lane / 9, gq = lane - 9 * gm, gr = gq / 3, gc = gq - 3 * gr;   // lanes < 27: plane, row, column
    for (int u = blockIdx.x * 4 + wave; u < tg.unit0[fp.n_octaves]; u += nwaves) {
        int o = 0;
        while (o + 1 < fp.n_octaves && u >= tg.unit0[o + 1]) o++;
        o = __builtin_amdgcn_readfirstlane(o);
        const OctaveDesc& od = fp.oct[o];
        const int W = od.wa, H = od.h, nwords = od.nwords;
        const long long npx = (long long)W * H, lstride = od.level_stride;
        const long long rows = (long long)fp.batch * H;       // rows of the level's mask region
        const long long r0 = (long long)(u - tg.unit0[o]) * kTopRows;
        const int b0 = (int)(r0 / H), y0 = (int)(r0 - (long long)b0 * H);
        uint32_t* mtop = mask + od.mask_off + jt * od.mask_level_stride;
        float* g0 = pyr + od.gauss_off;   // level 0, image 0
        // (image, row) of a list entry's row k, its plane pointers, and the entry's loads
        struct Px { int b, y, x, k; };
        auto locate_px = [&](int code) {
            Px p;
            p.k = code >> 12;
            p.x = code & 4095;
            p.b = b0;
            p.y = y0 + p.k;
            while (p.y >= H) { p.y -= H; p.b++; }
            return p;
        };
        for (int w0 = 0; w0 < nwords; w0 += 64) {
            uint32_t word[kTopRows];
#pragma unroll
            for (int k = 0; k < kTopRows; k++)
                word[k] = (r0 + k < rows && w0 + lane < nwords) ? mtop[(r0 + k) * nwords + w0 + lane] : 0u;
            for (;;) {
                int cnt = 0;
#pragma unroll
                for (int k = 0; k < kTopRows; k++) {
                    const bool has = word[k] != 0u;
                    const unsigned long long bal = __ballot(has);
                    if (has) {
                        const int bit = __ffs(word[k]) - 1;
                        word[k] &= word[k] - 1;
                        const int pos = cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                  __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                        list[pos] = (uint16_t)((k << 12) | (lane * 32 + bit));
                    }
                    cnt += __popcll(bal);
                }
                if (cnt == 0) break;
                asm volatile("" ::: "memory");
                float vc[G::NLD], vn[G::NLD], gvc, gvn;
                auto fetch = [&](int i, float (&v)[G::NLD], float& gv) {
                    const Px p = locate_px(__builtin_amdgcn_readfirstlane((int)list[i]));
                    const int x = w0 * 32 + p.x;
                    const float* g = g0 + (long long)p.b * npx;
                    top_window_load<FW>(g + (top - 1) * lstride, W, H, x, p.y, lane, v);
                    // planes nlev-4 .. nlev-2 around the pixel (clamped: only interior bits are
                    // ever set, and no address leaves the plane whatever the mask holds)
                    const int yy = top_clamp(p.y + gr - 1, 0, H - 1), xx = top_clamp(x + gc - 1, 0, W - 1);
                    gv = g[(top - 3 + min(gm, 2)) * lstride + (uint32_t)(yy * W + xx)];
                };
                fetch(0, vc, gvc);
                for (int i = 0; i < cnt; i++) {
                    fetch(min(i + 1, cnt - 1), vn, gvn);   // (the last round re-reads its own lines)
                    const Px p = locate_px(__builtin_amdgcn_readfirstlane((int)list[i]));
                    const int x = w0 * 32 + p.x, y = p.y;
                    const bool interior = x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2;
                    if (lane < 27) s.g[lane] = gvc;
                    top_level_eval<FW>(vc, tf.taps, s, lane);
                    float* g = g0 + (long long)p.b * npx;
                    if (lane < 9 && interior)
                        g[top * lstride + (long long)(y + gr - 1) * W + x + gc - 1] = s.top[lane];
                    if (lane == 0) {
                        auto get = [&](int m, int r, int c) {
                            const int q = 3 * r + c;
                            return (m == 2 ? s.top[q] : s.g[9 * (m + 1) + q]) - s.g[9 * m + q];
                        };
                        if (interior && key_test(get, fp.t0, fp.t, fp.edge, fp.subpixel).result != 0.f)
                            atomicAdd(&row_count[(long long)p.b * fp.rows_per_image + fp.row_off[o] + jt * H + y], 1u);
                        else
                            atomicAnd(&mtop[(r0 + p.k) * nwords + w0 + (p.x >> 5)], ~(1u << (p.x & 31)));
                    }
                    asm volatile("" ::: "memory");   // this pixel's LDS reads before the next one's writes
#pragma unroll
                    for (int q = 0; q < G::NLD; q++) vc[q] = vn[q];
                    gvc = gvn;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// Exclusive scan (uint32), 1024 elements per block.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

__global__ __launch_bounds__(256) void k_scan_block(const uint32_t* __restrict__ in,
                                                    uint32_t* __restrict__ out, size_t n,
                                                    uint32_t* __restrict__ block_sums) {
    __shared__ uint32_t s_w[4];
    const size_t base = (size_t)blockIdx.x * 1024 + threadIdx.x * 4;
    uint32_t v[4];
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = (base + i < n) ? in[base + i] : 0u;
    uint32_t tsum = v[0] + v[1] + v[2] + v[3];
    uint32_t incl = wave_incl_scan(tsum);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t wofs = 0, total = 0;
    for (int w = 0; w < 4; w++) {
        if (w < wave) wofs += s_w[w];
        total += s_w[w];
    }
    uint32_t run = wofs + incl - tsum;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (base + i < n) out[base + i] = run;
        run += v[i];
    }
    if (threadIdx.x == 0) {
        if (block_sums) block_sums[blockIdx.x] = total;
        else out[n] = total;   // single-block scan writes the total itself
    }
}

// Exclusive scan of a short array (a single image's rows or candidates: C2) by one workgroup
// in tiles of 4096, the running total carried across tiles: one launch instead of the three of
// the block scan (each a few microseconds of launch latency at these sizes).
__global__ __launch_bounds__(1024) void k_scan_single(const uint32_t* __restrict__ in,
                                                      uint32_t* __restrict__ out, size_t n) {
    // one pass: thread t owns the contiguous run [t c, t c + c), c = ceil(n / 1024) <= 32, loaded
    // at once (one round trip; round 5 walked 4,096-element tiles one after the other: a single
    // image's two scans took 6-7 us each)
    __shared__ uint32_t s_w[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t c = (n + 1023) / 1024;
    const size_t base = (size_t)threadIdx.x * c;
    uint32_t v[32];
    uint32_t tsum = 0;
#pragma unroll
    for (int i = 0; i < 32; i++) {
        v[i] = ((size_t)i < c && base + i < n) ? in[base + i] : 0u;
        tsum += v[i];
    }
    const uint32_t incl = wave_incl_scan(tsum);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t wofs = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) {
        const uint32_t sw = s_w[w];
        wofs += w < wave ? sw : 0u;
        total += sw;
    }
    uint32_t run = wofs + incl - tsum;
#pragma unroll
    for (int i = 0; i < 32; i++) {
        if ((size_t)i < c && base + i < n) out[base + i] = run;
        run += v[i];
    }
    if (threadIdx.x == 0) out[n] = total;
}

__global__ __launch_bounds__(256) void k_scan_add(uint32_t* __restrict__ out, size_t n,
                                                  const uint32_t* __restrict__ block_ofs) {
    const size_t base = (size_t)blockIdx.x * 1024 + threadIdx.x * 4;
    const uint32_t add = block_ofs[blockIdx.x];
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (base + i < n) out[base + i] += add;
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = block_ofs[gridDim.x];
}

// ------------------------------------------------------------------------------------------
// Feature-count limiting (-tc / -tc2 / -tc3), per image, on the level counts in octave-major
// order: the level skip of PyramidCU::GenerateFeatureList (PyramidCU.cpp:829-853; levels are
// visited coarsest first for -tc2, and a level is skipped once the running count exceeds the
// threshold) when list_stage, then SiftPyramid::LimitFeatureCount (SiftPyramid.cpp:219-260):
// -tc3 keeps the first levels until the threshold is reached, -tc / -tc2 drop the finest levels
// while the rest still exceeds it.
constexpr int kMaxLimitLevels = kMaxOctaves * 8;

__device__ void limit_levels(int* cnt, int nl, int T, int method, bool list_stage) {
    if (list_stage && method != 0) {
        int total = 0;
        for (int q = 0; q < nl; q++) {
            const int l = method == 1 ? nl - 1 - q : q;
            if (total > T) cnt[l] = 0;
            else total += cnt[l];
        }
    }
    int num = 0;
    for (int l = 0; l < nl; l++) num += cnt[l];
    if (method == 2) {
        int i = 0, kept = 0;
        for (; kept < T && i < nl; ++i) kept += cnt[i];
        for (; i < nl; ++i) cnt[i] = 0;
    } else {
        for (int i = 0; i < nl && num - cnt[i] > T; ++i) {
            num -= cnt[i];
            cnt[i] = 0;
        }
    }
}

__device__ __forceinline__ int level_of_row(const FeatureParams& fp, int r) {
    int o = 0;
    while (o + 1 < fp.n_octaves && fp.row_off[o + 1] <= r) o++;
    return o * fp.d + (r - fp.row_off[o]) / fp.oct[o].h;
}

// Stages 1-2 on the detected keypoints: the row counts of dropped levels are zeroed before the
// row scan, so their keypoints never enter the list.  One workgroup per image.
__global__ __launch_bounds__(256) void k_limit_rows(uint32_t* __restrict__ row_count,
                                                    const FeatureParams fp, int T, int method) {
    __shared__ int s_cnt[kMaxLimitLevels];
    const int nl = fp.n_octaves * fp.d;
    uint32_t* rc = row_count + (size_t)blockIdx.x * fp.rows_per_image;
    for (int l = threadIdx.x; l < nl; l += 256) s_cnt[l] = 0;
    __syncthreads();
    for (int r = threadIdx.x; r < fp.rows_per_image; r += 256) {
        const uint32_t v = rc[r];
        if (v) atomicAdd(&s_cnt[level_of_row(fp, r)], (int)v);
    }
    __syncthreads();
    if (threadIdx.x == 0) limit_levels(s_cnt, nl, T, method, true);
    __syncthreads();
    for (int r = threadIdx.x; r < fp.rows_per_image; r += 256)
        if (s_cnt[level_of_row(fp, r)] == 0) rc[r] = 0;
}

// Stage 3 (LimitFeatureCount(1) after ReshapeFeatureListCPU, SiftPyramid.cpp:152-160) on the
// oriented feature counts: the counts of dropped levels' keypoints are zeroed before the
// feature scan.  One workgroup per image.
__global__ __launch_bounds__(256) void k_limit_oriented(uint32_t* __restrict__ ocount,
                                                        const uint32_t* __restrict__ row_base,
                                                        const FeatureParams fp, int T, int method,
                                                        uint32_t cap) {
    __shared__ int s_cnt[kMaxLimitLevels];
    const int nl = fp.n_octaves * fp.d;
    const size_t r0 = (size_t)blockIdx.x * fp.rows_per_image;
    auto range = [&](int l, uint32_t& lo, uint32_t& hi) {
        const int o = l / fp.d, j = l - o * fp.d;
        const size_t first = r0 + fp.row_off[o] + (size_t)j * fp.oct[o].h;
        lo = min(row_base[first], cap);
        hi = min(row_base[first + fp.oct[o].h], cap);
    };
    for (int l = threadIdx.x; l < nl; l += 256) s_cnt[l] = 0;
    __syncthreads();
    for (int l = 0; l < nl; l++) {
        uint32_t lo, hi;
        range(l, lo, hi);
        int sum = 0;
        for (uint32_t f = lo + threadIdx.x; f < hi; f += 256) sum += (int)ocount[f];
        if (sum) atomicAdd(&s_cnt[l], sum);
    }
    __syncthreads();
    if (threadIdx.x == 0) limit_levels(s_cnt, nl, T, method, false);
    __syncthreads();
    for (int l = 0; l < nl; l++) {
        if (s_cnt[l] != 0) continue;
        uint32_t lo, hi;
        range(l, lo, hi);
        for (uint32_t f = lo + threadIdx.x; f < hi; f += 256) ocount[f] = 0;
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------
hipError_t launch_extrema(const float* pyr, uint32_t* mask, uint32_t* row_count,
                          const FeatureParams& fp, hipStream_t stream, bool tiles, bool lazy) {
    if (tiles && lazy) return hipErrorInvalidValue;   // the tile kernel reads every plane
    bool tile_ok = tiles && ((uintptr_t)pyr % 16) == 0;
    for (int o = 0; o < fp.n_octaves; o++)
        tile_ok = tile_ok && fp.oct[o].wa % 4 == 0 && fp.oct[o].wa >= 4 && fp.oct[o].gauss_off % 4 == 0 &&
                  fp.oct[o].level_stride % 4 == 0;
    if (tile_ok) {
        ExtremaTileGrid tg{};
        long long nb = 0;
        for (int o = 0; o < fp.n_octaves; o++) {
            tg.tile0[o] = (int)nb;
            tg.tx[o] = (fp.oct[o].wa + kEtW - 1) / kEtW;
            tg.ty[o] = (fp.oct[o].h + kEtH - 1) / kEtH;
            nb += (long long)tg.tx[o] * tg.ty[o] * fp.batch;
        }
        tg.tile0[fp.n_octaves] = (int)nb;
        if (nb <= 0 || nb >= (1ll << 31)) return hipErrorInvalidValue;
        switch (fp.d + 2) {
#define SGK_EXTT(ND) \
    case ND: hipLaunchKernelGGL((k_extrema_tile<ND>), dim3((unsigned)nb), dim3(256), 0, stream, pyr, mask, \
                                row_count, fp, tg); return hipGetLastError();
            SGK_EXTT(3) SGK_EXTT(4) SGK_EXTT(5) SGK_EXTT(6) SGK_EXTT(7) SGK_EXTT(8)
#undef SGK_EXTT
            default: return hipErrorInvalidValue;
        }
    }
    // one wave per (image, strip of tested columns, row segment); ~32k waves in all.  Two
    // columns per lane when every plane is 8-byte aligned (always, for pyramid levels: widths
    // are multiples of 4)
    bool pairs = SGK_EXT_CPL == 2 && ((uintptr_t)pyr % 8) == 0;
    for (int o = 0; o < fp.n_octaves; o++)
        pairs = pairs && fp.oct[o].wa % 2 == 0 && fp.oct[o].gauss_off % 2 == 0 &&
                fp.oct[o].level_stride % 2 == 0 && ((long long)fp.oct[o].wa * fp.oct[o].h) % 2 == 0;
    const int sw = pairs ? 126 : 62;
    ExtremaWaveGrid eg{};
    int nw = 0;
    for (int o = 0; o < fp.n_octaves; o++) {
        const OctaveDesc& od = fp.oct[o];
        const int strips_x = (od.wa + sw - 1) / sw;
        const long long per_col = (long long)strips_x * fp.batch;
        // segments of >= 16 rows; a single image >= 8 (C2: its ~1,100 octave-0 waves are
        // latency-bound walks, detection 35.6 vs 44.0 us, C2 0.371-0.377 vs 0.380-0.387 ms per
        // image, tests/diag/r04u.sh; batches keep 16: their halo rows are HBM bytes)
        const int minrows = fp.batch == 1 ? 8 : SGK_EXT_MINROWS;
        int nseg = (int)std::min<long long>(std::max<long long>(1, (SGK_EXT_WAVES + per_col - 1) / per_col),
                                            std::max(1, od.h / minrows));
        // a segment reads one halo row above and below it: 2/17 = 12 % extra bytes on the 17-row
        // segments of the batch's upper octaves, so there segments get >= SGK_EXT_SEG_MIN rows
        // while the octave keeps >= 8192 waves (a single image keeps its short segments: there
        // the latency of the longest wave is the kernel's time)
        if (o > 0 && per_col * (od.h / SGK_EXT_SEG_MIN) >= 8192)
            nseg = std::min(nseg, std::max(1, od.h / SGK_EXT_SEG_MIN));
        const int rows = (od.h + nseg - 1) / nseg;
        nseg = (od.h + rows - 1) / rows;
        eg.wave0[o] = nw;
        eg.seg_rows[o] = rows;
        eg.nseg[o] = nseg;
        nw += strips_x * nseg * fp.batch;
    }
    eg.wave0[fp.n_octaves] = nw;
    const unsigned nb = (unsigned)((nw + 3) / 4);
#define SGK_EXTW(ND, LAZY)                                                                       \
    case 2 * ND: hipLaunchKernelGGL((k_extrema_wave2<ND, 1, LAZY>), dim3(nb), dim3(256), 0, stream, \
                                    pyr, mask, row_count, fp, eg); break;                        \
    case 2 * ND + 1: hipLaunchKernelGGL((k_extrema_wave2<ND, 2, LAZY>), dim3(nb), dim3(256), 0,    \
                                        stream, pyr, mask, row_count, fp, eg); break;
    if (lazy) {
        switch ((fp.d + 2) * 2 + (pairs ? 1 : 0)) {
            SGK_EXTW(3, true) SGK_EXTW(4, true) SGK_EXTW(5, true) SGK_EXTW(6, true)
            SGK_EXTW(7, true) SGK_EXTW(8, true)
            default: return hipErrorInvalidValue;
        }
    } else {
        switch ((fp.d + 2) * 2 + (pairs ? 1 : 0)) {
            SGK_EXTW(3, false) SGK_EXTW(4, false) SGK_EXTW(5, false) SGK_EXTW(6, false)
            SGK_EXTW(7, false) SGK_EXTW(8, false)
            default: return hipErrorInvalidValue;
        }
    }
#undef SGK_EXTW
    return hipGetLastError();
}

hipError_t launch_extrema_top(float* pyr, uint32_t* mask, uint32_t* row_count,
                              const FeatureParams& fp, const TopLevelFilter& tf,
                              hipStream_t stream) {
    if (tf.fw < 1 || tf.fw > kTopMaxFW || !(tf.fw & 1) || fp.d < 1) return hipErrorInvalidValue;
    ExtremaTopGrid tg{};
    long long nu = 0;
    for (int o = 0; o < fp.n_octaves; o++) {
        tg.unit0[o] = (int)nu;
        nu += ((long long)fp.batch * fp.oct[o].h + kTopRows - 1) / kTopRows;
    }
    if (nu <= 0 || nu >= (1ll << 31)) return hipErrorInvalidValue;
    tg.unit0[fp.n_octaves] = (int)nu;
    // a resident grid (static stride: workgroups that start after the first residents would only
    // lengthen the tail)
    int dev = 0, cus = 0, per_cu = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    const bool known = top_level_dispatch(tf.fw, [&](auto FWC) {
        constexpr int FW = decltype(FWC)::value;
        static int resident = 0;   // per width; the same for every device of one kind
        if (!resident &&
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, k_extrema_top<FW>, 256, 0) != hipSuccess)
            resident = 0;
        per_cu = std::max(1, resident);
        const unsigned nb = (unsigned)std::min<long long>((nu + 3) / 4, (long long)std::max(1, cus) * per_cu);
        hipLaunchKernelGGL((k_extrema_top<FW>), dim3(nb), dim3(256), 0, stream, pyr, mask, row_count,
                           fp, tg, tf);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

static size_t scan_blocks(size_t n) { return (n + 1023) / 1024; }

size_t scan_tmp_words(size_t n) {
    size_t words = 0;
    while (n > 1024) {
        size_t nb = scan_blocks(n);
        words += nb + nb + 1;   // block sums + their scan
        n = nb;
    }
    return words + 16;
}

__global__ __launch_bounds__(256) void k_zero(uint32_t* __restrict__ a, size_t na,
                                              uint32_t* __restrict__ b, size_t nb,
                                              uint32_t* __restrict__ c, size_t nc) {
    const size_t step = (size_t)gridDim.x * 256;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q * 4 < na; q += step) zero_words(a, na, q);
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q * 4 < nb; q += step) zero_words(b, nb, q);
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q * 4 < nc; q += step) zero_words(c, nc, q);
}

hipError_t launch_zero(uint32_t* a, size_t na, uint32_t* b, size_t nb, uint32_t* c, size_t nc,
                       hipStream_t stream) {
    // the uint4 stores need 16-byte aligned buffers (hipMalloc's are)
    for (const uint32_t* p : {(const uint32_t*)a, (const uint32_t*)b, (const uint32_t*)c})
        if ((uintptr_t)p % 16) return hipErrorInvalidValue;
    if (!a) na = 0;
    if (!b) nb = 0;
    if (!c) nc = 0;
    const size_t quads = (std::max(na, std::max(nb, nc)) + 3) / 4;
    if (quads == 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((quads + 255) / 256, 4096);
    hipLaunchKernelGGL(k_zero, dim3(grid), dim3(256), 0, stream, a, na, b, nb, c, nc);
    return hipGetLastError();
}

hipError_t launch_scan(const uint32_t* in, uint32_t* out, size_t n, uint32_t* tmp,
                       hipStream_t stream) {
    if (n <= 1024) {
        hipLaunchKernelGGL(k_scan_block, dim3(1), dim3(256), 0, stream, in, out, n,
                           (uint32_t*)nullptr);
        return hipGetLastError();
    }
    if (n <= 32768) {   // one workgroup, <= 32 elements per thread
        hipLaunchKernelGGL(k_scan_single, dim3(1), dim3(1024), 0, stream, in, out, n);
        return hipGetLastError();
    }
    const size_t nb = scan_blocks(n);
    uint32_t* sums = tmp;
    uint32_t* sums_scan = tmp + nb;
    hipLaunchKernelGGL(k_scan_block, dim3((unsigned)nb), dim3(256), 0, stream, in, out, n, sums);
    hipError_t e = launch_scan(sums, sums_scan, nb, tmp + nb + nb + 1, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_scan_add, dim3((unsigned)nb), dim3(256), 0, stream, out, n, sums_scan);
    return hipGetLastError();
}

hipError_t launch_limit_rows(uint32_t* row_count, const FeatureParams& fp, int threshold,
                             int method, hipStream_t stream) {
    if (fp.n_octaves * fp.d > kMaxLimitLevels) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_limit_rows, dim3(fp.batch), dim3(256), 0, stream, row_count, fp,
                       threshold, method);
    return hipGetLastError();
}

hipError_t launch_limit_oriented(uint32_t* ocount, const uint32_t* row_base,
                                 const FeatureParams& fp, int threshold, int method,
                                 uint32_t cand_cap, hipStream_t stream) {
    if (fp.n_octaves * fp.d > kMaxLimitLevels) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_limit_oriented, dim3(fp.batch), dim3(256), 0, stream, ocount, row_base,
                       fp, threshold, method, cand_cap);
    return hipGetLastError();
}

}  // namespace sgk
