// sift_level.hip -- Gaussian level filters and input conversion (gfx950 / MI355X).
//
// Reference semantics: SiftGPU/ProgramCU.cu (FilterH / FilterV, the down- and upsample kernels)
// and SiftGPU/PyramidCU.cpp (stage order).  MI355X-first, not a translation (sift_kernels.h):
//   * one launch per (octave, level) covers the whole image batch;
//   * the separable Gaussian is one fused kernel (H pass into an LDS tile, V pass from LDS),
//     8 B/px of HBM traffic per level instead of the reference's 16, with the next octave's
//     2x downsample written from the same tile.
// Floating-point conventions are those of oracle/sift_oracle.cpp (fma contractions written
// out, transcendentals from sift_math.h); the build uses -ffp-contract=off.
#include <numeric>
#include <type_traits>
#include <utility>

#include "sift_device.h"

// Build-time tuning knobs (tests/build_variant.sh passes -D overrides; the values here ship).
#ifndef SGK_GW_WPB
#define SGK_GW_WPB 4          // waves per workgroup of k_gauss_lean / k_gauss_diag
#endif
#ifndef SGK_GW_HSPAD
#define SGK_GW_HSPAD 4        // padding floats of an H-ring row (row stride GT + pad)
#endif
#ifndef SGK_GW_NST_U8
#define SGK_GW_NST_U8 4       // input chunks a wave holds in registers on the u8 ingest level
#endif
#ifndef SGK_GW_XCD
#define SGK_GW_XCD 1          // workgroup order: 1 xcd_block, 2 xcd_group<SGK_GW_XCDG>
#endif
#ifndef SGK_GW_XCDG
#define SGK_GW_XCDG 4
#endif
#ifndef SGK_SHORT_BAND_MB
#define SGK_SHORT_BAND_MB 64  // levels up to this size may use one-chunk bands (gauss_wave_grid)
#endif

namespace sgk {
namespace {

// ------------------------------------------------------------------------------------------
// Gaussian level: FilterH<FW> then FilterV<FW> (ProgramCU.cu:115-222) in one kernel.
// A 256-thread workgroup owns a 64-column strip of `rows_per_strip` output rows and walks it top
// to bottom in chunks of SR2 = 32 rows:
//   * the input rows of chunk c+2 are loaded into registers while chunk c is filtered
//     (register-staged prefetch, written to LDS after the V pass), so HBM loads overlap the
//     filter arithmetic;
//   * the input chunk is stored in LDS as row PAIRS, s_in[pair][col] = (row 2p, row 2p+1);
//   * every FMA is a v_pk_fma_f32 on two independent outputs (gfx950 issues packed FP32 at twice
//     the scalar rate): a thread's H pass covers 2 rows x 4 columns and its V pass 4 rows x 2
//     columns, so every value read from LDS feeds 4 packed FMAs;
//   * the H pass writes 32 filtered rows into a 64-row LDS ring; the V pass emits output chunk
//     c-1 from the ring (lag one chunk: FW - 1 <= 32).
// Each input row is read from HBM once per strip (vertical halo (FW-1)/rows_per_strip), the
// horizontal halo (FW-1)/64 comes through L2.  Each packed lane is an IEEE fma and the taps are
// summed i = 0..FW-1 in order, so the levels are bit-identical to the oracle.
constexpr int GT = 64;

// Tap t of a width-FW filter.  make_filter's taps are symmetric bit for bit (tap i is
// exp(-i^2 / 2 sigma^2) / sum for i = t - FW/2), so the kernels holding two filters read only
// the first half: half the scalar registers (two full tap sets spilled SGPRs to VGPR lanes).
template <int FW>
__device__ __forceinline__ float tap(const Taps& taps, int t) {
    return taps.k[t < FW - 1 - t ? t : FW - 1 - t];
}

// p / 255.0f for an integer p in [0, 255] (GLTexImage.cpp:818: the reference's u8 -> float),
// correctly rounded without a division: q = p * (1/255) then one fma residual correction.  Exact
// for all 256 inputs (tests/test_oracle.py::test_u8_scale_is_exact_division).
__device__ __forceinline__ float u8_to_unit(uint32_t p) {
    const float x = (float)p, c = 1.0f / 255.0f;
    const float q = x * c;
    return fma_(fma_(-q, 255.0f, x), c, q);
}

constexpr int SR2 = 32;

// VEC: the input rows are fetched as 16-byte (f32) / 4-byte (u8) aligned quads instead of one
// element per lane: the strip's load window starts at a0 = x0 - HALF - OFF, OFF = (-HALF) & 3,
// so every quad is aligned, and quads left of column 0 / right of W-1 replicate the edge value
// (W is a multiple of 4, so a quad is entirely inside or entirely outside).  LDS column j holds
// input column a0 + j in both forms.
template <int FW, bool U8, bool VEC>
__global__ __launch_bounds__(256) void k_gauss_pk2(
    const float* __restrict__ src, const uint8_t* __restrict__ src8, int src_stride,
    long long src_img_stride, float* __restrict__ dst, long long dst_img_stride, int W, int H,
    Taps taps, float* __restrict__ ds, int dsw, int dsh, long long ds_img_stride,
    int rows_per_strip) {
    constexpr int HALF = FW >> 1;
    constexpr int OFF = VEC ? ((-HALF) & 3) : 0;      // LDS column of the strip's first input
    constexpr int IN_W = GT + FW - 1 + OFF;           // input columns held per row
    constexpr int NQ = (IN_W + 3) / 4;                // aligned quads per row (VEC)
    constexpr int NRD = (FW + 3) / 2;                 // ds_read_b128 per H-pass thread
    constexpr int IN_S = (GT + FW + 3 + OFF + 3) & ~3;   // float2 per row pair
    static_assert(!VEC || 4 * NQ <= IN_S, "quad stores stay inside the row pair");
    constexpr int RS = 64;                            // ring rows: (1 + 1) * 32 for FW <= 33
    constexpr int HS = GT + 4;                        // ring row stride (floats)
    constexpr int NLD = VEC ? ((SR2 / 2) * NQ + 255) / 256 : ((SR2 / 2) * IN_W + 255) / 256;
    constexpr int IN_SV = IN_S;                       // LDS row-pair stride
    static_assert(FW - 1 <= SR2, "ring holds one chunk of lag");
    __shared__ __attribute__((aligned(16))) f2v s_in[(SR2 / 2) * IN_SV];
    __shared__ __attribute__((aligned(16))) float s_h[RS * HS];

    const int tid = threadIdx.x;
    const int strips_x = (W + GT - 1) / GT;
    const int strips_y = (H + rows_per_strip - 1) / rows_per_strip;
    const int id = blockIdx.x;
    const int sx = id % strips_x, rest = id / strips_x;
    const int sy = rest % strips_y, b = rest / strips_y;
    const int x0 = sx * GT;
    const int yb = sy * rows_per_strip;
    const int ye = min(H, yb + rows_per_strip);
    const int nin = (ye - yb) + FW - 1;
    const int nchunk_in = (nin + SR2 - 1) / SR2;
    const int nchunk_out = (ye - yb + SR2 - 1) / SR2;

    const float* sf = U8 ? nullptr : src + (long long)b * src_img_stride;
    const uint8_t* s8 = U8 ? src8 + (long long)b * src_img_stride : nullptr;
    const int a0 = x0 - HALF - OFF;
    // stage element: VEC -> 4 pairs (rows 2p, 2p+1 of one aligned quad); else one pair
    typedef typename std::conditional<VEC, f2v[4], f2v[1]>::type Elem;
    Elem stA[NLD], stB[NLD];
    auto load_chunk = [&](Elem (&stage)[NLD], int c) {
#pragma unroll
        for (int m = 0; m < NLD; m++) {
            if (VEC) {
                const int e = min(tid + 256 * m, (SR2 / 2) * NQ - 1);
                const int p = e / NQ, j = e - p * NQ;
                const int gy0 = clampi(yb - HALF + c * SR2 + 2 * p, 0, H - 1);
                const int gy1 = clampi(yb - HALF + c * SR2 + 2 * p + 1, 0, H - 1);
                const int gq = a0 + 4 * j;                          // aligned first column
                const int lq = clampi(gq, 0, W - 4);
                float r0[4], r1[4];
                if (U8) {
                    const uint32_t w0 = *reinterpret_cast<const uint32_t*>(s8 + (long long)gy0 * src_stride + lq);
                    const uint32_t w1 = *reinterpret_cast<const uint32_t*>(s8 + (long long)gy1 * src_stride + lq);
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        r0[t] = u8_to_unit((w0 >> (8 * t)) & 255u);
                        r1[t] = u8_to_unit((w1 >> (8 * t)) & 255u);
                    }
                } else {
                    const float4 v0 = *reinterpret_cast<const float4*>(sf + (long long)gy0 * src_stride + lq);
                    const float4 v1 = *reinterpret_cast<const float4*>(sf + (long long)gy1 * src_stride + lq);
                    r0[0] = v0.x; r0[1] = v0.y; r0[2] = v0.z; r0[3] = v0.w;
                    r1[0] = v1.x; r1[1] = v1.y; r1[2] = v1.z; r1[3] = v1.w;
                }
                // clamp-to-edge: a quad left of column 0 repeats column 0, right of W-1 repeats W-1
                const bool left = gq < 0, right = gq > W - 4;
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const float u0 = left ? r0[0] : (right ? r0[3] : r0[t]);
                    const float u1 = left ? r1[0] : (right ? r1[3] : r1[t]);
                    stage[m][t] = f2v{u0, u1};
                }
            } else {
                const int e = min(tid + 256 * m, (SR2 / 2) * IN_W - 1);
                const int p = e / IN_W, col = e - p * IN_W;
                const int gy0 = clampi(yb - HALF + c * SR2 + 2 * p, 0, H - 1);
                const int gy1 = clampi(yb - HALF + c * SR2 + 2 * p + 1, 0, H - 1);
                const int gx = clampi(a0 + col, 0, W - 1);
                if (U8) {
                    stage[m][0] = f2v{u8_to_unit(s8[(long long)gy0 * src_stride + gx]),
                                      u8_to_unit(s8[(long long)gy1 * src_stride + gx])};
                } else {
                    stage[m][0] = f2v{sf[(long long)gy0 * src_stride + gx],
                                      sf[(long long)gy1 * src_stride + gx]};
                }
            }
        }
    };
    auto store_chunk = [&](const Elem (&stage)[NLD]) {
#pragma unroll
        for (int m = 0; m < NLD; m++) {
            const int e = tid + 256 * m;
            if (VEC) {
                if (e < (SR2 / 2) * NQ) {
                    const int p = e / NQ, j = e - p * NQ;
                    float4* q = reinterpret_cast<float4*>(&s_in[p * IN_SV + 4 * j]);
                    q[0] = make_float4(stage[m][0].x, stage[m][0].y, stage[m][1].x, stage[m][1].y);
                    q[1] = make_float4(stage[m][2].x, stage[m][2].y, stage[m][3].x, stage[m][3].y);
                }
            } else if (e < (SR2 / 2) * IN_W) {
                const int p = e / IN_W, col = e - p * IN_W;
                s_in[p * IN_SV + col] = stage[m][0];
            }
        }
    };

    load_chunk(stA, 0);
    store_chunk(stA);
    if (1 < nchunk_in) load_chunk(stA, 1);
    __syncthreads();
    float* d = dst + (long long)b * dst_img_stride;
    float* dd = ds ? ds + (long long)b * ds_img_stride : nullptr;
    const int hp = tid >> 4, hc = (tid & 15) * 4;     // H pass: rows 2hp, 2hp+1; columns hc..hc+3
    const int vq = tid >> 5, vc = (tid & 31) * 2;     // V pass: rows 4vq..4vq+3; columns vc, vc+1
    const int x = x0 + vc;
    // iteration c: chunk c is in LDS, chunk c+1 in `cur` registers; load chunk c+2 into `nxt`
    auto step = [&](int c, Elem (&cur)[NLD], Elem (&nxt)[NLD]) {
        const bool has_in = c < nchunk_in, has_next = c + 1 < nchunk_in;
        if (c + 2 < nchunk_in) load_chunk(nxt, c + 2);
        if (has_in) {   // H pass of input chunk c -> ring rows c*SR2 .. c*SR2+31
            const f2v* rowp = &s_in[hp * IN_SV + hc + OFF];
            f2v a[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};   // columns hc+i
#pragma unroll
            for (int q = 0; q < NRD; q++) {
                f2v e[2];                            // pair columns hc+2q, hc+2q+1
                if (OFF % 2 == 0) {
                    const float4 v = reinterpret_cast<const float4*>(rowp)[q];
                    e[0] = f2v{v.x, v.y};
                    e[1] = f2v{v.z, v.w};
                } else {
                    e[0] = rowp[2 * q];
                    e[1] = rowp[2 * q + 1];
                }
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const int m = 2 * q + u;
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (m - i >= 0 && m - i < FW) a[i] = pk_fma(e[u], taps.k[m - i], a[i]);
                }
            }
            const int r0 = (c * SR2 + 2 * hp) & (RS - 1);
            *reinterpret_cast<float4*>(&s_h[r0 * HS + hc]) = make_float4(a[0].x, a[1].x, a[2].x, a[3].x);
            *reinterpret_cast<float4*>(&s_h[(r0 + 1) * HS + hc]) = make_float4(a[0].y, a[1].y, a[2].y, a[3].y);
        }
        __syncthreads();
        const int kout = c - 1;
        if (kout >= 0) {   // V pass of output chunk kout (lag 1 chunk: FW - 1 <= SR2)
            const int t0 = kout * SR2 + 4 * vq;
            f2v acc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};   // rows t0+j
#pragma unroll
            for (int m = 0; m < FW + 3; m++) {
                const f2v v = *reinterpret_cast<const f2v*>(&s_h[((t0 + m) & (RS - 1)) * HS + vc]);
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (m - j >= 0 && m - j < FW) acc[j] = pk_fma(v, taps.k[m - j], acc[j]);
            }
            // the sums are complete here: without this, each row's FMA chain is sunk into its
            // conditional store below and every ring value of the pass stays live until then
            // (+2 VGPRs per tap: a wave per SIMD of occupancy, pyramid +9 %)
#pragma unroll
            for (int j = 0; j < 4; j++) asm volatile("" : "+v"(acc[j]));
            if (x < W) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int y = yb + t0 + j;
                    if (y < ye) {
                        *reinterpret_cast<f2v*>(&d[(long long)y * W + x]) = acc[j];
                        // DownsampleKernel<1> (ProgramCU.cu:287-298) into the next octave's
                        // level 0: dst(r, c) = src(2r, min(2c, W-1)); x is even, W is even.
                        if (dd && !(y & 1) && (y >> 1) < dsh) {
                            float* drow = dd + (long long)(y >> 1) * dsw;
                            if ((x >> 1) < dsw) drow[x >> 1] = acc[j].x;
                            if (x + 1 == W - 1)
                                for (int cc = W >> 1; cc < dsw; cc++) drow[cc] = acc[j].y;
                        }
                    }
                }
            }
        }
        if (has_next) store_chunk(cur);
        __syncthreads();
    };
    const int nsteps = nchunk_out + 1;
    for (int c = 0; c < nsteps; c += 2) {
        step(c, stA, stB);
        if (c + 1 < nsteps) step(c + 1, stB, stA);
    }
}

// ------------------------------------------------------------------------------------------
// Gaussian level, wave-streaming form (k_gauss_lean below): the same H-then-V filter as
// k_gauss_pk2 (same taps, same summation order i = 0..FW-1, so bit-identical outputs), but every
// WAVE owns a 64-column strip band and walks it on its own with a wave-private LDS row-pair buffer
// and H ring -- no workgroup barriers, so each wave keeps its row loads in flight independently
// of the other waves of its workgroup (the extremum kernel gained 3.9 -> 5.9 TB/s from the same
// change).  Per step a wave:
//   * H-filters input chunk c (8 rows: 4 row pairs x 16 lanes x 4 columns, packed FMAs) from
//     the row-pair buffer into ring rows 8c .. 8c+7;
//   * V-filters output chunk c - L (L = ceil((FW-1)/8) chunks of lag: 2 row groups x 32 lanes
//     x 2 columns x 4 rows) from the ring and stores it (plus the decimated next-octave level);
//   * moves input chunk c+1 from registers into the row-pair buffer and issues the loads of
//     chunk c+4.
// LDS ops of one wave execute in issue order, so a wave needs no barrier between writing a
// buffer and reading what other lanes wrote; the empty asm statements only stop the compiler
// from moving LDS accesses across the phase boundaries.  Every LDS access of a wave stays inside
// its own buffers (round 3's pad-slot overrun, fixed in k_gauss_lean's loaders).

constexpr int WCH = 8;   // rows per chunk (wave kernel)

struct GaussWaveGrid {
    int strips_x, nsy, rows_per_band, total_waves;
};

constexpr int kGwWaves = SGK_GW_WPB;   // waves per workgroup of k_gauss_lean

// band height of the level kernel: rows_hint > 0 forces it (test / tuning hook), else bands of
// the whole image unless that leaves fewer than ~8 waves per CU, then as many bands as needed.
// A band re-reads the level's FW-1 halo rows, so bands stay >= 4 chunks high while the level
// streams from HBM; a level of at most SGK_SHORT_BAND_MB (one image of a small batch, or the
// upper octaves of a batch, largely still in the 256 MB Infinity Cache from the previous level)
// may go down to one chunk: its launches are
// latency-bound (a wave walks band + lag chunks one after the other), and shorter bands are
// fewer steps per wave.  Measured against 128 MB with ~8,192 waves on such levels (alternating
// processes, tests/diag/r03h.sh): pyramid 3.69 vs 3.73-3.76 ms per 128 x 1080p, C4 3.55 vs 3.65.
static GaussWaveGrid gauss_wave_grid(int w, int h, int batch, int rows_hint, int nw,
                                     bool long_bands = false) {
    GaussWaveGrid g{};
    g.strips_x = (w + GT * nw - 1) / (GT * nw);
    const long long per_band = (long long)g.strips_x * nw * batch;   // waves per band
    int rows = h;
    if (rows_hint > 0) {
        rows = rows_hint;
    } else {
        // long_bands (A/B hook, per context: SGPU_DEBUG_GAUSS_LONG_BANDS, or SGPU_GAUSS_BANDS=long
        // read at context creation) keeps bands >= 4 chunks on every level (round 2)
        const bool short_ok = !long_bands && 4ll * w * h * batch <= ((long long)SGK_SHORT_BAND_MB << 20);
        const long long want = 8 * 256;
        const int nsy = (int)std::min<long long>((want + per_band - 1) / per_band,
                                                 std::max(1, h / ((short_ok ? 1 : 4) * WCH)));
        rows = (h + std::max(nsy, 1) - 1) / std::max(nsy, 1);
    }
    rows = std::max(WCH, (rows + WCH - 1) / WCH * WCH);
    g.rows_per_band = rows;
    g.nsy = (h + rows - 1) / rows;
    g.total_waves = (int)(per_band * g.nsy);
    return g;
}

// ------------------------------------------------------------------------------------------
// Gaussian level, lean form (the shipped kernel, FW <= 33): round 2's k_gauss_wave filter -- same
// strips, bands, chunks, row-pair buffer, H ring and lag, the same taps in the same order, so the
// levels are bit-identical -- with the per-step work that is not filtering taken off the vector
// ALU.  The kernel traces showed k_gauss_wave issuing ~150 non-FMA VALU instructions per 8-row
// step against 88 packed FMAs (FW 11): 64-bit load and store addresses, per-lane row clamps,
// clamp-to-edge selects, ring-row wrap arithmetic.  Here:
//   * the wave's geometry is uniform (readfirstlane of the wave index), so image, band and row
//     bases live in SGPRs and every global load / store is a uniform row pointer plus a lane
//     constant 32-bit offset (the saddr form);
//   * the loaders are laid out lane = 32 g + j: half-wave g loads the quads j of row pair 2m + g,
//     so a lane's column (and its clamp) is fixed for the whole kernel, and a chunk's rows are
//     uniform; only chunks that reach above row 0 or below row H-1 clamp per lane;
//   * clamp-to-edge column selects only in the strips at the image's left / right edge;
//   * the ring holds 4 chunk slots (RS = 32, LAG <= 3; 8 slots, RS = 64, for FW 27 .. 33) and the
//     step's slot is compile-time (the main loop is unrolled by the slot count), so ring reads and writes are lane-constant base + immediate
//     offset; the half-wave whose rows wrap first (vq = 1, 4 rows ahead) reads through a second
//     base for the 4 rows where only it has wrapped;
//   * u8 -> f32 (the ingest level) on row pairs with packed multiply / fma;
//   * the decimation into the next octave's level 0 is a template parameter.
// f(integral_constant<int, I>) for I in the sequence, in order (compile-time step indices)
template <int... I, class F>
__device__ __forceinline__ void unrolled_steps(std::integer_sequence<int, I...>, F&& f) {
    (f(std::integral_constant<int, I>{}), ...);
}

// One level filter job of a launch: source (u8 or f32), destination, geometry, taps, the
// optional decimation into the next octave's level 0, and the wave grid.
struct GaussJob {
    const float* src;
    const uint8_t* src8;
    int src_stride;
    long long src_img_stride;
    float* dst;
    long long dst_img_stride;
    int W, H;
    Taps taps;
    float* ds;
    int dsw, dsh;
    long long ds_img_stride;
    GaussWaveGrid gg;
    ZeroJob zero;   // buffers this launch zeroes besides filtering (the extract's first launch)
};

// a ZeroJob over the whole grid (uint4 stores; the buffers are hipMalloc'ed, 16-B aligned)
__device__ __forceinline__ void zero_job(const ZeroJob& z) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll
    for (int i = 0; i < 3; i++)
        for (size_t q = t0; q * 4 < z.n[i]; q += step) zero_words(z.p[i], z.n[i], q);
}

// LDS geometry of the level filter for width FW (per wave)
template <int FW>
struct LeanGeom {
    static constexpr int HALF = FW >> 1;
    static constexpr int OFF = (-HALF) & 3;                  // LDS column of the strip's first input
    static constexpr int IN_W = GT + FW - 1 + OFF;           // input columns held per row
    static constexpr int NQ = (IN_W + 3) / 4;                // aligned quads per row
    static constexpr int SH = OFF & 1;
    static constexpr int IN_S0 = (4 * NQ + SH + 3) & ~3;
    static constexpr int IN_S = IN_S0 + ((2 - IN_S0) & 31);  // float2 per row pair (= 2 mod 32)
    static constexpr int LAG = (FW - 1 + WCH - 1) / WCH;     // chunks between H and V of a row
    // ring rows: 4 slots of WCH for FW <= 25 (LAG <= 3), 8 for FW 27 .. 33 (LAG 4)
    static constexpr int RS = WCH * (LAG + 1) <= 32 ? 32 : 64;
    static constexpr int HS = GT + SGK_GW_HSPAD;             // ring row stride (floats)
    static constexpr int IN_WORDS = (WCH / 2) * IN_S + 8;    // float2: row pairs + 2 pad slots
    static constexpr int RING_WORDS = RS * HS;               // floats
};

// The level filter of one wave (global wave index gw of job J) with its LDS buffers s_in / s_h.
template <int FW, bool U8, bool DS>
__device__ __forceinline__ void gauss_lean_wave(const GaussJob& J, int gw, f2v* s_in, float* s_h) {
    using G = LeanGeom<FW>;
    constexpr int HALF = G::HALF, OFF = G::OFF, NQ = G::NQ, SH = G::SH, IN_S = G::IN_S;
    static_assert(NQ <= 32, "a row's quads fit half a wave");
    constexpr int NRD = (FW + 3) / 2;                 // ds_read_b128 per H-pass lane
    static_assert(IN_S % 32 == 2 && 4 * NQ + SH <= IN_S, "row-pair stride");
    constexpr int LAG = G::LAG, RS = G::RS, HS = G::HS;
    constexpr int NSLOT = RS / WCH;
    static_assert(WCH * (LAG + 1) <= RS && FW <= 33, "the ring's chunk slots hold the lag");
    constexpr int NPAIR = WCH / 2;
    constexpr int NST = U8 ? SGK_GW_NST_U8 : 4;       // chunks in registers (u8: 1 dword per row)
    const float* __restrict__ src = J.src;
    const uint8_t* __restrict__ src8 = J.src8;
    const int src_stride = J.src_stride;
    const long long src_img_stride = J.src_img_stride;
    float* __restrict__ dst = J.dst;
    const long long dst_img_stride = J.dst_img_stride;
    const int W = J.W, H = J.H;
    const Taps& taps = J.taps;
    float* __restrict__ ds = J.ds;
    const int dsw = J.dsw, dsh = J.dsh;
    const long long ds_img_stride = J.ds_img_stride;
    const GaussWaveGrid& gg = J.gg;

    const int lane = threadIdx.x & 63;
    if (gw >= gg.total_waves) return;                 // uniform per wave
    const int sx = gw % gg.strips_x, rest = gw / gg.strips_x;
    const int x0 = sx * GT;
    const int sy = rest % gg.nsy, b = rest / gg.nsy;
    const int yb = sy * gg.rows_per_band;
    const int ye = min(H, yb + gg.rows_per_band);
    const int nchunk_out = (ye - yb + WCH - 1) / WCH;

    const float* sf = U8 ? nullptr : src + (long long)b * src_img_stride;
    const uint8_t* s8 = U8 ? src8 + (long long)b * src_img_stride : nullptr;
    const int a0 = x0 - HALF - OFF;
    // loader lane: row pair g, quad j (lanes past the row's last quad re-load the last quad)
    // lane = 8 k + 4 g + i -> quad 4 k + i of row pair g: an 8-lane ds_write_b128 group covers
    // all 32 banks (rows 2p and 2p + 2's pairs are 2 IN_S = 4 mod 32 floats apart), and the lanes
    // past the row's last quad skip the row-pair store instead of sharing one pad slot
    // (conflict-free stores: 128 x 1080p pyramid 3.402 / 3.434 vs 3.440 / 3.441 ms per step
    // against round 5's lane = 32 g + j map, two alternating pairs, tests/diag/g6.sh)
    const int lj0 = (lane & 3) | ((lane >> 3) << 2);
    const int lg = (lane >> 2) & 1, lj = min(lj0, NQ - 1);
    const bool lreal = lj0 < NQ;
    const int gq = a0 + 4 * lj;
    const int lq = clampi(gq, 0, W - 4);
    const bool left = gq < 0, right = gq > W - 4;
    const bool edge = a0 < 0 || a0 + 4 * NQ > W;      // uniform: this strip clamps columns
    // element offsets of the lane's quad in rows 2 g and 2 g + 1 of a row group
    const uint32_t loff0 = (uint32_t)(2 * lg * src_stride + lq), loff1 = loff0 + (uint32_t)src_stride;
    // LDS float2 index of the lane's quad in row pairs lg (m = 0) and lg + 2 (m = 1); a lane past
    // the row's last quad gets a pad slot of its own per m, and store_chunk skips its store
    // altogether.  (Round 3 stored there, used one pad slot and
    // added the m = 1 pair offset to it too: those stores landed 2 IN_S float2 past the wave's
    // buffer -- in the next wave's row-pair padding, or past the workgroup's LDS for the last
    // wave -- harmless only by layout; the same pattern made k_gauss_pair's aliased mid buffer
    // nondeterministic)
    const int s_off0 = lreal ? lg * IN_S + 4 * lj + SH : NPAIR * IN_S;
    const int s_off1 = lreal ? s_off0 + 2 * IN_S : NPAIR * IN_S + 4;

    struct Elem { float4 v0, v1; };   // the raw fetch of rows 2p, 2p+1 (u8: .x as the u32)
    Elem st[NST][2];
    auto load_chunk = [&](Elem (&stage)[2], int c) __attribute__((always_inline)) {
        const int rb = yb - HALF + WCH * c;           // first input row of chunk c (uniform)
        if (rb >= 0 && rb + WCH <= H) {
#pragma unroll
            for (int m = 0; m < 2; m++) {
                const long long ro = (long long)(rb + 4 * m) * src_stride;   // uniform
                if (U8) {
                    const uint8_t* r = s8 + ro;
                    stage[m].v0.x = __uint_as_float(*reinterpret_cast<const uint32_t*>(r + loff0));
                    stage[m].v1.x = __uint_as_float(*reinterpret_cast<const uint32_t*>(r + loff1));
                } else {
                    const float* r = sf + ro;
                    stage[m].v0 = *reinterpret_cast<const float4*>(r + loff0);
                    stage[m].v1 = *reinterpret_cast<const float4*>(r + loff1);
                }
            }
        } else {   // the band reaches above row 0 or below row H-1: rows clamp per lane
#pragma unroll
            for (int m = 0; m < 2; m++) {
                const int y0 = clampi(rb + 4 * m + 2 * lg, 0, H - 1);
                const int y1 = clampi(rb + 4 * m + 2 * lg + 1, 0, H - 1);
                if (U8) {
                    stage[m].v0.x = __uint_as_float(*reinterpret_cast<const uint32_t*>(s8 + (long long)y0 * src_stride + lq));
                    stage[m].v1.x = __uint_as_float(*reinterpret_cast<const uint32_t*>(s8 + (long long)y1 * src_stride + lq));
                } else {
                    stage[m].v0 = *reinterpret_cast<const float4*>(sf + (long long)y0 * src_stride + lq);
                    stage[m].v1 = *reinterpret_cast<const float4*>(sf + (long long)y1 * src_stride + lq);
                }
            }
        }
    };
    auto store_chunk = [&](const Elem (&stage)[2]) __attribute__((always_inline)) {
#pragma unroll
        for (int m = 0; m < 2; m++) {
            f2v pr[4];   // column t of the quad: (row 2p, row 2p+1)
            if (U8) {
                const uint32_t w0 = __float_as_uint(stage[m].v0.x), w1 = __float_as_uint(stage[m].v1.x);
                const float c = 1.0f / 255.0f;
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    // u8_to_unit on the pair: q = x / 255 rounded, then one fma correction
                    const f2v x{(float)((w0 >> (8 * t)) & 255u), (float)((w1 >> (8 * t)) & 255u)};
                    const f2v q = x * f2v{c, c};
                    const f2v r = __builtin_elementwise_fma(-q, f2v{255.0f, 255.0f}, x);
                    pr[t] = __builtin_elementwise_fma(r, f2v{c, c}, q);
                }
            } else {
                pr[0] = f2v{stage[m].v0.x, stage[m].v1.x};
                pr[1] = f2v{stage[m].v0.y, stage[m].v1.y};
                pr[2] = f2v{stage[m].v0.z, stage[m].v1.z};
                pr[3] = f2v{stage[m].v0.w, stage[m].v1.w};
            }
            if (edge) {   // clamp-to-edge: a quad left of column 0 repeats column 0, right of W-1 W-1
                const f2v e0 = pr[0], e3 = pr[3];
#pragma unroll
                for (int t = 0; t < 4; t++) pr[t] = left ? e0 : (right ? e3 : pr[t]);
            }
            f2v* q = s_in + (m ? s_off1 : s_off0);
            if (!lreal) continue;
            if (SH == 0) {
                reinterpret_cast<float4*>(q)[0] = make_float4(pr[0].x, pr[0].y, pr[1].x, pr[1].y);
                reinterpret_cast<float4*>(q)[1] = make_float4(pr[2].x, pr[2].y, pr[3].x, pr[3].y);
            } else {   // 8-byte aligned
#pragma unroll
                for (int t = 0; t < 4; t++) q[t] = pr[t];
            }
        }
    };

#pragma unroll
    for (int k = 0; k < NST; k++) load_chunk(st[k], k);
    store_chunk(st[0]);
    float* d = dst + (long long)b * dst_img_stride;
    float* dd = DS ? ds + (long long)b * ds_img_stride : nullptr;
    const int hp = lane >> 4, hc = (lane & 15) * 4;    // H pass: rows 2hp, 2hp+1; columns hc..hc+3
    const int vq = lane >> 5, vc = (lane & 31) * 2;    // V pass: rows 4vq..4vq+3; columns vc, vc+1
    const int x = x0 + vc;
    const bool active = x0 < W;                      // uniform
    const bool full_cols = x0 + GT <= W;             // uniform: every lane's columns exist
    const f2v* h_rd = s_in + hp * IN_S + hc + OFF + SH;
    float* h_wr = s_h + 2 * hp * HS + hc;
    const float* v_rd = s_h + 4 * vq * HS + vc;              // rows before the wrap
    const float* v_rd_amb = v_rd - (vq ? RS * HS : 0);       // rows where only vq = 1 wrapped
    const uint32_t st_off = (uint32_t)(4 * vq * W + x);      // lane offset of the V-pass stores
    const uint32_t ds_off = (uint32_t)(2 * vq * dsw + (x >> 1));
    // step c (ring slot K = c mod 4): H pass of input chunk c, V pass of output chunk c - LAG,
    // loads of chunk c + NST into `nxt`, chunk c + 1 (`cur`) into the row-pair buffer
    auto step = [&](int c, auto KC, Elem (&cur)[2], Elem (&nxt)[2]) __attribute__((always_inline)) {
        constexpr int K = decltype(KC)::value;
        {   // H pass -> ring rows 8K .. 8K+7
            f2v a[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};   // columns hc+i
#pragma unroll
            for (int q = 0; q < NRD; q++) {
                const float4 v = reinterpret_cast<const float4*>(h_rd)[q];
                const f2v e[2] = {f2v{v.x, v.y}, f2v{v.z, v.w}};
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const int m = 2 * q + u;
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (m - i >= 0 && m - i < FW) a[i] = pk_fma(e[u], tap<FW>(taps, m - i), a[i]);
                }
            }
            *reinterpret_cast<float4*>(h_wr + WCH * K * HS) = make_float4(a[0].x, a[1].x, a[2].x, a[3].x);
            *reinterpret_cast<float4*>(h_wr + (WCH * K + 1) * HS) = make_float4(a[0].y, a[1].y, a[2].y, a[3].y);
        }
        asm volatile("" ::: "memory");
        const int kout = c - LAG;
        if (active && kout >= 0 && kout < nchunk_out) {   // V pass of output chunk kout (uniform)
            constexpr int KV = ((K - LAG) % NSLOT + NSLOT) % NSLOT;   // its ring slot
            f2v acc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};   // rows t0+j
#pragma unroll
            for (int m = 0; m < FW + 3; m++) {
                const int rc = WCH * KV + m;                 // ring row of half-wave 0
                const float* p = rc < RS - 4 ? v_rd + rc * HS
                               : rc >= RS ? v_rd + (rc - RS) * HS : v_rd_amb + rc * HS;
                const f2v v = *reinterpret_cast<const f2v*>(p);
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (m - j >= 0 && m - j < FW) acc[j] = pk_fma(v, tap<FW>(taps, m - j), acc[j]);
            }
#pragma unroll
            for (int j = 0; j < 4; j++) asm volatile("" : "+v"(acc[j]));
            const int yu = yb + WCH * kout;                  // first row of the chunk (uniform)
            if (full_cols && yu + WCH <= ye && (!DS || (yu + WCH) / 2 <= dsh)) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    float* row = d + (long long)(yu + j) * W;             // uniform
                    *reinterpret_cast<f2v*>(row + st_off) = acc[j];
                    if (DS && !(j & 1)) {
                        // DownsampleKernel<1> (ProgramCU.cu:287-298): dst(r, c) = src(2r, min(2c, W-1))
                        float* drow = dd + (long long)((yu + j) >> 1) * dsw;   // uniform
                        if ((x >> 1) < dsw) drow[ds_off] = acc[j].x;
                        if (x + 1 == W - 1)
                            for (int cc = W >> 1; cc < dsw; cc++) drow[2 * vq * dsw + cc] = acc[j].y;
                    }
                }
            } else if (x < W) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int y = yu + 4 * vq + j;
                    if (y < ye) {
                        *reinterpret_cast<f2v*>(&d[(long long)y * W + x]) = acc[j];
                        if (DS && !(y & 1) && (y >> 1) < dsh) {
                            float* drow = dd + (long long)(y >> 1) * dsw;
                            if ((x >> 1) < dsw) drow[x >> 1] = acc[j].x;
                            if (x + 1 == W - 1)
                                for (int cc = W >> 1; cc < dsw; cc++) drow[cc] = acc[j].y;
                        }
                    }
                }
            }
        }
        asm volatile("" ::: "memory");
        load_chunk(nxt, c + NST);
        store_chunk(cur);
        asm volatile("" ::: "memory");
    };
    const int nsteps = nchunk_out + LAG;
    // slot K = c mod NSLOT, register set c mod NST (steps past the end filter clamped rows and
    // store nothing): the loop is unrolled by lcm(NSLOT, NST) steps
    constexpr int U = std::lcm(NSLOT, NST);
    for (int c = 0; c < nsteps; c += U) {
        unrolled_steps(std::make_integer_sequence<int, U>{}, [&](auto KI) __attribute__((always_inline)) {
            constexpr int k = decltype(KI)::value;
            step(c + k, std::integral_constant<int, k % NSLOT>{}, st[(k + 1) % NST], st[k % NST]);
        });
    }
}

// the level kernels' workgroup order: xcd_block (SGK_GW_XCD 1, shipped) or xcd_group<SGK_GW_XCDG> (2)
__device__ __forceinline__ int gw_order(int bid, int nb) {
    return SGK_GW_XCD == 2 ? xcd_group<SGK_GW_XCDG>(bid, nb) : xcd_block(bid, nb);
}

template <int FW, bool U8, bool DS>
__global__ __launch_bounds__(64 * kGwWaves) void k_gauss_lean(const GaussJob J) {
    using G = LeanGeom<FW>;
    if (J.zero.n[0] | J.zero.n[1] | J.zero.n[2]) zero_job(J.zero);
    __shared__ __attribute__((aligned(16))) f2v s_in_all[kGwWaves][G::IN_WORDS];
    __shared__ __attribute__((aligned(16))) float s_h_all[kGwWaves][G::RING_WORDS];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // XCD-aware order (xcd_block)
    const int gw = gw_order(blockIdx.x, gridDim.x) * kGwWaves + wave;
    gauss_lean_wave<FW, U8, DS>(J, gw, s_in_all[wave], s_h_all[wave]);
}

// Two independent level jobs in one launch ("diagonal": octave o + 1's level k beside octave o's
// level k + kds): blocks [0, nbB) run job B (the small one, dispatched first),
// blocks [nbB, nbB + nbA) job A; nbB is a multiple of 8, so each job keeps the XCD-aware order.
// The LDS buffers are sized for the larger geometry; f32 levels without decimation only.
template <int FWA, int FWB>
__global__ __launch_bounds__(64 * kGwWaves) void k_gauss_diag(const GaussJob A, const GaussJob B,
                                                              int nbB) {
    using GA = LeanGeom<FWA>;
    using GB = LeanGeom<FWB>;
    constexpr int IW = GA::IN_WORDS > GB::IN_WORDS ? GA::IN_WORDS : GB::IN_WORDS;
    constexpr int RW = GA::RING_WORDS > GB::RING_WORDS ? GA::RING_WORDS : GB::RING_WORDS;
    __shared__ __attribute__((aligned(16))) f2v s_in_all[kGwWaves][IW];
    __shared__ __attribute__((aligned(16))) float s_h_all[kGwWaves][RW];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bid = blockIdx.x;
    if (bid < nbB) {
        gauss_lean_wave<FWB, false, false>(B, gw_order(bid, nbB) * kGwWaves + wave,
                                           s_in_all[wave], s_h_all[wave]);
    } else {
        const int nbA = (int)gridDim.x - nbB;
        gauss_lean_wave<FWA, false, false>(A, gw_order(bid - nbB, nbA) * kGwWaves + wave,
                                           s_in_all[wave], s_h_all[wave]);
    }
}

template <int FW>
hipError_t gauss_dispatch(const float* src, const uint8_t* src8, int src_stride,
                          long long src_img_stride, float* dst, long long dst_img_stride, int w,
                          int h, const Taps& taps, int batch, float* ds, int dsw, int dsh,
                          long long ds_img_stride, hipStream_t stream, int wave_rows,
                          bool long_bands, const ZeroJob& zero) {
    const bool vec = (src_stride % 4) == 0 && (src_img_stride % 4) == 0 && (w % 4) == 0 &&
                     w >= 4 && ((uintptr_t)(src8 ? (const void*)src8 : (const void*)src) % 16) == 0;
    if (vec && wave_rows >= 0) {
        const GaussWaveGrid gg = gauss_wave_grid(w, h, batch, wave_rows, 1, long_bands);
        const dim3 wgrid((unsigned)((gg.total_waves + kGwWaves - 1) / kGwWaves));
        const GaussJob J{src, src8, src_stride, src_img_stride, dst, dst_img_stride, w, h, taps,
                         ds, dsw, dsh, ds_img_stride, gg, zero};
#define SGK_LEAN(U8, DS)                                                                      \
        hipLaunchKernelGGL((k_gauss_lean<FW, U8, DS>), wgrid, dim3(64 * kGwWaves), 0, stream, J)
        if (src8) {
            if (ds) SGK_LEAN(true, true); else SGK_LEAN(true, false);
        } else {
            if (ds) SGK_LEAN(false, true); else SGK_LEAN(false, false);
        }
#undef SGK_LEAN
        return hipGetLastError();
    }
    if (zero.n[0] | zero.n[1] | zero.n[2]) {   // the block kernel does not zero: its own launch
        const hipError_t ez = launch_zero(zero.p[0], zero.n[0], zero.p[1], zero.n[1], zero.p[2],
                                          zero.n[2], stream);
        if (ez != hipSuccess) return ez;
    }
    // bands of at most 17 chunks (544 rows), and at least 1024 workgroups when the image is
    // short (kernel traces: 2 bands of 540 rows beat 1 band of 1080 on 1080p, and 1 band beats 2
    // on the 540- and 270-row octaves)
    const int strips_x = (w + GT - 1) / GT;
    const long long per_col = (long long)strips_x * batch;
    int nsy = (h + 17 * SR2 - 1) / (17 * SR2);
    const int need = (int)std::min<long long>((1024 + per_col - 1) / per_col, (h + SR2 - 1) / SR2);
    nsy = std::max(std::max(nsy, need), 1);
    int rows = (h + nsy - 1) / nsy;
    rows = (rows + SR2 - 1) / SR2 * SR2;
    nsy = (h + rows - 1) / rows;
    const dim3 grid((unsigned)(strips_x * nsy * batch));
    // aligned quads need 4-element row strides and image strides, a 16-B aligned base and a
    // width that is a multiple of 4 (always true for pyramid levels)
#define SGK_PK2(U8, VEC)                                                                   \
    hipLaunchKernelGGL((k_gauss_pk2<FW, U8, VEC>), grid, dim3(256), 0, stream, src, src8,    \
                       src_stride, src_img_stride, dst, dst_img_stride, w, h, taps, ds, dsw,  \
                       dsh, ds_img_stride, rows)
    if (src8) {
        if (vec) SGK_PK2(true, true); else SGK_PK2(true, false);
    } else {
        if (vec) SGK_PK2(false, true); else SGK_PK2(false, false);
    }
#undef SGK_PK2
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// -fo != 0: the first octave's input.  src value of input pixel k of the flat tw x h buffer
// the reference binds (_inputTex, PyramidCU.cpp:949-958): u8 -> p / 255.0f as the host
// conversion (GLTexImage.cpp:818); indices past the buffer read 0 (tex1Dfetch).
template <bool U8>
__device__ __forceinline__ float input_at(const float* sf, const uint8_t* s8, int stride, int tw,
                                          int h, long long k) {
    if (k >= (long long)tw * h) return 0.0f;
    const int r = (int)(k / tw), c = (int)(k - (long long)r * tw);
    return U8 ? u8_to_unit(s8[(long long)r * stride + c]) : sf[(long long)r * stride + c];
}

// DownsampleKernel (ProgramCU.cu:287-311): dst(r, c) = src(r << fo, min(c << fo, tw - 1)).
template <bool U8>
__global__ __launch_bounds__(256) void k_input_down(const float* __restrict__ src,
                                                    const uint8_t* __restrict__ src8, int stride,
                                                    long long src_img_stride, int tw, int h,
                                                    int fo, float* __restrict__ dst, int dw, int dh,
                                                    long long dst_img_stride) {
    const int b = blockIdx.z, r = blockIdx.y;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= dw || r >= dh) return;
    const long long so = (long long)b * src_img_stride;
    const int sc = min(c << fo, tw - 1), sr = r << fo;
    const float v = U8 ? u8_to_unit(src8[so + (long long)sr * stride + sc])
                       : src[so + (long long)sr * stride + sc];
    dst[(long long)b * dst_img_stride + (long long)r * dw + c] = v;
}

// UpsampleKernel<s> (ProgramCU.cu:225-270): output row R blends source rows R >> s and
// (R >> s) + 1 with w1 = (R & (S-1)) / S; each source column c writes S outputs at
// (tw R + c) S interpolating c and c + 1 of the flat buffer.  a*b + c*d -> fma(a, b, c*d).
template <bool U8>
__global__ __launch_bounds__(256) void k_input_up(const float* __restrict__ src,
                                                  const uint8_t* __restrict__ src8, int stride,
                                                  long long src_img_stride, int tw, int h, int s,
                                                  float* __restrict__ dst,
                                                  long long dst_img_stride) {
    const int b = blockIdx.z, R = blockIdx.y;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= tw) return;
    const int S = 1 << s;
    const float inv = 1.0f / float(S);
    const float* sf = U8 ? nullptr : src + (long long)b * src_img_stride;
    const uint8_t* s8 = U8 ? src8 + (long long)b * src_img_stride : nullptr;
    const int row = R >> s, helper = R & (S - 1);
    const long long index = (long long)row * tw + c;
    float v1, v2;
    if (helper) {
        const float v11 = input_at<U8>(sf, s8, stride, tw, h, index);
        const float v12 = input_at<U8>(sf, s8, stride, tw, h, index + 1);
        const float v21 = input_at<U8>(sf, s8, stride, tw, h, index + tw);
        const float v22 = input_at<U8>(sf, s8, stride, tw, h, index + tw + 1);
        const float w1 = inv * (float)helper, w2 = 1.0f - w1;   // (float)(1.0 - w1): exact
        v1 = fma_(v21, w1, w2 * v11);
        v2 = fma_(v22, w1, w2 * v12);
    } else {
        v1 = input_at<U8>(sf, s8, stride, tw, h, index);
        v2 = input_at<U8>(sf, s8, stride, tw, h, index + 1);
    }
    float* o = dst + (long long)b * dst_img_stride + ((long long)tw * R + c) * S;
    o[0] = v1;
    for (int i = 1; i < S; i++) {
        const float r2 = (float)i * inv, r1 = 1.0f - r2;
        o[i] = fma_(v1, r1, v2 * r2);
    }
}

// ------------------------------------------------------------------------------------------
// Color -> luminance: (19595 r + 38470 g + 7471 b) / (65535.0f * 255.0f).  The numerator is an
// exact integer below 2^24 and the denominator an exact float, so the IEEE division on the
// device gives the host conversion's bits.
template <int CH, bool BGR>
__global__ __launch_bounds__(256) void k_color_gray(const uint8_t* __restrict__ src, int tw, int h,
                                                    int stride, float* __restrict__ dst) {
    const int b = blockIdx.z, y = blockIdx.y;
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= tw) return;
    const uint8_t* p = src + ((long long)b * h + y) * stride + (long long)x * CH;
    const int r = BGR ? p[2] : p[0], g = p[1], bl = BGR ? p[0] : p[2];
    const int num = 19595 * r + 38470 * g + 7471 * bl;
    dst[((long long)b * h + y) * tw + x] = (float)num / (65535.0f * 255.0f);
}

}  // namespace

// ------------------------------------------------------------------------------------------
hipError_t launch_gauss(const float* src, const uint8_t* src_u8, int src_stride,
                        long long src_img_stride, float* dst, long long dst_img_stride, int w,
                        int h, int fw, const Taps& taps, int batch, float* ds_dst, int ds_w,
                        int ds_h, long long ds_img_stride, hipStream_t stream, int wave_rows,
                        bool long_bands, const ZeroJob& zero) {
#define SGK_GAUSS(FW)                                                                       \
    case FW:                                                                                  \
        return gauss_dispatch<FW>(src, src_u8, src_stride, src_img_stride, dst, dst_img_stride, \
                                  w, h, taps, batch, ds_dst, ds_w, ds_h, ds_img_stride, stream, \
                                  wave_rows, long_bands, zero);
    switch (fw) {
        SGK_GAUSS(5) SGK_GAUSS(7) SGK_GAUSS(9) SGK_GAUSS(11) SGK_GAUSS(13) SGK_GAUSS(15)
        SGK_GAUSS(17) SGK_GAUSS(19) SGK_GAUSS(21) SGK_GAUSS(23) SGK_GAUSS(25) SGK_GAUSS(27)
        SGK_GAUSS(29) SGK_GAUSS(31) SGK_GAUSS(33)
        default: return hipErrorInvalidValue;
    }
#undef SGK_GAUSS
}

hipError_t launch_gauss_op(const LevelOp& op, hipStream_t stream, int wave_rows, bool long_bands) {
    return launch_gauss(op.src, op.src_u8, op.src_stride, op.src_img_stride, op.dst,
                        op.dst_img_stride, op.w, op.h, op.fw, op.taps, op.batch, op.ds_dst,
                        op.ds_w, op.ds_h, op.ds_img_stride, stream, wave_rows, long_bands, op.zero);
}

static bool diag_ok(const LevelOp& op) {
    return !op.src_u8 && !op.ds_dst && op.src && (op.src_stride % 4) == 0 &&
           (op.src_img_stride % 4) == 0 && (op.w % 4) == 0 && op.w >= 4 &&
           ((uintptr_t)op.src % 16) == 0 && !(op.zero.n[0] | op.zero.n[1] | op.zero.n[2]);
}

template <int FWA, int FWB>
static hipError_t gauss_diag_launch(const LevelOp& a, const LevelOp& b, hipStream_t stream,
                                    int wave_rows, bool long_bands) {
    const GaussWaveGrid ga = gauss_wave_grid(a.w, a.h, a.batch, wave_rows, 1, long_bands);
    const GaussWaveGrid gb = gauss_wave_grid(b.w, b.h, b.batch, wave_rows, 1, long_bands);
    const int nbA = (ga.total_waves + kGwWaves - 1) / kGwWaves;
    const int nbB = (gb.total_waves + kGwWaves - 1) / kGwWaves;
    const int nbBp = (nbB + 7) / 8 * 8;   // job A starts on XCD 0 (blocks are dealt round-robin)
    const GaussJob A{a.src, nullptr, a.src_stride, a.src_img_stride, a.dst, a.dst_img_stride, a.w,
                     a.h, a.taps, nullptr, 0, 0, 0, ga, ZeroJob{}};
    GaussJob B{b.src, nullptr, b.src_stride, b.src_img_stride, b.dst, b.dst_img_stride, b.w,
               b.h, b.taps, nullptr, 0, 0, 0, gb, ZeroJob{}};
    // the padding blocks of job B map to waves past its grid (gauss_lean_wave returns)
    B.gg.total_waves = gb.total_waves;
    hipLaunchKernelGGL((k_gauss_diag<FWA, FWB>), dim3((unsigned)(nbBp + nbA)), dim3(64 * kGwWaves),
                       0, stream, A, B, nbBp);
    return hipGetLastError();
}

hipError_t launch_gauss_two(const LevelOp& a, const LevelOp& b, hipStream_t stream, int wave_rows,
                            bool long_bands, int* launches) {
    if (launches) *launches = 1;
    if (wave_rows >= 0 && diag_ok(a) && diag_ok(b)) {
        // the default schedule's pairs (-d 3: levels 4 / 5 of octave o beside levels 1 / 2 of
        // octave o + 1); the larger job is A
        const bool swap = (long long)a.w * a.h * a.batch < (long long)b.w * b.h * b.batch;
        const LevelOp& big = swap ? b : a;
        const LevelOp& small = swap ? a : b;
#define SGK_DIAG(A, B) \
        if (big.fw == A && small.fw == B) return gauss_diag_launch<A, B>(big, small, stream, wave_rows, long_bands);
        SGK_DIAG(21, 11) SGK_DIAG(25, 13)
#undef SGK_DIAG
    }
    if (launches) *launches = 2;
    hipError_t e = launch_gauss_op(a, stream, wave_rows, long_bands);
    if (e != hipSuccess) return e;
    return launch_gauss_op(b, stream, wave_rows, long_bands);
}

hipError_t launch_color_to_gray(const uint8_t* src, int n, int w, int h, int stride,
                                int channels, bool bgr, float* dst, hipStream_t stream) {
    const int tw = w & ~3;
    if (n <= 0 || tw <= 0 || (channels != 3 && channels != 4) || stride < w * channels)
        return hipErrorInvalidValue;
    const dim3 grid((tw + 255) / 256, h, n);
#define SGK_COLOR(CH, B) \
    hipLaunchKernelGGL((k_color_gray<CH, B>), grid, dim3(256), 0, stream, src, tw, h, stride, dst)
    if (channels == 3 && !bgr) SGK_COLOR(3, false);
    else if (channels == 3) SGK_COLOR(3, true);
    else if (!bgr) SGK_COLOR(4, false);
    else SGK_COLOR(4, true);
#undef SGK_COLOR
    return hipGetLastError();
}

hipError_t launch_first_octave_input(const float* src, const uint8_t* src_u8, int stride,
                                     long long src_img_stride, int tw, int h, int fo, float* dst,
                                     int dw, int dh, long long dst_img_stride, int batch,
                                     hipStream_t stream) {
    if (fo > 0) {
        if (dw > (tw >> fo) + 3 || dh > (h >> fo)) return hipErrorInvalidValue;
        const dim3 grid((dw + 255) / 256, dh, batch);
        if (src_u8)
            hipLaunchKernelGGL(k_input_down<true>, grid, dim3(256), 0, stream, src, src_u8, stride,
                               src_img_stride, tw, h, fo, dst, dw, dh, dst_img_stride);
        else
            hipLaunchKernelGGL(k_input_down<false>, grid, dim3(256), 0, stream, src, src_u8,
                               stride, src_img_stride, tw, h, fo, dst, dw, dh, dst_img_stride);
    } else if (fo < 0) {
        const int s = -fo;
        if (s > 3 || dw != (tw << s) || dh != (h << s)) return hipErrorInvalidValue;
        const dim3 grid((tw + 255) / 256, h << s, batch);
        if (src_u8)
            hipLaunchKernelGGL(k_input_up<true>, grid, dim3(256), 0, stream, src, src_u8, stride,
                               src_img_stride, tw, h, s, dst, dst_img_stride);
        else
            hipLaunchKernelGGL(k_input_up<false>, grid, dim3(256), 0, stream, src, src_u8, stride,
                               src_img_stride, tw, h, s, dst, dst_img_stride);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace sgk
