// sift_top_level.h -- the octave's last Gaussian level evaluated at single points,
// shared by the kernel that finishes the top DoG level's pending pixels (k_extrema_top,
// sift_detect.hip) and the test-hook library's one-point probe (sgpu_debug.hip).  Included after
// sift_kernels.h and sift_math.h (`using namespace sgm`).
//
// Level nlev-1 is a leaf: only the last DoG plane reads it, and ComputeKEY reads that plane only in
// the 3 x 3 neighbourhood of a candidate of DoG level d-1.  A lazy pyramid does not filter it;
// top_window_load + top_level_eval compute its nine values around one pixel with the dense
// kernels' arithmetic (k_gauss_lean, sift_level.hip: FilterH then FilterV of level nlev-2, every
// sum from 0 in tap order with fma, columns clamped to [0, wa-1], rows to [0, h-1], the H result
// rounded to float before the V pass), so the values are the dense level's bits.
#pragma once
#include <type_traits>

namespace sgk {
namespace {

constexpr int kTopMaxFW = 33;              // the widest level filter (sift_params.h)
constexpr int kTopWin = kTopMaxFW + 2;     // source window side: fw + 2

// One wave's LDS: the (fw+2)^2 source window, the (fw+2) x 3 H sums, the nine values, and the
// 3 x 3 of planes nlev-4 .. nlev-2 for the exact ComputeKEY test.
struct TopLds {
    float win[kTopWin * kTopWin];
    float hs[3 * kTopWin];
    float top[9];
    float g[27];
};

// How a wave holds a pixel's window in registers: a row takes 32 lanes while it fits (two rows per
// load round), else 64; element i of lane l is window row i * RSTEP + (l >> SH), column l & (2^SH - 1).
template <int FW>
struct TopGeom {
    static constexpr int N = FW + 2, HALF = FW >> 1;
    static constexpr int SH = N <= 32 ? 5 : 6;
    static constexpr int RSTEP = 64 >> SH;
    static constexpr int NLD = (N + RSTEP - 1) / RSTEP;
};

__device__ __forceinline__ int top_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The loads of the window around (x, y): rows y-1-HALF .. y+1+HALF, columns x-1-HALF .. x+1+HALF of
// src (one image's plane of w x h floats, rows w apart), clamped to the plane -- every lane's
// address is inside it.  Issued at once; nothing waits for them here.
template <int FW>
__device__ __forceinline__ void top_window_load(const float* __restrict__ src, int w, int h, int x,
                                                int y, int lane, float (&v)[TopGeom<FW>::NLD]) {
    using G = TopGeom<FW>;
    const int c = lane & ((1 << G::SH) - 1), rsub = lane >> G::SH;
    const int xx = top_clamp(x - 1 - G::HALF + c, 0, w - 1);
#pragma unroll
    for (int i = 0; i < G::NLD; i++) {
        const int yy = top_clamp(y - 1 - G::HALF + i * G::RSTEP + rsub, 0, h - 1);
        v[i] = src[(uint32_t)(yy * w + xx)];
    }
}

// The nine values of FilterV(FilterH(src)) at (x + c - 1, y + r - 1), r, c in 0..2, into
// s.top[3 r + c], from the window top_window_load fetched.  Called by a whole wave.  LDS accesses
// of one wave complete in issue order; the empty asm statements keep the compiler from moving them
// across the phases.
template <int FW>
__device__ __forceinline__ void top_level_eval(const float (&v)[TopGeom<FW>::NLD], const Taps& taps,
                                               TopLds& s, int lane) {
    using G = TopGeom<FW>;
    constexpr int N = G::N;
    const int c = lane & ((1 << G::SH) - 1), rsub = lane >> G::SH;
#pragma unroll
    for (int i = 0; i < G::NLD; i++) {
        const int r = i * G::RSTEP + rsub;
        if (c < N && r < N) s.win[r * N + c] = v[i];
    }
    asm volatile("" ::: "memory");
    // H sums: lane q filters window row q at its three output columns (FilterH: the sum over the
    // taps of window columns cc .. cc + FW - 1; three chains, each in tap order).  Rows are N (odd)
    // words apart: no bank conflicts.
    if (lane < N) {
        const float* p = &s.win[lane * N];
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int t = 0; t < N; t++) {
            const float e = p[t];
            if (t < FW) a0 = fma_(e, taps.k[t], a0);
            if (t >= 1 && t - 1 < FW) a1 = fma_(e, taps.k[t - 1], a1);
            if (t >= 2) a2 = fma_(e, taps.k[t - 2], a2);
        }
        s.hs[3 * lane] = a0;
        s.hs[3 * lane + 1] = a1;
        s.hs[3 * lane + 2] = a2;
    }
    asm volatile("" ::: "memory");
    // V sums: output row r uses H rows r .. r + FW - 1
    if (lane < 9) {
        const float* p = &s.hs[lane];   // 3 r + cc
        float a = 0.f;
#pragma unroll
        for (int t = 0; t < FW; t++) a = fma_(p[3 * t], taps.k[t], a);
        s.top[lane] = a;
    }
    asm volatile("" ::: "memory");
}

// f(std::integral_constant<int, FW>{}) for the level filter's width (odd, 5 .. 33: sift_params.h)
template <class F>
inline bool top_level_dispatch(int fw, F&& f) {
    switch (fw) {
#define SGK_TOPFW(FW) case FW: f(std::integral_constant<int, FW>{}); return true;
        SGK_TOPFW(5) SGK_TOPFW(7) SGK_TOPFW(9) SGK_TOPFW(11) SGK_TOPFW(13) SGK_TOPFW(15) SGK_TOPFW(17)
        SGK_TOPFW(19) SGK_TOPFW(21) SGK_TOPFW(23) SGK_TOPFW(25) SGK_TOPFW(27) SGK_TOPFW(29)
        SGK_TOPFW(31) SGK_TOPFW(33)
#undef SGK_TOPFW
        default: return false;
    }
}

}  // namespace
}  // namespace sgk
