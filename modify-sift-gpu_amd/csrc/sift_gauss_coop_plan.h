// sift_gauss_coop_plan.h -- strip geometry of the paired Gaussian's cooperative form (k_gauss_duo
// with COOP, sift_gauss_duo.hip).  No HIP include: the kernel's geometry, its
// launcher and the CPU check (tests/abi/duo_coop_plan_check.cpp) all use these functions.
//
// A workgroup of 4 waves shares one row of kRow = 512 mid columns (level k + 1, in LDS): wave w
// computes the 128 mid columns [m0, m0 + 128), m0 = xs - MOFF + 128 w, of the strip that starts
// at output column xs = strip * SWG, and stage B of wave w reads the mid columns of its own
// outputs [xs + 128 w, xs + 128 w + 2 nb) -- RB columns to each side of them, some in the
// neighbouring waves' blocks.  SWG = 480 output columns per strip for every compiled pair.
#pragma once

namespace sgk {
namespace coop {

constexpr int kWaves = 4;                      // waves of a workgroup
constexpr int kWaveCols = 128;                 // mid columns of a wave (2 per lane)
constexpr int kRow = kWaves * kWaveCols;       // mid columns of the shared row
constexpr int kStripAlign = 32;                // strips start on 128-B lines

// mid column of a wave's lane 0 = its first output column - MOFF (even), as DuoGeom
constexpr int moff(int fwb) { return fwb / 2 + ((fwb / 2) & 1); }
// output columns of a strip
constexpr int swg(int fwb) { return (kRow - 2 * moff(fwb)) / kStripAlign * kStripAlign; }
constexpr int strips(int W, int fwb) { return (W + swg(fwb) - 1) / swg(fwb); }
// output columns of a per-wave strip (DuoGeom::SW)
constexpr int sw_wave(int fwb) { return (kWaveCols - 2 * moff(fwb)) / kStripAlign * kStripAlign; }

// the plan rule: the form that issues fewer lane-columns for a row of W columns (the cooperative
// one at 1920, 960 and 480 columns, the per-wave one at 240)
constexpr bool fewer_lane_columns(int W, int fwb) {
    return strips(W, fwb) * kRow < (W + sw_wave(fwb) - 1) / sw_wave(fwb) * kWaveCols;
}

struct Wave {
    int xs;            // the strip's first output column
    int x0;            // the wave's first output column (stage B), xs + 128 w
    int m0;            // the wave's first mid column, x0 - MOFF: lane l holds m0 + 2 l, + 1
    int nb;            // stage B lanes: lane l < nb holds output columns x0 + 2 l, + 1
    int own_lo, own_hi;   // level k + 1 columns this wave stores: [own_lo, own_hi) (inside the image)
    bool outside;      // every mid column >= W: the wave only keeps the workgroup's barriers
    bool left, right;  // some mid column < 0 / >= W: those lanes take column 0 / W - 1 (clamp)
    int l_left;        // lane holding mid column 0 (its first column)
    int l_right;       // lane holding mid column W - 1 (its second column)
    int spill;         // lanes l < spill also write column W - 1's value into the next wave's
                       // block, float4 l (columns m0 + 128 + 2 l, + 1): the clamped columns up to
                       // W - 1 + MOFF that lie past this wave's block
};

// W: the level's width (a multiple of 4, >= 8), fwb: the second filter's width
constexpr Wave wave_plan(int W, int fwb, int strip, int w) {
    const int M = moff(fwb), S = swg(fwb);
    Wave v{};
    v.xs = strip * S;
    v.x0 = v.xs + kWaveCols * w;
    v.m0 = v.x0 - M;
    const int nb = (S - kWaveCols * w) / 2;
    v.nb = nb > kWaveCols / 2 ? kWaveCols / 2 : nb;
    const int lo = v.m0 > v.xs ? v.m0 : v.xs;
    int hi = v.m0 + kWaveCols < v.xs + S ? v.m0 + kWaveCols : v.xs + S;
    hi = hi < W ? hi : W;
    v.own_lo = lo;
    v.own_hi = hi > lo ? hi : lo;
    v.outside = v.m0 >= W;
    v.left = v.m0 < 0;
    v.right = !v.outside && W <= v.m0 + kWaveCols;   // the wave that holds column W - 1
    v.l_left = v.left ? (-v.m0) >> 1 : 0;
    v.l_right = v.right ? (W - 2 - v.m0) >> 1 : 0;
    int sp = v.right && w + 1 < kWaves ? (W + M - (v.m0 + kWaveCols)) / 2 : 0;
    v.spill = sp < 0 ? 0 : sp;
    return v;
}

}  // namespace coop
}  // namespace sgk
