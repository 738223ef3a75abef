// Stand-alone check of the paired Gaussian's cooperative strip plan (csrc/sift_gauss_coop_plan.h,
// no HIP): built with -fsanitize=address,undefined by tests/test_duo_coop_plan.py.  For every level
// width that is a multiple of 4 from 8 to 4,100 and every compiled filter pair it replays what the
// kernel does with the plan -- each wave writes its 128 mid columns (the lanes outside the image
// the clamped edge column) and its spill into the shared 512-column row, then stage B reads -- and
// asserts that
//   * each output column is owned by exactly one (strip, wave, lane), and each level k + 1
//     column is stored by exactly one;
//   * each mid column a stage B lane reads was written exactly once and holds the column the
//     clamp-to-edge rule names;
//   * no range leaves the 512-column row;
//   * strip rows start on multiples of 32 columns.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sift_gauss_coop_plan.h"

using namespace sgk::coop;

#define CHECK(c)                                                                             \
    do {                                                                                     \
        if (!(c)) {                                                                          \
            std::printf("FAILED %s (W %d, FWB %d, strip %d, wave %d) line %d\n", #c, W, fwb, \
                        s, w, __LINE__);                                                     \
            std::exit(1);                                                                    \
        }                                                                                    \
    } while (0)

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

static void check(int W, int fwb) {
    const int RB = fwb / 2, M = moff(fwb), OB = M - RB, S = swg(fwb);
    int s = -1, w = -1;
    CHECK(M % 2 == 0 && M >= RB && S % kStripAlign == 0 && S + 2 * M <= kRow && S > 3 * kWaveCols);
    const int ns = strips(W, fwb);
    CHECK(ns >= 1 && (ns - 1) * S < W && ns * S >= W);
    std::vector<int> out_owner(W, 0), mid_owner(W, 0);
    for (s = 0; s < ns; s++) {
        // the shared row: which image column each float2 holds, and how often it was written
        std::vector<int> col(kRow, -1), writes(kRow, 0);
        bool live_before = true;
        for (w = 0; w < kWaves; w++) {
            const Wave v = wave_plan(W, fwb, s, w);
            CHECK(v.xs == s * S && v.xs % kStripAlign == 0 && v.x0 % kStripAlign == 0);
            CHECK(v.m0 == v.x0 - M && v.m0 % 2 == 0);
            const int base = v.m0 - (v.xs - M);   // the wave's first float2 of the row
            CHECK(base == kWaveCols * w && base + kWaveCols <= kRow);
            CHECK(v.nb >= 1 && v.nb <= kWaveCols / 2);
            CHECK(v.outside == (v.m0 >= W));
            if (v.outside) {   // and so is every wave after it
                live_before = false;
                CHECK(!v.left && !v.right && v.spill == 0 && v.own_lo == v.own_hi);
                continue;
            }
            CHECK(live_before);
            CHECK(v.spill >= 0 && 2 * v.spill <= M);
            if (v.left) CHECK(v.m0 + 2 * v.l_left == 0 && v.l_left < kWaveCols / 2);
            if (v.right) CHECK(v.m0 + 2 * v.l_right + 1 == W - 1 && v.l_right >= 0 && v.l_right < kWaveCols / 2);
            for (int l = 0; l < kWaveCols / 2; l++)
                for (int u = 0; u < 2; u++) {
                    const int c = v.m0 + 2 * l + u;
                    if (c < 0) CHECK(v.left);    // fix_edges: column 0's value
                    if (c >= W) CHECK(v.right);  // column W - 1's
                    col[base + 2 * l + u] = clampi(c, 0, W - 1);
                    writes[base + 2 * l + u]++;
                    if (c >= v.own_lo && c < v.own_hi) {
                        CHECK(c >= 0 && c < W && c >= v.xs && c < v.xs + S);
                        mid_owner[c]++;
                    }
                }
            if (v.spill > 0) {
                CHECK(v.right && w + 1 < kWaves && wave_plan(W, fwb, s, w + 1).outside);
                for (int l = 0; l < v.spill; l++)
                    for (int u = 0; u < 2; u++) {
                        const int j = base + kWaveCols + 2 * l + u;
                        CHECK(j < kRow && v.xs - M + j >= W);
                        col[j] = W - 1;
                        writes[j]++;
                    }
            }
        }
        for (w = 0; w < kWaves; w++) {
            const Wave v = wave_plan(W, fwb, s, w);
            // (a wave with mid columns inside the image and no output column reads nothing it stores)
            for (int l = 0; l < v.nb && !v.outside; l++) {
                const int e = v.x0 + 2 * l;
                if (e >= W) continue;
                CHECK(e + 1 < W && e >= v.xs && e + 1 < v.xs + S);
                out_owner[e]++;
                out_owner[e + 1]++;
                // H2: float2 kWaveCols w + 2 l + OB + m, m = 0 .. FWB: tap m of column e, m - 1 of e + 1
                for (int m = 0; m <= fwb; m++) {
                    const int j = kWaveCols * w + 2 * l + OB + m;
                    CHECK(j >= 0 && j < kRow);
                    CHECK(writes[j] == 1);
                    CHECK(col[j] == clampi(e - RB + m, 0, W - 1));
                }
            }
            if (v.outside) CHECK(v.x0 >= W);
        }
        for (int j = 0; j < kRow; j++) CHECK(writes[j] <= 1);
    }
    s = w = -1;
    for (int x = 0; x < W; x++) CHECK(out_owner[x] == 1 && mid_owner[x] == 1);
}

int main() {
    // the second widths of the compiled pairs (13, 11), (11, 13), (13, 17), (17, 21), (21, 25):
    // the plan depends on the pair through RB only
    const int fwbs[] = {11, 13, 17, 21, 25};
    for (int fwb : fwbs) {
        if (swg(fwb) != 480) {
            std::printf("FAILED swg(%d) = %d\n", fwb, swg(fwb));
            return 1;
        }
        for (int W = 8; W <= 4100; W += 4) check(W, fwb);
    }
    // the plan rule: fewer issued lane-columns at 1920, 960 and 480 columns, not at 240
    for (int fwb : fwbs)
        if (!fewer_lane_columns(1920, fwb) || !fewer_lane_columns(960, fwb) ||
            !fewer_lane_columns(480, fwb) || fewer_lane_columns(240, fwb)) {
            std::printf("FAILED plan rule (FWB %d)\n", fwb);
            return 1;
        }
    std::printf("duo coop plan ok\n");
    return 0;
}
