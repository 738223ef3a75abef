// Stand-alone check of the Gaussian pyramid's launch planner (csrc/sift_pyramid_plan.h, no HIP):
// built with -fsanitize=address,undefined by tests/test_pyramid_plan.py.  The level lists come
// from the real parameter code (sift_params.h: make_schedule / make_filter give the filter
// widths, make_octaves the geometry); the support queries are the header's tables of compiled
// width combinations plus the geometry the launchers ask for (w % 4 == 0, w, h >= 8, an even
// width whose half is the next octave's padded width, an even height where level k + 1 of a pair
// is the decimated one).
//   a. Invariants of every plan over shapes x -d x rules: each level in exactly one launch; a
//      level's input written by a strictly earlier launch, or by an earlier level of the same
//      paired / three-level / tile-duo launch; multi-level launches only where the query says
//      yes, none with pairing off or the workgroup strip kernel forced; the side-stream layout's
//      event marks on (0, kds) and (1, 1), in that order, and only octaves >= 1 on the side stream.
//   b. The exact launch lists of the three benchmark shapes under the shipped rules.
// `pyramid_plan_check print` prints those three lists instead.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sift_params.h"
#include "sift_pyramid_plan.h"

using namespace sgpyr;

struct Pyramid {
    std::vector<LevelDesc> lv;
    std::vector<sgp::Octave> oct;
    int kds = 0;
    int index(int o, int k) const {
        for (size_t i = 0; i < lv.size(); i++)
            if (lv[i].o == o && lv[i].k == k) return (int)i;
        return -1;
    }
    // the level filter that writes level i's input (-1: the image)
    int input(int i) const {
        const LevelDesc& e = lv[i];
        if (e.k >= 2 || (e.k == 1 && e.o == 0)) return index(e.o, e.k - 1);
        return e.k == 1 ? index(e.o - 1, kds) : -1;
    }
};

// n u8 images of w x h, -no octaves (< 1: from the size), -d d; zero: a one-stream extract,
// whose first level launch carries the zero job
static Pyramid make_pyramid(int n, int w, int h, int octaves, int d, bool zero) {
    sgp::Options o;
    o.dog_level_num = d;
    o.octave_num = octaves;
    const sgp::Schedule S = sgp::make_schedule(o);
    Pyramid p;
    p.oct = sgp::make_octaves(w, h, octaves, 0);
    p.kds = S.level_ds - S.level_min;
    float taps[sgp::kMaxFilterWidth];
    const int noct = (int)p.oct.size();
    for (int oi = 0; oi < noct; oi++)
        for (int k = oi == 0 ? 0 : 1; k < S.level_num; k++) {
            const float sigma = k == 0 ? S.initial_smooth : S.sigma[k - 1];
            const int fw = sgp::make_filter(sigma, o.filter_width_factor, taps);
            p.lv.push_back(LevelDesc{oi, k, fw, p.oct[oi].wa, p.oct[oi].h, n,
                                     oi + 1 < noct && k == p.kds, oi == 0 && k == 0,
                                     zero && oi == 0 && k == 0});
        }
    return p;
}

struct Support {
    const Pyramid& p;
    bool next(int i, int j) const {
        return j == i + 1 && p.lv[i].o == p.lv[j].o && p.lv[j].k == p.lv[i].k + 1;
    }
    bool strip_geometry(int i) const {
        return p.lv[i].w % 4 == 0 && p.lv[i].w >= 8 && p.lv[i].h >= 8;
    }
    bool halves(int i) const {   // the decimation of level i is the next octave's level 0
        const LevelDesc& e = p.lv[i];
        return e.ds && e.w % 2 == 0 && p.oct[e.o + 1].wa * 2 == e.w;
    }
    bool tile(int i) const {
        const LevelDesc& e = p.lv[i];
        return e.fw >= 5 && e.fw <= 33 && (e.fw & 1) && e.w % 4 == 0 && e.w >= 4 && e.h >= 1;
    }
    bool tile_duo(int i, int j) const {
        const LevelDesc &a = p.lv[i], &b = p.lv[j];
        return tile(i) && tile(j) && next(i, j) && !b.u8 && !b.zero &&
               tile_duo_widths(a.fw, b.fw, a.u8, a.ds, b.ds);
    }
    bool duo(int i, int j) const {
        const LevelDesc &a = p.lv[i], &b = p.lv[j];
        return next(i, j) && duo_widths(a.fw, b.fw, a.u8, a.ds, b.ds) && !b.u8 && !b.zero &&
               (a.u8 || !a.zero) && strip_geometry(i) && (!b.ds || halves(j)) &&
               (!a.ds || (halves(i) && a.h % 2 == 0));
    }
    bool trio(int i, int j, int l) const {
        const LevelDesc &a = p.lv[i], &b = p.lv[j], &c = p.lv[l];
        return next(i, j) && next(j, l) && trio_widths(a.fw, b.fw, c.fw) && halves(l) && !a.ds &&
               !b.ds && !a.u8 && !a.zero && strip_geometry(i);
    }
};

static const char* kKindName[kKinds] = {"level", "tile", "two", "tile_two", "tile_duo",
                                        "tile_duo_one", "duo", "trio"};
static const char* g_what = "";

#define CHECK(c)                                                                     \
    do {                                                                             \
        if (!(c)) {                                                                  \
            std::printf("FAILED %s (%s, entry %d) line %d\n", #c, g_what, e, __LINE__); \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

static void check_invariants(const Pyramid& p, const Rules& R, const Plan& P) {
    const Support sup{p};
    const int n = (int)p.lv.size();
    std::vector<int> entry_of(n, -1);
    const bool pairing_off = R.duo_off || (!SGK_DUO_DEFAULT && !R.duo_always && !R.duo_on) ||
                             R.wave_rows < 0;
    int e = 0, rec_at = -1, wait_at = -1;
    for (; e < (int)P.launches.size(); e++) {
        const Launch& l = P.launches[e];
        CHECK(l.kind >= 0 && l.kind < kKinds);
        const int m = kind_ops(l.kind);
        // the levels of a paired, three-level or tile-duo launch that may read an earlier level
        // of the same launch: all but the first (the tile duo beside a single tile: only op[1])
        const bool chain = l.kind == kDuo || l.kind == kTrio || l.kind == kTileDuo || l.kind == kTileDuoOne;
        for (int j = 0; j < 3; j++) {
            CHECK((j < m) == (l.op[j] >= 0) && l.op[j] < n);
            if (j >= m) continue;
            const int i = l.op[j];
            CHECK(entry_of[i] < 0);   // in exactly one launch
            const int in = p.input(i);
            if (in >= 0) {
                const bool same = chain && j >= 1 && !(l.kind == kTileDuoOne && j == 2) && in == l.op[j - 1];
                CHECK(same || (entry_of[in] >= 0 && entry_of[in] < e));
            }
            CHECK(l.side == (P.side && p.lv[i].o >= 1));
        }
        for (int j = 0; j < m; j++) entry_of[l.op[j]] = e;
        if (l.kind == kDuo) CHECK(sup.duo(l.op[0], l.op[1]));
        if (l.kind == kTrio) CHECK(sup.trio(l.op[0], l.op[1], l.op[2]));
        if (l.kind == kTileDuo || l.kind == kTileDuoOne) CHECK(sup.tile_duo(l.op[0], l.op[1]));
        if (l.kind == kTile || l.kind == kTileTwo) CHECK(sup.tile(l.op[0]));
        if (l.kind == kTileTwo) CHECK(sup.tile(l.op[1]));
        if (l.kind == kTileDuoOne) CHECK(sup.tile(l.op[2]));
        if (l.kind == kDuo || l.kind == kTrio) CHECK(!pairing_off && P.trash);
        if (l.kind != kLevel && l.kind != kTwo && l.kind != kDuo && l.kind != kTrio)
            CHECK(R.wave_rows == 0 && !R.long_bands && !R.tiles_off);
        if (l.rec_ds) {
            CHECK(P.side && rec_at < 0 && p.lv[l.op[0]].o == 0 && p.lv[l.op[0]].k == p.kds);
            rec_at = e;
        }
        if (l.wait_ds) {
            CHECK(P.side && wait_at < 0 && rec_at >= 0 && p.lv[l.op[0]].o == 1 && p.lv[l.op[0]].k == 1);
            wait_at = e;
        }
    }
    e = -1;
    for (int i = 0; i < n; i++) CHECK(entry_of[i] >= 0);
    CHECK(P.side == (R.side_stream && !R.serial && p.oct.size() > 1));
    CHECK((rec_at >= 0) == P.side && (wait_at >= 0) == P.side);
}

struct Entry { int kind, o0, k0, o1, k1, o2, k2; };

static void print_plan(const char* name, const Pyramid& p, const Plan& P) {
    std::printf("%s: %zu entries\n", name, P.launches.size());
    for (const Launch& l : P.launches) {
        std::printf("    {k%s", kKindName[l.kind]);
        for (int j = 0; j < 3; j++)
            if (l.op[j] >= 0) std::printf(", %d, %d", p.lv[l.op[j]].o, p.lv[l.op[j]].k);
            else std::printf(", -1, -1");
        std::printf("},\n");
    }
}

static void check_pinned(const char* name, const Pyramid& p, const Plan& P, const Entry* want, size_t n) {
    g_what = name;
    int e = -1;
    CHECK(P.launches.size() == n);
    for (e = 0; e < (int)n; e++) {
        const Launch& l = P.launches[e];
        const int got[7] = {l.kind,
                            p.lv[l.op[0]].o, p.lv[l.op[0]].k,
                            l.op[1] < 0 ? -1 : p.lv[l.op[1]].o, l.op[1] < 0 ? -1 : p.lv[l.op[1]].k,
                            l.op[2] < 0 ? -1 : p.lv[l.op[2]].o, l.op[2] < 0 ? -1 : p.lv[l.op[2]].k};
        const int exp[7] = {want[e].kind, want[e].o0, want[e].k0, want[e].o1, want[e].k1, want[e].o2, want[e].k2};
        CHECK(std::memcmp(got, exp, sizeof got) == 0);
        CHECK(!l.side && !l.wait_ds && !l.rec_ds);
    }
}

enum { klevel = kLevel, ktile = kTile, ktwo = kTwo, ktile_two = kTileTwo, ktile_duo = kTileDuo,
       ktile_duo_one = kTileDuoOne, kduo = kDuo, ktrio = kTrio };

// The C3 shard, 128 x 1920x1080 u8, -no 4 -d 3 (kds = 3; op (o, k) in slot 3 o + k).  Octave 0
// (1,061 MB a level) takes the plan from its end: the u8 pair (0, 1), (2, 3) with level 3
// decimated, (4, 5) in slots 1, 3, 5.  Octave 1 (265 MB) pairs (1, 2) from the front (slot 5) and
// runs levels 3, 4, 5 singly (slots 6-8); octave 2 singly (slots 7-11), octave 3 (16.6 MB: under
// the 16 MiB tile bound) singly and tiled (slots 10-14).  Slots 7 and 8 hold two lean singles
// (one entry each), slots 10 and 11 a lean and a tiled one (two entries each).
static const Entry kC3[] = {
    {kduo, 0, 0, 0, 1, -1, -1},
    {kduo, 0, 2, 0, 3, -1, -1},
    {kduo, 0, 4, 0, 5, -1, -1},
    {kduo, 1, 1, 1, 2, -1, -1},
    {klevel, 1, 3, -1, -1, -1, -1},
    {ktwo, 1, 4, 2, 1, -1, -1},
    {ktwo, 1, 5, 2, 2, -1, -1},
    {klevel, 2, 3, -1, -1, -1, -1},
    {klevel, 2, 4, -1, -1, -1, -1},
    {ktile, 3, 1, -1, -1, -1, -1},
    {klevel, 2, 5, -1, -1, -1, -1},
    {ktile, 3, 2, -1, -1, -1, -1},
    {ktile, 3, 3, -1, -1, -1, -1},
    {ktile, 3, 4, -1, -1, -1, -1},
    {ktile, 3, 5, -1, -1, -1, -1},
};

// C2, one 1920x1080 image, -no 4 -d 3: every level cache-resident, so tiled; the diagonal
// schedule, octave o's levels 4, 5 beside octave o + 1's levels 1, 2.
static const Entry kC2[] = {
    {ktile, 0, 0, -1, -1, -1, -1},
    {ktile, 0, 1, -1, -1, -1, -1},
    {ktile, 0, 2, -1, -1, -1, -1},
    {ktile, 0, 3, -1, -1, -1, -1},
    {ktile_two, 0, 4, 1, 1, -1, -1},
    {ktile_two, 0, 5, 1, 2, -1, -1},
    {ktile, 1, 3, -1, -1, -1, -1},
    {ktile_two, 1, 4, 2, 1, -1, -1},
    {ktile_two, 1, 5, 2, 2, -1, -1},
    {ktile, 2, 3, -1, -1, -1, -1},
    {ktile_two, 2, 4, 3, 1, -1, -1},
    {ktile_two, 2, 5, 3, 2, -1, -1},
    {ktile, 3, 3, -1, -1, -1, -1},
    {ktile, 3, 4, -1, -1, -1, -1},
    {ktile, 3, 5, -1, -1, -1, -1},
};

// C4, 16 x 4096x4096, -no 6 -d 3: octave 0 (1,074 MB a level) is wider than SGK_DUO_PLAN_MAXW
// columns, so it does not take the plan from its end: level 0, the pairs (1, 2) and (3, 4) with
// level 3's decimation, level 5.  Octave 1 (268 MB) as C3's; octaves 3-5 (16.8, 4.2, 1 MB) tiled.
static const Entry kC4[] = {
    {klevel, 0, 0, -1, -1, -1, -1},
    {kduo, 0, 1, 0, 2, -1, -1},
    {kduo, 0, 3, 0, 4, -1, -1},
    {kduo, 1, 1, 1, 2, -1, -1},
    {klevel, 0, 5, -1, -1, -1, -1},
    {klevel, 1, 3, -1, -1, -1, -1},
    {ktwo, 1, 4, 2, 1, -1, -1},
    {ktwo, 1, 5, 2, 2, -1, -1},
    {klevel, 2, 3, -1, -1, -1, -1},
    {klevel, 2, 4, -1, -1, -1, -1},
    {ktile, 3, 1, -1, -1, -1, -1},
    {klevel, 2, 5, -1, -1, -1, -1},
    {ktile, 3, 2, -1, -1, -1, -1},
    {ktile, 3, 3, -1, -1, -1, -1},
    {ktile_two, 3, 4, 4, 1, -1, -1},
    {ktile_two, 3, 5, 4, 2, -1, -1},
    {ktile, 4, 3, -1, -1, -1, -1},
    {ktile_two, 4, 4, 5, 1, -1, -1},
    {ktile_two, 4, 5, 5, 2, -1, -1},
    {ktile, 5, 3, -1, -1, -1, -1},
    {ktile, 5, 4, -1, -1, -1, -1},
    {ktile, 5, 5, -1, -1, -1, -1},
};

int main(int argc, char** argv) {
    const bool print = argc > 1 && !std::strcmp(argv[1], "print");
    Plan P;   // reused, as the library reuses a part's
    if (!print) {
        // a. the invariants
        const int shapes[][4] = {{2, 16, 16, 0},     {3, 203, 97, 0},    {1, 104, 33, 0},
                                 {2, 296, 1203, 0},  {2, 64, 64, 0},     {2, 1920, 1080, 0},
                                 {2, 16, 16, 3},     {3, 203, 97, 3},    {2, 296, 1203, 5},
                                 {128, 1920, 1080, 4}, {1, 1920, 1080, 4}, {16, 4096, 4096, 6}};
        long long plans = 0, seen[kKinds] = {0};
        char what[160];
        g_what = what;
        for (const auto& s : shapes)
            for (int d = 3; d <= 4; d++)
                for (int stream = 0; stream < 3; stream++) {   // one stream, side stream, serial
                    const Pyramid p = make_pyramid(s[0], s[1], s[2], s[3], d, stream != 1);
                    const Support sup{p};
                    for (int duo = 0; duo < 3; duo++)          // shipped rule, off, always
                    for (int pairs = 0; pairs < 2; pairs++)
                    for (int trio = 0; trio < 3; trio++)
                    for (int tiles = 0; tiles < 3; tiles++)    // shipped rule, off, always
                    for (int tile_duo = 0; tile_duo < 2; tile_duo++)
                    for (int rows = 0; rows < 3; rows++) {
                        Rules R;
                        R.kds = p.kds;
                        R.side_stream = stream == 1;
                        R.serial = stream == 2;
                        R.duo_off = duo == 1;
                        R.duo_always = duo == 2;
                        R.duo_plan = pairs;
                        R.trio_mode = trio;
                        R.tiles_off = tiles == 1;
                        R.tiles_always = tiles == 2;
                        R.tile_duo = tile_duo != 0;
                        R.wave_rows = rows == 0 ? 0 : (rows == 1 ? -1 : 8);
                        std::snprintf(what, sizeof what,
                                      "%d x %dx%d -no %d -d %d stream %d duo %d pairs %d trio %d "
                                      "tiles %d tile_duo %d rows %d", s[0], s[1], s[2], s[3], d,
                                      stream, duo, pairs, trio, tiles, tile_duo, R.wave_rows);
                        plan_pyramid(p.lv.data(), (int)p.lv.size(), R, sup, P);
                        check_invariants(p, R, P);
                        for (const Launch& l : P.launches) seen[l.kind]++;
                        plans++;
                    }
                }
        for (int k = 0; k < kKinds; k++)   // the sweep reaches every kind of launch
            if (!seen[k]) {
                std::printf("FAILED no plan of the sweep has a %s launch\n", kKindName[k]);
                return 1;
            }
        std::printf("%lld plans hold the invariants\n", plans);
    }
    // b. the benchmark shapes under the shipped rules (one stream: the zero job on (0, 0))
    struct Pinned { const char* name; int n, w, h, no; const Entry* want; size_t count; };
    const Pinned pinned[] = {
        {"C3 128 x 1920x1080 -no 4", 128, 1920, 1080, 4, kC3, sizeof kC3 / sizeof kC3[0]},
        {"C2 1 x 1920x1080 -no 4", 1, 1920, 1080, 4, kC2, sizeof kC2 / sizeof kC2[0]},
        {"C4 16 x 4096x4096 -no 6", 16, 4096, 4096, 6, kC4, sizeof kC4 / sizeof kC4[0]},
    };
    for (const Pinned& c : pinned) {
        const Pyramid p = make_pyramid(c.n, c.w, c.h, c.no, 3, true);
        Rules R;
        R.kds = p.kds;
        plan_pyramid(p.lv.data(), (int)p.lv.size(), R, Support{p}, P);
        if (print) print_plan(c.name, p, P);
        else check_pinned(c.name, p, P, c.want, c.count);
    }
    if (!print) std::printf("pyramid plan ok\n");
    return 0;
}
