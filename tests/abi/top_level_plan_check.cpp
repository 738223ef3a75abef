// Stand-alone check of the pyramid planner (csrc/sift_pyramid_plan.h, no HIP) on level lists without
// the octaves' last level, built with -fsanitize=address,undefined by
// tests/test_top_level_plan.py; beside tests/abi/pyramid_plan_check.cpp, whose level lists,
// support queries and pinned dense plans it restates in short form.
//   * C3 (128 x 1920x1080, -no 4) and C4 (16 x 4096x4096, -no 6) geometry, -d 3, level 5 of every
//     octave left out: octave 0 pairs (0, 1), (2, 3) and leaves level 4 single from the end (a
//     forced end plan for C4, whose 4096 columns exceed SGK_DUO_PLAN_MAXW), and pairs (1, 2),
//     (3, 4) after a single level 0 from the front; no launch names level 5; every level is in
//     exactly one launch and after its input.
//   * The dense lists plan as before: octave 0's launches of C3 and C4 under the shipped rules.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sift_params.h"
#include "sift_pyramid_plan.h"

using namespace sgpyr;

struct Pyramid {
    std::vector<LevelDesc> lv;
    std::vector<sgp::Octave> oct;
    int kds = 0, nlev = 0;
    int index(int o, int k) const {
        for (size_t i = 0; i < lv.size(); i++)
            if (lv[i].o == o && lv[i].k == k) return (int)i;
        return -1;
    }
    int input(int i) const {   // the level filter that writes level i's input (-1: the image)
        const LevelDesc& e = lv[i];
        if (e.k >= 2 || (e.k == 1 && e.o == 0)) return index(e.o, e.k - 1);
        return e.k == 1 ? index(e.o - 1, kds) : -1;
    }
};

static Pyramid make_pyramid(int n, int w, int h, int octaves, int d, bool lazy) {
    sgp::Options o;
    o.dog_level_num = d;
    o.octave_num = octaves;
    const sgp::Schedule S = sgp::make_schedule(o);
    Pyramid p;
    p.oct = sgp::make_octaves(w, h, octaves, 0);
    p.kds = S.level_ds - S.level_min;
    p.nlev = S.level_num;
    float taps[sgp::kMaxFilterWidth];
    const int noct = (int)p.oct.size();
    for (int oi = 0; oi < noct; oi++)
        for (int k = oi == 0 ? 0 : 1; k < S.level_num - (lazy ? 1 : 0); k++) {
            const float sigma = k == 0 ? S.initial_smooth : S.sigma[k - 1];
            const int fw = sgp::make_filter(sigma, o.filter_width_factor, taps);
            p.lv.push_back(LevelDesc{oi, k, fw, p.oct[oi].wa, p.oct[oi].h, n,
                                     oi + 1 < noct && k == p.kds, oi == 0 && k == 0,
                                     oi == 0 && k == 0});
        }
    return p;
}

struct Support {
    const Pyramid& p;
    bool next(int i, int j) const {
        return j == i + 1 && p.lv[i].o == p.lv[j].o && p.lv[j].k == p.lv[i].k + 1;
    }
    bool strip_geometry(int i) const { return p.lv[i].w % 4 == 0 && p.lv[i].w >= 8 && p.lv[i].h >= 8; }
    bool halves(int i) const {
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

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s (%s) line %d\n", #c, g_what, __LINE__); \
            std::exit(1);                                               \
        }                                                               \
    } while (0)
static const char* g_what = "";

struct Entry { int kind, k0, k1; };   // a launch of octave 0: kind, levels written (-1: none)

// octave 0's launches in issue order, and the invariants of the whole plan
static std::vector<Entry> octave0(const Pyramid& p, const Plan& P, bool lazy) {
    std::vector<int> entry_of(p.lv.size(), -1);
    std::vector<Entry> out;
    for (size_t e = 0; e < P.launches.size(); e++) {
        const Launch& l = P.launches[e];
        const int m = kind_ops(l.kind);
        const bool chain = l.kind == kDuo || l.kind == kTrio || l.kind == kTileDuo || l.kind == kTileDuoOne;
        for (int j = 0; j < m; j++) {
            const int i = l.op[j];
            CHECK(i >= 0 && i < (int)p.lv.size() && entry_of[i] < 0);
            if (lazy) CHECK(p.lv[i].k != p.nlev - 1);   // no launch writes the last level
            const int in = p.input(i);
            if (in >= 0) {
                const bool same = chain && j >= 1 && !(l.kind == kTileDuoOne && j == 2) && in == l.op[j - 1];
                CHECK(same || (entry_of[in] >= 0 && entry_of[in] < (int)e));
            }
        }
        for (int j = 0; j < m; j++) entry_of[l.op[j]] = (int)e;
        // (a diagonal launch can hold a level of octave 0 beside one of octave 1: kTwo)
        Entry en{l.kind, -1, -1};
        int q = 0;
        for (int j = 0; j < m; j++)
            if (p.lv[l.op[j]].o == 0) (q++ == 0 ? en.k0 : en.k1) = p.lv[l.op[j]].k;
        if (q) out.push_back(en);
    }
    for (int e : entry_of) CHECK(e >= 0);
    return out;
}

static void expect(const std::vector<Entry>& got, const std::vector<Entry>& want) {
    CHECK(got.size() == want.size());
    for (size_t i = 0; i < got.size(); i++)
        CHECK(got[i].kind == want[i].kind && got[i].k0 == want[i].k0 && got[i].k1 == want[i].k1);
}

int main() {
    Plan P;
    struct Shape { const char* name; int n, w, h, no; bool wide; };
    const Shape shapes[] = {{"C3 128 x 1920x1080 -no 4", 128, 1920, 1080, 4, false},
                            {"C4 16 x 4096x4096 -no 6", 16, 4096, 4096, 6, true}};
    // level 4 shares its slot with octave 1's level 1 in the diagonal schedule; octave 1's (1, 2)
    // pairs on these shapes, so level 4 of octave 0 stays alone in its launch
    const std::vector<Entry> end_lazy = {{kDuo, 0, 1}, {kDuo, 2, 3}, {kLevel, 4, -1}};
    const std::vector<Entry> front_lazy = {{kLevel, 0, -1}, {kDuo, 1, 2}, {kDuo, 3, 4}};
    const std::vector<Entry> end_dense = {{kDuo, 0, 1}, {kDuo, 2, 3}, {kDuo, 4, 5}};
    const std::vector<Entry> front_dense = {{kLevel, 0, -1}, {kDuo, 1, 2}, {kDuo, 3, 4}, {kLevel, 5, -1}};
    for (const Shape& s : shapes) {
        g_what = s.name;
        for (int lazy = 0; lazy < 2; lazy++) {
            const Pyramid p = make_pyramid(s.n, s.w, s.h, s.no, 3, lazy != 0);
            CHECK(p.nlev == 6);
            CHECK((int)p.lv.size() == (p.nlev - lazy) * (int)p.oct.size() - ((int)p.oct.size() - 1));
            for (int pairs = 0; pairs < 2; pairs++) {
                Rules R;
                R.kds = p.kds;
                R.duo_plan = pairs;
                plan_pyramid(p.lv.data(), (int)p.lv.size(), R, Support{p}, P);
                const std::vector<Entry> got = octave0(p, P, lazy != 0);
                // the shipped rules take the end plan only up to SGK_DUO_PLAN_MAXW columns
                const bool end = pairs == kPairsEnd && !s.wide;
                expect(got, lazy ? (end ? end_lazy : front_lazy) : (end ? end_dense : front_dense));
            }
            if (s.wide && lazy) {   // the end plan of the wide shape: forced (duo_always)
                Rules R;
                R.kds = p.kds;
                R.duo_plan = kPairsEnd;
                R.duo_always = true;
                plan_pyramid(p.lv.data(), (int)p.lv.size(), R, Support{p}, P);
                // (with every pair forced, octave 1 also pairs from its end and its level 1 is
                // single: it shares level 4's slot and launch)
                expect(octave0(p, P, true), {{kDuo, 0, 1}, {kDuo, 2, 3}, {kTwo, 4, -1}});
            }
        }
    }
    std::printf("top level plan ok\n");
    return 0;
}
