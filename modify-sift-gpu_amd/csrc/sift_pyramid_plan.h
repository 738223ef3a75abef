// sift_pyramid_plan.h -- the launch schedule of the Gaussian pyramid.  No HIP
// include: the library (enqueue_part, sgpu_extract.cpp) and the CPU check
// (tests/abi/pyramid_plan_check.cpp) both run plan_pyramid(), a pure function from what the rules
// read -- the level filters' geometry, the rule switches, and which level combinations have a
// compiled kernel -- to the ordered list of launches.  The library walks that list; nothing else
// decides what the pyramid launches.  The tables of compiled width combinations at the end are
// the ones gauss_duo_supported / gauss_trio_supported / gauss_tile_duo_supported use.
#pragma once
#include <vector>

// paired-level Gaussian launches in the shipped schedule (1), or only when asked for by
// SGPU_DUO=on / the debug flags (0)
#ifndef SGK_DUO_DEFAULT
#define SGK_DUO_DEFAULT 1
#endif
// paired-level Gaussian launches only for levels of at least this many MB (smaller ones stay in
// the Infinity Cache between launches and are latency-bound: one level per launch, 1-chunk bands)
#ifndef SGK_DUO_MIN_MB
#define SGK_DUO_MIN_MB 128
#endif
// paired levels: (11, 13) from SGK_DUO_MIN_MB; (17, 21) with the decimation, whose arithmetic
// makes it latency-bound on smaller levels, from SGK_DUO_WIDE_MIN_MB (128 x 1080p: octave 0
// 903 us against 1,052 for two launches; octave 1 309 against ~270, tests/diag/r05i.sh); (21, 25)
// only by SGPU_DUO_WIDE=1 (1,016 us against ~1,050, and it would take level 4 from (17, 21))
#ifndef SGK_DUO_WIDE_MIN_MB
#define SGK_DUO_WIDE_MIN_MB 512
#endif
// the octave's level pairs taken from its end ((4, 5), (2, 3) with the decimation, (0, 1)): 1,
// or from its front: 0 (Rules::duo_plan); from the end only on levels of at most
// SGK_DUO_PLAN_MAXW columns (128 x 1080p: octave 0 2.575 vs 2.613 ms; 16 x 4096^2 (C4): 2.87 vs
// 2.80 ms -- every paired-level launch of the 4096-column levels runs ~10 % slower than on 1920
// columns)
#ifndef SGK_DUO_PLAN
#define SGK_DUO_PLAN 1
#endif
#ifndef SGK_DUO_PLAN_MAXW
#define SGK_DUO_PLAN_MAXW 2048
#endif
// three levels per launch (k_gauss_trio: widths (11, 13, 17), the third decimated into the next
// octave) for levels of at least this many MB; the octave's remaining (21, 25) pair then runs as a
// paired-level launch
#ifndef SGK_TRIO_MIN_MB
#define SGK_TRIO_MIN_MB 512
#endif
// 2-D tile launches (k_gauss_tile, sift_gauss_tile.hip) for levels of at most this many MB (one
// 1080p image: 8.3 MB at octave 0), where the wave walk of k_gauss_lean is latency-bound
#ifndef SGK_TILE_MB
#define SGK_TILE_MB 16
#endif

namespace sgpyr {

// One level filter as the rules see it: op (o, k) filters level k-1 of octave o into level k (op
// (0, 0) smooths the input into level 0).
struct LevelDesc {
    int o, k;        // octave, level written
    int fw;          // filter width
    int w, h, batch; // the level: w (padded) x h pixels, batch images
    bool ds;         // also writes its 2x decimation, level 0 of octave o + 1
    bool u8;         // reads the u8 input
    bool zero;       // carries the zero job (the first launch of a one-stream extract)
};

constexpr int kTrioOff = 0, kTrioOn = 1, kTrioAlways = 2;   // SGPU_TRIO_* of sgpu.h
constexpr int kPairsFront = 0, kPairsEnd = 1;               // SGPU_PAIRS_*

struct Rules {
    int kds = 0;                  // the level whose launch also decimates (level_ds - level_min)
    bool side_stream = false;     // the part has a side stream for octaves >= 1 (not one_stream)
    bool serial = false;          // SGPU_DEBUG_PYR_SERIAL: octave by octave on one stream
    int wave_rows = 0;            // < 0: k_gauss_pk2; > 0: forced band height; 0: the shipped rule
    bool long_bands = false;      // SGPU_DEBUG_GAUSS_LONG_BANDS
    bool tiles_off = false;       // SGPU_DEBUG_GAUSS_TILE_OFF
    bool tiles_always = false;    // SGPU_DEBUG_GAUSS_TILE_ALWAYS
    int tile_mb = SGK_TILE_MB;    // levels of at most this many MB are tiled
    bool tile_duo = false;        // SGPU_TILE_DUO=on: the tile-duo schedule when every level is tiled
    bool duo_off = false;         // SGPU_DEBUG_DUO_OFF
    bool duo_always = false;      // SGPU_DEBUG_DUO_ALWAYS
    bool duo_on = false;          // SGPU_DUO=on (matters only with SGK_DUO_DEFAULT 0)
    bool duo_wide = false;        // SGPU_DUO_WIDE=1: also the (21, 25) pairs
    bool duo_u8 = false;          // SGPU_DUO_U8=1: the u8 ingest pair (13, 11) from the front
    int trio_mode = kTrioOff;     // three-level launches: kTrio*
    int duo_plan = SGK_DUO_PLAN;  // kPairs*: pairs from the octave's end or front
};

enum Kind : int {
    kLevel = 0,     // one level, wave kernels (k_gauss_lean, or k_gauss_pk2 with wave_rows < 0)
    kTile,          // one level in 2-D tiles
    kTwo,           // two independent levels (launch_gauss_two: 1 or 2 kernel launches)
    kTileTwo,       // two independent tiled levels (launch_gauss_tile_two: 1 or 2)
    kTileDuo,       // op[0] -> op[1] per tile
    kTileDuoOne,    // tile duo op[0] -> op[1] beside the independent tile op[2] (1 or 2)
    kDuo,           // paired levels op[0] -> op[1] (k_gauss_duo)
    kTrio,          // three levels op[0] -> op[1] -> op[2] (k_gauss_trio)
    kKinds
};
constexpr int kind_ops(int kind) {
    return kind == kLevel || kind == kTile ? 1 : (kind == kTileDuoOne || kind == kTrio ? 3 : 2);
}

struct Launch {
    int kind;
    int op[3];       // indices into the level list (kind_ops(kind) of them, the rest -1)
    bool side;       // on the side stream
    bool wait_ds;    // the launch's stream first waits for ev_ds (octave 1's base written)
    bool rec_ds;     // ev_ds is recorded after the launch
};

struct Plan {
    std::vector<Launch> launches;
    bool side = false;    // the side-stream layout: octaves >= 1 on the side stream
    bool trash = false;   // some launch is a kDuo or kTrio (they need the scratch buffer)
    // scratch of plan_pyramid, kept so that a reused Plan allocates nothing
    std::vector<char> tiled, in_trio, trio_third, trio_octave, duo_second;
    std::vector<int> duo_next, job_of, singles;
    struct Job { int i0, n, launch; };
    std::vector<Job> jobs;
};

// sup answers which combinations have a kernel, by level index: sup.tile(i), sup.tile_duo(i, j),
// sup.duo(i, j), sup.trio(i, j, l).  lv: the level filters octave by octave, levels ascending.
template <class Support>
void plan_pyramid(const LevelDesc* lv, int n, const Rules& R, const Support& sup, Plan& P) {
    std::vector<Launch>& out = P.launches;
    out.clear();
    P.trash = false;
    const int kds = R.kds;
    const bool side = R.side_stream && !R.serial && n > 0 && lv[n - 1].o >= 1;
    P.side = side;
    // 2-D tiles for the cache-resident levels (sift_gauss_tile.hip): not with a forced kernel or
    // band height (those test the wave kernels)
    const bool tiles_on = R.wave_rows == 0 && !R.long_bands && !R.tiles_off;
    const bool tiles_all = tiles_on && R.tiles_always;
    P.tiled.assign((size_t)n, 0);
    for (int i = 0; i < n; i++)
        P.tiled[i] = tiles_on && sup.tile(i) &&
                     (tiles_all || 4ll * lv[i].w * lv[i].h * lv[i].batch <= ((long long)R.tile_mb << 20));
    const std::vector<char>& tiled = P.tiled;
    auto bytes_of = [&](int i) { return 4ll * lv[i].w * lv[i].h * lv[i].batch; };
    auto push = [&](int kind, int a, int b = -1, int c = -1) {
        out.push_back(Launch{kind, {a, b, c}, false, false, false});
    };
    auto level = [&](int i) { push(tiled[i] ? kTile : kLevel, i); };

    // every level tiled (a cache-resident pyramid: one image, C2) and tile duos asked for
    // (SGPU_TILE_DUO=on, or SGPU_DEBUG_DUO_ALWAYS with SGPU_DEBUG_GAUSS_TILE_ALWAYS): the tile-duo
    // schedule -- octave 0 pairs levels (0, 1), (2, 3), (4, 5) into tile duos (two levels per
    // launch from one load, sift_gauss_tile.hip), octaves >= 1 run level 1 alone and pair the
    // rest; a job launches right after the job holding its input, and octave o+1's level 1 shares
    // the launch of octave o's last duo (-no 4 -d 3: 9 launches instead of 15).  Measured slower
    // than the single-level tiles of the diagonal schedule (C2 pyramid 115-119 vs 97-99 us: a duo
    // tile's stage-1 halo region and its five barrier phases cost more than the launch and the
    // level's round trip it saves), so not the default.
    const bool want_duo = R.tile_duo || (R.duo_always && R.tiles_always);
    bool all_tiled = want_duo && !side && !R.serial && kds >= 1 && n > 0;
    for (int i = 0; i < n && all_tiled; i++) all_tiled = tiled[i];
    if (all_tiled) {
        std::vector<Plan::Job>& jobs = P.jobs;
        jobs.clear();
        P.job_of.assign((size_t)n, -1);
        auto op_index = [&](int o, int k) -> int {
            for (int i = 0; i < n; i++)
                if (lv[i].o == o && lv[i].k == k) return i;
            return -1;
        };
        for (int i = 0; i < n;) {
            const LevelDesc& e = lv[i];
            const bool pair = e.k % 2 == 0 && i + 1 < n && lv[i + 1].o == e.o &&
                              lv[i + 1].k == e.k + 1 && sup.tile_duo(i, i + 1);
            jobs.push_back({i, pair ? 2 : 1, 0});
            P.job_of[i] = (int)jobs.size() - 1;
            if (pair) P.job_of[i + 1] = (int)jobs.size() - 1;
            i += pair ? 2 : 1;
        }
        int last_launch = 0;
        for (Plan::Job& jb : jobs) {
            const LevelDesc& e = lv[jb.i0];
            int dep = -1;   // the op writing this job's input level
            if (e.k >= 2 || (e.k == 1 && e.o == 0)) dep = op_index(e.o, e.k - 1);
            else if (e.k == 1) dep = op_index(e.o - 1, kds);
            jb.launch = dep < 0 ? 0 : jobs[P.job_of[dep]].launch + 1;
            last_launch = last_launch > jb.launch ? last_launch : jb.launch;
        }
        for (int L = 0; L <= last_launch; L++) {
            std::vector<int>& in = P.singles;   // the jobs of launch L
            in.clear();
            for (size_t j = 0; j < jobs.size(); j++)
                if (jobs[j].launch == L) in.push_back((int)j);
            size_t q = 0;
            if (in.size() == 2 && jobs[in[0]].n != jobs[in[1]].n) {   // a duo beside a single level
                const Plan::Job& d = jobs[in[0]].n == 2 ? jobs[in[0]] : jobs[in[1]];
                const Plan::Job& o1 = jobs[in[0]].n == 2 ? jobs[in[1]] : jobs[in[0]];
                push(kTileDuoOne, d.i0, d.i0 + 1, o1.i0);
                q = 2;
            } else if (in.size() == 2 && jobs[in[0]].n == 1 && jobs[in[1]].n == 1) {
                push(kTileTwo, jobs[in[0]].i0, jobs[in[1]].i0);
                q = 2;
            }
            for (; q < in.size(); q++) {
                const Plan::Job& jb = jobs[in[q]];
                if (jb.n == 2) push(kTileDuo, jb.i0, jb.i0 + 1);
                else push(kTile, jb.i0);
            }
        }
        return;
    }
    if (side || R.serial || kds < 1) {
        // octave by octave, one level per launch (octaves >= 1 on the side stream in the stream
        // layout, which starts when octave 0's level kds has written octave 1's base)
        for (int i = 0; i < n; i++) {
            const LevelDesc& e = lv[i];
            level(i);
            Launch& l = out.back();
            l.side = side && e.o >= 1;
            l.wait_ds = side && e.o == 1 && e.k == 1;
            l.rec_ds = side && e.o == 0 && e.k == kds && e.ds;
        }
        return;
    }
    // Diagonal schedule: op (o, k) in slot o * kds + k.  Its inputs come from
    // earlier slots -- (o, k-1), and for k = 1 octave o-1's level kds (slot o * kds) -- so the ops
    // of a slot are independent and share a launch: octave o+1's levels 1, 2 run beside octave
    // o's levels kds+1, kds+2 (15 launches instead of 21 for -no 4 -d 3), the small jobs'
    // latency-bound waves filling the large ones' CU slots.
    // Paired levels: ops (o, k) and (o, k+1) of a streaming-size level
    // (>= SGK_DUO_MIN_MB: not left in the Infinity Cache by the previous launch) with a compiled
    // width pair run as one k_gauss_duo launch in slot o * kds + k + 1 -- level k read once,
    // levels k+1 and k+2 written (12 instead of 16 B per pixel).
    const bool duo_all = R.duo_always;
    const bool duo_off = R.duo_off || (!SGK_DUO_DEFAULT && !duo_all && !R.duo_on);
    const bool pairing = !duo_off && R.wave_rows >= 0;
    // Three levels: ops (o, k), (o, k+1), (o, k+2) with the widths (11, 13, 17)
    // and the third decimated into octave o+1 run as one k_gauss_trio launch in slot
    // o * kds + k + 2 (level k read once, levels k+1 .. k+3 and the decimation written: 17
    // instead of 25 B per pixel), on levels >= SGK_TRIO_MIN_MB (any size with kTrioAlways); the
    // octave's (21, 25) pair after it then pairs too.
    std::vector<char>&trio_third = P.trio_third, &in_trio = P.in_trio, &trio_octave = P.trio_octave;
    trio_third.assign((size_t)n, 0);
    in_trio.assign((size_t)n, 0);
    trio_octave.assign(n > 0 ? (size_t)lv[n - 1].o + 1 : 0, 0);
    if (pairing && R.trio_mode != kTrioOff) {
        for (int i = 0; i + 2 < n; i++) {
            const LevelDesc &a = lv[i], &b = lv[i + 1], &c = lv[i + 2];
            if (in_trio[i] || a.o != b.o || a.o != c.o || b.k != a.k + 1 || c.k != a.k + 2) continue;
            if (R.trio_mode != kTrioAlways && bytes_of(i) < ((long long)SGK_TRIO_MIN_MB << 20)) continue;
            if (!sup.trio(i, i + 1, i + 2)) continue;
            in_trio[i] = in_trio[i + 1] = in_trio[i + 2] = 1;
            trio_third[i + 2] = 1;
            trio_octave[a.o] = 1;
            P.trash = true;
        }
    }
    std::vector<int>& duo_next = P.duo_next;   // op i pairs with op duo_next[i]
    std::vector<char>& duo_second = P.duo_second;
    duo_next.assign((size_t)n, -1);
    duo_second.assign((size_t)n, 0);
    // Pairs from the octave's end: on a level of >= SGK_DUO_WIDE_MIN_MB (any size
    // with duo_always), octave o's levels pair as (4, 5) = (21, 25), (2, 3) = (13, 17) with level
    // 3's decimation, (0, 1) = the u8 ingest pair (13, 11) -- three launches for octave 0 instead
    // of four (level 0, (1, 2), (3, 4), level 5), 34 instead of 38 B per pixel -- when the (2, 3)
    // pair is supported; otherwise the pairs from the front.
    if (pairing && R.duo_plan == kPairsEnd) {
        for (int j = n; j >= 2; j--) {
            const int i = j - 2;   // candidate pair (i, i + 1)
            const LevelDesc &a = lv[i], &b = lv[i + 1];
            if (a.o != b.o || b.k != a.k + 1 || (b.k % 2) != 1) continue;
            if (in_trio[i] || in_trio[i + 1] || duo_second[i] || duo_next[i + 1] >= 0) continue;
            if (!duo_all && (bytes_of(i) < ((long long)SGK_DUO_WIDE_MIN_MB << 20) ||
                             a.w > SGK_DUO_PLAN_MAXW))
                continue;
            // the octave takes the plan only with its (2, 3) pair: look it up first
            bool mid_ok = false;
            for (int q = 0; q + 1 < n; q++)
                if (lv[q].o == a.o && lv[q].k == 2 && lv[q + 1].k == 3 && lv[q + 1].o == a.o)
                    mid_ok = sup.duo(q, q + 1) && lv[q + 1].ds;
            if (!mid_ok || !sup.duo(i, i + 1)) continue;
            duo_next[i] = i + 1;
            duo_second[i + 1] = 1;
            P.trash = true;
        }
    }
    if (pairing) {
        for (int i = 0; i + 1 < n; i++) {
            const LevelDesc &a = lv[i], &b = lv[i + 1];
            if (in_trio[i] || in_trio[i + 1]) continue;
            if (duo_second[i] || duo_next[i] >= 0 || duo_second[i + 1] || duo_next[i + 1] >= 0) continue;
            if (a.o != b.o || b.k != a.k + 1) continue;
            const long long bytes = bytes_of(i);
            if (!duo_all && bytes < ((long long)SGK_DUO_MIN_MB << 20)) continue;
            if (!duo_all && a.fw + b.fw > 24) {
                const bool ds_pair = a.ds;
                if (!ds_pair && !R.duo_wide && !trio_octave[a.o]) continue;
                if (bytes < ((long long)SGK_DUO_WIDE_MIN_MB << 20)) continue;
            }
            // the u8 ingest pair (levels 0, 1: 725 us) displaces the (11, 13) pair of levels
            // 1, 2 (750 us, level 0 alone 390): opt-in
            if (!duo_all && !R.duo_u8 && a.u8) continue;
            // (a pair that decimates its second level only in the plan from the octave's end)
            if (b.ds || !sup.duo(i, i + 1)) continue;
            duo_next[i] = i + 1;
            duo_second[i + 1] = 1;
            P.trash = true;
        }
    }
    int last = 0;
    for (int i = 0; i < n; i++) last = last > lv[i].o * kds + lv[i].k ? last : lv[i].o * kds + lv[i].k;
    for (int slot = 0; slot <= last; slot++) {
        // the launches that end in this slot in op order, then the slot's single levels two by two
        std::vector<int>& in_slot = P.singles;
        in_slot.clear();
        for (int i = 0; i < n; i++) {
            if (lv[i].o * kds + lv[i].k != slot) continue;
            if (trio_third[i]) push(kTrio, i - 2, i - 1, i);
            else if (duo_second[i]) push(kDuo, i - 1, i);
            else if (!in_trio[i] && duo_next[i] < 0) in_slot.push_back(i);
        }
        const int m = (int)in_slot.size();
        int i = 0;
        for (; i + 1 < m; i += 2) {
            const int a = in_slot[i], b = in_slot[i + 1];
            if (tiled[a] && tiled[b]) push(kTileTwo, a, b);
            else if (!tiled[a] && !tiled[b]) push(kTwo, a, b);
            else {   // one tiled, one not: a launch each
                level(a);
                level(b);
            }
        }
        if (i < m) level(in_slot[i]);
    }
}

// ---- the compiled width combinations ----
// u8: the first level reads the u8 input; ds_first / ds_second: that level of the pair also
// writes its decimation.

// k_gauss_duo (sift_gauss_duo.hip): f32 pairs (11, 13), (21, 25), (17, 21) with level k + 1
// decimated into the next octave, (13, 17) with level k + 2 decimated; the u8 ingest pair (13, 11)
// (level 0 from the image, level 1)
constexpr bool duo_widths(int fa, int fb, bool u8, bool ds_first, bool ds_second) {
    return u8 ? (fa == 13 && fb == 11 && !ds_first && !ds_second)
           : ds_second ? (fa == 13 && fb == 17 && !ds_first)
           : ds_first ? (fa == 17 && fb == 21)
                      : ((fa == 11 && fb == 13) || (fa == 21 && fb == 25));
}

// k_gauss_trio (sift_gauss_trio.hip): f32 widths (11, 13, 17), the third level decimated
constexpr bool trio_widths(int fa, int fb, int fc) { return fa == 11 && fb == 13 && fc == 17; }

// k_gauss_tile_duo (sift_gauss_tile.hip; the default -d 3 schedule: octave 0's (13 u8, 11),
// (13, 17 + decimation), (21, 25); octaves >= 1: (13, 17 [+ decimation]), (21, 25); (13, 11) from
// a float first level, (11, 13) and (17, 21) for other pairings)
constexpr bool tile_duo_widths(int fa, int fb, bool u8, bool ds_first, bool ds_second) {
    return ds_first || (u8 && ds_second) ? false
           : ds_second ? (fa == 13 && fb == 17)
                       : ((fa == 13 && fb == 11) || (fa == 13 && fb == 17) || (fa == 21 && fb == 25) ||
                          (fa == 11 && fb == 13) || (fa == 17 && fb == 21));
}

}  // namespace sgpyr
