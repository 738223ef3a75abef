// Host-only check of the grouped pair matcher's planner (csrc/sift_match_plan.h): built with
// -fsanitize=address,undefined and run by tests/test_match_plan.py.  Exit status 0 = every
// property holds; a failure prints the property and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <tuple>
#include <utility>
#include <vector>

#include "sift_match_plan.h"

using namespace sgplan;

#define REQUIRE(...)                                                          \
    do {                                                                      \
        if (!(__VA_ARGS__)) {                                                 \
            std::fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, \
                         #__VA_ARGS__, g_case);                               \
            std::exit(1);                                                     \
        }                                                                     \
    } while (0)

static const char* g_case = "";
constexpr int kCUs = 256;   // compute units of an MI355X

struct Range { int64_t b, e; };
static void no_overlap(std::vector<Range> r, int64_t total) {
    std::sort(r.begin(), r.end(), [](const Range& x, const Range& y) { return x.b < y.b; });
    int64_t at = 0;
    for (const Range& x : r) {
        REQUIRE(x.b >= at);
        REQUIRE(x.e >= x.b);
        at = x.e;
    }
    REQUIRE(at <= total);
}

static void check(const char* name, const std::vector<int>& sizes,
                  const std::vector<std::pair<int, int>>& pairs, bool mutual, int max_match) {
    g_case = name;
    std::vector<int64_t> off(sizes.size() + 1, 0);
    for (size_t s = 0; s < sizes.size(); s++) off[s + 1] = off[s] + sizes[s];
    std::vector<int> flat;
    for (auto& p : pairs) { flat.push_back(p.first); flat.push_back(p.second); }
    Plan plan;
    REQUIRE(build_plan(off.data(), (int)sizes.size(), flat.data(), (int)pairs.size(), mutual,
                       max_match, plan) == kPlanOk);
    REQUIRE(plan.pairs.size() == pairs.size());

    // the sides a plan must have: both sets non-empty; direction 1 only for mutual matching
    std::map<std::pair<int, int>, int> side_of;   // (pair, dir) -> side
    for (size_t s = 0; s < plan.sides.size(); s++) {
        const Side& sd = plan.sides[s];
        REQUIRE(sd.pair >= 0 && sd.pair < (int)pairs.size());
        REQUIRE(sd.dir == 0 || (mutual && sd.dir == 1));
        REQUIRE(side_of.emplace(std::make_pair(sd.pair, sd.dir), (int)s).second);
        const int sa = sd.dir ? pairs[sd.pair].second : pairs[sd.pair].first;
        const int sb = sd.dir ? pairs[sd.pair].first : pairs[sd.pair].second;
        REQUIRE(sd.a_off == off[sa] && sd.a_n == sizes[sa]);
        REQUIRE(sizes[sa] > 0 && sizes[sb] > 0);
        REQUIRE(sd.tie32 == (sd.dir == 0));
        REQUIRE(sd.chunks >= 1);
    }
    int64_t bound = 0;
    for (size_t p = 0; p < pairs.size(); p++) {
        const bool live = sizes[pairs[p].first] > 0 && sizes[pairs[p].second] > 0;
        for (int dir = 0; dir < 2; dir++)
            REQUIRE((side_of.count({(int)p, dir}) == 1) == (live && (dir == 0 || mutual)));
        const PairRec& pr = plan.pairs[p];
        REQUIRE(pr.n_a == (live ? sizes[pairs[p].first] : 0));
        if (live) {
            REQUIRE(pr.dec0 == plan.sides[side_of[{(int)p, 0}]].dec_off);
            REQUIRE(pr.dec1 == (mutual ? plan.sides[side_of[{(int)p, 1}]].dec_off : -1));
            bound += std::min(pr.n_a, std::max(max_match, 0));
        }
    }
    REQUIRE(plan.out_bound == bound);

    // every (pair, direction, panel, chunk) exactly once; chunks tile [0, n_b)
    std::set<std::tuple<int, int, int, int>> seen;
    std::map<std::tuple<int, int, int>, std::pair<int, int>> chunk_cols;   // (pair, dir, chunk)
    std::vector<Range> part_ranges, dec_ranges;
    for (const Item& it : plan.items) {
        REQUIRE(side_of.count({it.pair, it.dir}) == 1);
        const Side& sd = plan.sides[side_of[{it.pair, it.dir}]];
        const int sb = it.dir ? pairs[it.pair].first : pairs[it.pair].second;
        REQUIRE(it.a_off == sd.a_off && it.a_n == sd.a_n);
        REQUIRE(it.b_off == off[sb] && it.b_n == sizes[sb]);
        REQUIRE(it.panel >= 0 && it.panel * kPanelRows < it.a_n);
        REQUIRE(it.chunk >= 0 && it.chunk < sd.chunks);
        REQUIRE(it.c_begin < it.c_end && it.c_end <= it.b_n);
        REQUIRE(it.c_begin % kTileCols == 0);
        REQUIRE(it.c_end % kTileCols == 0 || it.c_end == it.b_n);
        REQUIRE(it.part_base == sd.part_off + it.chunk * sd.a_n);
        REQUIRE(seen.emplace(it.pair, it.dir, it.panel, it.chunk).second);
        auto ins = chunk_cols.emplace(std::make_tuple(it.pair, it.dir, it.chunk),
                                      std::make_pair(it.c_begin, it.c_end));
        REQUIRE(ins.first->second == std::make_pair(it.c_begin, it.c_end));
    }
    size_t expect_items = 0;
    for (const Side& sd : plan.sides) {
        const int panels = (sd.a_n + kPanelRows - 1) / kPanelRows;
        expect_items += (size_t)panels * sd.chunks;
        const int sb = sd.dir ? pairs[sd.pair].first : pairs[sd.pair].second;
        int at = 0;
        for (int c = 0; c < sd.chunks; c++) {
            auto f = chunk_cols.find(std::make_tuple(sd.pair, sd.dir, c));
            REQUIRE(f != chunk_cols.end());
            REQUIRE(f->second.first == at);
            at = f->second.second;
            part_ranges.push_back(Range{(int64_t)sd.part_off + (int64_t)c * sd.a_n,
                                        (int64_t)sd.part_off + (int64_t)(c + 1) * sd.a_n});
        }
        REQUIRE(at == sizes[sb]);
        dec_ranges.push_back(Range{sd.dec_off, (int64_t)sd.dec_off + sd.a_n});
    }
    REQUIRE(plan.items.size() == expect_items);
    no_overlap(part_ranges, plan.part_total);
    no_overlap(dec_ranges, plan.dec_total);

    // the finish covers every (side, panel) once
    std::set<std::pair<int, int>> fseen;
    for (const FinishPanel& fp : plan.fpanels) {
        REQUIRE(fp.side >= 0 && fp.side < (int)plan.sides.size());
        REQUIRE(fp.panel >= 0 && fp.panel * kPanelRows < plan.sides[fp.side].a_n);
        REQUIRE(fseen.emplace(fp.side, fp.panel).second);
    }
    size_t expect_fp = 0;
    for (const Side& sd : plan.sides) expect_fp += (sd.a_n + kPanelRows - 1) / kPanelRows;
    REQUIRE(plan.fpanels.size() == expect_fp);
}

static void build_for(const std::vector<int>& sizes, const std::vector<std::pair<int, int>>& pairs,
                      bool mutual, int max_match, Plan& plan) {
    std::vector<int64_t> off(sizes.size() + 1, 0);
    for (size_t s = 0; s < sizes.size(); s++) off[s + 1] = off[s] + sizes[s];
    std::vector<int> flat;
    for (auto& p : pairs) { flat.push_back(p.first); flat.push_back(p.second); }
    REQUIRE(build_plan(off.data(), (int)sizes.size(), flat.data(), (int)pairs.size(), mutual,
                       max_match, plan) == kPlanOk);
}

// The table block (table_layout, pack_tables, view_tables): the size is the sum of the four tables
// and a multiple of 8, packing and viewing round-trip every table byte for byte, and a trailer
// written at `bytes` leaves the last table alone.  The block is allocated at its exact size, so
// that ASan sees a write past it.
template <class T>
static void same_bytes(const T* seen, const std::vector<T>& want) {
    REQUIRE(want.empty() || std::memcmp(seen, want.data(), want.size() * sizeof(T)) == 0);
}
static void check_tables(const char* name, const std::vector<int>& sizes,
                         const std::vector<std::pair<int, int>>& pairs, bool mutual) {
    Plan plan;
    build_for(sizes, pairs, mutual, 1 << 30, plan);
    g_case = name;
    const TableLayout l = table_layout(plan);
    REQUIRE(l.bytes == plan.items.size() * sizeof(Item) + plan.sides.size() * sizeof(Side) +
                           plan.fpanels.size() * sizeof(FinishPanel) +
                           plan.pairs.size() * sizeof(PairRec));
    REQUIRE(l.bytes % 8 == 0);
    REQUIRE(l.items == 0 && l.items <= l.sides && l.sides <= l.fpanels && l.fpanels <= l.pairs &&
            l.pairs <= l.bytes);
    const size_t trailer = 24;
    std::vector<unsigned char> block(l.bytes + trailer, 0xA5);
    pack_tables(plan, block.data());
    for (size_t k = 0; k < trailer; k++) REQUIRE(block[l.bytes + k] == 0xA5);   // packing stops at bytes
    std::memset(block.data() + l.bytes, 0x5A, trailer);
    const TableView v = view_tables(l, block.data());
    same_bytes(v.items, plan.items);
    same_bytes(v.sides, plan.sides);
    same_bytes(v.fpanels, plan.fpanels);
    same_bytes(v.pairs, plan.pairs);
    REQUIRE(reinterpret_cast<const unsigned char*>(v.pairs + plan.pairs.size()) == block.data() + l.bytes);
}

int main() {
    for (int mutual = 0; mutual < 2; mutual++) {
        check_tables("tables 1x1", {1, 1}, {{0, 1}}, mutual != 0);
        check_tables("tables 129x257", {129, 257}, {{0, 1}}, mutual != 0);
        check_tables("tables with an empty set", {0, 5, 130}, {{0, 1}, {1, 2}, {2, 0}}, mutual != 0);
    }
    {
        g_case = "empty tables";
        const Plan none;   // no pair at all: nothing to pack, dst is not touched
        REQUIRE(table_layout(none).bytes == 0);
        pack_tables(none, nullptr);
    }
    // the sets and pair list of the GPU size test
    const std::vector<int> sizes = {0, 1, 127, 128, 129, 257, 700, 3000};
    std::vector<std::pair<int, int>> pairs;
    for (int s = 0; s + 1 < (int)sizes.size(); s++) pairs.push_back({s, s + 1});
    pairs.insert(pairs.end(), {{3, 3}, {5, 2}, {2, 5}, {6, 7}, {6, 7}, {0, 4}, {4, 0}, {0, 0}});
    for (int mutual = 0; mutual < 2; mutual++)
        for (int mm : {0, 100, 1 << 30}) check("sizes", sizes, pairs, mutual != 0, mm);

    // one huge pair: the split must still fill the chip
    for (int mutual = 0; mutual < 2; mutual++) {
        check("huge", {50000, 50000}, {{0, 1}}, mutual != 0, 50000);
        g_case = "huge items";
        const int64_t off[3] = {0, 50000, 100000};
        const int pr[2] = {0, 1};
        Plan plan;
        REQUIRE(build_plan(off, 2, pr, 1, mutual != 0, 50000, plan) == kPlanOk);
        REQUIRE((int)plan.items.size() >= kCUs);
    }
    // one pair of two images: few panels, so the columns are chunked
    {
        g_case = "two images";
        const int64_t off[3] = {0, 3000, 6000};
        const int pr[2] = {0, 1};
        Plan plan;
        REQUIRE(build_plan(off, 2, pr, 1, true, 3000, plan) == kPlanOk);
        REQUIRE((int)plan.items.size() >= kCUs);
    }
    // Filler pairs (tests/test_gpu_match_batch.py): thousands of one-row mutual pairs add two
    // panels each, so the real pairs of the same call get the panel-limited plans (1, 2 or 3
    // chunks per side) that a shard's pair list gets.
    {
        // 3000 x 9000 with 2100 fillers: one chunk per side, 71 and 24 tiles
        std::vector<int> fsizes = {3000, 9000, 1, 1};
        std::vector<std::pair<int, int>> fpairs = {{0, 1}};
        for (int k = 0; k < 2100; k++) fpairs.push_back({2, 3});
        check("filler ties", fsizes, fpairs, true, 3000);
        g_case = "filler ties tiles";
        Plan plan;
        build_for(fsizes, fpairs, true, 3000, plan);
        int tiles[2] = {0, 0}, items[2] = {0, 0};
        for (const Side& sd : plan.sides)
            if (sd.pair == 0) REQUIRE(sd.chunks == 1);
        for (const Item& it : plan.items)
            if (it.pair == 0) {
                REQUIRE(it.c_begin == 0);
                tiles[it.dir] = std::max(tiles[it.dir], (it.c_end - it.c_begin + kTileCols - 1) / kTileCols);
                items[it.dir]++;
            }
        REQUIRE(tiles[0] == 71 && tiles[1] == 24);
        REQUIRE(items[0] == 24 && items[1] == 71);   // one item per panel
    }
    {
        // the GPU size test's sets and pairs under 1010 fillers: at most 2 chunks per side, and
        // some side has 2
        std::vector<int> fsizes = {0, 1, 127, 128, 129, 257, 385, 513, 700, 897, 3000, 1, 1};
        std::vector<std::pair<int, int>> fpairs;
        for (int s = 0; s + 1 < 11; s++) fpairs.push_back({s, s + 1});
        fpairs.insert(fpairs.end(), {{5, 5}, {7, 4}, {4, 7}, {9, 10}, {8, 6}, {6, 8}, {0, 4}, {4, 0}, {0, 0}});
        const size_t real = fpairs.size();
        for (int k = 0; k < 1010; k++) fpairs.push_back({11, 12});
        for (int mutual = 0; mutual < 2; mutual++) check("filler sizes", fsizes, fpairs, mutual != 0, 3000);
        g_case = "filler sizes chunks";
        Plan plan;
        build_for(fsizes, fpairs, true, 3000, plan);
        int most = 0;
        for (const Side& sd : plan.sides) {
            REQUIRE(sd.chunks <= 2);
            if (sd.pair >= (int)real) REQUIRE(sd.chunks == 1);
            most = std::max(most, sd.chunks);
        }
        REQUIRE(most == 2);
    }
    check("no pairs", sizes, {}, true, 10);
    check("all empty", {0, 0}, {{0, 1}, {1, 0}}, true, 10);

    // rejected arguments
    g_case = "bad arguments";
    {
        Plan plan;
        const int64_t off[3] = {0, 10, 5};
        const int pr[2] = {0, 1};
        REQUIRE(build_plan(off, 2, pr, 1, true, 10, plan) == kPlanBadArgument);   // decreasing
        const int64_t ok[3] = {0, 10, 20};
        const int hi[2] = {0, 2}, neg[2] = {-1, 0};
        REQUIRE(build_plan(ok, 2, hi, 1, true, 10, plan) == kPlanBadArgument);
        REQUIRE(build_plan(ok, 2, neg, 1, true, 10, plan) == kPlanBadArgument);
        REQUIRE(build_plan(ok, 2, pr, 1, true, 10, plan) == kPlanOk);
        const int64_t big[2] = {0, (int64_t)1 << 32};
        const int self[2] = {0, 0};
        REQUIRE(build_plan(big, 1, self, 1, true, 10, plan) == kPlanTooLarge);
    }
    std::puts("match plan ok");
    return 0;
}
