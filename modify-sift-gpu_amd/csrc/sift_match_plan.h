// sift_match_plan.h -- host planner of the grouped pair matcher (sgpu_match_batch): plain C++,
// no HIP, so that a host-only program can check it (tests/abi/match_plan_check.cpp).
//
// A batch is a list of descriptor sets in one buffer (set s = rows [off[s], off[s + 1])) and a
// list of set pairs (a, b).  Each pair has one or two sides: direction 0 decides the rows of set a
// over the columns of set b (RowMatch_Kernel's decision), direction 1 -- mutual matching only --
// the rows of set b over the columns of set a (ColMatch_Kernel's).  A side is cut into work
// items (128-row panel of A, column chunk of B), one workgroup of k_match_pairs each; the
// chunks of a side are merged by k_match_pairs_finish, one workgroup per (side, panel).
//
// The plan holds the tables the kernels read and the offsets of everything they write:
//   part  [part_total] Top2   item (side, chunk, panel) writes part[part_base + row in A]
//   dec   [dec_total]  int    side's decision of row r at dec[dec_off + r]
//   out                       pair p's matches at the exclusive scan of the counts (device)
#ifndef SIFT_MATCH_PLAN_H
#define SIFT_MATCH_PLAN_H
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <vector>

namespace sgplan {

constexpr int kPanelRows = 128;     // A rows per work item
constexpr int kTileCols = 128;      // chunk boundaries are multiples of this
constexpr int kTargetItems = 4096;  // work items aimed at per call (about 5 per resident slot)

struct Item {
    int a_off, a_n;      // set A: first row in the buffer, rows
    int b_off, b_n;      // set B
    int panel;           // rows [panel * 128, ...) of A
    int c_begin, c_end;  // columns of B (c_begin a multiple of 128, c_end <= b_n)
    int part_base;       // part[part_base + row in A]
    int pair, dir, chunk;
    int pad;
};
struct Side {
    int a_off, a_n;
    int chunks;
    int part_off;        // chunk c's partials at part_off + c * a_n
    int dec_off;
    int tie32;           // direction 0: equal dots resolve in RowMatch_Kernel's order
    int pair, dir;
};
struct FinishPanel { int side, panel; };
struct PairRec {
    int n_a;             // rows to scan (0: a pair with an empty set)
    int dec0;            // direction 0's decisions
    int dec1;            // direction 1's (-1: not mutual)
    int pad;
};

struct Plan {
    std::vector<Item> items;
    std::vector<Side> sides;
    std::vector<FinishPanel> fpanels;
    std::vector<PairRec> pairs;
    int64_t part_total = 0, dec_total = 0;
    int64_t out_bound = 0;   // upper bound of the matches of all pairs (sum of min(n_a, max_match))
};

enum { kPlanOk = 0, kPlanBadArgument = -1, kPlanTooLarge = -2 };

// Column chunks of a side of n_b columns when every panel of the call gets `want` chunks: at
// least two tiles per chunk, chunks of equal whole tiles except the last; returns the chunk count
// and the columns per chunk.
inline int split_columns(int n_b, int want, int* cols_per_chunk) {
    const int tiles = (n_b + kTileCols - 1) / kTileCols;
    const int max_chunks = std::max(1, (tiles + 1) / 2);
    const int chunks = std::max(1, std::min(want, max_chunks));
    const int tiles_per = (tiles + chunks - 1) / chunks;
    *cols_per_chunk = tiles_per * kTileCols;
    return (tiles + tiles_per - 1) / tiles_per;
}

inline int build_plan(const int64_t* off, int nsets, const int* set_pairs, int npairs, bool mutual,
                      int max_match, Plan& plan, int target_items = kTargetItems) {
    plan = Plan{};
    if (nsets < 0 || npairs < 0 || (nsets > 0 && !off) || (npairs > 0 && !set_pairs))
        return kPlanBadArgument;
    if (nsets > 0 && off[0] < 0) return kPlanBadArgument;
    for (int s = 0; s < nsets; s++)
        if (off[s + 1] < off[s]) return kPlanBadArgument;
    if (nsets > 0 && off[nsets] > INT_MAX) return kPlanTooLarge;
    for (int p = 0; p < npairs; p++)
        for (int k = 0; k < 2; k++)
            if (set_pairs[2 * p + k] < 0 || set_pairs[2 * p + k] >= nsets) return kPlanBadArgument;
    auto rows = [&](int s) { return (int)(off[s + 1] - off[s]); };
    // every panel of the call gets the same chunk target, so that few pairs still fill the chip
    int64_t total_panels = 0;
    for (int p = 0; p < npairs; p++) {
        const int na = rows(set_pairs[2 * p]), nb = rows(set_pairs[2 * p + 1]);
        if (na <= 0 || nb <= 0) continue;
        total_panels += (na + kPanelRows - 1) / kPanelRows;
        if (mutual) total_panels += (nb + kPanelRows - 1) / kPanelRows;
    }
    const int want = total_panels > 0
        ? (int)std::min<int64_t>((target_items + total_panels - 1) / total_panels, INT_MAX) : 1;
    plan.pairs.resize(npairs);
    const int lim = std::max(max_match, 0);
    for (int p = 0; p < npairs; p++) {
        const int sa = set_pairs[2 * p], sb = set_pairs[2 * p + 1];
        const int na = rows(sa), nb = rows(sb);
        PairRec& pr = plan.pairs[p];
        pr = PairRec{0, 0, -1, 0};
        if (na <= 0 || nb <= 0) continue;
        pr.n_a = na;
        plan.out_bound += std::min(na, lim);
        for (int dir = 0; dir < (mutual ? 2 : 1); dir++) {
            const int a_off = (int)off[dir ? sb : sa], a_n = dir ? nb : na;
            const int b_off = (int)off[dir ? sa : sb], b_n = dir ? na : nb;
            int per = 0;
            const int chunks = split_columns(b_n, want, &per);
            const int panels = (a_n + kPanelRows - 1) / kPanelRows;
            if (plan.part_total + (int64_t)chunks * a_n > INT_MAX ||
                plan.dec_total + a_n > INT_MAX ||
                (int64_t)plan.items.size() + (int64_t)chunks * panels > INT_MAX)
                return kPlanTooLarge;
            const int side = (int)plan.sides.size();
            const int part_off = (int)plan.part_total, dec_off = (int)plan.dec_total;
            plan.sides.push_back(Side{a_off, a_n, chunks, part_off, dec_off, dir == 0, p, dir});
            (dir ? pr.dec1 : pr.dec0) = dec_off;
            // chunk-major: the workgroups that run together share their columns of B
            for (int c = 0; c < chunks; c++)
                for (int q = 0; q < panels; q++)
                    plan.items.push_back(Item{a_off, a_n, b_off, b_n, q, c * per,
                                              (int)std::min<int64_t>(b_n, (int64_t)(c + 1) * per),
                                              part_off + c * a_n,
                                              p, dir, c, 0});
            for (int q = 0; q < panels; q++) plan.fpanels.push_back(FinishPanel{side, q});
            plan.part_total += (int64_t)chunks * a_n;
            plan.dec_total += a_n;
        }
    }
    return kPlanOk;
}

// The four tables as the kernels read them, in one block: [items][sides][finish panels][pairs].
// The layout is the same in the host block that is packed and in its device copy; a caller's own
// trailer starts at `bytes`.
struct TableLayout {
    size_t items = 0, sides = 0, fpanels = 0, pairs = 0;   // byte offsets
    size_t bytes = 0;
};
struct TableView {
    const Item* items;
    const Side* sides;
    const FinishPanel* fpanels;
    const PairRec* pairs;
};
static_assert(sizeof(sgplan::Item) % 8 == 0 && sizeof(sgplan::Side) % 8 == 0 &&
              sizeof(sgplan::FinishPanel) % 8 == 0 && sizeof(sgplan::PairRec) % 8 == 0,
              "every table, and the trailer after them, stays 8-byte aligned");

template <class T> size_t table_bytes(const std::vector<T>& v) { return v.size() * sizeof(T); }

inline TableLayout table_layout(const Plan& plan) {
    TableLayout l;
    l.sides = l.items + table_bytes(plan.items);
    l.fpanels = l.sides + table_bytes(plan.sides);
    l.pairs = l.fpanels + table_bytes(plan.fpanels);
    l.bytes = l.pairs + table_bytes(plan.pairs);
    return l;
}

// dst: table_layout(plan).bytes bytes (not read or written when that is 0)
inline void pack_tables(const Plan& plan, unsigned char* dst) {
    const TableLayout l = table_layout(plan);
    auto put = [dst](size_t at, const auto& v) {
        if (!v.empty()) std::memcpy(dst + at, v.data(), table_bytes(v));
    };
    put(l.items, plan.items);
    put(l.sides, plan.sides);
    put(l.fpanels, plan.fpanels);
    put(l.pairs, plan.pairs);
}

// the tables of a block at base, host or device memory (nothing is dereferenced here)
inline TableView view_tables(const TableLayout& l, const unsigned char* base) {
    return TableView{reinterpret_cast<const Item*>(base + l.items),
                     reinterpret_cast<const Side*>(base + l.sides),
                     reinterpret_cast<const FinishPanel*>(base + l.fpanels),
                     reinterpret_cast<const PairRec*>(base + l.pairs)};
}

}  // namespace sgplan
#endif  // SIFT_MATCH_PLAN_H
