// sift_tracks.h -- the rule by which a pair list's matches become feature tracks (sgpu_tracks_*;
// DESIGN.md 4.20), after Wu, "Towards Linear-time Incremental Structure from Motion" (3DV 2013),
// where tracks are built between matching and reconstruction.  Plain C++, no HIP: SGTRK_HD is
// `__host__ __device__` under hipcc and nothing under g++, so that the kernels (sift_tracks.hip),
// the host path (sgpu_tracks.cpp) and a host-only program (tests/abi/tracks_check.cpp) share it.
//
// Rule.  Inputs: set_offsets[nsets + 1], set_pairs[npairs][2], matches[sum counts][2] (set-local
// {i, j}, concatenated in pair order), match_counts[npairs], min_length >= 2: the out_pairs /
// out_counts of the pair matchers with the offsets and pair list they took.
//   Nodes.  A node is a buffer row r = set_offsets[s] + i; rows = set_offsets[nsets].
//   Edges.  Match {i, j} of pair (a, b) is the edge (set_offsets[a] + i, set_offsets[b] + j).  A
//           self-loop (pair (a, a), i == j) is no edge.  Repeated pairs, both orders and (a, a)
//           are legal pair lists.
//   Components.  The connected components of that graph; a component's label is its smallest row,
//           which makes the result independent of the order of the edges.  With n its rows:
//           n < min_length                        short;
//           else n > nsets                        inconsistent (two rows must share a set);
//           else two of its rows lie in one set   inconsistent;
//           else                                  a track.
//   Output.  Tracks are numbered 0 .. T - 1 in ascending label order.  out_track[row] = the track
//           id, kTrackNone (-1) for an unmatched row or a row of a short component,
//           kTrackInconsistent (-2) for a row of an inconsistent one.  CSR: out_offsets[0 .. T]
//           (64-bit, rows / 2 + 1 entries provided), out_rows[out_offsets[t] ..) = track t's rows
//           in ascending order, which is set order too (rows entries provided).  out_stats[4] =
//           {components of >= 2 rows, tracks, inconsistent components, short components of >= 2
//           rows}.  The result is a pure function of the inputs.
#ifndef SIFT_TRACKS_H
#define SIFT_TRACKS_H
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define SGTRK_HD __host__ __device__ inline
#else
#define SGTRK_HD inline
#endif

namespace sgtrk {

constexpr int kTrackNone = -1, kTrackInconsistent = -2;
constexpr int kMinLength = 2;
enum { kArgsOk = 0, kArgsBad = 1 };
// what a component's size alone says of it
enum { kShort = 0, kCandidate = 1, kOversize = 2 };

SGTRK_HD int classify(long long size, int min_length, int nsets) {
    if (size < min_length) return kShort;
    return size > nsets ? kOversize : kCandidate;
}

// The set of row x: the s with off[s] <= x < off[s + 1], for off[0] <= x < off[nsets] (empty sets
// have no rows and are never the answer).  The interval [lo, hi] shrinks with every step.
SGTRK_HD int set_of_row(const long long* off, int nsets, long long x) {
    int lo = 0, hi = nsets - 1;
    for (int step = 0; step < 32 && lo < hi; step++) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// The pair of match position e: the p with start[p] <= e < start[p + 1], start = the scan of the
// counts (start[npairs] = their sum > e).  Pairs without matches are never the answer.
SGTRK_HD int pair_of_match(const long long* start, int npairs, long long e) {
    return set_of_row(start, npairs, e);
}

// What sgpu_tracks_batch refuses (SGPU_EINVAL) before anything is queued, in one place.  On kArgsOk
// *rows = set_offsets[nsets] and *total = the sum of the counts.
inline int check_args(const int64_t* set_offsets, int nsets, const int* set_pairs, int npairs,
                      const int* matches, const int* match_counts, int min_length,
                      const char** why, int64_t* rows, int64_t* total) {
    *rows = *total = 0;
    *why = "bad tracks arguments";
    if (nsets < 0 || npairs < 0 || !set_offsets) return kArgsBad;
    *why = "min_length < 2";
    if (min_length < kMinLength) return kArgsBad;
    *why = "bad set offsets";
    if (set_offsets[0] < 0) return kArgsBad;
    for (int s = 0; s < nsets; s++)
        if (set_offsets[s + 1] < set_offsets[s]) return kArgsBad;
    *why = "2^31 rows or more";
    if (set_offsets[nsets] > 0x7fffffffLL) return kArgsBad;
    *why = "null pair list or counts";
    if (npairs > 0 && (!set_pairs || !match_counts)) return kArgsBad;
    int64_t sum = 0;
    for (int p = 0; p < npairs; p++) {
        const int a = set_pairs[2 * p], b = set_pairs[2 * p + 1];
        *why = "bad pair indices";
        if (a < 0 || a >= nsets || b < 0 || b >= nsets) return kArgsBad;
        *why = "a negative match count";
        if (match_counts[p] < 0) return kArgsBad;
        sum += match_counts[p];
    }
    *why = "null matches";
    if (sum > 0 && !matches) return kArgsBad;
    *why = "a match index lies outside its set";
    int64_t k = 0;
    for (int p = 0; p < npairs; p++) {
        const int a = set_pairs[2 * p], b = set_pairs[2 * p + 1];
        const int64_t na = set_offsets[a + 1] - set_offsets[a], nb = set_offsets[b + 1] - set_offsets[b];
        for (int e = 0; e < match_counts[p]; e++, k++) {
            const int i = matches[2 * k], j = matches[2 * k + 1];
            if (i < 0 || i >= na || j < 0 || j >= nb) return kArgsBad;
        }
    }
    *why = "";
    *rows = set_offsets[nsets];
    *total = sum;
    return kArgsOk;
}

// The reference loop of the rule: a serial union-find (the smaller root wins, so a component's
// root is its label) and one ascending sweep over the rows.  The arguments must have passed
// check_args; out_offsets / out_rows both or neither, out_stats optional.  Returns T.
inline int tracks_host(const int64_t* set_offsets, int nsets, const int* set_pairs, int npairs,
                       const int* matches, const int* match_counts, int min_length, int* out_track,
                       int64_t* out_offsets, int* out_rows, long long* out_stats) {
    const int64_t rows = set_offsets[nsets];
    std::vector<int> parent((size_t)rows);
    for (int64_t r = 0; r < rows; r++) parent[(size_t)r] = (int)r;
    auto find = [&](int x) {
        while (parent[(size_t)x] != x) {   // parent[x] < x: strictly down
            parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
            x = parent[(size_t)x];
        }
        return x;
    };
    int64_t k = 0;
    for (int p = 0; p < npairs; p++) {
        const int64_t ba = set_offsets[set_pairs[2 * p]], bb = set_offsets[set_pairs[2 * p + 1]];
        for (int e = 0; e < match_counts[p]; e++, k++) {
            const int ru = find((int)(ba + matches[2 * k])), rv = find((int)(bb + matches[2 * k + 1]));
            if (ru < rv) parent[(size_t)rv] = ru;
            else if (rv < ru) parent[(size_t)ru] = rv;
        }
    }
    // label, size; rows ascending, so a root is met before its component's other rows
    std::vector<int> label((size_t)rows), size((size_t)rows, 0);
    for (int64_t r = 0; r < rows; r++) size[(size_t)(label[(size_t)r] = find((int)r))]++;
    // verdict[root]: kTrackNone (one row, or short), kTrackInconsistent, or 0 = a candidate
    std::vector<int> verdict((size_t)rows, kTrackNone);
    long long stats[4] = {0, 0, 0, 0};
    for (int64_t r = 0; r < rows; r++) {
        if (label[(size_t)r] != r || size[(size_t)r] < 2) continue;
        stats[0]++;
        const int kind = classify(size[(size_t)r], min_length, nsets);
        if (kind == kShort) stats[3]++;
        verdict[(size_t)r] = kind == kShort ? kTrackNone : kind == kOversize ? kTrackInconsistent : 0;
    }
    // a candidate with two rows in one set: its rows come in ascending order, so set by set
    {
        std::vector<int> last((size_t)rows, -1);
        int s = 0;
        for (int64_t r = 0; r < rows; r++) {
            while (s + 1 < nsets && set_offsets[s + 1] <= r) s++;
            const size_t L = (size_t)label[(size_t)r];
            if (verdict[L] == kTrackNone) continue;
            if (last[L] == s) verdict[L] = kTrackInconsistent;
            last[L] = s;
        }
    }
    // numbering in ascending label order: id[root], CSR start[root]
    std::vector<int> id((size_t)rows, kTrackNone);
    std::vector<int64_t> start((size_t)rows, 0);
    int T = 0;
    int64_t at = 0;
    for (int64_t r = 0; r < rows; r++) {
        if (label[(size_t)r] != r) continue;
        if (verdict[(size_t)r] == kTrackInconsistent) stats[2]++;
        id[(size_t)r] = verdict[(size_t)r];
        if (verdict[(size_t)r] != 0) continue;
        id[(size_t)r] = T;
        start[(size_t)r] = at;
        if (out_offsets) out_offsets[T] = at;
        at += size[(size_t)r];
        T++;
    }
    if (out_offsets) out_offsets[T] = at;
    stats[1] = T;
    for (int64_t r = 0; r < rows; r++) {
        const size_t L = (size_t)label[(size_t)r];
        out_track[r] = id[L];
        if (id[L] >= 0 && out_rows) out_rows[start[L]++] = (int)r;
    }
    if (out_stats)
        for (int i = 0; i < 4; i++) out_stats[i] = stats[i];
    return T;
}

}  // namespace sgtrk
#endif  // SIFT_TRACKS_H
