// tracks_check.cpp -- the track rule (csrc/sift_tracks.h) on the host: includes only that header,
// so that g++ builds it without HIP, under AddressSanitizer and UBSan (tests/test_tracks.py).
//
//   tracks_check                 self-test: tracks_host against a label propagation written here
//                                on small random graphs, check_args' refusals; prints "tracks ok"
//   tracks_check <in> <out>      file mode: runs tracks_host on the cases of <in>, writes the
//                                results to <out> and prints the loop's milliseconds per case
// <in>:  int32 cases, then per case int32 nsets, npairs, min_length, int64 offsets[nsets + 1],
//        int32 pairs[npairs][2], int32 counts[npairs], int32 matches[sum counts][2].
// <out>: per case int32 T, int64 stats[4], int32 rows, int32 track[rows], int64 offsets[T + 1],
//        int32 out_rows[offsets[T]].
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sift_tracks.h"

namespace {

bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
void write_all(FILE* f, const void* p, size_t bytes) {
    if (bytes) fwrite(p, 1, bytes, f);
}

int file_mode(const char* in_path, const char* out_path) {
    FILE* in = fopen(in_path, "rb");
    FILE* out = fopen(out_path, "wb");
    if (!in || !out) return fprintf(stderr, "cannot open the case files\n"), 2;
    int32_t cases = 0;
    if (!read_all(in, &cases, sizeof(cases)) || cases < 0) return fprintf(stderr, "bad header\n"), 2;
    for (int c = 0; c < cases; c++) {
        int32_t hdr[3];
        if (!read_all(in, hdr, sizeof(hdr)) || hdr[0] < 0 || hdr[1] < 0)
            return fprintf(stderr, "bad case %d\n", c), 2;
        const int nsets = hdr[0], npairs = hdr[1], min_length = hdr[2];
        std::vector<int64_t> off((size_t)nsets + 1);
        std::vector<int> pairs((size_t)npairs * 2), counts((size_t)npairs);
        if (!read_all(in, off.data(), off.size() * 8) || !read_all(in, pairs.data(), pairs.size() * 4) ||
            !read_all(in, counts.data(), counts.size() * 4))
            return fprintf(stderr, "short case %d\n", c), 2;
        int64_t sum = 0;
        for (int n : counts) sum += n < 0 ? 0 : n;
        std::vector<int> matches((size_t)sum * 2);
        if (!read_all(in, matches.data(), matches.size() * 4))
            return fprintf(stderr, "short matches in case %d\n", c), 2;
        const char* why = "";
        int64_t rows = 0, total = 0;
        if (sgtrk::check_args(off.data(), nsets, pairs.data(), npairs, matches.data(), counts.data(),
                              min_length, &why, &rows, &total) != sgtrk::kArgsOk)
            return fprintf(stderr, "case %d refused: %s\n", c, why), 1;
        // exactly the capacities the rule promises to stay within
        std::vector<int> track((size_t)rows), out_rows((size_t)rows);
        std::vector<int64_t> offsets((size_t)rows / 2 + 1);
        long long stats[4];
        const auto t0 = std::chrono::steady_clock::now();
        const int32_t T = sgtrk::tracks_host(off.data(), nsets, pairs.data(), npairs, matches.data(),
                                             counts.data(), min_length, track.data(), offsets.data(),
                                             out_rows.data(), stats);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("case %d: tracks_host %.3f ms\n", c, ms);
        const int32_t r32 = (int32_t)rows;
        const int64_t st[4] = {stats[0], stats[1], stats[2], stats[3]};
        write_all(out, &T, 4);
        write_all(out, st, sizeof(st));
        write_all(out, &r32, 4);
        write_all(out, track.data(), (size_t)rows * 4);
        write_all(out, offsets.data(), ((size_t)T + 1) * 8);
        write_all(out, out_rows.data(), (size_t)offsets[(size_t)T] * 4);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}

uint32_t rng_state = 24680u;
uint32_t rnd() {   // xorshift32
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

struct Graph {
    std::vector<int64_t> off;
    std::vector<int> pairs, counts, matches;
    int nsets() const { return (int)off.size() - 1; }
    int npairs() const { return (int)counts.size(); }
};

// the rule once more, without union-find: minimum labels to a fixed point, then a sort
int by_propagation(const Graph& g, int min_length, std::vector<int>& track, std::vector<int64_t>& offsets,
                   std::vector<int>& out_rows, long long* stats) {
    const int rows = (int)g.off.back(), nsets = g.nsets();
    std::vector<int> label((size_t)rows);
    for (int r = 0; r < rows; r++) label[(size_t)r] = r;
    for (bool changed = true; changed;) {
        changed = false;
        size_t k = 0;
        for (int p = 0; p < g.npairs(); p++)
            for (int e = 0; e < g.counts[(size_t)p]; e++, k++) {
                const size_t u = (size_t)(g.off[(size_t)g.pairs[2 * (size_t)p]] + g.matches[2 * k]);
                const size_t v = (size_t)(g.off[(size_t)g.pairs[2 * (size_t)p + 1]] + g.matches[2 * k + 1]);
                const int m = std::min(label[u], label[v]);
                changed |= label[u] != m || label[v] != m;
                label[u] = label[v] = m;
            }
    }
    auto set_of = [&](int r) {
        int s = 0;
        while (g.off[(size_t)s + 1] <= r) s++;
        return s;
    };
    track.assign((size_t)rows, sgtrk::kTrackNone);
    offsets.assign(1, 0);
    out_rows.clear();
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    for (int L = 0; L < rows; L++) {
        std::vector<int> members;
        for (int r = 0; r < rows; r++)
            if (label[(size_t)r] == L) members.push_back(r);
        if (members.size() < 2) continue;
        stats[0]++;
        if ((int)members.size() < min_length) {
            stats[3]++;
            continue;
        }
        bool bad = (int)members.size() > nsets;
        for (size_t i = 0; i + 1 < members.size(); i++) bad |= set_of(members[i]) == set_of(members[i + 1]);
        stats[bad ? 2 : 1]++;
        for (int r : members) track[(size_t)r] = bad ? sgtrk::kTrackInconsistent : (int)offsets.size() - 1;
        if (bad) continue;
        out_rows.insert(out_rows.end(), members.begin(), members.end());
        offsets.push_back((int64_t)out_rows.size());
    }
    return (int)offsets.size() - 1;
}

int self_test() {
    // set_of_row with empty sets at every place
    const long long off[] = {0, 0, 3, 3, 3, 7, 8, 8};
    const int want_set[] = {1, 1, 1, 4, 4, 4, 4, 5};
    for (int r = 0; r < 8; r++)
        if (sgtrk::set_of_row(off, 7, r) != want_set[r]) return printf("set_of_row(%d)\n", r), 1;
    if (sgtrk::classify(1, 2, 5) != sgtrk::kShort || sgtrk::classify(5, 2, 5) != sgtrk::kCandidate ||
        sgtrk::classify(6, 2, 5) != sgtrk::kOversize || sgtrk::classify(6, 7, 5) != sgtrk::kShort)
        return printf("classify\n"), 1;
    for (int iter = 0; iter < 1500; iter++) {
        Graph g;
        const int nsets = (int)(rnd() % 7);
        g.off.assign(1, 0);
        for (int s = 0; s < nsets; s++) g.off.push_back(g.off.back() + (int64_t)(rnd() % 6));
        const int npairs = nsets ? (int)(rnd() % 9) : 0;
        for (int p = 0; p < npairs; p++) {
            const int a = (int)(rnd() % (uint32_t)nsets), b = (int)(rnd() % (uint32_t)nsets);
            const int64_t na = g.off[(size_t)a + 1] - g.off[(size_t)a], nb = g.off[(size_t)b + 1] - g.off[(size_t)b];
            const int m = na && nb ? (int)(rnd() % 4) : 0;
            g.pairs.push_back(a);
            g.pairs.push_back(b);
            g.counts.push_back(m);
            for (int e = 0; e < m; e++) {
                g.matches.push_back((int)(rnd() % (uint32_t)na));
                g.matches.push_back((int)(rnd() % (uint32_t)nb));
            }
        }
        const int min_length = 2 + (int)(rnd() % 3);
        const char* why = "";
        int64_t rows = 0, total = 0;
        if (sgtrk::check_args(g.off.data(), nsets, g.pairs.data(), npairs, g.matches.data(), g.counts.data(),
                              min_length, &why, &rows, &total) != sgtrk::kArgsOk ||
            rows != g.off.back() || total != (int64_t)g.matches.size() / 2)
            return printf("check_args refuses a legal graph: %s\n", why), 1;
        std::vector<int> want_track, want_rows, track((size_t)rows, -9), out_rows((size_t)rows, -9);
        std::vector<int64_t> want_off, offsets((size_t)rows / 2 + 1, -9);
        long long want_stats[4], stats[4];
        const int want_T = by_propagation(g, min_length, want_track, want_off, want_rows, want_stats);
        const int T = sgtrk::tracks_host(g.off.data(), nsets, g.pairs.data(), npairs, g.matches.data(),
                                         g.counts.data(), min_length, track.data(), offsets.data(),
                                         out_rows.data(), stats);
        offsets.resize((size_t)T + 1);
        out_rows.resize((size_t)offsets.back());
        if (T != want_T || track != want_track || offsets != want_off || out_rows != want_rows ||
            !std::equal(stats, stats + 4, want_stats))
            return printf("tracks_host differs: iter %d\n", iter), 1;
        // labels alone: the same, and nothing else is touched
        std::vector<int> only((size_t)rows, -9);
        if (sgtrk::tracks_host(g.off.data(), nsets, g.pairs.data(), npairs, g.matches.data(), g.counts.data(),
                               min_length, only.data(), nullptr, nullptr, nullptr) != T || only != track)
            return printf("labels alone differ: iter %d\n", iter), 1;
    }
    // what check_args refuses
    const int64_t o2[] = {0, 2, 5}, down[] = {0, 3, 2}, neg[] = {-1, 2, 5}, huge[] = {0, 2, 0x80000000LL};
    const int pr[] = {0, 1}, pr_bad[] = {0, 2}, pr_neg[] = {-1, 1}, one[] = {1}, minus[] = {-1};
    const int m_ok[] = {1, 2}, m_hi[] = {2, 0}, m_hj[] = {0, 3}, m_neg[] = {0, -1};
    const char* why = "";
    int64_t rows = 0, total = 0;
    auto refused = [&](const int64_t* o, int nsets, const int* p, int npairs, const int* m, const int* c, int ml) {
        return sgtrk::check_args(o, nsets, p, npairs, m, c, ml, &why, &rows, &total) == sgtrk::kArgsBad &&
               why[0] != 0;
    };
    if (refused(o2, 2, pr, 1, m_ok, one, 2)) return printf("a legal call refused: %s\n", why), 1;
    if (!refused(nullptr, 2, pr, 1, m_ok, one, 2) || !refused(o2, -1, pr, 1, m_ok, one, 2) ||
        !refused(o2, 2, pr, -1, m_ok, one, 2) || !refused(o2, 2, pr, 1, m_ok, one, 1) ||
        !refused(down, 2, pr, 1, m_ok, one, 2) || !refused(neg, 2, pr, 1, m_ok, one, 2) ||
        !refused(huge, 2, nullptr, 0, nullptr, nullptr, 2) || !refused(o2, 2, nullptr, 1, m_ok, one, 2) ||
        !refused(o2, 2, pr, 1, m_ok, nullptr, 2) || !refused(o2, 2, pr, 1, nullptr, one, 2) ||
        !refused(o2, 2, pr_bad, 1, m_ok, one, 2) || !refused(o2, 2, pr_neg, 1, m_ok, one, 2) ||
        !refused(o2, 2, pr, 1, m_ok, minus, 2) || !refused(o2, 2, pr, 1, m_hi, one, 2) ||
        !refused(o2, 2, pr, 1, m_hj, one, 2) || !refused(o2, 2, pr, 1, m_neg, one, 2))
        return printf("check_args accepts a bad call\n"), 1;
    printf("tracks ok\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3) return file_mode(argv[1], argv[2]);
    if (argc == 1) return self_test();
    fprintf(stderr, "usage: tracks_check [<cases in> <results out>]\n");
    return 2;
}
