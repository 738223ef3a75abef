// Stand-alone check of csrc/sift_geom.h (no HIP, no library): self-checks of the sampler, the two
// solvers and the planner, and a file mode that runs sgeo::estimate_host on a scene written by a
// test (tests/test_geom.py under sanitizers; tests/test_gpu_estimate.py for the expected values of
// the device call; tests/estimate_images_time.py for the host timing).
//
//   geom_check                 self-checks; prints "geom ok"
//   geom_check info            prints "tile <kMatchTile> block <kBlockHyp>"
//   geom_check run DIR [reps]  reads DIR/{params,loc,offsets,pairs,matches,counts}.bin, writes
//                              DIR/{models,inliers,mask}.bin; prints the host time per repeat (ms)
//     params.bin  int32 model, int32 iterations, uint32 seed, float32 threshold
//     loc.bin     float32 [rows][2]       offsets.bin int64 [nsets + 1]
//     pairs.bin   int32 [npairs][2]       matches.bin int32 [total][2]    counts.bin int32 [npairs]
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "sift_geom.h"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

template <int S> static void check_sampler(int m) {
    std::set<int> seen;
    for (uint32_t t = 0; t < 2000; t++) {
        int idx[S];
        sgeo::sample<S>(12345u, 7u, t, m, idx);
        std::set<int> u;
        for (int k = 0; k < S; k++) {
            CHECK(idx[k] >= 0 && idx[k] < m);
            u.insert(idx[k]);
            seen.insert(idx[k]);
        }
        CHECK((int)u.size() == S);
        int again[S];
        sgeo::sample<S>(12345u, 7u, t, m, again);
        CHECK(std::memcmp(idx, again, sizeof(idx)) == 0);
    }
    // every index of a small set is drawn at some time
    if (m <= 9) CHECK((int)seen.size() == m);
    // another pair position or seed draws differently somewhere
    int differs = 0;
    for (uint32_t t = 0; t < 16 && m > S; t++) {
        int a[S], b[S], c[S];
        sgeo::sample<S>(1u, 0u, t, m, a);
        sgeo::sample<S>(1u, 1u, t, m, b);
        sgeo::sample<S>(2u, 0u, t, m, c);
        differs += std::memcmp(a, b, sizeof(a)) != 0 && std::memcmp(a, c, sizeof(a)) != 0;
    }
    CHECK(m == S || differs > 0);
}

static void check_h() {
    const double P[9] = {0.9, 0.05, 12.0, -0.04, 1.1, -7.0, 1e-4, -2e-4, 1.0};
    const double x1[4] = {10, 600, 580, 30}, y1[4] = {20, 40, 440, 400};
    double x2[4], y2[4];
    for (int i = 0; i < 4; i++) {
        const double w = P[6] * x1[i] + P[7] * y1[i] + P[8];
        x2[i] = (P[0] * x1[i] + P[1] * y1[i] + P[2]) / w;
        y2[i] = (P[3] * x1[i] + P[4] * y1[i] + P[5]) / w;
    }
    double H[9];
    CHECK(sgeo::solve_h(x1, y1, x2, y2, H));
    double n2 = 0;
    for (int i = 0; i < 9; i++) n2 += H[i] * H[i];
    CHECK(std::fabs(n2 - 1.0) < 1e-12);
    for (int i = 0; i < 4; i++) {
        const double w = H[6] * x1[i] + H[7] * y1[i] + H[8];
        CHECK(std::fabs((H[0] * x1[i] + H[1] * y1[i] + H[2]) / w - x2[i]) < sgeo::kSolveTol);
        CHECK(std::fabs((H[3] * x1[i] + H[4] * y1[i] + H[5]) / w - y2[i]) < sgeo::kSolveTol);
    }
    // a repeated point, three collinear points (either image): invalid
    double rx[4] = {10, 600, 10, 30}, ry[4] = {20, 40, 20, 400};
    CHECK(!sgeo::solve_h(rx, ry, x2, y2, H));
    CHECK(!sgeo::solve_h(x1, y1, rx, ry, H));
    double cx[4] = {0, 100, 200, 30}, cy[4] = {0, 50, 100, 400};
    CHECK(!sgeo::solve_h(cx, cy, x2, y2, H));
    CHECK(!sgeo::solve_h(x1, y1, cx, cy, H));
    double lx[4] = {10, 600, 580, 305}, ly[4] = {20, 40, 440, 30};   // the 4th on the line 1-2
    CHECK(!sgeo::solve_h(lx, ly, x2, y2, H));
}

// two pinhole views of 3-D points: view 1 = [I | 0], view 2 = [R | t]; f = 500, centre (320, 240)
static void project(const double R[9], const double t[3], int n, const double (*X)[3], double* x1,
                    double* y1, double* x2, double* y2) {
    for (int i = 0; i < n; i++) {
        x1[i] = 500 * X[i][0] / X[i][2] + 320;
        y1[i] = 500 * X[i][1] / X[i][2] + 240;
        double c[3];
        for (int r = 0; r < 3; r++)
            c[r] = R[3 * r] * X[i][0] + R[3 * r + 1] * X[i][1] + R[3 * r + 2] * X[i][2] + t[r];
        x2[i] = 500 * c[0] / c[2] + 320;
        y2[i] = 500 * c[1] / c[2] + 240;
    }
}

static void check_f() {
    const double X[8][3] = {{-1.5, -1.0, 4.2}, {1.2, -0.8, 5.1}, {0.3, 1.1, 6.3}, {-0.9, 0.7, 7.4},
                            {1.6, 1.3, 4.8},   {-0.2, -1.4, 5.9}, {0.8, 0.1, 7.9}, {-1.1, 0.2, 4.4}};
    const double a = 0.1, ca = std::cos(a), sa = std::sin(a);
    const double Ry[9] = {ca, 0, sa, 0, 1, 0, -sa, 0, ca};
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    // a general motion, and a sideways translation without rotation: F33 = 0 (and more of F)
    const double ts[2][3] = {{0.5, 0.1, 0.2}, {1.0, 0.0, 0.0}};
    const double* Rs[2] = {Ry, I};
    for (int c = 0; c < 2; c++) {
        double x1[8], y1[8], x2[8], y2[8], F[9];
        project(Rs[c], ts[c], 8, X, x1, y1, x2, y2);
        CHECK(sgeo::solve_f(x1, y1, x2, y2, F));
        double n2 = 0;
        for (int i = 0; i < 9; i++) n2 += F[i] * F[i];
        CHECK(std::fabs(n2 - 1.0) < 1e-12);
        for (int i = 0; i < 8; i++) {
            const double f0 = F[0] * x1[i] + F[1] * y1[i] + F[2];
            const double f1 = F[3] * x1[i] + F[4] * y1[i] + F[5];
            const double f2 = F[6] * x1[i] + F[7] * y1[i] + F[8];
            CHECK(std::fabs(x2[i] * f0 + y2[i] * f1 + f2) < sgeo::kSolveTol);
        }
        if (c == 1) CHECK(std::fabs(F[8]) < 1e-9 && std::fabs(F[0]) < 1e-9);
        // a repeated correspondence: rank below 8
        x1[5] = x1[2], y1[5] = y1[2], x2[5] = x2[2], y2[5] = y2[2];
        CHECK(!sgeo::solve_f(x1, y1, x2, y2, F));
    }
    double sx[8], sy[8], F[9];
    for (int i = 0; i < 8; i++) sx[i] = 100, sy[i] = 50;   // all the same point
    CHECK(!sgeo::solve_f(sx, sy, sx, sy, F));
}

static void check_predicate() {
    const float Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    CHECK(!sgeo::inlier(sgeo::kModelH, Z, 1, 2, 1, 2, 1e20f));
    CHECK(!sgeo::inlier(sgeo::kModelF, Z, 1, 2, 1, 2, 1e20f));
    const float T[9] = {1, 0, 3, 0, 1, -2, 0, 0, 1};
    CHECK(sgeo::inlier(sgeo::kModelH, T, 10, 10, 13, 8, 0.5f));
    CHECK(!sgeo::inlier(sgeo::kModelH, T, 10, 10, 13.5f, 8, 0.5f));
    CHECK(!sgeo::inlier(sgeo::kModelH, T, 10, 10, 13, 8.5f, 0.5f));
}

static void check_planner() {
    const int64_t off[5] = {5, 105, 105, 400, 1000};
    const int pairs[] = {0, 2, 2, 0, 1, 3, 0, 2, 3, 3, 2, 3, 0, 3};
    const int counts[] = {50, 3, 0, 4, 7, 8, 9};
    for (int model = 0; model < 2; model++) {
        const int S = sgeo::min_sample(model);
        for (int it : {1, 255, 256, 257, 1000, 65536}) {
            sgeo::Plan pl;
            CHECK(sgeo::build_plan(off, 4, pairs, 7, counts, model, it, pl) == sgeo::kPlanOk);
            CHECK(pl.pairs.size() == 7 && pl.total == 81);
            const int blocks = (it + sgeo::kBlockHyp - 1) / sgeo::kBlockHyp;
            std::set<std::pair<int, int>> seen;
            for (const sgeo::Item& i : pl.items) {
                CHECK(i.pair >= 0 && i.pair < 7 && i.block >= 0 && i.block < blocks);
                CHECK(counts[i.pair] >= S);
                CHECK(i.block * sgeo::kBlockHyp < it);
                CHECK(seen.insert({i.pair, i.block}).second);   // once
            }
            size_t want = 0;
            long long moff = 0;
            for (int p = 0; p < 7; p++) {
                want += counts[p] >= S ? blocks : 0;
                CHECK(pl.pairs[p].moff == moff && pl.pairs[p].m == counts[p]);
                CHECK(pl.pairs[p].a_off == off[pairs[2 * p]] && pl.pairs[p].b_off == off[pairs[2 * p + 1]]);
                moff += counts[p];
            }
            CHECK(seen.size() == want);   // every (pair, block) of a pair with a minimal sample
        }
    }
    sgeo::Plan pl;
    const int bad_pair[] = {0, 4}, neg_pair[] = {-1, 0}, one[] = {4}, neg[] = {-1}, ok_pair[] = {0, 2};
    const int64_t dec[3] = {0, 10, 9};
    CHECK(sgeo::build_plan(off, 4, bad_pair, 1, one, 0, 10, pl) == sgeo::kPlanBadArgument);
    CHECK(sgeo::build_plan(off, 4, neg_pair, 1, one, 0, 10, pl) == sgeo::kPlanBadArgument);
    CHECK(sgeo::build_plan(off, 4, ok_pair, 1, neg, 0, 10, pl) == sgeo::kPlanBadArgument);
    CHECK(sgeo::build_plan(dec, 2, ok_pair, 0, one, 0, 10, pl) == sgeo::kPlanBadArgument);
    CHECK(sgeo::build_plan(off, 4, ok_pair, 1, one, 0, 0, pl) == sgeo::kPlanBadArgument);
    CHECK(sgeo::build_plan(off, 4, ok_pair, 1, one, 0, 65537, pl) == sgeo::kPlanBadArgument);
    CHECK(sgeo::build_plan(off, 4, ok_pair, 1, one, 2, 10, pl) == sgeo::kPlanBadArgument);
    CHECK(sgeo::build_plan(off, 4, ok_pair, 1, one, 1, 65536, pl) == sgeo::kPlanOk && pl.items.empty());
    const int m_ok[] = {99, 294}, m_hi_i[] = {100, 0}, m_hi_j[] = {0, 295}, m_neg[] = {0, -1};
    const int c1[] = {1};
    CHECK(sgeo::check_matches(off, ok_pair, 1, m_ok, c1));
    CHECK(!sgeo::check_matches(off, ok_pair, 1, m_hi_i, c1));
    CHECK(!sgeo::check_matches(off, ok_pair, 1, m_hi_j, c1));
    CHECK(!sgeo::check_matches(off, ok_pair, 1, m_neg, c1));
}

template <class T> static std::vector<T> read_all(const std::string& path) {
    std::vector<T> v;
    FILE* f = std::fopen(path.c_str(), "rb");
    CHECK(f != nullptr);
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    CHECK(n >= 0 && n % (long)sizeof(T) == 0);
    v.resize((size_t)n / sizeof(T));
    if (n > 0) CHECK(std::fread(v.data(), 1, (size_t)n, f) == (size_t)n);
    std::fclose(f);
    return v;
}
template <class T> static void write_all(const std::string& path, const std::vector<T>& v) {
    FILE* f = std::fopen(path.c_str(), "wb");
    CHECK(f != nullptr);
    if (!v.empty()) CHECK(std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size());
    std::fclose(f);
}

static int run_files(const std::string& dir, int reps) {
    const auto params = read_all<int32_t>(dir + "/params.bin");
    CHECK(params.size() == 4);
    const int model = params[0], iterations = params[1];
    uint32_t seed;
    float threshold;
    std::memcpy(&seed, &params[2], 4);
    std::memcpy(&threshold, &params[3], 4);
    const auto loc = read_all<float>(dir + "/loc.bin");
    const auto off = read_all<int64_t>(dir + "/offsets.bin");
    const auto pairs = read_all<int32_t>(dir + "/pairs.bin");
    const auto matches = read_all<int32_t>(dir + "/matches.bin");
    const auto counts = read_all<int32_t>(dir + "/counts.bin");
    const int nsets = (int)off.size() - 1, npairs = (int)counts.size();
    CHECK(nsets >= 0 && pairs.size() == 2 * counts.size());
    sgeo::Plan pl;
    CHECK(sgeo::build_plan(off.data(), nsets, pairs.data(), npairs, counts.data(), model, iterations,
                           pl) == sgeo::kPlanOk);
    CHECK((size_t)pl.total * 2 == matches.size() && (size_t)off[nsets] * 2 <= loc.size());
    CHECK(sgeo::check_matches(off.data(), pairs.data(), npairs, matches.data(), counts.data()));
    std::vector<float> models((size_t)npairs * 9);
    std::vector<int32_t> inliers((size_t)npairs);
    std::vector<uint8_t> mask((size_t)pl.total);
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        sgeo::estimate_host(loc.data(), 2, off.data(), pairs.data(), npairs, matches.data(),
                            counts.data(), model, threshold, iterations, seed, models.data(),
                            inliers.data(), mask.data());
        const auto t1 = std::chrono::steady_clock::now();
        std::printf("host_ms %.3f\n", std::chrono::duration<double, std::milli>(t1 - t0).count());
    }
    write_all(dir + "/models.bin", models);
    write_all(dir + "/inliers.bin", inliers);
    write_all(dir + "/mask.bin", mask);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::string(argv[1]) == "info") {
        std::printf("tile %d block %d\n", sgeo::kMatchTile, sgeo::kBlockHyp);
        return 0;
    }
    if (argc >= 3 && std::string(argv[1]) == "run")
        return run_files(argv[2], argc >= 4 ? std::atoi(argv[3]) : 1);
    for (int m : {4, 5, 8, 9, 1000}) check_sampler<4>(m);
    for (int m : {8, 9, 1000}) check_sampler<8>(m);
    check_h();
    check_f();
    check_predicate();
    check_planner();
    std::printf("geom ok\n");
    return 0;
}
