// Stand-alone check of the local refinement of csrc/sift_geom.h (no HIP, no library): self-checks
// of the Jacobi eigen-solver and the refit, the sweep measurement behind sgeo::kJacobiSweeps, and
// a file mode that runs sgeo::refine_host on a scene written by a test (tests/test_geom_refine.py
// under sanitizers; tests/test_gpu_estimate_refine.py for the expected values of the device call).
//
//   geom_refine_check                  self-checks; prints "sweeps_random <max>" and "refine ok"
//   geom_refine_check info             prints "sweeps <kJacobiSweeps> lanes <kRefineLanes>"
//   geom_refine_check run DIR ROUNDS   reads DIR/{params,loc,offsets,pairs,matches,counts}.bin as
//                                      geom_check does, writes DIR/{models,inliers,mask,rounds}.bin;
//                                      prints "pair <p> rounds <accepted> stop <reason>" per pair
//                                      (budget, fixed point, rejected, invalid, no model) and
//                                      "sweeps_scene <max>": the sweeps the refit matrices of the
//                                      unrefined and of the returned models needed
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sift_geom.h"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

static uint32_t g_state = 0x2545F491u;
static double uniform() {   // [-1, 1)
    g_state = g_state * 1664525u + 1013904223u;
    return (double)(g_state >> 8) / 8388608.0 - 1.0;
}

static double frobenius(const double* A) {
    double s = 0;
    for (int i = 0; i < 81; i++) s += A[i] * A[i];
    return std::sqrt(s);
}
static double off_norm(const double* A) {
    double s = 0;
    for (int i = 0; i < 9; i++)
        for (int j = 0; j < 9; j++)
            if (i != j) s += A[9 * i + j] * A[9 * i + j];
    return std::sqrt(s);
}
// sweeps until the off-diagonal norm is <= 1e-14 of the Frobenius norm (40 = never)
static int sweeps_needed(const double* N45) {
    double A[81], V[81];
    sgeo::jacobi_start_host(N45, A, V);
    for (int s = 0; s < 40; s++) {
        if (off_norm(A) <= 1e-14 * frobenius(A)) return s;
        sgeo::jacobi_sweep_host(A, V);
    }
    return 40;
}
// the contract's solver on N: residual and minimality of the returned pair
static void check_eigen(const double* N45) {
    double A0[81], A[81], V[81], g[9];
    sgeo::jacobi_start_host(N45, A0, V);
    std::memcpy(A, A0, sizeof(A));
    sgeo::jacobi_host(A, V, g);
    const int c = sgeo::jacobi_min_index(A);
    const double lambda = A[10 * c];
    for (int i = 0; i < 9; i++) CHECK(lambda <= A[10 * i]);
    for (int i = 0; i < c; i++) CHECK(lambda < A[10 * i]);   // ties: the lowest index
    double r2 = 0, n2 = 0;
    for (int i = 0; i < 9; i++) {
        double v = -lambda * g[i];
        for (int j = 0; j < 9; j++) v += A0[9 * i + j] * g[j];
        r2 += v * v;
        n2 += g[i] * g[i];
    }
    CHECK(std::fabs(n2 - 1.0) < 1e-12);
    CHECK(std::sqrt(r2) <= 1e-12 * frobenius(A0));
}

static int check_jacobi() {
    double N[sgeo::kNormalEntries] = {0};
    const double diag[9] = {5, 3, 0.5, 7, 0.5, 2, 9, 4, 6};   // the smallest twice: index 2 wins
    int e = 0;
    for (int i = 0; i < 9; i++)
        for (int j = i; j < 9; j++) N[e++] = i == j ? diag[i] : 0.0;
    double A[81], V[81], g[9];
    sgeo::jacobi_start_host(N, A, V);
    sgeo::jacobi_host(A, V, g);
    for (int i = 0; i < 9; i++) CHECK(g[i] == (i == 2 ? 1.0 : 0.0) && A[10 * i] == diag[i]);
    CHECK(sweeps_needed(N) == 0);
    check_eigen(N);
    // 1,000 random PSD matrices B' B, B of 6 .. 14 rows (fewer than 9: singular, as a refit's)
    int worst = 0;
    for (int t = 0; t < 1000; t++) {
        const int rows = 6 + t % 9;
        const double scale = std::pow(10.0, (t % 7) - 3);
        for (int k = 0; k < sgeo::kNormalEntries; k++) N[k] = 0.0;
        for (int r = 0; r < rows; r++) {
            double a[9];
            for (int i = 0; i < 9; i++) a[i] = scale * uniform() * (i % 3 == 2 && t % 2 ? 1e-3 : 1.0);
            sgeo::normal_add(a, N);
        }
        check_eigen(N);
        const int s = sweeps_needed(N);
        worst = s > worst ? s : worst;
    }
    return worst;
}

// all n rows of pts inliers of M at threshold thr: the refit of exact data
static void check_exact() {
    // H: an affine map with dyadic entries on integer points is exact in float
    std::vector<float> pts;
    for (int i = 0; i < 100; i++) {
        const float x = (float)(int)(320 + 300 * uniform()), y = (float)(int)(240 + 220 * uniform());
        pts.insert(pts.end(), {x, y, 1.5f * x + 0.25f * y + 8.0f, -0.5f * x + 0.75f * y - 5.0f});
    }
    const double P[9] = {1.5, 0.25, 8, -0.5, 0.75, -5, 0, 0, 1};
    double U[9], D[9];
    float M[9];
    CHECK(sgeo::unit_norm(P, U));
    for (int i = 0; i < 9; i++) M[i] = (float)U[i];
    CHECK(sgeo::refit_host<sgeo::kModelH>(pts.data(), 100, M, 1.0f, D));
    double n2 = 0;
    for (int i = 0; i < 9; i++) n2 += D[i] * D[i];
    CHECK(std::fabs(n2 - 1.0) < 1e-12);
    for (int k = 0; k < 100; k++) {
        const double x = pts[4 * k], y = pts[4 * k + 1];
        const double w = D[6] * x + D[7] * y + D[8];
        CHECK(std::fabs((D[0] * x + D[1] * y + D[2]) / w - pts[4 * k + 2]) < sgeo::kSolveTol);
        CHECK(std::fabs((D[3] * x + D[4] * y + D[5]) / w - pts[4 * k + 3]) < sgeo::kSolveTol);
    }
    // the refit reads the inliers only: an outlier row changes nothing
    std::vector<float> more = pts;
    more.insert(more.begin() + 4 * 37, {50.f, 60.f, 400.f, 13.f});
    double D2[9];
    CHECK(sgeo::refit_host<sgeo::kModelH>(more.data(), 101, M, 1.0f, D2));
    for (int k = 0; k < 101; k++) {
        if (k == 37) continue;
        const double x = more[4 * k], y = more[4 * k + 1];
        const double w = D2[6] * x + D2[7] * y + D2[8];
        CHECK(std::fabs((D2[0] * x + D2[1] * y + D2[2]) / w - more[4 * k + 2]) < sgeo::kSolveTol);
    }
    // F: a sideways translation, integer points and disparities: x2' F x1 = y1 - y2 = 0 exactly
    pts.clear();
    for (int i = 0; i < 100; i++) {
        const float x = (float)(int)(320 + 250 * uniform()), y = (float)(int)(240 + 220 * uniform());
        pts.insert(pts.end(), {x, y, x + (float)(int)(30 + 25 * uniform()), y});
    }
    const double E[9] = {0, 0, 0, 0, 0, -1, 0, 1, 0};
    CHECK(sgeo::unit_norm(E, U));
    for (int i = 0; i < 9; i++) M[i] = (float)U[i];
    CHECK(sgeo::refit_host<sgeo::kModelF>(pts.data(), 100, M, 1.0f, D));
    n2 = 0;
    for (int i = 0; i < 9; i++) n2 += D[i] * D[i];
    CHECK(std::fabs(n2 - 1.0) < 1e-12);
    for (int k = 0; k < 100; k++) {
        const double x1 = pts[4 * k], y1 = pts[4 * k + 1], x2 = pts[4 * k + 2], y2 = pts[4 * k + 3];
        const double f0 = D[0] * x1 + D[1] * y1 + D[2], f1 = D[3] * x1 + D[4] * y1 + D[5];
        const double f2 = D[6] * x1 + D[7] * y1 + D[8];
        CHECK(std::fabs(x2 * f0 + y2 * f1 + f2) < sgeo::kSolveTol);
    }
    // the round loop on exact data: one accepted round, then the same mask
    int c = 100, why = -1;
    const int done = sgeo::refine_pair_host<sgeo::kModelF>(pts.data(), 100, 1.0f, 5, M, c, &why);
    CHECK(done == 1 && c == 100 && why == sgeo::kStopFixedPoint);
    // fewer inliers than the minimal sample; every point at one location
    CHECK(!sgeo::refit_host<sgeo::kModelF>(pts.data(), 7, M, 1.0f, D));
    std::vector<float> same;
    for (int i = 0; i < 20; i++) same.insert(same.end(), {100.5f, 50.25f, 100.5f, 50.25f});
    const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    CHECK(sgeo::inlier(sgeo::kModelH, I, 100.5f, 50.25f, 100.5f, 50.25f, 1.0f));
    CHECK(!sgeo::refit_host<sgeo::kModelH>(same.data(), 20, I, 1.0f, D));
    float J[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    c = 20;
    CHECK(sgeo::refine_pair_host<sgeo::kModelH>(same.data(), 20, 1.0f, 3, J, c, &why) == 0);
    CHECK(why == sgeo::kStopInvalid && c == 20 && std::memcmp(I, J, sizeof(I)) == 0);
    c = 3;
    CHECK(sgeo::refine_pair_host<sgeo::kModelH>(same.data(), 20, 1.0f, 3, J, c, &why) == 0);
    CHECK(why == sgeo::kStopNoModel);
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

static int scene_sweeps(int model, const std::vector<float>& pts, const float* M, float threshold) {
    sgeo::RefitNorm nm;
    double N[sgeo::kNormalEntries];
    const int m = (int)(pts.size() / 4);
    const bool ok = model == sgeo::kModelF
                        ? sgeo::refit_normal_host<sgeo::kModelF>(pts.data(), m, M, threshold, nm, N)
                        : sgeo::refit_normal_host<sgeo::kModelH>(pts.data(), m, M, threshold, nm, N);
    return ok ? sweeps_needed(N) : 0;
}

static int run_files(const std::string& dir, int rounds) {
    const auto params = read_all<int32_t>(dir + "/params.bin");
    CHECK(params.size() == 4 && rounds >= 0 && rounds <= sgeo::kMaxRefineRounds);
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
    std::vector<float> models((size_t)npairs * 9), first((size_t)npairs * 9);
    std::vector<int32_t> inliers((size_t)npairs), none((size_t)npairs), done((size_t)npairs),
        stop((size_t)npairs);
    std::vector<uint8_t> mask((size_t)pl.total);
    sgeo::estimate_host(loc.data(), 2, off.data(), pairs.data(), npairs, matches.data(), counts.data(),
                        model, threshold, iterations, seed, first.data(), none.data(), nullptr);
    sgeo::refine_host(loc.data(), 2, off.data(), pairs.data(), npairs, matches.data(), counts.data(),
                      model, threshold, iterations, seed, rounds, models.data(), inliers.data(),
                      mask.data(), done.data(), stop.data());
    static const char* kWhy[] = {"budget", "fixed point", "rejected", "invalid", "no model"};
    int worst = 0;
    long long moff = 0;
    for (int p = 0; p < npairs; p++) {
        std::printf("pair %d rounds %d stop %s\n", p, done[p], kWhy[stop[p]]);
        std::vector<float> pts;
        for (int k = 0; k < counts[p]; k++) {
            const float* a = &loc[2 * (off[pairs[2 * p]] + matches[2 * (moff + k)])];
            const float* b = &loc[2 * (off[pairs[2 * p + 1]] + matches[2 * (moff + k) + 1])];
            pts.insert(pts.end(), {a[0], a[1], b[0], b[1]});
        }
        for (const float* M : {&first[9 * (size_t)p], &models[9 * (size_t)p]}) {
            const int s = scene_sweeps(model, pts, M, threshold);
            worst = s > worst ? s : worst;
        }
        moff += counts[p];
    }
    std::printf("sweeps_scene %d\n", worst);
    write_all(dir + "/models.bin", models);
    write_all(dir + "/inliers.bin", inliers);
    write_all(dir + "/mask.bin", mask);
    write_all(dir + "/rounds.bin", done);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::string(argv[1]) == "info") {
        std::printf("sweeps %d lanes %d\n", sgeo::kJacobiSweeps, sgeo::kRefineLanes);
        return 0;
    }
    if (argc >= 4 && std::string(argv[1]) == "run") return run_files(argv[2], std::atoi(argv[3]));
    const int worst = check_jacobi();
    std::printf("sweeps_random %d\n", worst);
    CHECK(worst + 2 <= sgeo::kJacobiSweeps);
    check_exact();
    std::printf("refine ok\n");
    return 0;
}
