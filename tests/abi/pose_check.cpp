// Stand-alone check of csrc/sift_pose.h (no HIP, no library): self-checks of the decomposition and
// the triangulation, the Jacobi sweep measurement, and a file mode that runs spose::pose_host on a
// pair list written by a test (tests/test_pose.py under sanitizers; tests/test_gpu_pose.py for the
// expected values of the device call; tests/pose_time.py for the host timing).
//
//   pose_check                 self-checks; prints "sweeps_max <n>" over 1,000 random E and "pose ok"
//   pose_check info            prints "sweeps <kPoseSweeps> ratio <kSigmaRatioMin> eps <kParallelEps>"
//   pose_check run DIR [reps]  reads DIR/{params,loc,offsets,intrinsics,pairs,matches,counts,F}.bin,
//                              writes DIR/{R,t,out_counts,mask,points,front}.bin; prints
//                              "sweeps_max <n>" over the list's E and the host time per repeat (ms)
//     params.bin      float32 f_threshold, float32 min_angle
//     loc.bin         float32 [rows][2]       offsets.bin int64 [nsets + 1]
//     intrinsics.bin  float32 [nsets][4]      F.bin       float32 [npairs][9]
//     pairs.bin       int32 [npairs][2]       matches.bin int32 [total][2]    counts.bin int32 [npairs]
//     front.bin       int32 [npairs][4]: every candidate's in-front count
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "sift_pose.h"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

// sweeps until the off-diagonal Frobenius norm of E'E is <= 1e-14 of the matrix's
static int sweeps_needed(const double* E) {
    double A[9], V[9];
    spose::gram_start(E, A, V);
    for (int s = 0; s <= 50; s++) {
        double all = 0, off = 0;
        for (int i = 0; i < 9; i++) {
            all += A[i] * A[i];
            if (i % 4 != 0) off += A[i] * A[i];
        }
        if (std::sqrt(off) <= 1e-14 * std::sqrt(all)) return s;
        spose::jacobi3_sweep(A, V);
    }
    return 51;
}

struct Rng {
    uint64_t s;
    double uniform() {   // [0, 1)
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        return (double)(s >> 11) * (1.0 / 9007199254740992.0);
    }
    double sym() { return 2.0 * uniform() - 1.0; }
};

static void rotation(double ax, double ay, double az, double* R) {
    const double cx = std::cos(ax), sx = std::sin(ax), cy = std::cos(ay), sy = std::sin(ay);
    const double cz = std::cos(az), sz = std::sin(az);
    const double Rx[9] = {1, 0, 0, 0, cx, -sx, 0, sx, cx}, Ry[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy};
    const double Rz[9] = {cz, -sz, 0, sz, cz, 0, 0, 0, 1};
    double T[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            T[3 * i + j] = 0;
            for (int k = 0; k < 3; k++) T[3 * i + j] += Ry[3 * i + k] * Rx[3 * k + j];
        }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            R[3 * i + j] = 0;
            for (int k = 0; k < 3; k++) R[3 * i + j] += Rz[3 * i + k] * T[3 * k + j];
        }
}
// E = [t]x R
static void essential_of(const double* R, const double* t, double* E) {
    const double S[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            E[3 * i + j] = 0;
            for (int k = 0; k < 3; k++) E[3 * i + j] += S[3 * i + k] * R[3 * k + j];
        }
}

// 500 essential matrices of random motions, perturbed by up to 1e-3 per entry, and 500 matrices of
// random entries, all at unit norm
static int measure_random_sweeps() {
    Rng g{20240521};
    int worst = 0;
    for (int n = 0; n < 1000; n++) {
        double M[9], E[9];
        if (n < 500) {
            double R[9], t[3] = {g.sym(), g.sym(), g.sym()};
            rotation(g.sym(), g.sym(), g.sym(), R);
            essential_of(R, t, M);
            for (int i = 0; i < 9; i++) M[i] += 1e-3 * g.sym();
        } else {
            for (int i = 0; i < 9; i++) M[i] = g.sym();
        }
        CHECK(sgeo::unit_norm(M, E));
        worst = std::max(worst, sweeps_needed(E));
    }
    return worst;
}

static double det3x3(const double* R) {
    return R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) +
           R[2] * (R[3] * R[7] - R[4] * R[6]);
}

// a planted motion between two cameras of different intrinsics: the decomposition holds the
// planted (R, t) as exactly one of its candidates, every candidate is a rotation, and a point in
// front of both cameras triangulates to itself under that candidate alone
static void check_planted() {
    const float Ka[4] = {500, 520, 320, 240}, Kb[4] = {610, 600, 300, 260};
    double R0[9], t0[3] = {0.6, 0.05, 0.1};
    rotation(-0.03, 0.08, 0.01, R0);
    const double tn = std::sqrt(t0[0] * t0[0] + t0[1] * t0[1] + t0[2] * t0[2]);
    double E0[9];
    essential_of(R0, t0, E0);
    // F = inv(Kb)' E inv(Ka), at unit norm, as float
    const double iKa[9] = {1.0 / Ka[0], 0, -Ka[2] / (double)Ka[0], 0, 1.0 / Ka[1], -Ka[3] / (double)Ka[1], 0, 0, 1};
    const double iKb[9] = {1.0 / Kb[0], 0, -Kb[2] / (double)Kb[0], 0, 1.0 / Kb[1], -Kb[3] / (double)Kb[1], 0, 0, 1};
    double T[9], Fd[9], Fn[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            T[3 * i + j] = 0;
            for (int k = 0; k < 3; k++) T[3 * i + j] += E0[3 * i + k] * iKa[3 * k + j];
        }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            Fd[3 * i + j] = 0;
            for (int k = 0; k < 3; k++) Fd[3 * i + j] += iKb[3 * k + i] * T[3 * k + j];
        }
    CHECK(sgeo::unit_norm(Fd, Fn));
    float F[9];
    for (int i = 0; i < 9; i++) F[i] = (float)Fn[i];
    spose::Pose P;
    CHECK(spose::decompose(F, Ka, Kb, P));
    spose::Cams cam;
    spose::cameras(Ka, Kb, cam);
    const double X0[3] = {0.4, -0.3, 5.0};
    double Y0[3];
    for (int i = 0; i < 3; i++) Y0[i] = R0[3 * i] * X0[0] + R0[3 * i + 1] * X0[1] + R0[3 * i + 2] * X0[2] + t0[i];
    const float x1 = (float)(Ka[0] * X0[0] / X0[2] + Ka[2]), y1 = (float)(Ka[1] * X0[1] / X0[2] + Ka[3]);
    const float x2 = (float)(Kb[0] * Y0[0] / Y0[2] + Kb[2]), y2 = (float)(Kb[1] * Y0[1] / Y0[2] + Kb[3]);
    const int bits = spose::front_bits(cam, P, x1, y1, x2, y2);
    int planted = -1;
    for (int k = 0; k < 4; k++) {
        double R[9], t[3];
        spose::candidate(P, k, R, t);
        CHECK(std::fabs(det3x3(R) - 1.0) < 1e-9);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                double d = 0;
                for (int l = 0; l < 3; l++) d += R[3 * l + i] * R[3 * l + j];
                CHECK(std::fabs(d - (i == j ? 1.0 : 0.0)) < 1e-9);
            }
        double dr = 0, dt = 0;
        for (int i = 0; i < 9; i++) dr = std::max(dr, std::fabs(R[i] - R0[i]));
        for (int i = 0; i < 3; i++) dt = std::max(dt, std::fabs(t[i] - t0[i] / tn));
        if (dr < 1e-5 && dt < 1e-5) {
            CHECK(planted < 0);
            planted = k;
        }
    }
    CHECK(planted >= 0 && bits == (1 << planted));
    double R[9], t[3];
    spose::candidate(P, planted, R, t);
    float X[3];
    bool wd = false;
    CHECK(spose::resolve(cam, R, t, std::cos(0.01), x1, y1, x2, y2, X, &wd));
    for (int i = 0; i < 3; i++) CHECK(std::fabs(X[i] * tn - X0[i]) < 1e-2);
    // the rays meet under 6.5 degrees or so: wide at 1 degree, not at 30
    CHECK(wd);
    CHECK(spose::resolve(cam, R, t, std::cos(0.5), x1, y1, x2, y2, X, &wd) && !wd);
    // no pose: zero, rank 1, a NaN, an infinity
    float Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, R1[9], N[9], I[9];
    const float u[3] = {0.3f, -0.5f, 0.8f}, v[3] = {1e-3f, 2e-3f, 0.9f};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R1[3 * i + j] = u[i] * v[j];
    std::memcpy(N, F, sizeof(N));
    std::memcpy(I, F, sizeof(I));
    N[4] = std::numeric_limits<float>::quiet_NaN();
    I[2] = std::numeric_limits<float>::infinity();
    CHECK(!spose::decompose(Z, Ka, Kb, P));
    CHECK(!spose::decompose(R1, Ka, Kb, P));
    CHECK(!spose::decompose(N, Ka, Kb, P));
    CHECK(!spose::decompose(I, Ka, Kb, P));
    const int f1[4] = {3, 7, 7, 2}, f2[4] = {0, 0, 0, 0}, f3[4] = {1, 1, 1, 5};
    int most = -1;
    CHECK(spose::winner(f1, &most) == 1 && most == 7);
    CHECK(spose::winner(f2, &most) == 0 && most == 0);
    CHECK(spose::winner(f3, &most) == 3 && most == 5);
}

static void check_arguments() {
    const int64_t off[3] = {0, 4, 8};
    const float K[8] = {500, 500, 320, 240, 600, 600, 300, 200};
    const int pairs[2] = {0, 1}, m[4] = {0, 1, 3, 3}, counts[1] = {2};
    const float F[9] = {0, 0, 0, 0, 0, -1, 0, 1, 0};
    float R[9], t[3];
    int c[3];
    sgeo::Plan pl;
    const char* why = nullptr;
    auto call = [&](const float* Kx, float thr, float ang, const float* Fx, const int* mx) {
        return spose::check_args(off, 2, Kx, pairs, 1, mx, counts, Fx, thr, ang, R, t, c, pl, &why);
    };
    CHECK(call(K, 4.f, 0.03f, F, m) == spose::kArgsOk && pl.pairs.size() == 1 && pl.total == 2);
    CHECK(call(K, 0.f, 0.f, F, m) == spose::kArgsOk);
    CHECK(call(K, 1e20f, (float)spose::kHalfPi, F, m) == spose::kArgsOk);
    CHECK(call(K, -1.f, 0.03f, F, m) == spose::kArgsBad);
    CHECK(call(K, std::numeric_limits<float>::infinity(), 0.03f, F, m) == spose::kArgsBad);
    CHECK(call(K, std::numeric_limits<float>::quiet_NaN(), 0.03f, F, m) == spose::kArgsBad);
    CHECK(call(K, 4.f, -0.01f, F, m) == spose::kArgsBad);
    CHECK(call(K, 4.f, 1.58f, F, m) == spose::kArgsBad);
    CHECK(call(K, 4.f, std::numeric_limits<float>::quiet_NaN(), F, m) == spose::kArgsBad);
    CHECK(call(nullptr, 4.f, 0.03f, F, m) == spose::kArgsBad);
    CHECK(call(K, 4.f, 0.03f, nullptr, m) == spose::kArgsBad);
    CHECK(call(K, 4.f, 0.03f, F, nullptr) == spose::kArgsBad);
    const int far[4] = {0, 1, 4, 3};
    CHECK(call(K, 4.f, 0.03f, F, far) == spose::kArgsBad);
    for (int e = 0; e < 8; e++) {
        float B[8];
        std::memcpy(B, K, sizeof(B));
        B[e] = std::numeric_limits<float>::quiet_NaN();
        CHECK(call(B, 4.f, 0.03f, F, m) == spose::kArgsBad);
        B[e] = std::numeric_limits<float>::infinity();
        CHECK(call(B, 4.f, 0.03f, F, m) == spose::kArgsBad);
        if (e % 4 < 2) {
            B[e] = 0.f;
            CHECK(call(B, 4.f, 0.03f, F, m) == spose::kArgsBad);
            B[e] = -500.f;
            CHECK(call(B, 4.f, 0.03f, F, m) == spose::kArgsBad);
        }
    }
    // a set that no pair names may hold anything
    const int64_t off3[4] = {0, 4, 8, 8};
    float K3[12];
    std::memcpy(K3, K, sizeof(K));
    for (int e = 8; e < 12; e++) K3[e] = std::numeric_limits<float>::quiet_NaN();
    CHECK(spose::check_args(off3, 3, K3, pairs, 1, m, counts, F, 4.f, 0.03f, R, t, c, pl, &why) == spose::kArgsOk);
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
    const auto params = read_all<float>(dir + "/params.bin");
    CHECK(params.size() == 2);
    const auto loc = read_all<float>(dir + "/loc.bin");
    const auto off = read_all<int64_t>(dir + "/offsets.bin");
    const auto K = read_all<float>(dir + "/intrinsics.bin");
    const auto pairs = read_all<int32_t>(dir + "/pairs.bin");
    const auto matches = read_all<int32_t>(dir + "/matches.bin");
    const auto counts = read_all<int32_t>(dir + "/counts.bin");
    const auto F = read_all<float>(dir + "/F.bin");
    const int nsets = (int)off.size() - 1, npairs = (int)counts.size();
    CHECK(nsets >= 0 && pairs.size() == 2 * counts.size() && F.size() == 9 * counts.size());
    CHECK(K.size() == 4 * (size_t)nsets);
    std::vector<float> R((size_t)npairs * 9), t((size_t)npairs * 3);
    std::vector<int32_t> oc((size_t)npairs * 3), front((size_t)npairs * 4);
    sgeo::Plan pl;
    const char* why = "";
    const int rc = spose::check_args(off.data(), nsets, K.data(), pairs.data(), npairs, matches.data(),
                                     counts.data(), F.data(), params[0], params[1], R.data(), t.data(),
                                     oc.data(), pl, &why);
    if (rc != spose::kArgsOk) std::printf("check_args: %s\n", why);
    CHECK(rc == spose::kArgsOk);
    CHECK((size_t)pl.total * 2 == matches.size() && (size_t)off[nsets] * 2 <= loc.size());
    std::vector<uint8_t> mask((size_t)pl.total);
    std::vector<float> points((size_t)pl.total * 3);
    int worst = 0;
    for (int p = 0; p < npairs; p++) {
        double E[9];
        if (counts[p] > 0 && spose::essential(F.data() + 9 * (size_t)p, K.data() + 4 * (size_t)pairs[2 * p],
                                              K.data() + 4 * (size_t)pairs[2 * p + 1], E))
            worst = std::max(worst, sweeps_needed(E));
    }
    std::printf("sweeps_max %d\n", worst);
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        spose::pose_host(loc.data(), 2, off.data(), K.data(), pairs.data(), npairs, matches.data(),
                         counts.data(), F.data(), params[0], params[1], R.data(), t.data(), oc.data(),
                         mask.data(), points.data(), front.data());
        const auto t1 = std::chrono::steady_clock::now();
        std::printf("host_ms %.3f\n", std::chrono::duration<double, std::milli>(t1 - t0).count());
    }
    write_all(dir + "/R.bin", R);
    write_all(dir + "/t.bin", t);
    write_all(dir + "/out_counts.bin", oc);
    write_all(dir + "/mask.bin", mask);
    write_all(dir + "/points.bin", points);
    write_all(dir + "/front.bin", front);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::string(argv[1]) == "info") {
        std::printf("sweeps %d ratio %.17g eps %.17g\n", spose::kPoseSweeps, spose::kSigmaRatioMin,
                    spose::kParallelEps);
        return 0;
    }
    if (argc >= 3 && std::string(argv[1]) == "run")
        return run_files(argv[2], argc >= 4 ? std::atoi(argv[3]) : 1);
    check_planted();
    check_arguments();
    std::printf("sweeps_max %d\n", measure_random_sweeps());
    std::printf("pose ok\n");
    return 0;
}
