// sift_geom.h -- the geometry estimator of sgpu_estimate_batch: sampler, the two minimal solvers,
// the inlier predicate, a host loop that implements the whole contract, and the planner.  Plain
// C++, no HIP: SGEO_HD is `__host__ __device__` under hipcc and nothing under g++, so that a
// host-only program can check every function the kernels run (tests/abi/geom_check.cpp).
//
// Contract.  Pair position p with m matches {i, j} (x1 = set a's point i, x2 =
// set b's point j) and hypotheses t = 0 .. iterations - 1:
//   sample   S = 4 (H) or 8 (F) distinct match indices, a virtual Fisher-Yates shuffle whose k-th
//            draw is hash(seed, p, t, k) mod (m - k): a pure function of those four numbers;
//   solve    in double, round to float[9] at unit Frobenius norm;
//   score    the guided matcher's own test in float (inlier()), counted over all m matches;
//   winner   the most inliers, then the lowest t; a pair with m < S or no valid hypothesis has no
//            model: zeros, 0 inliers, a zero mask.
//   refine   (sgpu_estimate_*_refined only) up to `rounds` least-squares refits of the winner on
//            its inliers, each accepted only when it loses no inlier: "local refinement" below.
// F is the minimal-sample solution WITHOUT rank-2 enforcement: the Sampson test does not need it; a
// caller that wants epipoles enforces rank 2 itself.
//
// Floating point: compiled without contraction on both sides, every fma is
// written out, double steps stay double, divisions and the one square root are IEEE.  Host and
// device therefore produce the same bits.  The solvers use named scalars and fully unrolled
// compile-time indices only: a runtime-indexed per-lane array would live in scratch memory.
#ifndef SIFT_GEOM_H
#define SIFT_GEOM_H
#include <algorithm>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define SGEO_HD __host__ __device__ inline
#else
#define SGEO_HD inline
#endif
#if defined(__clang__)
#define SGEO_UNROLL _Pragma("unroll")
#else
#define SGEO_UNROLL
#endif

namespace sgeo {

constexpr int kModelH = 0, kModelF = 1;   // SGPU_MODEL_HOMOGRAPHY / SGPU_MODEL_FUNDAMENTAL
constexpr int kBlockHyp = 256;            // hypotheses per work item: one per lane of a workgroup
constexpr int kMatchTile = 512;           // matches (float4) staged through LDS at a time
constexpr int kMaxIterations = 65536;

// Degeneracy thresholds, in double.
//   kAreaEps   H: a triple of sample points (either image) whose determinant -- twice the
//              triangle's area, in square pixels -- is at most this in magnitude counts as
//              collinear (a repeated point gives exactly 0).
//   kPivotEps  F: a pivot of the normalised 8 x 9 system (entries of order 1) at most this in
//              magnitude, or a sample whose mean absolute deviation from its centroid is at most
//              this many pixels, makes the sample invalid.
//   kSolveTol  what the solvers guarantee on an exact, well-spread sample, and the tolerance of
//              the self-checks: H maps its four points back within kSolveTol pixels, and the
//              unit-norm F gives |x2' F x1| <= kSolveTol on its eight correspondences (double
//              arithmetic on coordinates below 2^11 loses about 2^22 * 2^-53 ~ 5e-10 relative in
//              the products; 1e-7 leaves two orders for the elimination's growth).
constexpr double kAreaEps = 1e-9;
constexpr double kPivotEps = 1e-10;
constexpr double kSolveTol = 1e-7;

SGEO_HD int min_sample(int model) { return model == kModelF ? 8 : 4; }

// ---- sampler ---------------------------------------------------------------------------------

SGEO_HD uint32_t fmix32(uint32_t x) {   // the 32-bit finaliser of MurmurHash3
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}
// counter-based: no state, a function of (seed, pair position, hypothesis, draw number) alone
SGEO_HD uint32_t draw_hash(uint32_t seed, uint32_t p, uint32_t t, uint32_t k) {
    uint32_t x = fmix32(seed * 0x9E3779B1u + p);
    x = fmix32(x * 0x85EBCA77u + t);
    return fmix32(x * 0xC2B2AE3Du + k);
}
// S distinct indices in [0, m), m >= S: step k of a Fisher-Yates shuffle of 0 .. m - 1 swaps
// position k with position j_k = k + hash mod (m - k).  The array is virtual: position j_k holds
// its own index unless an earlier step i wrote position i's value there, which is traced back.
template <int S>
SGEO_HD void sample(uint32_t seed, uint32_t p, uint32_t t, int m, int idx[S]) {
    int j[S];
    SGEO_UNROLL
    for (int k = 0; k < S; k++) {
        j[k] = k + (int)(draw_hash(seed, p, t, (uint32_t)k) % (uint32_t)(m - k));
        int v = j[k];
        SGEO_UNROLL
        for (int i = k - 1; i >= 0; i--)
            if (j[i] == v) v = i;
        idx[k] = v;
    }
}

// ---- inlier predicate ------------------------------------------------------------------------

// The guided matcher's test of one match under M, in the float operation order of
// oracle::guided_pass, k_guided_mask and guided_words (a / b = a * (1 / b)): exactly what a guided
// pass says about M with the other test disabled.
//   H: |H x1 - x2| < threshold in both coordinates;  F: Sampson error of x2' F x1 < threshold
//   (squared pixels).  A zero matrix passes nothing (0 * inf is NaN).
SGEO_HD bool inlier(int model, const float* M, float x1, float y1, float x2, float y2,
                    float threshold) {
    if (model == kModelH) {
        const float h0 = __builtin_fmaf(M[0], x1, __builtin_fmaf(M[1], y1, M[2]));
        const float h1 = __builtin_fmaf(M[3], x1, __builtin_fmaf(M[4], y1, M[5]));
        const float h2 = __builtin_fmaf(M[6], x1, __builtin_fmaf(M[7], y1, M[8]));
        const float rh = 1.0f / h2;
        const float d0 = __builtin_fabsf(h0 * rh - x2), d1 = __builtin_fabsf(h1 * rh - y2);
        return (d0 < threshold) & (d1 < threshold);
    }
    const float f0 = __builtin_fmaf(M[0], x1, __builtin_fmaf(M[1], y1, M[2]));
    const float f1 = __builtin_fmaf(M[3], x1, __builtin_fmaf(M[4], y1, M[5]));
    const float f2 = __builtin_fmaf(M[6], x1, __builtin_fmaf(M[7], y1, M[8]));
    const float t0 = __builtin_fmaf(M[0], x2, __builtin_fmaf(M[3], y2, M[6]));
    const float t1 = __builtin_fmaf(M[1], x2, __builtin_fmaf(M[4], y2, M[7]));
    const float x2fx1 = __builtin_fmaf(x2, f0, __builtin_fmaf(y2, f1, f2));
    float den = f0 * f0;
    den = __builtin_fmaf(f1, f1, den);
    den = __builtin_fmaf(t0, t0, den);
    den = __builtin_fmaf(t1, t1, den);
    const float se = (x2fx1 * x2fx1) * (1.0f / den);
    return se < threshold;
}

// ---- solvers ---------------------------------------------------------------------------------

// scale to unit Frobenius norm; false when the norm is zero, infinite or NaN
SGEO_HD bool unit_norm(const double* M, double* out) {
    double n2 = M[0] * M[0];
    SGEO_UNROLL
    for (int i = 1; i < 9; i++) n2 = __builtin_fma(M[i], M[i], n2);
    if (!(n2 > 0.0 && n2 < 1.0e300)) return false;
    const double inv = 1.0 / __builtin_sqrt(n2);
    SGEO_UNROLL
    for (int i = 0; i < 9; i++) out[i] = M[i] * inv;
    return true;
}

// det [p q r] of three points (x, y, 1): twice the signed area of their triangle
SGEO_HD double det3(double px, double py, double qx, double qy, double rx, double ry) {
    const double ax = qx - px, ay = qy - py, bx = rx - px, by = ry - py;
    return __builtin_fma(ax, by, -(ay * bx));
}

// One image's part of the four-point closed form.  n_i = p_j x p_k (i, j, k cyclic) are the rows of
// adj [p1 p2 p3]; l_i = n_i . p4.  [l1 p1, l2 p2, l3 p3] maps the canonical frame (e1, e2, e3,
// (1, 1, 1)) onto (p1, p2, p3, p4) up to scale.  False when three of the points are collinear.
struct Frame4 {
    double n[3][3];   // n_i
    double l[3];      // l_i
};
SGEO_HD bool frame4(const double* x, const double* y, Frame4& f) {
    SGEO_UNROLL
    for (int i = 0; i < 3; i++) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        f.n[i][0] = y[j] - y[k];
        f.n[i][1] = x[k] - x[j];
        f.n[i][2] = __builtin_fma(x[j], y[k], -(x[k] * y[j]));
        f.l[i] = det3(x[j], y[j], x[k], y[k], x[3], y[3]);
    }
    const double d = det3(x[0], y[0], x[1], y[1], x[2], y[2]);
    bool ok = __builtin_fabs(d) > kAreaEps;
    SGEO_UNROLL
    for (int i = 0; i < 3; i++) ok = ok & (__builtin_fabs(f.l[i]) > kAreaEps);
    return ok;
}

// Homography of four correspondences (x1, y1) -> (x2, y2), row-major, unit Frobenius norm:
// H = [m1 q1, m2 q2, m3 q3] adj [l1 p1, l2 p2, l3 p3] up to scale = sum_i (m_i / l_i) q_i n_i'.
// No pivoting, no runtime indices.
SGEO_HD bool solve_h(const double* x1, const double* y1, const double* x2, const double* y2,
                     double* H) {
    Frame4 a, b;
    const bool oka = frame4(x1, y1, a);
    const bool okb = frame4(x2, y2, b);
    if (!(oka & okb)) return false;
    double w[3];
    SGEO_UNROLL
    for (int i = 0; i < 3; i++) w[i] = b.l[i] / a.l[i];
    double M[9];
    SGEO_UNROLL
    for (int c = 0; c < 3; c++) {
        M[c] = __builtin_fma(w[2] * x2[2], a.n[2][c],
                             __builtin_fma(w[1] * x2[1], a.n[1][c], (w[0] * x2[0]) * a.n[0][c]));
        M[3 + c] = __builtin_fma(w[2] * y2[2], a.n[2][c],
                                 __builtin_fma(w[1] * y2[1], a.n[1][c], (w[0] * y2[0]) * a.n[0][c]));
        M[6 + c] = __builtin_fma(w[2], a.n[2][c], __builtin_fma(w[1], a.n[1][c], w[0] * a.n[0][c]));
    }
    return unit_norm(M, H);
}

// isotropic normalisation of eight points: centroid to the origin, mean absolute deviation per
// coordinate to 1 (no square root); u = s (x - cx)
SGEO_HD bool normalise8(const double* x, const double* y, double& cx, double& cy, double& s) {
    double sx = x[0], sy = y[0];
    SGEO_UNROLL
    for (int i = 1; i < 8; i++) {
        sx += x[i];
        sy += y[i];
    }
    cx = sx * 0.125;
    cy = sy * 0.125;
    double d = 0.0;
    SGEO_UNROLL
    for (int i = 0; i < 8; i++) d += __builtin_fabs(x[i] - cx) + __builtin_fabs(y[i] - cy);
    d *= 0.0625;
    if (!(d > kPivotEps)) return false;
    s = 1.0 / d;
    return true;
}

// Fundamental matrix of eight correspondences, x2' F x1 = 0, row-major, unit Frobenius norm, no
// rank-2 enforcement.  The null vector of the normalised 8 x 9 system by Gaussian elimination with
// complete pivoting (ties: the first position in row-major order), so that a vanishing F33 -- or
// any other entry -- is no obstacle; rows and columns are exchanged by selects over compile-time
// positions.
SGEO_HD bool solve_f(const double* x1, const double* y1, const double* x2, const double* y2,
                     double* F) {
    double c1x, c1y, s1, c2x, c2y, s2;
    const bool ok1 = normalise8(x1, y1, c1x, c1y, s1);
    const bool ok2 = normalise8(x2, y2, c2x, c2y, s2);
    if (!(ok1 & ok2)) return false;
    double a[8][9];
    SGEO_UNROLL
    for (int i = 0; i < 8; i++) {
        const double u1 = (x1[i] - c1x) * s1, v1 = (y1[i] - c1y) * s1;
        const double u2 = (x2[i] - c2x) * s2, v2 = (y2[i] - c2y) * s2;
        a[i][0] = u2 * u1;
        a[i][1] = u2 * v1;
        a[i][2] = u2;
        a[i][3] = v2 * u1;
        a[i][4] = v2 * v1;
        a[i][5] = v2;
        a[i][6] = u1;
        a[i][7] = v1;
        a[i][8] = 1.0;
    }
    int perm[9];
    SGEO_UNROLL
    for (int j = 0; j < 9; j++) perm[j] = j;
    bool ok = true;
    SGEO_UNROLL
    for (int k = 0; k < 8; k++) {
        double best = 0.0;
        int pr = k, pc = k;
        SGEO_UNROLL
        for (int i = k; i < 8; i++) {
            SGEO_UNROLL
            for (int j = k; j < 9; j++) {
                const double v = __builtin_fabs(a[i][j]);
                const bool gt = v > best;
                best = gt ? v : best;
                pr = gt ? i : pr;
                pc = gt ? j : pc;
            }
        }
        ok = ok & (best > kPivotEps);
        SGEO_UNROLL
        for (int i = k + 1; i < 8; i++) {   // row k <-> row pr (columns < k are zero in both)
            const bool sw = pr == i;
            SGEO_UNROLL
            for (int j = k; j < 9; j++) {
                const double t0 = a[k][j], t1 = a[i][j];
                a[k][j] = sw ? t1 : t0;
                a[i][j] = sw ? t0 : t1;
            }
        }
        SGEO_UNROLL
        for (int j = k + 1; j < 9; j++) {   // column k <-> column pc, in every row
            const bool sw = pc == j;
            SGEO_UNROLL
            for (int i = 0; i < 8; i++) {
                const double t0 = a[i][k], t1 = a[i][j];
                a[i][k] = sw ? t1 : t0;
                a[i][j] = sw ? t0 : t1;
            }
            const int q0 = perm[k], q1 = perm[j];
            perm[k] = sw ? q1 : q0;
            perm[j] = sw ? q0 : q1;
        }
        const double piv = ok ? a[k][k] : 1.0;
        SGEO_UNROLL
        for (int i = k + 1; i < 8; i++) {
            const double f = a[i][k] / piv;
            SGEO_UNROLL
            for (int j = k + 1; j < 9; j++) a[i][j] = __builtin_fma(-f, a[k][j], a[i][j]);
        }
    }
    if (!ok) return false;
    // back substitution with z[8] = 1, then the columns back to their places
    double z[9];
    z[8] = 1.0;
    SGEO_UNROLL
    for (int k = 7; k >= 0; k--) {
        double acc = a[k][8];   // a[k][8] * z[8]
        SGEO_UNROLL
        for (int j = 7; j > k; j--) acc = __builtin_fma(a[k][j], z[j], acc);
        z[k] = -acc / a[k][k];
    }
    double g[9];
    SGEO_UNROLL
    for (int c = 0; c < 9; c++) {
        double v = 0.0;
        SGEO_UNROLL
        for (int j = 0; j < 9; j++) v = perm[j] == c ? z[j] : v;
        g[c] = v;
    }
    // F = T2' G T1, T = [s 0 -s cx; 0 s -s cy; 0 0 1]
    double r[9];
    SGEO_UNROLL
    for (int i = 0; i < 3; i++) {
        r[3 * i] = g[3 * i] * s1;
        r[3 * i + 1] = g[3 * i + 1] * s1;
        r[3 * i + 2] = g[3 * i + 2] - __builtin_fma(r[3 * i], c1x, r[3 * i + 1] * c1y);
    }
    double M[9];
    SGEO_UNROLL
    for (int c = 0; c < 3; c++) {
        M[c] = r[c] * s2;
        M[3 + c] = r[3 + c] * s2;
        M[6 + c] = r[6 + c] - __builtin_fma(M[c], c2x, M[3 + c] * c2y);
    }
    return unit_norm(M, F);
}

// Hypothesis t of pair position p: sample, solve, round.  pts = the pair's matches as rows
// (x1, y1, x2, y2).  False (M untouched) for a degenerate sample.
template <int MODEL>
SGEO_HD bool hypothesis(const float* pts, int m, uint32_t seed, uint32_t p, uint32_t t, float* M) {
    constexpr int S = MODEL == kModelF ? 8 : 4;
    int idx[S];
    sample<S>(seed, p, t, m, idx);
    double x1[S], y1[S], x2[S], y2[S];
    SGEO_UNROLL
    for (int k = 0; k < S; k++) {
        const float* q = pts + 4 * (long long)idx[k];
        x1[k] = (double)q[0];
        y1[k] = (double)q[1];
        x2[k] = (double)q[2];
        y2[k] = (double)q[3];
    }
    double D[9];
    const bool ok = MODEL == kModelF ? solve_f(x1, y1, x2, y2, D) : solve_h(x1, y1, x2, y2, D);
    if (!ok) return false;
    SGEO_UNROLL
    for (int i = 0; i < 9; i++) M[i] = (float)D[i];
    return true;
}

// the 64-bit key hypotheses are compared by: more inliers first, then the lower t; 0 = none
SGEO_HD unsigned long long hyp_key(int count, uint32_t t) {
    return ((unsigned long long)(uint32_t)count << 32) | (unsigned long long)(0xFFFFFFFFu - t);
}

// ---- the whole contract on the host, one pair list ----------------------------------------------

// loc: x, y of buffer row r at loc[r * loc_stride]; matches / counts as sgpu_match_batch wrote
// them; out_mask may be null.  Inputs are taken as valid (sgpu_estimate_batch checks them).
inline void estimate_host(const float* loc, int loc_stride, const int64_t* set_offsets,
                          const int* set_pairs, int npairs, const int* matches,
                          const int* match_counts, int model, float threshold, int iterations,
                          uint32_t seed, float* out_models, int* out_inliers, uint8_t* out_mask) {
    const int S = min_sample(model);
    std::vector<float> pts;
    int64_t moff = 0;
    for (int p = 0; p < npairs; p++) {
        const int m = match_counts[p];
        const int64_t a0 = set_offsets[set_pairs[2 * p]], b0 = set_offsets[set_pairs[2 * p + 1]];
        pts.resize((size_t)m * 4);
        for (int k = 0; k < m; k++) {
            const float* pa = loc + (a0 + matches[2 * (moff + k)]) * loc_stride;
            const float* pb = loc + (b0 + matches[2 * (moff + k) + 1]) * loc_stride;
            pts[4 * k] = pa[0];
            pts[4 * k + 1] = pa[1];
            pts[4 * k + 2] = pb[0];
            pts[4 * k + 3] = pb[1];
        }
        float best[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        unsigned long long best_key = 0;
        for (int t = 0; m >= S && t < iterations; t++) {
            float M[9];
            const bool ok = model == kModelF
                                ? hypothesis<kModelF>(pts.data(), m, seed, (uint32_t)p, (uint32_t)t, M)
                                : hypothesis<kModelH>(pts.data(), m, seed, (uint32_t)p, (uint32_t)t, M);
            if (!ok) continue;
            int count = 0;
            for (int k = 0; k < m; k++)
                count += inlier(model, M, pts[4 * k], pts[4 * k + 1], pts[4 * k + 2], pts[4 * k + 3],
                                threshold);
            const unsigned long long key = hyp_key(count, (uint32_t)t);
            if (key > best_key) {
                best_key = key;
                for (int i = 0; i < 9; i++) best[i] = M[i];
            }
        }
        for (int i = 0; i < 9; i++) out_models[9 * (size_t)p + i] = best[i];
        int n = 0;
        for (int k = 0; k < m; k++) {
            const bool in = best_key != 0 && inlier(model, best, pts[4 * k], pts[4 * k + 1],
                                                    pts[4 * k + 2], pts[4 * k + 3], threshold);
            if (out_mask) out_mask[moff + k] = in ? 1 : 0;
            n += in;
        }
        out_inliers[p] = n;
        moff += m;
    }
}

// ---- local refinement ----------------------------------------------------------------------------
//
// Contract.  The winner gives M, its mask and its count c.  Round r = 1 .. rounds:
//   1  stop when c < S;
//   2  refit<MODEL> over the inliers of M: a double[9] at unit Frobenius norm; invalid -> stop;
//   3  round to float: M'; score M' with inlier() over all m matches: mask', c';
//   4  c' < c: reject, keep M, stop;
//   5  accept M', mask', c'; mask' equal to the mask before: stop (the next refit would give M').
// So the count never falls, and the mask stays the guided test of the returned float matrix.
//
// refit: both images' inlier points normalised as normalise8 does (centroid to the origin, mean
// absolute deviation per coordinate to 1, an IEEE division by the inlier count), the 9 x 9 normal
// matrix N = sum a a' of the rows a (F: solve_f's row; H: the two DLT rows of the normalised
// correspondence), the eigenvector of N's smallest eigenvalue by cyclic Jacobi, denormalised
// (H: inv(T2) G T1; F: T2' G T1) and scaled by unit_norm.  No sign convention, no rank-2 step.
// Invalid: fewer than S inliers, a mean deviation <= kPivotEps, or unit_norm fails.
//
// Summation order: every sum over the inliers is kRefineLanes partial sums, partial l over the
// inlier matches k = l (mod 64) in ascending k, then part[l] += part[l + stride] for l < stride,
// stride = 32, 16 .. 1 (fold_lanes; a xor butterfly over a wave's lanes associates the same way).
// Jacobi: rotations (p, q), p < q in row order, kJacobiSweeps sweeps, a rotation skipped when the
// off-diagonal entry is exactly 0; row k of A and V is one lane's work on the device (k_estimate_
// refine keeps both in LDS), and the element arithmetic below is shared, so the bits are too.

constexpr int kRefineLanes = 64;
constexpr int kMaxRefineRounds = 16;
constexpr int kNormalEntries = 45;   // the upper triangle of N, row-major
// The measured maximum plus two.  Sweeps until the off-diagonal Frobenius norm is <= 1e-14 of the
// matrix's: at most 6 over the refit matrices of the test scenes, at most 7 over 1,000 random PSD
// 9 x 9 matrices (tests/abi/geom_refine_check.cpp measures; tests/test_geom_refine.py fails when
// the maximum + 2 differs from this).
constexpr int kJacobiSweeps = 9;

enum { kStopBudget = 0, kStopFixedPoint = 1, kStopRejected = 2, kStopInvalid = 3, kStopNoModel = 4 };

// the normalisation of the two images: centroids, mean deviations d and their inverses s
struct RefitNorm {
    double c1x, c1y, c2x, c2y;
    double d1, s1, d2, s2;
};
// sum[4] = the sums of x1, y1, x2, y2 over n inliers
SGEO_HD void refit_centroids(const double* sum, int n, RefitNorm& nm) {
    const double dn = (double)n;
    nm.c1x = sum[0] / dn;
    nm.c1y = sum[1] / dn;
    nm.c2x = sum[2] / dn;
    nm.c2y = sum[3] / dn;
}
// one inlier's terms of the two deviation sums
SGEO_HD void refit_deviation(const RefitNorm& nm, double x1, double y1, double x2, double y2,
                             double& t1, double& t2) {
    t1 = __builtin_fabs(x1 - nm.c1x) + __builtin_fabs(y1 - nm.c1y);
    t2 = __builtin_fabs(x2 - nm.c2x) + __builtin_fabs(y2 - nm.c2y);
}
SGEO_HD bool refit_scales(double dev1, double dev2, int n, RefitNorm& nm) {
    const double dn = 2.0 * (double)n;
    nm.d1 = dev1 / dn;
    nm.d2 = dev2 / dn;
    if (!((nm.d1 > kPivotEps) & (nm.d2 > kPivotEps))) return false;
    nm.s1 = 1.0 / nm.d1;
    nm.s2 = 1.0 / nm.d2;
    return true;
}
// N (45 entries, the upper triangle in row-major order) += a a' of one inlier's row(s)
SGEO_HD void normal_add(const double* a, double* N) {
    int e = 0;
    SGEO_UNROLL
    for (int i = 0; i < 9; i++) {
        SGEO_UNROLL
        for (int j = i; j < 9; j++) {
            N[e] = __builtin_fma(a[i], a[j], N[e]);
            e++;
        }
    }
}
template <int MODEL>
SGEO_HD void refit_accumulate(const RefitNorm& nm, double x1, double y1, double x2, double y2,
                              double* N) {
    const double u1 = (x1 - nm.c1x) * nm.s1, v1 = (y1 - nm.c1y) * nm.s1;
    const double u2 = (x2 - nm.c2x) * nm.s2, v2 = (y2 - nm.c2y) * nm.s2;
    if (MODEL == kModelF) {
        const double a[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.0};
        normal_add(a, N);
    } else {
        // h . a = 0, h . b = 0 for (u2, v2, 1) x (H (u1, v1, 1)) = 0
        const double a[9] = {0.0, 0.0, 0.0, -u1, -v1, -1.0, v2 * u1, v2 * v1, v2};
        const double b[9] = {u1, v1, 1.0, 0.0, 0.0, 0.0, -(u2 * u1), -(u2 * v1), -u2};
        normal_add(a, N);
        normal_add(b, N);
    }
}
// the eigenvector g (normalised coordinates) back to pixels, at unit Frobenius norm
template <int MODEL>
SGEO_HD bool refit_denormalise(const RefitNorm& nm, const double* g, double* out) {
    double r[9];   // G T1, T = [s 0 -s cx; 0 s -s cy; 0 0 1]
    SGEO_UNROLL
    for (int i = 0; i < 3; i++) {
        r[3 * i] = g[3 * i] * nm.s1;
        r[3 * i + 1] = g[3 * i + 1] * nm.s1;
        r[3 * i + 2] = g[3 * i + 2] - __builtin_fma(r[3 * i], nm.c1x, r[3 * i + 1] * nm.c1y);
    }
    double M[9];
    SGEO_UNROLL
    for (int c = 0; c < 3; c++) {
        if (MODEL == kModelF) {   // T2' R
            M[c] = r[c] * nm.s2;
            M[3 + c] = r[3 + c] * nm.s2;
            M[6 + c] = r[6 + c] - __builtin_fma(M[c], nm.c2x, M[3 + c] * nm.c2y);
        } else {                  // inv(T2) R, inv(T) = [d 0 cx; 0 d cy; 0 0 1]
            M[c] = __builtin_fma(r[c], nm.d2, nm.c2x * r[6 + c]);
            M[3 + c] = __builtin_fma(r[3 + c], nm.d2, nm.c2y * r[6 + c]);
            M[6 + c] = r[6 + c];
        }
    }
    return unit_norm(M, out);
}

// The Jacobi rotation that annihilates a_pq (a_pq != 0): t = tan, c = cos, s = sin of the angle.
struct JacobiRot { double t, c, s; };
SGEO_HD JacobiRot jacobi_rotation(double app, double aqq, double apq) {
    const double tau = (aqq - app) / (2.0 * apq);
    const double root = __builtin_sqrt(__builtin_fma(tau, tau, 1.0));
    JacobiRot r;
    r.t = (tau >= 0.0 ? 1.0 : -1.0) / (__builtin_fabs(tau) + root);
    r.c = 1.0 / __builtin_sqrt(__builtin_fma(r.t, r.t, 1.0));
    r.s = r.t * r.c;
    return r;
}
// columns p, q of one row (of A off the 2 x 2 block, or of V): (x, y) -> (c x - s y, s x + c y)
SGEO_HD void jacobi_apply(const JacobiRot& r, double x, double y, double& xo, double& yo) {
    xo = __builtin_fma(r.c, x, -(r.s * y));
    yo = __builtin_fma(r.s, x, r.c * y);
}
SGEO_HD double jacobi_app(const JacobiRot& r, double app, double apq) { return __builtin_fma(-r.t, apq, app); }
SGEO_HD double jacobi_aqq(const JacobiRot& r, double aqq, double apq) { return __builtin_fma(r.t, apq, aqq); }

// one sweep over A (symmetric, 9 x 9, both triangles stored) and V, in place
inline void jacobi_sweep_host(double* A, double* V) {
    for (int p = 0; p < 8; p++) {
        for (int q = p + 1; q < 9; q++) {
            const double app = A[9 * p + p], aqq = A[9 * q + q], apq = A[9 * p + q];
            if (apq == 0.0) continue;
            const JacobiRot r = jacobi_rotation(app, aqq, apq);
            for (int k = 0; k < 9; k++) {
                jacobi_apply(r, V[9 * k + p], V[9 * k + q], V[9 * k + p], V[9 * k + q]);
                if (k == p) {
                    A[9 * p + p] = jacobi_app(r, app, apq);
                    A[9 * p + q] = 0.0;
                } else if (k == q) {
                    A[9 * q + q] = jacobi_aqq(r, aqq, apq);
                    A[9 * q + p] = 0.0;
                } else {
                    double x, y;
                    jacobi_apply(r, A[9 * k + p], A[9 * k + q], x, y);
                    A[9 * k + p] = A[9 * p + k] = x;
                    A[9 * k + q] = A[9 * q + k] = y;
                }
            }
        }
    }
}
// the index of the smallest diagonal entry, the lowest among equal ones
SGEO_HD int jacobi_min_index(const double* A) {
    int best = 0;
    double v = A[0];
    SGEO_UNROLL
    for (int i = 1; i < 9; i++) {
        const double d = A[10 * i];
        const bool lt = d < v;
        v = lt ? d : v;
        best = lt ? i : best;
    }
    return best;
}
// N (45) -> A (81, both triangles), V = I
inline void jacobi_start_host(const double* N, double* A, double* V) {
    int e = 0;
    for (int i = 0; i < 9; i++)
        for (int j = i; j < 9; j++) A[9 * i + j] = A[9 * j + i] = N[e++];
    for (int i = 0; i < 81; i++) V[i] = (i % 10 == 0) ? 1.0 : 0.0;
}
// g = the eigenvector of the smallest eigenvalue of A after kJacobiSweeps sweeps (A, V overwritten)
inline void jacobi_host(double* A, double* V, double* g) {
    for (int s = 0; s < kJacobiSweeps; s++) jacobi_sweep_host(A, V);
    const int c = jacobi_min_index(A);
    for (int k = 0; k < 9; k++) g[k] = V[9 * k + c];
}

inline double fold_lanes(double* part) {
    for (int stride = kRefineLanes / 2; stride >= 1; stride >>= 1)
        for (int l = 0; l < stride; l++) part[l] += part[l + stride];
    return part[0];
}

// The normal matrix of the matches of pts (rows x1, y1, x2, y2) that are inliers of M: N[45] and
// the normalisation.  False when the refit is invalid.
template <int MODEL>
inline bool refit_normal_host(const float* pts, int m, const float* M, float threshold,
                              RefitNorm& nm, double* N) {
    constexpr int S = MODEL == kModelF ? 8 : 4;
    std::vector<uint8_t> in((size_t)m);
    int n = 0;
    for (int k = 0; k < m; k++) {
        in[k] = inlier(MODEL, M, pts[4 * k], pts[4 * k + 1], pts[4 * k + 2], pts[4 * k + 3], threshold);
        n += in[k];
    }
    if (n < S) return false;
    std::vector<double> part((size_t)kRefineLanes * kNormalEntries, 0.0);
    auto lane = [&](int e) { return part.data() + (size_t)e * kRefineLanes; };   // 64 partials of sum e
    for (int k = 0; k < m; k++)
        if (in[k])
            for (int e = 0; e < 4; e++) lane(e)[k % kRefineLanes] += (double)pts[4 * k + e];
    double sum[4];
    for (int e = 0; e < 4; e++) sum[e] = fold_lanes(lane(e));
    refit_centroids(sum, n, nm);
    for (int e = 0; e < 2; e++) std::fill(lane(e), lane(e) + kRefineLanes, 0.0);
    for (int k = 0; k < m; k++) {
        if (!in[k]) continue;
        double t1, t2;
        refit_deviation(nm, (double)pts[4 * k], (double)pts[4 * k + 1], (double)pts[4 * k + 2],
                        (double)pts[4 * k + 3], t1, t2);
        lane(0)[k % kRefineLanes] += t1;
        lane(1)[k % kRefineLanes] += t2;
    }
    const double dev1 = fold_lanes(lane(0)), dev2 = fold_lanes(lane(1));
    if (!refit_scales(dev1, dev2, n, nm)) return false;
    std::fill(part.begin(), part.end(), 0.0);
    for (int k = 0; k < m; k++) {
        if (!in[k]) continue;
        double acc[kNormalEntries];
        for (int e = 0; e < kNormalEntries; e++) acc[e] = lane(e)[k % kRefineLanes];
        refit_accumulate<MODEL>(nm, (double)pts[4 * k], (double)pts[4 * k + 1], (double)pts[4 * k + 2],
                                (double)pts[4 * k + 3], acc);
        for (int e = 0; e < kNormalEntries; e++) lane(e)[k % kRefineLanes] = acc[e];
    }
    for (int e = 0; e < kNormalEntries; e++) N[e] = fold_lanes(lane(e));
    return true;
}

// refit over the inliers of M: D = double[9] at unit Frobenius norm; false when invalid
template <int MODEL>
inline bool refit_host(const float* pts, int m, const float* M, float threshold, double* D) {
    RefitNorm nm;
    double N[kNormalEntries], A[81], V[81], g[9];
    if (!refit_normal_host<MODEL>(pts, m, M, threshold, nm, N)) return false;
    jacobi_start_host(N, A, V);
    jacobi_host(A, V, g);
    return refit_denormalise<MODEL>(nm, g, D);
}

// The round loop on one pair: M (float[9]) and its count c are the winner's, or an earlier
// round's; returns the accepted rounds, *stop = why the loop ended (kStop*).
template <int MODEL>
inline int refine_pair_host(const float* pts, int m, float threshold, int rounds, float* M, int& c,
                            int* stop) {
    constexpr int S = MODEL == kModelF ? 8 : 4;
    int done = 0, why = kStopBudget;
    for (int r = 0; r < rounds; r++) {
        if (c < S) {
            why = kStopNoModel;
            break;
        }
        double D[9];
        if (!refit_host<MODEL>(pts, m, M, threshold, D)) {
            why = kStopInvalid;
            break;
        }
        float M2[9];
        for (int i = 0; i < 9; i++) M2[i] = (float)D[i];
        int c2 = 0;
        bool changed = false;
        for (int k = 0; k < m; k++) {
            const float* q = pts + 4 * (size_t)k;
            const bool a = inlier(MODEL, M, q[0], q[1], q[2], q[3], threshold);
            const bool b = inlier(MODEL, M2, q[0], q[1], q[2], q[3], threshold);
            c2 += b;
            changed |= a != b;
        }
        if (c2 < c) {
            why = kStopRejected;
            break;
        }
        for (int i = 0; i < 9; i++) M[i] = M2[i];
        c = c2;
        done++;
        if (!changed) {
            why = kStopFixedPoint;
            break;
        }
    }
    if (stop) *stop = why;
    return done;
}

// estimate_host followed by `rounds` rounds of refinement; rounds = 0 is estimate_host.
// out_rounds / out_stop: [npairs], may be null.
inline void refine_host(const float* loc, int loc_stride, const int64_t* set_offsets,
                        const int* set_pairs, int npairs, const int* matches,
                        const int* match_counts, int model, float threshold, int iterations,
                        uint32_t seed, int rounds, float* out_models, int* out_inliers,
                        uint8_t* out_mask, int* out_rounds, int* out_stop) {
    estimate_host(loc, loc_stride, set_offsets, set_pairs, npairs, matches, match_counts, model,
                  threshold, iterations, seed, out_models, out_inliers, out_mask);
    std::vector<float> pts;
    int64_t moff = 0;
    for (int p = 0; p < npairs; p++) {
        const int m = match_counts[p];
        int done = 0, why = kStopBudget;
        if (rounds > 0) {
            const int64_t a0 = set_offsets[set_pairs[2 * p]], b0 = set_offsets[set_pairs[2 * p + 1]];
            pts.resize((size_t)m * 4);
            for (int k = 0; k < m; k++) {
                const float* pa = loc + (a0 + matches[2 * (moff + k)]) * loc_stride;
                const float* pb = loc + (b0 + matches[2 * (moff + k) + 1]) * loc_stride;
                pts[4 * k] = pa[0];
                pts[4 * k + 1] = pa[1];
                pts[4 * k + 2] = pb[0];
                pts[4 * k + 3] = pb[1];
            }
            float* M = out_models + 9 * (size_t)p;
            done = model == kModelF
                       ? refine_pair_host<kModelF>(pts.data(), m, threshold, rounds, M, out_inliers[p], &why)
                       : refine_pair_host<kModelH>(pts.data(), m, threshold, rounds, M, out_inliers[p], &why);
            if (done > 0 && out_mask)
                for (int k = 0; k < m; k++)
                    out_mask[moff + k] = inlier(model, M, pts[4 * k], pts[4 * k + 1], pts[4 * k + 2],
                                                pts[4 * k + 3], threshold) ? 1 : 0;
        }
        if (out_rounds) out_rounds[p] = done;
        if (out_stop) out_stop[p] = why;
        moff += m;
    }
}

// ---- planner -----------------------------------------------------------------------------------

// what the kernels read of a pair, and one work item of k_estimate_pairs: hypotheses
// [block * kBlockHyp, min(iterations, (block + 1) * kBlockHyp)) of pair `pair`
struct PairRec {
    long long moff;   // the pair's first match in the concatenated list
    int a_off, b_off; // first buffer rows of its sets
    int m, pad;
};
struct Item { int pair, block; };

struct Plan {
    std::vector<PairRec> pairs;
    std::vector<Item> items;
    long long total = 0;   // matches of all pairs
};

enum { kPlanOk = 0, kPlanBadArgument = 1, kPlanTooLarge = 2 };

// Pairs below the minimal sample get no items (they have no model); every other pair gets
// ceil(iterations / kBlockHyp).  Validates offsets, pair indices and counts; match indices are the
// caller's to check against the set sizes (check_matches).
inline int build_plan(const int64_t* set_offsets, int nsets, const int* set_pairs, int npairs,
                      const int* match_counts, int model, int iterations, Plan& plan) {
    plan.pairs.clear();
    plan.items.clear();
    plan.total = 0;
    if (nsets < 0 || npairs < 0 || !set_offsets) return kPlanBadArgument;
    if (iterations < 1 || iterations > kMaxIterations) return kPlanBadArgument;
    if (model != kModelH && model != kModelF) return kPlanBadArgument;
    if (set_offsets[0] < 0) return kPlanBadArgument;
    for (int s = 0; s < nsets; s++)
        if (set_offsets[s + 1] < set_offsets[s]) return kPlanBadArgument;
    if (set_offsets[nsets] > 0x7fffffffLL) return kPlanTooLarge;
    if (npairs > 0 && (!set_pairs || !match_counts)) return kPlanBadArgument;
    const int S = min_sample(model), blocks = (iterations + kBlockHyp - 1) / kBlockHyp;
    plan.pairs.reserve((size_t)npairs);
    for (int p = 0; p < npairs; p++) {
        const int a = set_pairs[2 * p], b = set_pairs[2 * p + 1], m = match_counts[p];
        if (a < 0 || a >= nsets || b < 0 || b >= nsets || m < 0) return kPlanBadArgument;
        PairRec r;
        r.moff = plan.total;
        r.a_off = (int)set_offsets[a];
        r.b_off = (int)set_offsets[b];
        r.m = m;
        r.pad = 0;
        plan.pairs.push_back(r);
        plan.total += m;
        if (plan.total > 0x7fffffffLL) return kPlanTooLarge;
        if (m >= S) {
            if (plan.items.size() + (size_t)blocks > 0x7fffffffULL) return kPlanTooLarge;
            for (int b2 = 0; b2 < blocks; b2++) plan.items.push_back(Item{p, b2});
        }
    }
    return kPlanOk;
}

// every match index lies inside its set
inline bool check_matches(const int64_t* set_offsets, const int* set_pairs, int npairs,
                          const int* matches, const int* match_counts) {
    long long k = 0;
    for (int p = 0; p < npairs; p++) {
        const int a = set_pairs[2 * p], b = set_pairs[2 * p + 1];
        const long long na = set_offsets[a + 1] - set_offsets[a], nb = set_offsets[b + 1] - set_offsets[b];
        for (int e = 0; e < match_counts[p]; e++, k++) {
            const int i = matches[2 * k], j = matches[2 * k + 1];
            if (i < 0 || i >= na || j < 0 || j >= nb) return false;
        }
    }
    return true;
}

}  // namespace sgeo
#endif
