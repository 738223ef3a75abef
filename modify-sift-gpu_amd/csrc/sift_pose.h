// sift_pose.h -- relative pose and two-view triangulation of verified pairs (sgpu_pose_batch,
// sgpu_pose_images): the rule, its element functions, a host loop that implements
// the whole contract (pose_host) and the argument checks that need no device.  Plain C++, no HIP,
// in the manner of sift_geom.h: k_pose (sift_pose.hip) and pose_host call the same SGEO_HD
// functions, compiled without contraction, every fma written out, double throughout, IEEE division
// and square root -- host and device produce the same bits.
//
// Contract.  Pair position p = sets (a, b) with intrinsics Ka, Kb (fx, fy, cx, cy: pinhole, no skew,
// no distortion), matches {i, j} (x1 = set a's point i, x2 = set b's point j) and F_p with
// x2' F x1 = 0:
//   participants  the matches with sgeo::inlier(kModelF, F_p, x1, y1, x2, y2, f_threshold): the
//                 guided matcher's own float test;
//   essential     E = Kb' F Ka at unit Frobenius norm; the eigen-decomposition of E'E by cyclic
//                 Jacobi, rotations (0, 1), (0, 2), (1, 2), kPoseSweeps sweeps, a rotation skipped
//                 when its off-diagonal entry is exactly 0; v1, v2 = the eigenvectors of the two
//                 largest eigenvalues (the lower index among equal ones first), s_i = sqrt(l_i),
//                 u_i = E v_i / s_i, u3 = u1 x u2, v3 = v1 x v2: both bases right-handed, every
//                 candidate R has determinant +1.  No pose: F zero or not finite, or s2 not above
//                 kSigmaRatioMin s1 (a NaN falls on this side);
//   candidates    (U W V', +u3), (U W V', -u3), (U W' V', +u3), (U W' V', -u3),
//                 W = [0 -1 0; 1 0 0; 0 0 1];  x_cam2 = R x_cam1 + t;
//   triangulate   a participant under (R, t) by the midpoint method: rays a = inv(Ka) (x1, y1, 1),
//                 b = inv(Kb) (x2, y2, 1), c = R a; the 2 x 2 normal equations of
//                 l1 c - l2 b = -t, determinant |c x b|^2.  In front: determinant > kParallelEps,
//                 l1 > 0, l2 > 0.  X = (l1 a + R' (l2 b - t)) / 2, first camera's frame, |t| = 1.
//                 Wide: in front and c . b <= cos(min_angle) sqrt((c . c) (b . b));
//   winner        the candidate with the most participants in front, the lowest index among equal
//                 counts.  No pose, no participant or a best count of 0: zeros for R, t, mask and
//                 points, counts {participants, 0, 0}.
// Counts are integers: nothing depends on a summation order.
#ifndef SIFT_POSE_H
#define SIFT_POSE_H
#include "sift_geom.h"

namespace spose {

// The measured maximum plus two.  Sweeps until the off-diagonal Frobenius norm of E'E is <= 1e-14
// of the matrix's: tests/abi/pose_check.cpp measures the maximum over the test scenes' E and
// 1,000 random ones, and tests/test_pose.py fails when the maximum + 2 differs from this.
constexpr int kPoseSweeps = 6;
// An essential matrix has s1 = s2; an F estimated from noisy matches stays close to that (0.99 on
// the tests' noisy scene).  A rank-1 F rounded to float has s2 / s1 of at most the order of 2^-24
// (the rounding of its entries), and sqrt of an eigenvalue of E'E resolves s2 / s1 down to about
// 2^-26: 1e-3 lies four orders above both and two below any F worth decomposing.
constexpr double kSigmaRatioMin = 1e-3;
// |c x b|^2 of two rays with third component 1 (before the rotation) is at least sin^2 of their
// angle: rays closer than 1e-6 rad (0.2 arc seconds; a 1,000-pixel focal length resolves 1e-3 rad
// per pixel) are parallel and have no intersection.
constexpr double kParallelEps = 1e-12;
constexpr double kHalfPi = 1.5707963267948966;

// what triangulation reads of the two cameras
struct Cams {
    double ifx1, ify1, cx1, cy1, ifx2, ify2, cx2, cy2;
};
// the two rotations U W V' and U W' V', and u3: candidate k = (k < 2 ? Ra : Rb, k odd ? -u3 : u3)
struct Pose {
    double Ra[9], Rb[9], u3[3];
};

SGEO_HD bool finite_positive(float v) { return v > 0.f && v < 3.0e38f; }
SGEO_HD bool finite(float v) { return v > -3.0e38f && v < 3.0e38f; }

// one Jacobi rotation (P, Q) of the symmetric 3 x 3 A (both triangles stored) and of V, in place;
// K is the third index
template <int P, int Q>
SGEO_HD void jacobi3_rotate(double* A, double* V) {
    constexpr int K = 3 - P - Q;
    const double app = A[4 * P], aqq = A[4 * Q], apq = A[3 * P + Q];
    if (apq == 0.0) return;
    const sgeo::JacobiRot r = sgeo::jacobi_rotation(app, aqq, apq);
    SGEO_UNROLL
    for (int k = 0; k < 3; k++) sgeo::jacobi_apply(r, V[3 * k + P], V[3 * k + Q], V[3 * k + P], V[3 * k + Q]);
    A[4 * P] = sgeo::jacobi_app(r, app, apq);
    A[4 * Q] = sgeo::jacobi_aqq(r, aqq, apq);
    A[3 * P + Q] = A[3 * Q + P] = 0.0;
    double x, y;
    sgeo::jacobi_apply(r, A[3 * K + P], A[3 * K + Q], x, y);
    A[3 * K + P] = A[3 * P + K] = x;
    A[3 * K + Q] = A[3 * Q + K] = y;
}
SGEO_HD void jacobi3_sweep(double* A, double* V) {
    jacobi3_rotate<0, 1>(A, V);
    jacobi3_rotate<0, 2>(A, V);
    jacobi3_rotate<1, 2>(A, V);
}

// E = Kb' F Ka at unit Frobenius norm, K = [fx 0 cx; 0 fy cy; 0 0 1]; false for a zero or
// non-finite F
SGEO_HD bool essential(const float* F, const float* Ka, const float* Kb, double* E) {
    const double fx1 = (double)Ka[0], fy1 = (double)Ka[1], cx1 = (double)Ka[2], cy1 = (double)Ka[3];
    const double fx2 = (double)Kb[0], fy2 = (double)Kb[1], cx2 = (double)Kb[2], cy2 = (double)Kb[3];
    double G[9];   // F Ka
    SGEO_UNROLL
    for (int i = 0; i < 3; i++) {
        const double f0 = (double)F[3 * i], f1 = (double)F[3 * i + 1], f2 = (double)F[3 * i + 2];
        G[3 * i] = f0 * fx1;
        G[3 * i + 1] = f1 * fy1;
        G[3 * i + 2] = __builtin_fma(f0, cx1, __builtin_fma(f1, cy1, f2));
    }
    double M[9];   // Kb' G
    SGEO_UNROLL
    for (int j = 0; j < 3; j++) {
        M[j] = fx2 * G[j];
        M[3 + j] = fy2 * G[3 + j];
        M[6 + j] = __builtin_fma(cx2, G[j], __builtin_fma(cy2, G[3 + j], G[6 + j]));
    }
    return sgeo::unit_norm(M, E);
}

// A = E'E (both triangles), V = I
SGEO_HD void gram_start(const double* E, double* A, double* V) {
    SGEO_UNROLL
    for (int i = 0; i < 3; i++) {
        SGEO_UNROLL
        for (int j = i; j < 3; j++) {
            const double v = __builtin_fma(E[6 + i], E[6 + j], __builtin_fma(E[3 + i], E[3 + j], E[i] * E[j]));
            A[3 * i + j] = v;
            A[3 * j + i] = v;
        }
    }
    SGEO_UNROLL
    for (int i = 0; i < 9; i++) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
}

SGEO_HD void cross3(const double* a, const double* b, double* o) {
    o[0] = __builtin_fma(a[1], b[2], -(a[2] * b[1]));
    o[1] = __builtin_fma(a[2], b[0], -(a[0] * b[2]));
    o[2] = __builtin_fma(a[0], b[1], -(a[1] * b[0]));
}
SGEO_HD double dot3(const double* a, const double* b) {
    return __builtin_fma(a[2], b[2], __builtin_fma(a[1], b[1], a[0] * b[0]));
}
// exchange eigenpair (la, va) with (lb, vb) when sw: selects over compile-time positions, so that
// the columns stay named values
SGEO_HD void eigen_swap(bool sw, double& la, double& lb, double* va, double* vb) {
    const double t0 = la, t1 = lb;
    la = sw ? t1 : t0;
    lb = sw ? t0 : t1;
    SGEO_UNROLL
    for (int k = 0; k < 3; k++) {
        const double x = va[k], y = vb[k];
        va[k] = sw ? y : x;
        vb[k] = sw ? x : y;
    }
}

// The bases of the diagonalised A = E'E (eigenvalues on its diagonal, eigenvectors V's columns)
// and the two rotations; false: no pose.
SGEO_HD bool pose_from_eigen(const double* E, const double* A, const double* V, Pose& P) {
    double e1 = A[0], e2 = A[4], e3 = A[8];
    double v1[3], v2[3], w[3], v3[3], u1[3], u2[3];
    SGEO_UNROLL
    for (int k = 0; k < 3; k++) {
        v1[k] = V[3 * k];
        v2[k] = V[3 * k + 1];
        w[k] = V[3 * k + 2];
    }
    // descending, the lower index first among equal eigenvalues: three exchanges of neighbours,
    // each only for a strictly larger successor
    eigen_swap(e2 > e1, e1, e2, v1, v2);
    eigen_swap(e3 > e2, e2, e3, v2, w);
    eigen_swap(e2 > e1, e1, e2, v1, v2);
    if (!(e1 > 0.0)) return false;
    const double s1 = __builtin_sqrt(e1), s2 = __builtin_sqrt(e2);   // e2 < 0: NaN, no pose
    if (!(s2 > kSigmaRatioMin * s1)) return false;
    cross3(v1, v2, v3);
    SGEO_UNROLL
    for (int k = 0; k < 3; k++) {
        u1[k] = __builtin_fma(E[3 * k + 2], v1[2], __builtin_fma(E[3 * k + 1], v1[1], E[3 * k] * v1[0])) / s1;
        u2[k] = __builtin_fma(E[3 * k + 2], v2[2], __builtin_fma(E[3 * k + 1], v2[1], E[3 * k] * v2[0])) / s2;
    }
    cross3(u1, u2, P.u3);
    // U W V' = u2 v1' - u1 v2' + u3 v3';  U W' V' = u1 v2' - u2 v1' + u3 v3'
    SGEO_UNROLL
    for (int i = 0; i < 3; i++) {
        SGEO_UNROLL
        for (int j = 0; j < 3; j++) {
            const double w = P.u3[i] * v3[j];
            P.Ra[3 * i + j] = __builtin_fma(u2[i], v1[j], __builtin_fma(-u1[i], v2[j], w));
            P.Rb[3 * i + j] = __builtin_fma(u1[i], v2[j], __builtin_fma(-u2[i], v1[j], w));
        }
    }
    return true;
}

// steps 2 and 3 of the contract for one pair; false: no pose
SGEO_HD bool decompose(const float* F, const float* Ka, const float* Kb, Pose& P) {
    double E[9], A[9], V[9];
    if (!essential(F, Ka, Kb, E)) return false;
    gram_start(E, A, V);
    SGEO_UNROLL
    for (int s = 0; s < kPoseSweeps; s++) jacobi3_sweep(A, V);
    return pose_from_eigen(E, A, V, P);
}

SGEO_HD void cameras(const float* Ka, const float* Kb, Cams& c) {
    c.ifx1 = 1.0 / (double)Ka[0];
    c.ify1 = 1.0 / (double)Ka[1];
    c.cx1 = (double)Ka[2];
    c.cy1 = (double)Ka[3];
    c.ifx2 = 1.0 / (double)Kb[0];
    c.ify2 = 1.0 / (double)Kb[1];
    c.cx2 = (double)Kb[2];
    c.cy2 = (double)Kb[3];
}

// candidate k's rotation and translation
SGEO_HD void candidate(const Pose& P, int k, double* R, double* t) {
    SGEO_UNROLL
    for (int i = 0; i < 9; i++) R[i] = k < 2 ? P.Ra[i] : P.Rb[i];
    SGEO_UNROLL
    for (int i = 0; i < 3; i++) t[i] = (k & 1) ? -P.u3[i] : P.u3[i];
}

// one match's rays under a rotation, and what the normal equations need of them
struct Rays {
    double a[3], b[3], c[3];
    double cc, bb, cb, det;
};
SGEO_HD void rays(const Cams& cam, const double* R, float x1, float y1, float x2, float y2, Rays& r) {
    r.a[0] = ((double)x1 - cam.cx1) * cam.ifx1;
    r.a[1] = ((double)y1 - cam.cy1) * cam.ify1;
    r.a[2] = 1.0;
    r.b[0] = ((double)x2 - cam.cx2) * cam.ifx2;
    r.b[1] = ((double)y2 - cam.cy2) * cam.ify2;
    r.b[2] = 1.0;
    SGEO_UNROLL
    for (int i = 0; i < 3; i++)
        r.c[i] = __builtin_fma(R[3 * i], r.a[0], __builtin_fma(R[3 * i + 1], r.a[1], R[3 * i + 2]));
    double n[3];
    cross3(r.c, r.b, n);
    r.cc = dot3(r.c, r.c);
    r.bb = dot3(r.b, r.b);
    r.cb = dot3(r.c, r.b);
    r.det = dot3(n, n);
}
// the depths along a and b under translation t; true: in front of both cameras
SGEO_HD bool depths(const Rays& r, const double* t, double& l1, double& l2) {
    const double ct = dot3(r.c, t), bt = dot3(r.b, t);
    l1 = __builtin_fma(r.cb, bt, -(r.bb * ct)) / r.det;
    l2 = __builtin_fma(r.cc, bt, -(r.cb * ct)) / r.det;
    return (r.det > kParallelEps) & (l1 > 0.0) & (l2 > 0.0);
}
SGEO_HD bool wide(const Rays& r, double cos_min) {
    return r.cb <= cos_min * __builtin_sqrt(r.cc * r.bb);
}
// X = (l1 a + R' (l2 b - t)) / 2
SGEO_HD void midpoint(const Rays& r, const double* R, const double* t, double l1, double l2, double* X) {
    double d[3];
    SGEO_UNROLL
    for (int i = 0; i < 3; i++) d[i] = __builtin_fma(l2, r.b[i], -t[i]);
    SGEO_UNROLL
    for (int i = 0; i < 3; i++) {
        const double q = __builtin_fma(R[6 + i], d[2], __builtin_fma(R[3 + i], d[1], R[i] * d[0]));
        X[i] = 0.5 * __builtin_fma(l1, r.a[i], q);
    }
}

// pass one on one match: bit k of the result = in front under candidate k
SGEO_HD int front_bits(const Cams& cam, const Pose& P, float x1, float y1, float x2, float y2) {
    int bits = 0;
    SGEO_UNROLL
    for (int k = 0; k < 4; k++) {
        double R[9], t[3], l1, l2;
        candidate(P, k, R, t);
        Rays r;
        rays(cam, R, x1, y1, x2, y2, r);
        bits |= depths(r, t, l1, l2) ? (1 << k) : 0;
    }
    return bits;
}
// the winner of the four in-front counts: the most (*count), the lowest index among equal counts
SGEO_HD int winner(const int* front, int* count) {
    int best = 0, most = front[0];
    SGEO_UNROLL
    for (int k = 1; k < 4; k++) {
        const bool gt = front[k] > most;
        most = gt ? front[k] : most;
        best = gt ? k : best;
    }
    *count = most;
    return best;
}
// pass two on one participant under the winner (R, t): returns in front; X and *is_wide are set
// for an in-front match
SGEO_HD bool resolve(const Cams& cam, const double* R, const double* t, double cos_min, float x1,
                     float y1, float x2, float y2, float* X, bool* is_wide) {
    Rays r;
    rays(cam, R, x1, y1, x2, y2, r);
    double l1, l2;
    if (!depths(r, t, l1, l2)) return false;
    double D[3];
    midpoint(r, R, t, l1, l2, D);
    SGEO_UNROLL
    for (int i = 0; i < 3; i++) X[i] = (float)D[i];
    *is_wide = wide(r, cos_min);
    return true;
}

// cos(min_angle) as both sides take it: the host's double cosine of the float argument
inline double cos_min_angle(float min_angle) { return __builtin_cos((double)min_angle); }

// ---- the whole contract on the host, one pair list ------------------------------------------------

// loc: x, y of buffer row r at loc[r * loc_stride]; intrinsics [nsets][4]; F [npairs][9]; out_mask
// and out_points may be null.  Inputs are taken as valid (check_args).  out_front_all (or null)
// [npairs][4]: every candidate's in-front count, for the tests.
inline void pose_host(const float* loc, int loc_stride, const int64_t* set_offsets,
                      const float* intrinsics, const int* set_pairs, int npairs, const int* matches,
                      const int* match_counts, const float* F, float f_threshold, float min_angle,
                      float* out_R, float* out_t, int* out_counts, uint8_t* out_mask,
                      float* out_points, int* out_front_all = nullptr) {
    const double cos_min = cos_min_angle(min_angle);
    std::vector<float> pts;
    std::vector<uint8_t> part;
    int64_t moff = 0;
    for (int p = 0; p < npairs; p++) {
        const int m = match_counts[p], sa = set_pairs[2 * p], sb = set_pairs[2 * p + 1];
        const int64_t a0 = set_offsets[sa], b0 = set_offsets[sb];
        const float* Fp = F + 9 * (size_t)p;
        const float *Ka = intrinsics + 4 * (size_t)sa, *Kb = intrinsics + 4 * (size_t)sb;
        pts.resize((size_t)m * 4);
        part.resize((size_t)m);
        for (int k = 0; k < m; k++) {
            const float* pa = loc + (a0 + matches[2 * (moff + k)]) * loc_stride;
            const float* pb = loc + (b0 + matches[2 * (moff + k) + 1]) * loc_stride;
            pts[4 * k] = pa[0];
            pts[4 * k + 1] = pa[1];
            pts[4 * k + 2] = pb[0];
            pts[4 * k + 3] = pb[1];
        }
        float* oR = out_R + 9 * (size_t)p;
        float* ot = out_t + 3 * (size_t)p;
        int* oc = out_counts + 3 * (size_t)p;
        for (int i = 0; i < 9; i++) oR[i] = 0.f;
        for (int i = 0; i < 3; i++) ot[i] = 0.f;
        oc[0] = oc[1] = oc[2] = 0;
        int front[4] = {0, 0, 0, 0};
        if (m > 0) {
            if (out_mask) std::fill(out_mask + moff, out_mask + moff + m, (uint8_t)0);
            if (out_points) std::fill(out_points + 3 * moff, out_points + 3 * (moff + m), 0.f);
            Pose P;
            Cams cam;
            const bool ok = decompose(Fp, Ka, Kb, P);
            cameras(Ka, Kb, cam);
            int n = 0;
            for (int k = 0; k < m; k++) {
                const float* q = pts.data() + 4 * (size_t)k;
                part[k] = sgeo::inlier(sgeo::kModelF, Fp, q[0], q[1], q[2], q[3], f_threshold);
                n += part[k];
                if (part[k] && ok) {
                    const int bits = front_bits(cam, P, q[0], q[1], q[2], q[3]);
                    for (int c = 0; c < 4; c++) front[c] += (bits >> c) & 1;
                }
            }
            oc[0] = n;
            int most = 0;
            const int w = winner(front, &most);
            if (ok && most > 0) {
                double R[9], t[3];
                candidate(P, w, R, t);
                for (int i = 0; i < 9; i++) oR[i] = (float)R[i];
                for (int i = 0; i < 3; i++) ot[i] = (float)t[i];
                int nf = 0, nw = 0;
                for (int k = 0; k < m; k++) {
                    if (!part[k]) continue;
                    const float* q = pts.data() + 4 * (size_t)k;
                    float X[3];
                    bool wd = false;
                    if (!resolve(cam, R, t, cos_min, q[0], q[1], q[2], q[3], X, &wd)) continue;
                    nf++;
                    nw += wd;
                    if (out_mask) out_mask[moff + k] = 1;
                    if (out_points)
                        for (int i = 0; i < 3; i++) out_points[3 * (moff + k) + i] = X[i];
                }
                oc[1] = nf;
                oc[2] = nw;
            }
        }
        if (out_front_all)
            for (int c = 0; c < 4; c++) out_front_all[4 * (size_t)p + c] = front[c];
        moff += m;
    }
}

// ---- argument checks (everything sgpu_pose_batch refuses that needs no device) -----------------------

enum { kArgsOk = 0, kArgsBad = 1, kArgsTooLarge = 2 };

// The shared arguments as sgpu_estimate_batch checks them (sgeo::build_plan fills plan.pairs, which
// the kernels read; sgeo::check_matches), then this call's own.  *why names the first failure.
inline int check_args(const int64_t* set_offsets, int nsets, const float* intrinsics,
                      const int* set_pairs, int npairs, const int* matches, const int* match_counts,
                      const float* F, float f_threshold, float min_angle, const float* out_R,
                      const float* out_t, const int* out_counts, sgeo::Plan& plan, const char** why) {
    *why = "";
    const int prc = sgeo::build_plan(set_offsets, nsets, set_pairs, npairs, match_counts, sgeo::kModelF,
                                     1, plan);
    if (prc == sgeo::kPlanTooLarge) {
        *why = "pose batch too large";
        return kArgsTooLarge;
    }
    if (prc != sgeo::kPlanOk) {
        *why = "bad offsets, pair indices or counts";
        return kArgsBad;
    }
    if (!(f_threshold >= 0.f && f_threshold < 3.0e38f)) {
        *why = "f_threshold negative or not finite";
        return kArgsBad;
    }
    if (!(min_angle >= 0.f && (double)min_angle <= kHalfPi + 1e-7)) {
        *why = "min_angle outside [0, pi/2]";
        return kArgsBad;
    }
    if (npairs == 0) return kArgsOk;
    if (!F || !intrinsics || !out_R || !out_t || !out_counts) {
        *why = "null F, intrinsics or outputs";
        return kArgsBad;
    }
    if (plan.total > 0 && !matches) {
        *why = "null matches";
        return kArgsBad;
    }
    if (!sgeo::check_matches(set_offsets, set_pairs, npairs, matches, match_counts)) {
        *why = "a match index lies outside its set";
        return kArgsBad;
    }
    for (int p = 0; p < 2 * npairs; p++) {
        const float* K = intrinsics + 4 * (size_t)set_pairs[p];
        if (!(finite_positive(K[0]) && finite_positive(K[1]) && finite(K[2]) && finite(K[3]))) {
            *why = "an intrinsic row is not finite or has fx, fy <= 0";
            return kArgsBad;
        }
    }
    return kArgsOk;
}

}  // namespace spose
#endif
