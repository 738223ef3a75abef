// sift_kernels.hip -- SIFT descriptors (gfx950 / MI355X): the exact, relaxed, dual-cell and
// flat pixel-parallel forms, and the host-output copy.  The levels, detection and orientation,
// which this file also held, are sift_level.hip, sift_detect.hip and sift_orient.hip; the name
// stays until a rename of its own (to sift_descriptor.hip).
//
// Reference semantics: SiftGPU/ProgramCU.cu (ComputeDescriptor_Kernel, ComputeDescriptorRECT_Kernel,
// NormalizeDescriptor_Kernel).  MI355X-first, not a translation (sift_kernels.h): gradient images
// are never stored, the descriptor kernels evaluate gradients from the Gaussian level on the fly.
// Floating-point conventions are those of oracle/sift_oracle.cpp (fma contractions written
// out, transcendentals from sift_math.h); the build uses -ffp-contract=off.
#include <algorithm>
#include <cstdlib>

#include "sift_device.h"

// Build-time tuning knobs (tests/build_variant.sh passes -D overrides; the values here ship).
#ifndef SGK_DESC_RSTEP
#define SGK_DESC_RSTEP 4      // descriptor_fast: rows a quad walks side by side (0: flat strip order)
#endif
#ifndef SGK_DESC_WPE
#define SGK_DESC_WPE 0        // k_descriptor_fast: waves per SIMD the allocation must allow (0: compiler's choice)
#endif
#ifndef SGK_DUAL_WPE
#define SGK_DUAL_WPE 4        // k_descriptor_dual: the same; 4 = <= 128 VGPRs, no spills (132 free)
#endif
#ifndef SGK_FLAT_WPE
#define SGK_FLAT_WPE 8        // the flat kernels: the same; 8 = 64 VGPRs, no spills
#endif
#ifndef SGK_FLAT_COPIES
#define SGK_FLAT_COPIES 4     // copies of the flat kernels' LDS histogram (lane mod copies)
#endif
#ifndef SGK_FLAT_PAD
#define SGK_FLAT_PAD 0        // padding words between a (cell, bin)'s copies and the next's
#endif

namespace sgk {
namespace {

// ------------------------------------------------------------------------------------------
// Gradient of a Gaussian level at an interior pixel, as ComputeDOG_Kernel stores it
// (ProgramCU.cu:495-502): (0.5 |grad|, atan2(dy, dx)), atan2 skipped when the magnitude is 0.
__device__ __forceinline__ float2 grad_at(const float* __restrict__ g, int W, int x, int y) {
    const float* p = g + (long long)y * W + x;
    const float dx = p[1] - p[-1];
    const float dy = p[W] - p[-W];
    const float grd = 0.5f * sqrt_(fma_(dx, dx, dy * dy));
    const float rot = grd == 0.0f ? 0.0f : atan2_(dy, dx);
    return make_float2(grd, rot);
}

// ------------------------------------------------------------------------------------------
// ComputeDescriptor_Kernel<false> (ProgramCU.cu:1013-1101) + NormalizeDescriptor_Kernel
// (:1173-1208).  16 lanes per feature (one 4x4 grid cell each, as the reference), 4 features
// per wave; normalisation sums are formed in the reference's sequential order via shuffles.
__device__ __forceinline__ float sq4(float a, float b, float c, float d) {
    float t = a * a;
    t = fma_(b, b, t);
    t = fma_(c, c, t);
    return fma_(d, d, t);
}

// RECT: ComputeDescriptorRECT_Kernel<false> (ProgramCU.cu:1104-1171) for keys given with
// keys_have_orientation == -1: the 4 x 4 grid spans the rectangle [x, x+z] x [y, y+w], cells
// are axis-aligned (nx = dx / sptx), no Gaussian window, theta = -angle.
template <bool RECT>
__device__ __forceinline__ void descriptor_one(uint32_t e, int lane,
                                               const float* __restrict__ pyr,
                                               const float4* __restrict__ feat,
                                               const int2* __restrict__ feat_info,
                                               const FeatureParams& fp,
                                               float* __restrict__ desc, uint32_t out,
                                               float* __restrict__ hdesc = nullptr) {
    // one wave per feature: lanes 4c..4c+3 own grid cell c (the reference's 16 threads per
    // feature, ProgramCU.cu:1017-1021); the quad evaluates consecutive window samples in
    // parallel and every lane applies the 4 contributions in the reference's (y, x) order, so
    // the 9 accumulators see the reference's exact sequence of fma's.
    const int cell = lane >> 2, sub = lane & 3;
    const int ix = cell & 3, iy = cell >> 2;
    // each quad lane owns two of the cell's 8 orientation bins (lane 0 also bin 8): every bin's
    // fma chain is the reference's, and a sample costs 4 compares instead of an 8-way select
    const int kb = 2 * sub;
    float acc0 = 0.0f, acc1 = 0.0f, acc8 = 0.0f;
    const float4 key = feat[e];
    const int2 in = feat_info[e];
    const int o = in.y / fp.d, j = in.y - o * fp.d;
    const OctaveDesc& od = fp.oct[o];
    const int W = od.wa, H = od.h;
    const float* g = pyr + od.gauss_off + (long long)(1 + j) * od.level_stride +
                     (long long)in.x * W * H;
    const float rpi = (float)(4.0 / 3.14159265358979323846);
    float spt = 0.f, anglef = 0.f, cspt = 0.f, sspt = 0.f, crspt = 0.f, srspt = 0.f;
    float ox = 0.f, oy = 0.f, ptx, pty, bszx, bszy;
    const float sptx = key.z * 0.25f, spty = key.w * 0.25f;   // RECT (exact: key * 0.25 double)
    if (RECT) {
        ptx = fma_(sptx, ix + 0.5f, key.x);
        pty = fma_(spty, iy + 0.5f, key.y);
        bszx = sptx;
        bszy = spty;
    } else {
        spt = fabs_(key.z * fp.window_factor);
        float s, c;
        sincos_(key.w, &s, &c);
        anglef = (double)key.w > 3.14159265358979323846
                     ? (float)((double)key.w - (2.0 * 3.14159265358979323846))
                     : key.w;
        cspt = c * spt;
        sspt = s * spt;
        crspt = c / spt;
        srspt = s / spt;
        ox = ix - 1.5f;
        oy = iy - 1.5f;
        ptx = fma_(cspt, ox, -(sspt * oy)) + key.x;
        pty = fma_(cspt, oy, sspt * ox) + key.y;
        bszx = bszy = fabs_(cspt) + fabs_(sspt);
    }
    const float xmin = fmax_(1.5f, floor_(ptx - bszx) + 0.5f);
    const float ymin = fmax_(1.5f, floor_(pty - bszy) + 0.5f);
    const float xmax = fmin_(W - 1.5f, floor_(ptx + bszx) + 0.5f);
    const float ymax = fmin_(H - 1.5f, floor_(pty + bszy) + 0.5f);
    const int ncols = xmax >= xmin ? (int)(xmax - xmin) + 1 : 0;
    const int nrows = ymax >= ymin ? (int)(ymax - ymin) + 1 : 0;
    // The reference visits every sample of the cell's axis-aligned box and keeps those with
    // |nx| < 1 and |ny| < 1 (the rotated square).  Only the samples it keeps contribute, so the
    // quad walks, row by row, a column span that covers the square with a 0.01-pixel margin
    // (the float bounds and the float test differ by ~1e-5 pixel; the exact test below still
    // decides each sample) -- same samples, same (y, x) order, ~45% fewer iterations.
    // (RECT: every column of the box; the exact test below decides)
    const bool use_c = !RECT && fabs_(crspt) > 1e-4f / spt;
    const bool use_s = !RECT && fabs_(srspt) > 1e-4f / spt;
    const float icr = use_c ? 1.0f / crspt : 0.0f, isr = use_s ? 1.0f / srspt : 0.0f;
    const float kInf = as_float(0x7f800000u);
    auto row_span = [&](int r, int& lo, int& len) {
        const float dy = (ymin + (float)r) - pty;
        float a = -kInf, bnd = kInf;
        if (use_c) {
            const float p = (-1.0f - srspt * dy) * icr, q = (1.0f - srspt * dy) * icr;
            a = fmax_(a, fmin_(p, q));
            bnd = fmin_(bnd, fmax_(p, q));
        }
        if (use_s) {
            const float p = (crspt * dy - 1.0f) * isr, q = (crspt * dy + 1.0f) * isr;
            a = fmax_(a, fmin_(p, q));
            bnd = fmin_(bnd, fmax_(p, q));
        }
        const float cl = fmax_(0.0f, ceilf(ptx + a - xmin - 0.01f));
        const float ch = fmin_((float)(ncols - 1), floor_(ptx + bnd - xmin + 0.01f));
        lo = (int)cl;
        len = ch >= cl ? (int)ch - lo + 1 : 0;
    };
    // lane sub starts at sample sub of the span sequence, then advances 4 samples per step
    int wr = 0, wc = sub, wlo = 0, wlen = 0;
    if (nrows > 0 && ncols > 0) row_span(0, wlo, wlen);
    else wr = nrows;
    auto normalize = [&]() {
        while (wr < nrows && wc >= wlen) {
            wc -= wlen;
            if (++wr < nrows) row_span(wr, wlo, wlen);
        }
    };
    normalize();
    for (;;) {
        // the quad's lane 0 holds its earliest sample: the quad stops together
        if (qbcast<0>(wr < nrows ? 1 : 0) == 0) break;
        int fidx = -1;
        float weight = 0.f, weight1 = 0.f, weight2 = 0.f;
        if (wr < nrows) {
            const float x = xmin + (float)(wlo + wc), y = ymin + (float)wr;
            const float dx = x - ptx, dy = y - pty;
            float nx, ny;
            if (RECT) {
                nx = dx / sptx;
                ny = dy / spty;
            } else {
                nx = fma_(crspt, dx, srspt * dy);
                ny = fma_(crspt, dy, -(srspt * dx));
            }
            const float nxn = fabs_(nx), nyn = fabs_(ny);
            if (nxn < 1.0f && nyn < 1.0f) {
                const float2 cc = grad_at(g, W, (int)x, (int)y);
                // (float)(1.0 - (double)n) of the reference: 1 - n is exact in double, so the
                // single float subtraction rounds to the same value
                const float wx = 1.0f - nxn, wy = 1.0f - nyn;
                float theta;
                if (RECT) {
                    weight = wx * wy * cc.x;
                    theta = (-cc.y) * rpi;
                } else {
                    const float dnx = nx + ox, dny = ny + oy;
                    const float ww = exp_mid_(-0.125f * fma_(dnx, dnx, dny * dny));   // in [-1.6, 0]
                    weight = ww * wx * wy * cc.x;
                    theta = (anglef - cc.y) * rpi;
                }
                if (theta < 0) theta += 8.0f;
                const float fo = floor_(theta);
                fidx = (int)fo;
                weight1 = fo + 1.0f - theta;
                weight2 = theta - fo;
            }
            wc += 4;
            normalize();
        }
        const int f4[4] = {qbcast<0>(fidx), qbcast<1>(fidx), qbcast<2>(fidx), qbcast<3>(fidx)};
        const float w4[4] = {qbcastf<0>(weight), qbcastf<1>(weight), qbcastf<2>(weight),
                             qbcastf<3>(weight)};
        const float a4[4] = {qbcastf<0>(weight1), qbcastf<1>(weight1), qbcastf<2>(weight1),
                             qbcastf<3>(weight1)};
        const float b4[4] = {qbcastf<0>(weight2), qbcastf<1>(weight2), qbcastf<2>(weight2),
                             qbcastf<3>(weight2)};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            // sample q adds w1*w to bin f and w2*w to bin f+1, for f in 0..7 only (the
            // reference's unrolled k == fidx test drops fidx == 8 at theta == 8)
            // Branch-free: a non-matching bin adds fma(0, w, acc) = acc exactly (accumulators
            // and weights are >= +0, and an invalid sample has w = 0).
            const int f = f4[q];
            const float s0 = f == kb ? a4[q] : (f + 1 == kb ? b4[q] : 0.0f);
            const float s1 = f == kb + 1 ? a4[q] : (f == kb ? b4[q] : 0.0f);
            const float s8 = f == 7 ? b4[q] : 0.0f;
            acc0 = fma_(s0, w4[q], acc0);
            acc1 = fma_(s1, w4[q], acc1);
            acc8 = fma_(s8, w4[q], acc8);
        }
    }
    if (sub == 0) acc0 += acc8;   // des[0] += des[8]
    float des[8];
    des[0] = qbcastf<0>(acc0); des[1] = qbcastf<0>(acc1);
    des[2] = qbcastf<1>(acc0); des[3] = qbcastf<1>(acc1);
    des[4] = qbcastf<2>(acc0); des[5] = qbcastf<2>(acc1);
    des[6] = qbcastf<3>(acc0); des[7] = qbcastf<3>(acc1);
    if (fp.normalize) {
        // NormalizeDescriptor_Kernel: sums over the 32 float4s in order (cells 0..15)
        const int g0 = lane & ~63;
        float a = sq4(des[0], des[1], des[2], des[3]);
        float bq = sq4(des[4], des[5], des[6], des[7]);
        float norm1 = 0.f;
        for (int q = 0; q < 16; q++) {
            norm1 += __shfl(a, g0 + 4 * q, 64);
            norm1 += __shfl(bq, g0 + 4 * q, 64);
        }
        norm1 = rsqrt_(norm1);
#pragma unroll
        for (int i = 0; i < 8; i++) des[i] = fmin_(0.2f, des[i] * norm1);
        a = sq4(des[0], des[1], des[2], des[3]);
        bq = sq4(des[4], des[5], des[6], des[7]);
        float norm2 = 0.f;
        for (int q = 0; q < 16; q++) {
            norm2 += __shfl(a, g0 + 4 * q, 64);
            norm2 += __shfl(bq, g0 + 4 * q, 64);
        }
        norm2 = rsqrt_(norm2);
#pragma unroll
        for (int i = 0; i < 8; i++) des[i] *= norm2;
    }
    if (sub < 2) {
        float4* dst = reinterpret_cast<float4*>(desc + (size_t)out * 128 + cell * 8 + sub * 4);
        *dst = sub == 0 ? make_float4(des[0], des[1], des[2], des[3])
                        : make_float4(des[4], des[5], des[6], des[7]);
        if (hdesc)   // the row also to page-locked host memory (k_descriptor_wide)
            *reinterpret_cast<float4*>(hdesc + (size_t)out * 128 + cell * 8 + sub * 4) = *dst;
    }
}

// ------------------------------------------------------------------------------------------
// Relaxed-order descriptor (the shipped default).  Same samples, same weights, same bins as
// descriptor_one -- the reference's ComputeDescriptor_Kernel / ComputeDescriptorRECT_Kernel
// (ProgramCU.cu:1013-1171) -- but each sample's contribution is formed and accumulated by ONE
// lane, in any order:
//   * each of the quad's 4 lanes walks every 4th sample of its cell and keeps all 8 bins in
//     registers; the 4 partial histograms are summed by DPP at the end (descriptor_one instead
//     broadcasts every sample to the 4 lanes so that each bin sees the reference's fma order);
//   * the linear bin interpolation is the tent max(0, 1 - |theta - k|) per bin (bin 0 also
//     takes the wrap-around of bin 8, ProgramCU.cu:1094): 2 VALU + 1 fma per bin, no selects;
//   * gradient magnitude, atan2, the Gaussian window and the normalisation use the hardware
//     v_sqrt / v_rcp / v_exp (1 ulp) and a short atan2 series (|error| < 1e-6 rad), except
//     near the one discontinuity of the reference's binning (a sample whose theta rounds to
//     8.0 is dropped), where the oracle's atan2 decides.
// Every difference to the reference's arithmetic is continuous in the inputs and of the order of
// a float ulp, so descriptors agree with the oracle to L2 ~1e-6 (tests: < 1e-4, the north star's
// bound; descriptor_one stays the bit-exact test mode, SGPU_DEBUG_EXACT_DESCRIPTOR).
__device__ __forceinline__ float atan2_relaxed(float y, float x) {
    const float ax = fabs_(x), ay = fabs_(y);
    const float mx = fmax_(ax, ay), mn = fmin_(ax, ay);
    const bool red = mn > 0.414213562f * mx;           // reduce to |t| <= tan(pi/8)
    const float t = (red ? mn - mx : mn) * __builtin_amdgcn_rcpf(red ? mn + mx : mx);
    const float z = t * t;
    float p = -0.0909090909f;                           // odd series to t^11: |err| < 1e-6
    p = fma_(p, z, 0.111111111f);
    p = fma_(p, z, -0.142857143f);
    p = fma_(p, z, 0.2f);
    p = fma_(p, z, -0.333333333f);
    float r = fma_(p * z, t, t) + (red ? 0.785398163f : 0.0f);
    r = ay > ax ? 1.57079633f - r : r;
    r = (as_uint(x) >> 31) ? 3.14159265f - r : r;
    return (as_uint(y) >> 31) ? -r : r;
}

// Quad (xor) butterfly sum: every lane of the quad ends with the quad's total.
__device__ __forceinline__ float quad_sum(float v) {
    v += as_float((uint32_t)__builtin_amdgcn_mov_dpp((int)as_uint(v), 0xB1, 0xF, 0xF, false));  // [1,0,3,2]
    v += as_float((uint32_t)__builtin_amdgcn_mov_dpp((int)as_uint(v), 0x4E, 0xF, 0xF, false));  // [2,3,0,1]
    return v;
}

static_assert(SGK_DESC_RSTEP == 0 || SGK_DESC_RSTEP == 1 || SGK_DESC_RSTEP == 2 ||
                  SGK_DESC_RSTEP == 4, "rows per quad step (0: flat strip order)");

template <bool RECT>
__device__ __forceinline__ void descriptor_fast(uint32_t e, int lane,
                                                const float* __restrict__ pyr,
                                                const float4* __restrict__ feat,
                                                const int2* __restrict__ feat_info,
                                                const FeatureParams& fp,
                                                float* __restrict__ desc, uint32_t out) {
    const int cell = lane >> 2, sub = lane & 3;
    const int ix = cell & 3, iy = cell >> 2;
    const float4 key = feat[e];
    const int2 in = feat_info[e];
    const int o = in.y / fp.d, j = in.y - o * fp.d;
    const OctaveDesc& od = fp.oct[o];
    const int W = od.wa, H = od.h;
    const float* g = pyr + od.gauss_off + (long long)(1 + j) * od.level_stride +
                     (long long)in.x * W * H;
    const float rpi = (float)(4.0 / 3.14159265358979323846);
    // cell geometry exactly as descriptor_one (so both visit the same samples)
    float spt = 0.f, anglef = 0.f, cspt = 0.f, sspt = 0.f, crspt = 0.f, srspt = 0.f;
    float ox = 0.f, oy = 0.f, ptx, pty, bszx, bszy;
    const float sptx = key.z * 0.25f, spty = key.w * 0.25f;
    if (RECT) {
        ptx = fma_(sptx, ix + 0.5f, key.x);
        pty = fma_(spty, iy + 0.5f, key.y);
        bszx = sptx;
        bszy = spty;
    } else {
        spt = fabs_(key.z * fp.window_factor);
        float s, c;
        sincos_(key.w, &s, &c);
        anglef = (double)key.w > 3.14159265358979323846
                     ? (float)((double)key.w - (2.0 * 3.14159265358979323846))
                     : key.w;
        cspt = c * spt;
        sspt = s * spt;
        crspt = c / spt;
        srspt = s / spt;
        ox = ix - 1.5f;
        oy = iy - 1.5f;
        ptx = fma_(cspt, ox, -(sspt * oy)) + key.x;
        pty = fma_(cspt, oy, sspt * ox) + key.y;
        bszx = bszy = fabs_(cspt) + fabs_(sspt);
    }
    const float xmin = fmax_(1.5f, floor_(ptx - bszx) + 0.5f);
    const float ymin = fmax_(1.5f, floor_(pty - bszy) + 0.5f);
    const float xmax = fmin_(W - 1.5f, floor_(ptx + bszx) + 0.5f);
    const float ymax = fmin_(H - 1.5f, floor_(pty + bszy) + 0.5f);
    const int ncols = xmax >= xmin ? (int)(xmax - xmin) + 1 : 0;
    const int nrows = ymax >= ymin ? (int)(ymax - ymin) + 1 : 0;
    const bool use_c = !RECT && fabs_(crspt) > 1e-4f / spt;
    const bool use_s = !RECT && fabs_(srspt) > 1e-4f / spt;
    // The row's column span as the intersection of the two slabs |nx| <= 1 and |ny| <= 1, each
    // linear in dy: descriptor_one's row_span refactored into 4 fma and no selects on the signs
    // of the coefficients (the 0.01-pixel margin absorbs the different rounding; the per-sample
    // test decides).  RECT: the whole row of the box.
    const float icr = use_c ? 1.0f / crspt : 0.0f, isr = use_s ? 1.0f / srspt : 0.0f;
    const float hu = use_c ? fabs_(icr) : 1e30f, su = use_c ? srspt * icr : 0.0f;
    const float hv = use_s ? fabs_(isr) : 1e30f, cv = use_s ? crspt * isr : 0.0f;
    const float k_lo = ptx - xmin - 0.01f, k_hi = ptx - xmin + 0.01f;
    const float dy0 = ymin - pty;
    auto row_span = [&](int r, int& lo, int& len) {
        const float dy = dy0 + (float)r;
        const float a = fmax_(fma_(-su, dy, -hu), fma_(cv, dy, -hv));
        const float bnd = fmin_(fma_(-su, dy, hu), fma_(cv, dy, hv));
        const float cl = fmax_(0.0f, ceilf(a + k_lo));
        const float ch = fmin_((float)(ncols - 1), floor_(bnd + k_hi));
        lo = (int)cl;
        len = ch >= cl ? (int)ch - lo + 1 : 0;
    };
    const float irx = RECT ? __builtin_amdgcn_rcpf(sptx) : 0.f;
    const float iry = RECT ? __builtin_amdgcn_rcpf(spty) : 0.f;
    const float kexp = -0.125f * 1.44269504f;           // e^(-x/8) = 2^(kexp x)
    const int ixmin = (int)xmin, iymin = (int)ymin;
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; k++) acc[k] = 0.0f;
    // One sample: its cell coordinates from the row offset dy and column offset dx (both from
    // the reference's rounded cell centre), its gradient (gx, gy); adds nothing when !valid.
    auto sample = [&](float dx, float dy, float gx, float gy, bool valid) {
        float nx, ny;
        if (RECT) {
            nx = dx * irx;
            ny = dy * iry;
        } else {
            nx = fma_(crspt, dx, srspt * dy);
            ny = fma_(crspt, dy, -(srspt * dx));
        }
        const float wx = 1.0f - fabs_(nx), wy = 1.0f - fabs_(ny);
        const float m2 = fma_(gx, gx, gy * gy);
        const float m = 0.5f * __builtin_amdgcn_sqrtf(m2);
        float rot = atan2_relaxed(gy, gx);   // NaN at (0, 0)
        // theta = (anglef - rot) * 4/pi, +8 if negative, is dropped when it rounds to 8.0
        // (ProgramCU.cu:1071-1090): a discontinuity at anglef - rot in (-2^-21, 0] and near +2pi.
        // Within 1e-5 rad of those points (rare) rot is recomputed with the oracle's atan2, so
        // the drop decisions are the reference's exactly; elsewhere |error| < 1e-6 cannot reach
        // them.
        const float dd = fabs_(anglef - rot);
        if (dd < 1e-5f || dd > 6.2831753f) rot = atan2_(gy, gx);
        rot = m2 == 0.0f ? 0.0f : rot;
        float w = m * wx * wy;
        float theta;
        if (RECT) {
            theta = -rot * rpi;
        } else {
            const float dnx = nx + ox, dny = ny + oy;
            w *= __builtin_amdgcn_exp2f(kexp * fma_(dnx, dnx, dny * dny));
            theta = (anglef - rot) * rpi;
        }
        if (theta < 0) theta += 8.0f;
        // outside the rotated square (|n| >= 1) or theta == 8 (the reference's fidx == 8 is
        // dropped) the sample adds nothing
        w = (valid && wx > 0.0f && wy > 0.0f && theta < 8.0f) ? w : 0.0f;
        acc[0] = fma_(__builtin_amdgcn_fmed3f(fmax_(1.0f - theta, theta - 7.0f), 0.0f, 1.0f), w,
                      acc[0]);
#pragma unroll
        for (int k = 1; k < 8; k++)
            acc[k] = fma_(__builtin_amdgcn_fmed3f(1.0f - fabs_(theta - (float)k), 0.0f, 1.0f), w,
                          acc[k]);
    };
    // Lane sub walks rows sub, sub + 4, ... of its cell's box, each row's span in strips of 4
    // consecutive samples: the strip's gradient neighbours come from 4 vector loads -- row y at
    // columns x-1 .. x+2 and x+1 .. x+4, rows y-1 and y+1 at x .. x+3 -- instead of 16 scalar
    // gathers (the gathers of 16 cells saturate the texture-address/L1 path: 42 cache-line
    // lookups per load instruction), and the 4 samples are independent dependency chains.
    const char* gb = reinterpret_cast<const char*>(g);
    typedef float f4v __attribute__((ext_vector_type(4)));
    auto ld4 = [&](uint32_t b) { return *reinterpret_cast<const f4v*>(gb + b); };
    // The strips are walked as one flat sequence with the next strip's 4 loads issued before the
    // current strip's samples (software pipelining: a strip's gathers overlap the previous
    // strip's arithmetic).  The loads are unconditional 16-byte loads: at the right edge a strip
    // may read up to 4 floats past the row end, which are the next row's (a sample is at most in
    // column W-2 and row H-2) and feed no valid sample; past the last strip a lane re-reads its
    // last strip.
    // DESC_RSTEP rows walked by the quad side by side: lanes per row LPR = 4 / RSTEP, lane
    // (rsub, csub) walks rows rsub, rsub + RSTEP, ... in strips starting 4 csub columns into the
    // span, 4 LPR apart (RSTEP 4: every lane its own rows; 2: two lanes on adjacent strips of one
    // row, so a load instruction touches half the cache lines)
    // RSTEP 0 (flat): the cell's strips in row-major order, strip f to lane f mod 4, so the
    // quad's 4 lanes read 16 consecutive columns of one row (or the end of one row and the start
    // of the next): one or two cache lines per quad and load instead of four, and no lane idles
    // on a short row.  Each lane keeps its own cursor (row r, strip s of the row) and moves it 4
    // strips per step.
    constexpr int RSTEP = SGK_DESC_RSTEP;
    constexpr int LPR = 4 / (RSTEP ? RSTEP : 4);
    const int rsub = RSTEP ? sub / LPR : 0, c4 = RSTEP ? 4 * (sub % LPR) : 0;
    int r = rsub, c = 0, lo = 0, len = 0, s = sub, ns = 0;
    auto next_row = [&]() {   // advance r (by RSTEP) to the next row with samples for this lane
        for (; r < nrows; r += RSTEP) {
            row_span(r, lo, len);
            if (len > c4) break;
        }
    };
    auto flat_norm = [&]() {   // move (r, s) forward over rows until strip s exists in row r
        while (s >= ns && r < nrows) {
            s -= ns;
            if (++r < nrows) {
                row_span(r, lo, len);
                ns = (len + 3) >> 2;
            }
        }
    };
    if (RSTEP == 0) {
        r = ncols > 0 ? 0 : nrows;
        if (r < nrows) {
            row_span(0, lo, len);
            ns = (len + 3) >> 2;
        }
        flat_norm();
        c = lo + 4 * s;
    } else {
        if (ncols > 0) next_row(); else r = nrows;
        c = lo + c4;
    }
    f4v na, nb, nu, nd;
    // the address loaded when no sample is left: row 1, column 1 of the plane, whose 4 loads
    // (columns 0 .. 5 of row 1, columns 1 .. 4 of rows 0 and 2) stay inside it for any feature --
    // a caller keypoint far outside the image has an empty box and unbounded ixmin / iymin
    uint32_t npo = 4u * (uint32_t)(W + 1);
    auto fetch = [&]() {
        if (r < nrows) npo = 4u * (uint32_t)((iymin + r) * W + ixmin + c);
        na = ld4(npo - 4u);            // x-1 .. x+2
        nb = ld4(npo + 4u);            // x+1 .. x+4
        nu = ld4(npo - 4u * W);        // row y-1, x .. x+3
        nd = ld4(npo + 4u * W);        // row y+1, x .. x+3
    };
    fetch();
    while (r < nrows) {
        const f4v a = na, b = nb, up = nu, dn = nd;
        const float dy = (ymin + (float)r) - pty;
        const int nv = lo + len - c;   // samples of this strip inside the span
        const float dx0 = (xmin + (float)c) - ptx;
        if (RSTEP == 0) {
            s += 4;
            flat_norm();
            c = lo + 4 * s;
        } else {
            c += 4 * LPR;
            if (c >= lo + len) {
                r += RSTEP;
                next_row();
                c = lo + c4;
            }
        }
        fetch();
        sample(dx0, dy, b.x - a.x, dn.x - up.x, true);
        sample(dx0 + 1.0f, dy, b.y - a.y, dn.y - up.y, nv > 1);
        sample(dx0 + 2.0f, dy, b.z - a.z, dn.z - up.z, nv > 2);
        sample(dx0 + 3.0f, dy, b.w - a.w, dn.w - up.w, nv > 3);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) acc[k] = quad_sum(acc[k]);
    // lane sub owns bins 2 sub, 2 sub + 1 of its cell
    float b0 = acc[0], b1 = acc[1];
    b0 = sub == 1 ? acc[2] : b0; b1 = sub == 1 ? acc[3] : b1;
    b0 = sub == 2 ? acc[4] : b0; b1 = sub == 2 ? acc[5] : b1;
    b0 = sub == 3 ? acc[6] : b0; b1 = sub == 3 ? acc[7] : b1;
    if (fp.normalize) {
        float s = fma_(b0, b0, b1 * b1);
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) s += __shfl_xor(s, k, 64);
        const float n1 = __builtin_amdgcn_rsqf(s);
        b0 = fmin_(0.2f, b0 * n1);
        b1 = fmin_(0.2f, b1 * n1);
        s = fma_(b0, b0, b1 * b1);
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) s += __shfl_xor(s, k, 64);
        const float n2 = __builtin_amdgcn_rsqf(s);
        b0 *= n2;
        b1 *= n2;
    }
    *reinterpret_cast<float2*>(desc + (size_t)out * 128 + cell * 8 + sub * 2) = make_float2(b0, b1);
}

// ------------------------------------------------------------------------------------------
// Pixel-major descriptor (round 4, the shipped default for detected features).  descriptor_fast
// visits a window pixel once per cell whose rotated square holds it -- 2.56 times on average, up to
// 4 -- and pays the pixel's gradient magnitude, atan2, Gaussian weight and bin split on every visit,
// while only the spatial weight (1 - |nx|)(1 - |ny|) depends on the cell.  Here every pixel is
// evaluated once: the window |dnx|, |dny| < 2.5 (feature frame, cell units, dnx = nx + ox) is cut
// into the 5 x 5 "dual" cells of the half-cell-shifted grid, dual cell (a, b) = floor(dnx + 2.5),
// floor(dny + 2.5); a pixel of dual cell (a, b) lies in the squares of exactly the cells (a-1, b-1),
// (a, b-1), (a-1, b), (a, b), with the bilinear weights (1-u)(1-v), u(1-v), (1-u)v, uv (u, v its
// offsets inside the dual cell), which are the reference's (1 - |nx|)(1 - |ny|) for those cells
// (ProgramCU.cu:1044-1094).  Two lanes own each dual cell (lanes 0..49, alternate rows); a pixel's
// 8 contributions (4 cells x the 2 interpolated orientation bins) go to the wave's LDS histogram
// as no-return ds_add_f32 (IEEE adds in the LDS), laid out [bin][6 x 6 cells][lane copy]: the
// 6 x 6 grid gives the 4 cells of a dual cell constant offsets (0, 1, 6, 7 cells) and absorbs the
// border cells -1 and 4, which are never read; the two lanes of a dual cell add to their own copy,
// so no two lanes of an instruction hit one address.  Membership of a pixel is decided from dnx,
// dny, which every lane computes with the same operations, so each pixel is counted by exactly one
// lane.  Same samples, weights and bins as descriptor_fast (relaxed order and transcendentals):
// L2 ~1e-6 from the oracle; descriptor_one remains the bit-exact mode.
constexpr int kDualWords = 50 * 33;   // reduction words per wave
// One wave per feature for every feature count.  Two-wave forms for few features (a single
// image) were measured in round 4: splitting each dual cell's rows between the
// pair (C2 30.9 vs 41 us) changes the sums' order, so a batch's descriptors no longer equalled a
// single image's; the bit-identical forms lost -- the pair splitting the bins 49.3 us (both waves
// walk every row), the one-wave kernel walking the pair's row groups in turn 1.786-1.80 vs
// 1.725-1.74 ms per 128 x 1080p step.
#if SGK_DUAL_WPE
#define SGK_DUAL_ATTR __attribute__((amdgpu_waves_per_eu(SGK_DUAL_WPE)))
#else
#define SGK_DUAL_ATTR
#endif
__device__ __forceinline__ void descriptor_dual(uint32_t e, int lane, const float* __restrict__ pyr,
                                                const float4* __restrict__ feat,
                                                const int2* __restrict__ feat_info,
                                                const FeatureParams& fp, float* __restrict__ desc,
                                                uint32_t out, float* __restrict__ hist) {
    const float4 key = feat[e];
    const int2 in = feat_info[e];
    const int o = in.y / fp.d, j = in.y - o * fp.d;
    const OctaveDesc& od = fp.oct[o];
    const int W = od.wa, H = od.h;
    const float* g = pyr + od.gauss_off + (long long)(1 + j) * od.level_stride +
                     (long long)in.x * W * H;
    const float rpi = (float)(4.0 / 3.14159265358979323846);
    const float spt = fabs_(key.z * fp.window_factor);
    float s, c;
    sincos_(key.w, &s, &c);
    const float anglef = (double)key.w > 3.14159265358979323846
                             ? (float)((double)key.w - (2.0 * 3.14159265358979323846))
                             : key.w;
    const float cspt = c * spt, sspt = s * spt, crspt = c / spt, srspt = s / spt;
    // this lane's dual cell (a, b) and histogram copy; lanes 50..63 walk nothing
    const int q = lane >> 1, cp = lane & 1;
    const int a = q % 5, b = q / 5;
    const float fa = (float)a, fb = (float)b;
    // the dual cell's square: centre (a - 2, b - 2) cells from the keypoint, side spt
    const float fx = fa - 2.0f, fy = fb - 2.0f;
    const float cxi = key.x + fma_(cspt, fx, -(sspt * fy));
    const float cyi = key.y + fma_(sspt, fx, cspt * fy);
    const float hb = 0.5f * (fabs_(cspt) + fabs_(sspt)) + 0.01f;
    // pixel p has its sample at p + 0.5; rows and columns 1 .. H-2 / W-2 (the reference's box
    // clamp to [1.5, W - 1.5])
    // (clamped as floats first: a caller keypoint far outside the image must not saturate the
    // int conversion, whose y0 + 1 would wrap)
    const float fH = (float)H, fW = (float)W;
    const int y0 = (int)fmax_(1.0f, fmin_(fH, ceilf(cyi - hb - 0.5f)));
    int y1 = (int)fmin_(fH - 2.0f, fmax_(-1.0f, floor_(cyi + hb - 0.5f)));
    const int bx0 = (int)fmax_(1.0f, fmin_(fW, ceilf(cxi - hb - 0.5f)));
    const int bx1 = (int)fmin_(fW - 2.0f, fmax_(-1.0f, floor_(cxi + hb - 0.5f)));
    if (q >= 25 || !(spt > 0.0f)) y1 = y0 - 1;
    // row span: the columns whose u = dnx + 2.5 - a and v = dny + 2.5 - b can lie in [0, 1],
    // dnx = crspt dxk + srspt dyk, dny = crspt dyk - srspt dxk (dxk, dyk from the keypoint); the
    // 0.01-pixel margin absorbs rounding, the per-pixel test decides
    const bool use_c = fabs_(crspt) > 1e-4f / spt, use_s = fabs_(srspt) > 1e-4f / spt;
    const float icr = use_c ? 1.0f / crspt : 0.0f, isr = use_s ? 1.0f / srspt : 0.0f;
    auto row_span = [&](int py, int& lo, int& len) {
        const float dyk = ((float)py + 0.5f) - key.y;
        float l = -1e30f, h = 1e30f;
        if (use_c) {   // crspt dxk in [-Ku, 1 - Ku], Ku = srspt dyk + 2.5 - a
            const float p = -fma_(srspt, dyk, 2.5f - fa) * icr;
            l = fmax_(l, p + fmin_(0.0f, icr));
            h = fmin_(h, p + fmax_(0.0f, icr));
        }
        if (use_s) {   // -srspt dxk in [-Kv, 1 - Kv], Kv = crspt dyk + 2.5 - b
            const float p = fma_(crspt, dyk, 2.5f - fb) * isr;
            l = fmax_(l, p + fmin_(0.0f, -isr));
            h = fmin_(h, p + fmax_(0.0f, -isr));
        }
        const float xl = ceilf(l + key.x - 0.5f - 0.01f), xh = floor_(h + key.x - 0.5f + 0.01f);
        const int il = max(bx0, (int)fmax_(xl, -1.0f)), ih = min(bx1, (int)fmin_(xh, fW));
        lo = il;
        len = ih >= il ? ih - il + 1 : 0;
    };
    const float kexp = -0.125f * 1.44269504f;   // e^(-x/8) = 2^(kexp x)
    // The reference measures nx, ny from each cell's centre (ptx, pty), rounded to a float at
    // image-coordinate magnitude (ulp up to 1.2e-4 pixel at x ~ 2000; ProgramCU.cu:1044-1062).
    // Measured from the keypoint instead, the weights differ from the reference's by ~1e-5
    // (descriptor L2 up to 1.2e-5); so the 4 cells' weights use the reference's rounded centres:
    // nx = dnx - ox', ox' = crspt (ptx - x_key) + srspt (pty - y_key) (both differences exact),
    // and for the dual cell's left / right cells |nx| = nx / -nx, so that 1 - |nx| is one
    // subtraction (at the dual cell's edges the weights cross 0 by a rounding, continuously).
    float oxl[4], oyl[4];   // 1 -/+ ox', 1 -/+ oy' of cells (a-1,b-1), (a,b-1), (a-1,b), (a,b)
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float ox = (float)(a - 1 + (k & 1)) - 1.5f, oy = (float)(b - 1 + (k >> 1)) - 1.5f;
        const float ptx = fma_(cspt, ox, -(sspt * oy)) + key.x;
        const float pty = fma_(cspt, oy, sspt * ox) + key.y;
        const float ex = ptx - key.x, ey = pty - key.y;
        const float oxp = fma_(crspt, ex, srspt * ey), oyp = fma_(crspt, ey, -(srspt * ex));
        oxl[k] = (k & 1) ? 1.0f - oxp : 1.0f + oxp;
        oyl[k] = (k >> 1) ? 1.0f - oyp : 1.0f + oyp;
    }
    // the lane's 4 cells x 8 bins, cells in pairs: acc[h][k] = bin k of cell slots 2h, 2h + 1
    // (slot 0: cell (a-1, b-1), 1: (a, b-1), 2: (a-1, b), 3: (a, b)), so that each packed fma
    // takes one scalar tent weight and a pair of cell weights
    f2v acc[2][8];
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int k = 0; k < 8; k++) acc[h][k] = f2v{0.0f, 0.0f};
    // a pixel's angle: the relaxed atan2, and within 1e-5 rad of the reference's one binning
    // discontinuity (theta rounding to 8.0 is dropped) the oracle's atan2 (descriptor_fast's
    // rule); the exact form is evaluated in one shared loop for the strip's flagged pixels (rare)
    auto pixel = [&](float dxk, float sdy, float cdy, float gx, float gy, bool valid) {
        const float m2 = fma_(gx, gx, gy * gy);
        // the relaxed atan2, and within 1e-5 rad of the reference's one binning discontinuity
        // (theta rounding to 8.0 is dropped) the oracle's atan2 (descriptor_fast's rule; rare)
        float rot = atan2_relaxed(gy, gx);
        const float dd = fabs_(anglef - rot);
        if (dd < 1e-5f || dd > 6.2831753f) rot = atan2_(gy, gx);
        rot = m2 == 0.0f ? 0.0f : rot;
        const float dnx = fma_(crspt, dxk, sdy);          // sdy = srspt dyk
        const float dny = fma_(-srspt, dxk, cdy);         // cdy = crspt dyk
        const float t = dnx + 2.5f, tv = dny + 2.5f;
        const float ft = floor_(t), fv = floor_(tv);
        const float m = 0.5f * __builtin_amdgcn_sqrtf(m2);
        const float w = m * __builtin_amdgcn_exp2f(kexp * fma_(dnx, dnx, dny * dny));
        float theta = (anglef - rot) * rpi;
        if (theta < 0) theta += 8.0f;
        // theta outside [0, 8) (a caller orientation far outside (-pi, pi]) adds to no bin, as the
        // reference's k == fidx test; it would also index outside the histogram
        const bool take = valid && ft == fa && fv == fb && theta >= 0.0f && theta < 8.0f;
        // branch-free: a pixel not taken adds fma(tent, 0, acc) = acc (its theta replaced by 0 so
        // that no tent is NaN)
        const float wt = take ? w : 0.0f;
        const float th = take ? theta : 0.0f;
        const f2v cpa = wt * (f2v{oxl[0], oxl[1]} + f2v{-dnx, dnx}) * (f2v{oyl[0], oyl[1]} - dny);
        const f2v cpb = wt * (f2v{oxl[2], oxl[3]} + f2v{-dnx, dnx}) * (f2v{oyl[2], oyl[3]} + dny);
        // tent weights max(0, 1 - |theta - k|), bin 0 also taking the wrap of bin 8
        // (ProgramCU.cu:1094), as descriptor_fast; then the outer product with the cell weights
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const float tk = k == 0 ? __builtin_amdgcn_fmed3f(fmax_(1.0f - th, th - 7.0f), 0.0f, 1.0f)
                                    : __builtin_amdgcn_fmed3f(1.0f - fabs_(th - (float)k), 0.0f, 1.0f);
            acc[0][k] = pk_fma(cpa, tk, acc[0][k]);
            acc[1][k] = pk_fma(cpb, tk, acc[1][k]);
        }
    };
    // walk: rows y0 + cp, y0 + cp + 2, ...; each row's span in strips of 4 pixels whose gradient
    // neighbours come from 4 vector loads (as descriptor_fast), the next strip's loads issued
    // before the current strip's pixels
    const char* gb = reinterpret_cast<const char*>(g);
    typedef float f4v __attribute__((ext_vector_type(4)));
    auto ld4 = [&](uint32_t byte) { return *reinterpret_cast<const f4v*>(gb + byte); };
    constexpr int RSTEP = 2;   // lane cp walks rows y0 + cp, y0 + cp + 2, ...
    int r = 0, lo = 0, len = 0, cx = 0;
    auto next_row = [&]() {   // advance r (by RSTEP) to the next row with a nonempty span
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
        for (; r <= y1; r += RSTEP) {
            row_span(r, lo, len);
            if (len > 0) break;
        }
        cx = lo;
    };
    f4v na, nb, nu, nd;
    uint32_t npo = 4u * (uint32_t)(W + 1);   // row 1, column 1 when nothing is left (in-plane)
    auto fetch = [&]() {
        if (r <= y1) npo = 4u * (uint32_t)(r * W + cx);
        na = ld4(npo - 4u);            // x-1 .. x+2
        nb = ld4(npo + 4u);            // x+1 .. x+4
        nu = ld4(npo - 4u * W);        // row y-1, x .. x+3
        nd = ld4(npo + 4u * W);        // row y+1, x .. x+3
    };
    auto walk = [&](int r0) {
        r = r0;
        next_row();
        fetch();
        while (r <= y1) {
            const f4v gx = nb - na, gy = nd - nu;   // the strip's gradients (dx, dy per pixel)
            const float dyk = ((float)r + 0.5f) - key.y;
            const float sdy = srspt * dyk, cdy = crspt * dyk;
            const int nv = lo + len - cx;
            const float xc = (float)cx + 0.5f;   // (xc + i) - x_key: the same value in every lane
            cx += 4;
            if (cx >= lo + len) {
                r += RSTEP;
                next_row();
            }
            fetch();
            // one pixel at a time (sched_barrier): four interleaved took ~150 VGPRs
            pixel((xc) - key.x, sdy, cdy, gx.x, gy.x, true);
            __builtin_amdgcn_sched_barrier(0);
            pixel((xc + 1.0f) - key.x, sdy, cdy, gx.y, gy.y, nv > 1);
            __builtin_amdgcn_sched_barrier(0);
            pixel((xc + 2.0f) - key.x, sdy, cdy, gx.z, gy.z, nv > 2);
            __builtin_amdgcn_sched_barrier(0);
            pixel((xc + 3.0f) - key.x, sdy, cdy, gx.w, gy.w, nv > 3);
        }
    };
    // reduction: lanes 0..49 store their 32 bins ([lane][slot][bin], stride 33 floats against
    // bank conflicts); lane L then sums bins 2 sub, 2 sub + 1 of cell L >> 2 (descriptor_fast's
    // output layout) over the 4 dual cells x 2 lanes that hold that cell
    auto store_bins = [&]() {
        if (q < 25) {
            float* my = hist + lane * 33;
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    my[8 * (2 * h) + k] = acc[h][k].x;
                    my[8 * (2 * h + 1) + k] = acc[h][k].y;
                }
        }
        asm volatile("" ::: "memory");
    };
    const int cell = lane >> 2, sub = lane & 3;
    const int ix = cell & 3, iy = cell >> 2;
    float b0 = 0.0f, b1 = 0.0f;
    auto add_region = [&](const float* reg) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            // slot k of dual cell (ix + 1 - (k & 1), iy + 1 - (k >> 1)) is this cell
            const int dq = (iy + 1 - (k >> 1)) * 5 + ix + 1 - (k & 1);
#pragma unroll
            for (int c2 = 0; c2 < 2; c2++) {
                const float* src = reg + (2 * dq + c2) * 33 + 8 * k + 2 * sub;
                b0 += src[0];
                b1 += src[1];
            }
        }
        asm volatile("" ::: "memory");
    };
    walk(y0 + cp);
    store_bins();
    add_region(hist);
    if (fp.normalize) {
        float sn = fma_(b0, b0, b1 * b1);
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) sn += __shfl_xor(sn, k, 64);
        const float n1 = __builtin_amdgcn_rsqf(sn);
        b0 = fmin_(0.2f, b0 * n1);
        b1 = fmin_(0.2f, b1 * n1);
        sn = fma_(b0, b0, b1 * b1);
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) sn += __shfl_xor(sn, k, 64);
        const float n2 = __builtin_amdgcn_rsqf(sn);
        b0 *= n2;
        b1 *= n2;
    }
    *reinterpret_cast<float2*>(desc + (size_t)out * 128 + cell * 8 + sub * 2) = make_float2(b0, b1);
}

// One wave per feature (grid-stride), each wave with its own LDS histogram.
__global__ __launch_bounds__(256) SGK_DUAL_ATTR void k_descriptor_dual(const float* __restrict__ pyr,
                                                         const float4* __restrict__ feat,
                                                         const int2* __restrict__ feat_info,
                                                         const uint32_t* __restrict__ n_feat_dev,
                                                         const FeatureParams fp,
                                                         float* __restrict__ desc,
                                                         const int* __restrict__ out_index) {
    __shared__ float s_hist[4][kDualWords];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* hist = s_hist[wave];
    const uint32_t n = *n_feat_dev;
    for (uint32_t e = blockIdx.x * 4 + wave; e < n; e += gridDim.x * 4)
        descriptor_dual(e, lane, pyr, feat, feat_info, fp, desc,
                           out_index ? (uint32_t)out_index[e] : e, hist);
}

// ------------------------------------------------------------------------------------------
// Flat pixel-parallel descriptor (round 5, the shipped default for detected features).  The
// dual-cell kernel above gives every lane one dual cell and its own register histogram: 50 of 64
// lanes walk (lanes 50..63 idle), each lane's 4-pixel strips run past its row spans (masked
// pixels evaluated), and its gradient loads are 16-B gathers scattered over 25 cells.  Here the
// window's pixels are enumerated row-major over the rotated 5 x 5-cell square's row spans and
// dealt to the 64 lanes in turn (pixel p -> lane p mod 64): every lane busy, no masked tails,
// neighbouring lanes on neighbouring pixels (coalesced loads).  A pixel's dual cell (a, b) and
// its weights are those of descriptor_dual (the same dnx, dny, the reference's rounded cell
// centres, ProgramCU.cu:1044-1094, from a 6 x 6 per-feature table), its 4 cells x 2 orientation
// bins are 8 no-return 64-bit integer LDS adds (ds_add_u64 of a fixed-point word, to_fix32) into
// the wave's histogram, kept in kFlatCopies copies (lane mod kFlatCopies) against same-address
// serialisation and summed at the end.  Integer sums do not depend on their order, so a
// feature's descriptor does not depend on the batch around it or on how its pixels are split
// over waves (k_descriptor_wide); against the exact kernel the sums differ by the float order
// (L2 ~1e-6, tests/test_gpu_parity.py::test_shipped_descriptor_vs_exact).
constexpr int kFlatCopies = SGK_FLAT_COPIES;
static_assert(kFlatCopies >= 1 && kFlatCopies <= 32 && (kFlatCopies & (kFlatCopies - 1)) == 0,
              "histogram copies");
// [4 x 4 cells][8 bins][copies] 64-bit words, a (cell, bin)'s copies kFlatStride words apart from
// the next's.  Measured per 128 x 1080p step (tests/diag/r05m.sh): 4 copies 1.51 ms, 1 / 2 / 8 /
// 16 copies 2.83 / 1.91 / 2.07 / 3.79 ms; a padded stride (copies + 1) 1.68 ms
constexpr int kFlatStride = kFlatCopies + SGK_FLAT_PAD;
constexpr int kFlatHist = 16 * 8 * kFlatStride;
constexpr int kFlatRows = 64;                      // window rows per chunk (one per lane)
// + the 36-entry cell table (144 floats) + one flag word (kFlatFlag; padded to 16 bytes): set
// when a sample of the window has a weight that is not finite.  The reference adds such a
// weight like any other (ProgramCU.cu:1054-1082): a NaN then reaches every component through the
// norm, and min(0.2, NaN) = 0.2 makes the row uniform; an Inf leaves 0.2 in its bins and 0
// elsewhere (:1173-1208).  Integer sums cannot carry that: a flagged feature's row is stored as
// NaN, and k_descriptor_nonfinite, launched after these kernels for a caller's float input
// (FeatureParams::unit_input == 0), gives every NaN row to the exact kernel's descriptor_one.  descriptor_one
// inside these kernels instead cost them 76-100 bytes of scratch at their 64 VGPRs.
constexpr int kFlatFlag = 2 * kFlatHist + 144;
constexpr int kFlatWords = kFlatFlag + 4;

// A contribution as a 64-bit fixed-point word, 32 fraction bits (two's complement; |v| < 2^31):
// the integer part by floor, the fraction (exact in float) scaled by 2^32 and truncated (error <
// 2^-32).  LDS integer adds are full rate where float adds (ds_add_f32) serialise their lanes
// (~4 cycles per lane, 7.8 ms per 128 x 1080p step against 1.37 with integer adds,
// tests/diag/r05l.sh), and integer sums do not depend on their order.
typedef __attribute__((address_space(3))) unsigned long long lds_u64;

__device__ __forceinline__ unsigned long long to_fix32(float v) {
    const float fl = floor_(v);
    const uint32_t lo = (uint32_t)((v - fl) * 4294967296.0f);
    return ((unsigned long long)(uint32_t)(int)fl << 32) | lo;
}

// Inclusive wave scan by DPP (row_shr 1 / 2 / 4 / 8 within each row of 16 lanes, then
// row_bcast:15 and row_bcast:31 carry the row totals into the rows above): 6 VALU with DPP
// operands instead of 6 ds_bpermute round trips through the LDS crossbar.
__device__ __forceinline__ int wave_incl_scan_dpp(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 (rows 1, 3)
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 (rows 2, 3)
    return v;
}

// Sum over the wave, in every lane: DPP within each row of 16 (quad_perm swaps, row_ror 4 / 8),
// then the four row sums read as scalars (v_readlane) and added in row order.
__device__ __forceinline__ float wave_sum_dpp(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xb1, 0xf, 0xf, false));  // quad_perm [1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4e, 0xf, 0xf, false));  // quad_perm [2,3,0,1]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xf, 0xf, false)); // row_ror:4
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false)); // row_ror:8
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return (r0 + r1) + (r2 + r3);
}

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        const int u = __shfl_up(v, k, 64);
        if (lane >= k) v += u;
    }
    return v;
}

// The accumulation of feature e's window into the histogram at sh (kFlatWords floats): wave wv
// of nwv takes the window's 64-pixel steps wv, wv + nwv, ... (every step when nwv = 1).
__device__ __forceinline__ void flat_accumulate(uint32_t e, int lane, const float* __restrict__ pyr,
                                                const float4* __restrict__ feat,
                                                const int2* __restrict__ feat_info,
                                                const FeatureParams& fp, float* __restrict__ sh,
                                                int wv, int nwv) {
    // the histogram as an LDS-space pointer, stated: its adds can only be ds_add_u64 (an LDS
    // offset outside the allocation is dropped by the LDS), never flat atomics through a generic
    // address, which the compiler would have to fall back to if the LDS origin of `sh` were lost
    // (round 5's fi64 variant faulted with an aperture violation)
    lds_u64* hist = (lds_u64*)sh;   // kFlatHist
    // 36: (1 + ox', 1 - ox', 1 + oy', 1 - oy') of cell (i, j)
    float4* ctab = reinterpret_cast<float4*>(sh + 2 * kFlatHist);
    const float4 key = feat[e];
    const int2 in = feat_info[e];
    const int o = in.y / fp.d, j = in.y - o * fp.d;
    const OctaveDesc& od = fp.oct[o];
    const int W = od.wa, H = od.h;
    const float* g = pyr + od.gauss_off + (long long)(1 + j) * od.level_stride +
                     (long long)in.x * W * H;
    const float rpi = (float)(4.0 / 3.14159265358979323846);
    const float spt = fabs_(key.z * fp.window_factor);
    float s, c;
    sincos_(key.w, &s, &c);
    const float anglef = (double)key.w > 3.14159265358979323846
                             ? (float)((double)key.w - (2.0 * 3.14159265358979323846))
                             : key.w;
    const float cspt = c * spt, sspt = s * spt, crspt = c / spt, srspt = s / spt;
    // the histogram (every copy) to zero; the cell centre table: cell (i, j), i, j = -1 .. 4 at
    // (j + 1) * 6 + i + 1 -- the reference's rounded centre, measured in the feature frame
    // (descriptor_dual's oxl / oyl)
#pragma unroll
    for (int i = lane; i < kFlatHist / 2; i += 64)
        reinterpret_cast<float4*>(sh)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < 36) {
        const float ox = (float)(lane % 6 - 1) - 1.5f, oy = (float)(lane / 6 - 1) - 1.5f;
        const float ptx = fma_(cspt, ox, -(sspt * oy)) + key.x;
        const float pty = fma_(cspt, oy, sspt * ox) + key.y;
        const float ex = ptx - key.x, ey = pty - key.y;
        const float oxp = fma_(crspt, ex, srspt * ey), oyp = fma_(crspt, ey, -(srspt * ex));
        ctab[lane] = make_float4(1.0f + oxp, 1.0f - oxp, 1.0f + oyp, 1.0f - oyp);
    }
    unsigned long long badw = 0;   // lanes that met a weight that is not finite (uniform)
    // the window's bounding rows and columns: the 5 x 5-cell square (side 5 spt, rotated) around
    // the keypoint, clamped to rows / columns 1 .. H-2 / W-2 (the reference's [1.5, W - 1.5] box)
    const float hb = 2.5f * (fabs_(cspt) + fabs_(sspt)) + 0.01f;
    const float fH = (float)H, fW = (float)W;
    const int y0 = (int)fmax_(1.0f, fmin_(fH, ceilf(key.y - hb - 0.5f)));
    int y1 = (int)fmin_(fH - 2.0f, fmax_(-1.0f, floor_(key.y + hb - 0.5f)));
    const int bx0 = (int)fmax_(1.0f, fmin_(fW, ceilf(key.x - hb - 0.5f)));
    const int bx1 = (int)fmin_(fW - 2.0f, fmax_(-1.0f, floor_(key.x + hb - 0.5f)));
    if (!(spt > 0.0f)) y1 = y0 - 1;
    // a row's span: the columns whose dnx, dny can lie in [-2.5, 2.5) (0.05-pixel margin; the
    // per-pixel test decides)
    const bool use_c = fabs_(crspt) > 1e-4f / spt, use_s = fabs_(srspt) > 1e-4f / spt;
    const float icr = use_c ? 1.0f / crspt : 0.0f, isr = use_s ? 1.0f / srspt : 0.0f;
    const float kexp = -0.125f * 1.44269504f;   // e^(-x/8) = 2^(kexp x)
    const int copy = lane & (kFlatCopies - 1);
    asm volatile("" ::: "memory");
    for (int rb = y0; rb <= y1; rb += kFlatRows) {
        // this chunk's rows: lane L holds row rb + L's first column and first pixel index
        int lo = 0, len = 0;
        {
            const int py = rb + lane;
            if (py <= y1) {
                const float dyk = ((float)py + 0.5f) - key.y;
                float l = -1e30f, h = 1e30f;
                if (use_c) {   // crspt dxk in [-2.5 - srspt dyk, 2.5 - srspt dyk]
                    const float sd = srspt * dyk;
                    const float p0 = (-2.5f - sd) * icr, p1 = (2.5f - sd) * icr;
                    l = fmax_(l, fmin_(p0, p1));
                    h = fmin_(h, fmax_(p0, p1));
                }
                if (use_s) {   // -srspt dxk in [-2.5 - crspt dyk, 2.5 - crspt dyk]
                    const float cd = crspt * dyk;
                    const float p0 = (2.5f + cd) * isr, p1 = -(2.5f - cd) * isr;
                    l = fmax_(l, fmin_(p0, p1));
                    h = fmin_(h, fmax_(p0, p1));
                }
                const float xl = ceilf(l + key.x - 0.5f - 0.05f), xh = floor_(h + key.x - 0.5f + 0.05f);
                const int il = max(bx0, (int)fmax_(xl, -1.0f)), ih = min(bx1, (int)fmin_(xh, fW));
                lo = il;
                len = ih >= il ? ih - il + 1 : 0;
            }
        }
        const int incl = wave_incl_scan_dpp(len);
        const int rs = incl - len;                                   // row L's first pixel index
        const int total = __builtin_amdgcn_readlane(incl, kFlatRows - 1);
        int rcur = 0;   // a row at or before pixel `base`'s (uniform)
        for (int base = 64 * wv; base < total; base += 64 * nwv) {
            const int p = base + lane;
            const bool valid = p < total;
            // pixel p's row: rcur + the rows after it starting at or before p (their starts read
            // as uniform values; the loop stops at the first row past this step's pixels)
            int r = rcur;
            for (int k = rcur + 1; k < kFlatRows; k++) {
                const int sk = __builtin_amdgcn_readlane(rs, k);
                if (sk > base + 63 || sk >= total) break;
                r += p >= sk ? 1 : 0;
            }
            rcur = __builtin_amdgcn_readlane(r, 63);
            const int y = rb + r;
            // (the shuffles with every lane active: a lane outside the valid ones may be the
            // source; the asm keeps the compiler from moving them under the valid test)
            const int rsr = __shfl(rs, r, 64);        // row r's first pixel
            int xr = __shfl(lo, r, 64) + (p - rsr);
            asm volatile("" : "+v"(xr));
            const int x = valid ? xr : bx0;
            const int yc = valid ? y : y0;
            // 32-bit byte offsets from the level image's base (an image plane is < 4 GB)
            const char* gp = reinterpret_cast<const char*>(g) + 4u * (uint32_t)(yc * W + x);
            const uint32_t W4 = 4u * (uint32_t)W;
            // the gradient's 4 neighbours as 4 gathers (the left / right ones taken from the
            // neighbouring lanes by DPP measured slower)
            const float gx = *reinterpret_cast<const float*>(gp + 4) - *reinterpret_cast<const float*>(gp - 4);
            const float gy = *reinterpret_cast<const float*>(gp + W4) - *reinterpret_cast<const float*>(gp - W4);
            const float m2 = fma_(gx, gx, gy * gy);
            float rot = atan2_relaxed(gy, gx);
            const float dd = fabs_(anglef - rot);
            if (dd < 1e-5f || dd > 6.2831753f) rot = atan2_(gy, gx);
            rot = m2 == 0.0f ? 0.0f : rot;
            const float dxk = ((float)x + 0.5f) - key.x;
            const float dyk = ((float)yc + 0.5f) - key.y;
            const float dnx = fma_(crspt, dxk, srspt * dyk);
            const float dny = fma_(-srspt, dxk, crspt * dyk);
            const float ft = floor_(dnx + 2.5f), fv = floor_(dny + 2.5f);
            const float m = 0.5f * __builtin_amdgcn_sqrtf(m2);
            const float w = m * __builtin_amdgcn_exp2f(kexp * fma_(dnx, dnx, dny * dny));
            float theta = (anglef - rot) * rpi;
            if (theta < 0) theta += 8.0f;
            const bool take = valid && ft >= 0.0f && ft <= 4.0f && fv >= 0.0f && fv <= 4.0f &&
                              theta >= 0.0f && theta < 8.0f;
            // w >= 0 wherever it is finite; a NaN or Inf gradient makes it NaN or Inf.  Every
            // pixel of the step counts, inside the window or not (a comparison and a scalar OR):
            // a feature flagged for a pixel just outside its window gets the exact kernel's row.
            badw |= __ballot(!(w < __builtin_inff()));
            if (take) {
                const int a = (int)ft, b = (int)fv;
                const int c00 = b * 6 + a;                 // cell (a - 1, b - 1) in the 6 x 6 table
                const float4 t0 = ctab[c00], t1 = ctab[c00 + 1], t2 = ctab[c00 + 6], t3 = ctab[c00 + 7];
                const float w0 = (w * (t0.x - dnx)) * (t0.z - dny);
                const float w1 = (w * (t1.y + dnx)) * (t1.z - dny);
                const float w2 = (w * (t2.x - dnx)) * (t2.w + dny);
                const float w3 = (w * (t3.y + dnx)) * (t3.w + dny);
                // orientation bins: floor(theta) and the next (8 -> 0), tent weights as
                // descriptor_dual's max(0, 1 - |theta - k|)
                const int b0 = min((int)theta, 7), b1 = (b0 + 1) & 7;
                const float tk0 = 1.0f - (theta - (float)b0);
                const float tk1 = b0 == 7 ? theta - 7.0f : 1.0f - ((float)(b0 + 1) - theta);
                // the 4 cells (a - 1 + dx, b - 1 + dy); cells outside 0 .. 3 (the dual cells on the
                // window's border) are not descriptor cells and take nothing
                const bool x0in = a >= 1, x1in = a <= 3, y0in = b >= 1, y1in = b <= 3;
                lds_u64* hp = hist + (((b - 1) * 4 + (a - 1)) * 8) * kFlatStride + copy;
                const int o0 = b0 * kFlatStride, o1 = b1 * kFlatStride;
                constexpr int CX = 8 * kFlatStride, CY = 4 * 8 * kFlatStride;
                auto add2 = [&](bool in, int off, float wc) {
                    if (in) {
                        __hip_atomic_fetch_add(hp + off + o0, to_fix32(wc * tk0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_fetch_add(hp + off + o1, to_fix32(wc * tk1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                };
                add2(x0in && y0in, 0, w0);
                add2(x1in && y0in, CX, w1);
                add2(x0in && y1in, CY, w2);
                add2(x1in && y1in, CY + CX, w3);
            }
        }
        asm volatile("" ::: "memory");
    }
    if (lane == 63) *reinterpret_cast<uint32_t*>(sh + kFlatFlag) = badw != 0 ? 1u : 0u;
    asm volatile("" ::: "memory");
}

// The descriptor from nh histograms (kFlatWords floats apart from sh on): cell (ix, iy) =
// lane >> 2, bins 2 sub, 2 sub + 1, every copy of every histogram summed as 64-bit integers --
// the same totals however the window's pixels were split over waves and copies -- then
// normalised (NormalizeDescriptor, ProgramCU.cu:1173-1208) and stored as row `out`; a row of NaN
// where a histogram's flag says that the window held a weight that is not finite (kFlatFlag).
__device__ __forceinline__ void flat_finish(int lane, const FeatureParams& fp,
                                            float* __restrict__ desc, uint32_t out,
                                            const float* __restrict__ sh, int nh,
                                            float* __restrict__ hdesc = nullptr) {
    const int cell = lane >> 2, sub = lane & 3;
    const int ix = cell & 3, iy = cell >> 2;
    unsigned long long s0 = 0, s1 = 0;
    const int hi = ((iy * 4 + ix) * 8 + 2 * sub) * kFlatStride;
    uint32_t nonfinite = 0;
    for (int w = 0; w < nh; w++)
        nonfinite |= *reinterpret_cast<const uint32_t*>(sh + w * kFlatWords + kFlatFlag);
    // (uniform; u8, colour and -prep input is finite at every level and has no such launch)
    const bool redo = !fp.unit_input && __builtin_amdgcn_readfirstlane(nonfinite) != 0;
    for (int w = 0; w < nh; w++) {
        const lds_u64* hc = (const lds_u64*)(sh + w * kFlatWords) + hi;
#pragma unroll
        for (int k = 0; k < kFlatCopies; k++) {
            s0 += hc[k];
            s1 += hc[kFlatStride + k];
        }
    }
    const double scale = 0x1p-32;
    float b0 = (float)((double)(long long)s0 * scale), b1 = (float)((double)(long long)s1 * scale);
    asm volatile("" ::: "memory");
    if (redo) {
        b0 = b1 = __builtin_nanf("");
    } else if (fp.normalize) {
        float sn = wave_sum_dpp(fma_(b0, b0, b1 * b1));
        const float n1 = __builtin_amdgcn_rsqf(sn);
        b0 = fmin_(0.2f, b0 * n1);
        b1 = fmin_(0.2f, b1 * n1);
        sn = wave_sum_dpp(fma_(b0, b0, b1 * b1));
        const float n2 = __builtin_amdgcn_rsqf(sn);
        b0 *= n2;
        b1 *= n2;
    }
    *reinterpret_cast<float2*>(desc + (size_t)out * 128 + cell * 8 + sub * 2) = make_float2(b0, b1);
    if (hdesc)   // the row also to page-locked host memory (sgpu_set_host_output)
        *reinterpret_cast<float2*>(hdesc + (size_t)out * 128 + cell * 8 + sub * 2) = make_float2(b0, b1);
}

__device__ __forceinline__ void descriptor_flat(uint32_t e, int lane, const float* __restrict__ pyr,
                                                const float4* __restrict__ feat,
                                                const int2* __restrict__ feat_info,
                                                const FeatureParams& fp, float* __restrict__ desc,
                                                uint32_t out, float* __restrict__ sh) {
    flat_accumulate(e, lane, pyr, feat, feat_info, fp, sh, 0, 1);
    flat_finish(lane, fp, desc, out, sh, 1);
}

// waves per SIMD the allocation must allow: 8 (64 VGPRs, no spills): 1.448-1.451 ms per
// 128 x 1080p step against 1.520-1.524 at the compiler's 70 VGPRs / 7 waves (alternating
// processes, tests/diag/r05r.sh); 0 leaves it to the compiler
#if SGK_FLAT_WPE
#define SGK_FLAT_ATTR __attribute__((amdgpu_waves_per_eu(SGK_FLAT_WPE)))
#else
#define SGK_FLAT_ATTR
#endif
__global__ __launch_bounds__(256) SGK_FLAT_ATTR void k_descriptor_flat(const float* __restrict__ pyr,
                                                         const float4* __restrict__ feat,
                                                         const int2* __restrict__ feat_info,
                                                         const uint32_t* __restrict__ n_feat_dev,
                                                         const FeatureParams fp,
                                                         float* __restrict__ desc,
                                                         const int* __restrict__ out_index) {
    __shared__ __attribute__((aligned(16))) float s_flat[4][kFlatWords];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t n = *n_feat_dev;
    for (uint32_t e = blockIdx.x * 4 + wave; e < n; e += gridDim.x * 4)
        descriptor_flat(e, lane, pyr, feat, feat_info, fp, desc,
                        out_index ? (uint32_t)out_index[e] : e, s_flat[wave]);
}

// k_descriptor_flat as resident workgroups of NW waves (1; 2 where a compute unit holds more
// waves that way) fed from work counters: the grid is what the device holds at
// once, and each wave takes one feature at a time until *n_feat_dev are done, into a histogram
// of its own, so its slot is refilled as soon as its own feature is finished.  Feature e is
// computed by the same code and written to the same row as above.  The counters are zero at the
// launch; surplus waves find nothing to do and exit (no wave waits for another).
template <int NW>
__global__ __launch_bounds__(64 * NW) SGK_FLAT_ATTR void k_descriptor_queue(
    const float* __restrict__ pyr, const float4* __restrict__ feat,
    const int2* __restrict__ feat_info, const uint32_t* __restrict__ n_feat_dev,
    const FeatureParams fp, float* __restrict__ desc, const int* __restrict__ out_index,
    uint32_t* __restrict__ next) {
    __shared__ __attribute__((aligned(16))) float s_flat[NW][kFlatWords];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = NW == 1 ? 0u : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* sh = s_flat[wave];
    const uint32_t n = *n_feat_dev;
    const uint32_t wv = blockIdx.x * NW + wave, nwaves = gridDim.x * NW;
    for (uint32_t e = wv; e < n;) {   // descriptor_flat(e), and:
        flat_accumulate(e, lane, pyr, feat, feat_info, fp, sh, 0, 1);
        const uint32_t out = out_index ? (uint32_t)out_index[e] : e;
        // the next feature asked for once this one's window is read: the counter's round trip
        // (memory-side, microseconds) runs beside the histogram's summing and normalisation,
        // which load nothing
        const uint32_t ticket = queue_ask(next, wv);
        flat_finish(lane, fp, desc, out, sh, 1);
        e = queue_unit(ticket, wv, nwaves);
    }
}

// A workgroup of NWV (4) waves per feature, for few features (one image: ~1,500 features are ~1.5
// waves per SIMD under one wave each, and each wave walks its window alone).  The waves take every
// NWV-th 64-pixel step of the window into histograms of their own; wave 0 sums all of them.  The
// sums are integers, so the descriptor is k_descriptor_flat's bit for bit, in any batch.
template <int NWV>
__global__ __launch_bounds__(64 * NWV) SGK_FLAT_ATTR void k_descriptor_wide(const float* __restrict__ pyr,
                                                         const float4* __restrict__ feat,
                                                         const int2* __restrict__ feat_info,
                                                         const uint32_t* __restrict__ n_feat_dev,
                                                         const FeatureParams fp,
                                                         float* __restrict__ desc,
                                                         const int* __restrict__ out_index,
                                                         const HostCopy hc) {
    __shared__ __attribute__((aligned(16))) float s_flat[NWV][kFlatWords];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t n = *n_feat_dev;
    // host output (one image, sgpu_set_host_output): the count record, the first cap keys and
    // descriptors also go to page-locked host memory from here -- written over the host link
    // while the descriptors are computed, instead of by a k_copy_out launch after them
    if (hc.hrec && blockIdx.x == 0 && threadIdx.x < (unsigned)hc.rec_n) hc.hrec[threadIdx.x] = hc.rec[threadIdx.x];
    for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {   // uniform per workgroup
        flat_accumulate(e, lane, pyr, feat, feat_info, fp, s_flat[wave], wave, NWV);
        __syncthreads();
        const uint32_t out = out_index ? (uint32_t)out_index[e] : e;
        const bool to_host = hc.hkeys && out < hc.cap;
        if (wave == 0)
            flat_finish(lane, fp, desc, out, &s_flat[0][0], NWV, to_host ? hc.hdesc : nullptr);
        else if (wave == 1 && lane == 0 && to_host)
            hc.hkeys[out] = hc.keys[e];
        __syncthreads();   // wave 0 has read every histogram before the next feature zeroes them
    }
}

// The rows that k_descriptor_flat / _queue / _wide stored as NaN (a window sample's weight was
// not finite, kFlatFlag) from the exact kernel's descriptor_one, which propagates NaN and Inf as
// the reference does; launched after them.  A wave reads the first float of every 4 g-th row
// and finds none to do on finite input.  hdesc: k_descriptor_wide's host rows (the first hcap).
__global__ __launch_bounds__(256) void k_descriptor_nonfinite(const float* __restrict__ pyr,
                                                              const float4* __restrict__ feat,
                                                              const int2* __restrict__ feat_info,
                                                              const uint32_t* __restrict__ n_feat_dev,
                                                              const FeatureParams fp,
                                                              float* __restrict__ desc,
                                                              const int* __restrict__ out_index,
                                                              float* __restrict__ hdesc, uint32_t hcap) {
    const int lane = threadIdx.x & 63;
    const uint32_t n = *n_feat_dev;
    for (uint32_t e = blockIdx.x * 4 + (threadIdx.x >> 6); e < n; e += gridDim.x * 4) {   // uniform per wave
        const uint32_t out = out_index ? (uint32_t)out_index[e] : e;
        const float first = desc[(size_t)out * 128];
        if (first == first) continue;
        descriptor_one<false>(e, lane, pyr, feat, feat_info, fp, desc, out,
                              hdesc && out < hcap ? hdesc : nullptr);
    }
}

// One wave per feature, grid-stride over the features (count read on the device).
// SGK_DESC_WPE: waves per SIMD the register allocation must allow (0: the compiler's choice, 91
// VGPRs = 5 waves; A/B knob)
#if SGK_DESC_WPE
#define SGK_DESC_ATTR __attribute__((amdgpu_waves_per_eu(SGK_DESC_WPE)))
#else
#define SGK_DESC_ATTR
#endif
template <bool RECT>
__global__ __launch_bounds__(256) SGK_DESC_ATTR void k_descriptor_fast(const float* __restrict__ pyr,
                                                         const float4* __restrict__ feat,
                                                         const int2* __restrict__ feat_info,
                                                         const uint32_t* __restrict__ n_feat_dev,
                                                         const FeatureParams fp,
                                                         float* __restrict__ desc,
                                                         const int* __restrict__ out_index) {
    const int lane = threadIdx.x & 63;
    const uint32_t n = *n_feat_dev;
    // the feature index is wave-uniform: say so, so that the feature's record, level pointer and
    // geometry live in SGPRs and the gathers use the SGPR-base + 32-bit-offset form
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint32_t e = blockIdx.x * 4 + wave; e < n; e += gridDim.x * 4)
        descriptor_fast<RECT>(e, lane, pyr, feat, feat_info, fp, desc,
                              out_index ? (uint32_t)out_index[e] : e);
}

// One wave per feature, grid-stride over the features (count read on the device).
template <bool RECT>
__global__ __launch_bounds__(256) void k_descriptor(const float* __restrict__ pyr,
                                                    const float4* __restrict__ feat,
                                                    const int2* __restrict__ feat_info,
                                                    const uint32_t* __restrict__ n_feat_dev,
                                                    const FeatureParams fp,
                                                    float* __restrict__ desc,
                                                    const int* __restrict__ out_index) {
    const int lane = threadIdx.x & 63;
    const uint32_t n = *n_feat_dev;
    for (uint32_t e = blockIdx.x * 4 + (threadIdx.x >> 6); e < n; e += gridDim.x * 4)   // uniform per wave
        descriptor_one<RECT>(e, lane, pyr, feat, feat_info, fp, desc,
                             out_index ? (uint32_t)out_index[e] : e);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// One image's keys and descriptors (up to cap features) and its count record straight into
// page-locked host memory (sgpu_set_host_output): one launch in the extract's stream in place of
// the record's copy and the two downloads of sgpu_copy_features -- on one 1080p image each of
// those copies costs ~20 us of DMA start-up and host round trip beside 5 + 19 us of transfer
// (tests/diag/c2_ab.sh timeline).  16-B stores; the host reads them after the stream's
// synchronisation.
__global__ __launch_bounds__(256) void k_copy_out(const float4* __restrict__ keys,
                                                  const float4* __restrict__ desc,
                                                  const uint32_t* __restrict__ n_dev, uint32_t cap,
                                                  const int64_t* __restrict__ rec, int rec_n,
                                                  float4* __restrict__ hkeys, float4* __restrict__ hdesc,
                                                  int64_t* __restrict__ hrec) {
    const uint32_t n = min(*n_dev, cap);
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    if (t0 < (size_t)rec_n) hrec[t0] = rec[t0];
    for (size_t i = t0; i < n; i += step) hkeys[i] = keys[i];
    if (hdesc)
        for (size_t i = t0; i < (size_t)n * 32; i += step) hdesc[i] = desc[i];
}

hipError_t launch_copy_out(const float4* keys, const float* desc, const uint32_t* n_dev, int cap,
                           const int64_t* rec, int rec_n, float* hkeys, float* hdesc,
                           int64_t* hrec, hipStream_t stream) {
    if (cap < 0 || rec_n < 0 || rec_n > 256 || !hkeys || !hrec) return hipErrorInvalidValue;
    const long long work = std::max<long long>(1, (long long)cap * (hdesc ? 32 : 1));
    const unsigned nb = (unsigned)std::min<long long>(256, std::max<long long>(1, (work + 1023) / 1024));
    hipLaunchKernelGGL(k_copy_out, dim3(nb), dim3(256), 0, stream, keys,
                       reinterpret_cast<const float4*>(desc), n_dev, (uint32_t)cap, rec, rec_n,
                       reinterpret_cast<float4*>(hkeys), reinterpret_cast<float4*>(hdesc), hrec);
    return hipGetLastError();
}

hipError_t descriptor_queue_occupancy(int* blocks_one_wave, int* blocks_two_waves) {
    const hipError_t e =
        hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_one_wave, k_descriptor_queue<1>, 64, 0);
    if (e != hipSuccess) return e;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_two_waves, k_descriptor_queue<2>, 128, 0);
}

hipError_t launch_descriptor(const float* pyr, const float4* feat, const int2* feat_info,
                             const uint32_t* n_feat_dev, int n_feat_cap, const FeatureParams& fp,
                             float* desc, const DescriptorForm& form, hipStream_t stream) {
    const int* out_index = form.out_index;
    const bool rect = form.rect, exact = form.exact, dual = form.dual, wide = form.wide;
    const HostCopy* host = form.host;
    const FeatureQueue* queue = form.queue;
    if (n_feat_cap <= 0) return hipSuccess;
    if (host && (!wide || exact || rect || dual || host->rec_n < 0 || host->rec_n > 256 ||
                 !host->hkeys || !host->hrec || !host->keys || !host->rec))
        return hipErrorInvalidValue;   // only the workgroup-per-feature kernel writes the host
    const unsigned grid = (unsigned)std::min(((long long)n_feat_cap + 3) / 4, 65536LL);
    // after the integer-sum kernels: their NaN rows (kFlatFlag) from descriptor_one
    auto redo_nonfinite = [&](float* hdesc, uint32_t hcap) {
        if (hipError_t err = hipGetLastError()) return err;
        if (fp.unit_input) return hipSuccess;   // pixels in [0, 1]: every level is finite
        hipLaunchKernelGGL(k_descriptor_nonfinite, dim3(std::min(grid, 1024u)), dim3(256), 0, stream,
                           pyr, feat, feat_info, n_feat_dev, fp, desc, out_index, hdesc, hcap);
        return hipGetLastError();
    };
    if (!exact && !rect && !dual && wide) {
        // A/B knobs: SGPU_WIDE_DESC_WAVES (4 or 8 waves per feature), SGPU_WIDE_DESC_GRID (at most
        // this many workgroups, each taking every grid-th feature)
        static const int nwv = [] {
            const char* e = getenv("SGPU_WIDE_DESC_WAVES");
            return e && atoi(e) == 8 ? 8 : 4;
        }();
        static const long long gmax = [] {
            const char* e = getenv("SGPU_WIDE_DESC_GRID");
            return e && atoll(e) > 0 ? atoll(e) : 65536LL;
        }();
        const unsigned wgrid = (unsigned)std::min((long long)n_feat_cap, gmax);
        const HostCopy hc = host ? *host : HostCopy{};
        if (nwv == 8)
            hipLaunchKernelGGL(k_descriptor_wide<8>, dim3(wgrid), dim3(512), 0, stream, pyr, feat,
                               feat_info, n_feat_dev, fp, desc, out_index, hc);
        else
            hipLaunchKernelGGL(k_descriptor_wide<4>, dim3(wgrid), dim3(256), 0, stream, pyr, feat,
                               feat_info, n_feat_dev, fp, desc, out_index, hc);
        return redo_nonfinite(hc.hkeys ? hc.hdesc : nullptr, hc.cap);
    }
    if (!exact && !rect && !dual && queue) {
        const int nw = queue->desc_waves;
        if (!queue->next || queue->desc_grid <= 0 || (nw != 1 && nw != 2)) return hipErrorInvalidValue;
        // the descriptor's counters follow the orientation's; the grid as in launch_orientation
        uint32_t* qa = queue->next + kQueueCounters * kQueueStride;
        const long long wgs = ((long long)n_feat_cap + nw - 1) / nw;
        const unsigned qgrid = (unsigned)std::max<long long>(kQueueCounters, std::min<long long>(wgs, queue->desc_grid));
        if (nw == 2)
            hipLaunchKernelGGL(k_descriptor_queue<2>, dim3(qgrid), dim3(128), 0, stream, pyr, feat,
                               feat_info, n_feat_dev, fp, desc, out_index, qa);
        else
            hipLaunchKernelGGL(k_descriptor_queue<1>, dim3(qgrid), dim3(64), 0, stream, pyr, feat,
                               feat_info, n_feat_dev, fp, desc, out_index, qa);
        return redo_nonfinite(nullptr, 0);
    }
    if (!exact && !rect && !dual) {
        hipLaunchKernelGGL(k_descriptor_flat, dim3(grid), dim3(256), 0, stream, pyr, feat,
                           feat_info, n_feat_dev, fp, desc, out_index);
        return redo_nonfinite(nullptr, 0);
    }
    if (!exact && !rect) {
        hipLaunchKernelGGL(k_descriptor_dual, dim3(grid), dim3(256), 0, stream, pyr, feat,
                           feat_info, n_feat_dev, fp, desc, out_index);
        return hipGetLastError();
    }
    if (!exact) {
        if (rect)
            hipLaunchKernelGGL(k_descriptor_fast<true>, dim3(grid), dim3(256), 0, stream, pyr,
                               feat, feat_info, n_feat_dev, fp, desc, out_index);
        else
            hipLaunchKernelGGL(k_descriptor_fast<false>, dim3(grid), dim3(256), 0, stream, pyr,
                               feat, feat_info, n_feat_dev, fp, desc, out_index);
        return hipGetLastError();
    }
    if (rect)
        hipLaunchKernelGGL(k_descriptor<true>, dim3(grid), dim3(256), 0, stream, pyr, feat,
                           feat_info, n_feat_dev, fp, desc, out_index);
    else
        hipLaunchKernelGGL(k_descriptor<false>, dim3(grid), dim3(256), 0, stream, pyr, feat,
                           feat_info, n_feat_dev, fp, desc, out_index);
    return hipGetLastError();
}

}  // namespace sgk
