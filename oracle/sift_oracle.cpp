// sift_oracle.cpp -- CPU restatement of the SiftGPU CUDA hot path.
//
// TEST INFRASTRUCTURE ONLY (see sift_oracle.h).  Written to follow the reference line by line,
// in its own data layout (a float4 key image, the histogram pyramid, per-level lists), so that a
// mistake in the HIP kernels' different structure shows up as a mismatch.
//
// Floating-point conventions (shared with the HIP kernels): nvcc contracts
// a*b+c into FMA; we fix one contraction per expression and write it out with fma_():
//   acc += a*b          -> fma(a, b, acc)          acc -= a*b  -> fma(-a, b, acc)
//   a*a + b*b           -> fma(a, a, b*b)          a*b - c*d   -> fma(a, b, -(c*d))
// Everything else is evaluated without contraction (-ffp-contract=off on both sides).
// Transcendentals come from sift_math.h (deterministic, shared with the kernels).
#include "sift_oracle.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <stdexcept>

#include "../modify-sift-gpu_amd/csrc/sift_math.h"

using namespace sgm;

namespace oracle {
namespace {

// --- ingest: GLTexInput::SetImageData + DownSamplePixelDataI2F<u8> (GLTexImage.cpp:918-1009,
//     808-831): width truncated to a multiple of 4, value p / 255.0f.
Image ingest(const uint8_t* img, int w, int h, int stride) {
    Image o;
    o.w = w & ~3;
    o.h = h;
    o.px.resize((size_t)o.w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < o.w; x++) o.px[(size_t)y * o.w + x] = img[(size_t)y * stride + x] / 255.0f;
    return o;
}

// --- float luminance input: the same truncated width, values as given.
Image ingest_f32(const float* img, int w, int h, int stride) {
    Image o;
    o.w = w & ~3;
    o.h = h;
    o.px.resize((size_t)o.w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < o.w; x++) o.px[(size_t)y * o.w + x] = img[(size_t)y * stride + x];
    return o;
}

// --- FilterH<FW> + FilterV<FW> (ProgramCU.cu:115-222, driven by FilterImage :406-446):
//     horizontal pass clamps within the row, vertical pass clamps to rows 0..H-1; each output
//     sums taps i = 0..FW-1 in order (value += data[..]*k[i] -> fma).
Image filter(const Image& src, const float* k, int fw) {
    const int W = src.w, H = src.h, half = fw >> 1;
    Image tmp, dst;
    tmp.w = dst.w = W;
    tmp.h = dst.h = H;
    tmp.px.resize(src.px.size());
    dst.px.resize(src.px.size());
    for (int y = 0; y < H; y++) {
        const float* row = &src.px[(size_t)y * W];
        for (int x = 0; x < W; x++) {
            float v = 0.0f;
            for (int i = 0; i < fw; i++) {
                int xx = std::min(std::max(x - half + i, 0), W - 1);
                v = fma_(row[xx], k[i], v);
            }
            tmp.px[(size_t)y * W + x] = v;
        }
    }
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            float v = 0.0f;
            for (int i = 0; i < fw; i++) {
                int yy = std::min(std::max(y - half + i, 0), H - 1);
                v = fma_(tmp.px[(size_t)yy * W + x], k[i], v);
            }
            dst.px[(size_t)y * W + x] = v;
        }
    return dst;
}

// --- DownsampleKernel<1> (ProgramCU.cu:287-298): dst(r,c) = src(2r, min(2c, Wsrc-1)).
Image downsample(const Image& src, int wdst, int hdst) {
    Image d;
    d.w = wdst;
    d.h = hdst;
    d.px.resize((size_t)wdst * hdst);
    for (int r = 0; r < hdst; r++)
        for (int c = 0; c < wdst; c++)
            d.px[(size_t)r * wdst + c] = src.at(std::min(c << 1, src.w - 1), r << 1);
    return d;
}

// --- SampleImageD (ProgramCU.cu:300-328) from the input for -fo > 0: dst(r, c) =
//     src(r << s, min(c << s, Wsrc - 1)) into the first octave's wa x h.
Image downsample_input(const Image& src, int s, int wdst, int hdst) {
    Image d;
    d.w = wdst;
    d.h = hdst;
    d.px.resize((size_t)wdst * hdst);
    for (int r = 0; r < hdst; r++)
        for (int c = 0; c < wdst; c++)
            d.px[(size_t)r * wdst + c] = src.at(std::min(c << s, src.w - 1), r << s);
    return d;
}

// --- UpsampleKernel<s> (ProgramCU.cu:225-285) for -fo < 0, on the input as the flat W x H
//     buffer it is bound as (tex1Dfetch: index + 1 at the end of a row is the next row's first
//     pixel, indices past the buffer read 0).  Output row R, source row R >> s, blend weight
//     w1 = (R & (S-1)) / S; every source column c writes S consecutive outputs at (W R + c) S.
//     Contractions as elsewhere: a*b + c*d -> fma(a, b, c*d).
Image upsample_input(const Image& src, int s) {
    const int S = 1 << s, W = src.w, H = src.h;
    const float inv = 1.0f / float(S);
    Image d;
    d.w = W * S;
    d.h = H * S;
    d.px.resize((size_t)d.w * d.h);
    auto in = [&](long k) { return k < (long)src.px.size() ? src.px[(size_t)k] : 0.0f; };
    for (int R = 0; R < d.h; R++) {
        const int row = R >> s, helper = R & (S - 1);
        for (int c = 0; c < W; c++) {
            const long index = (long)row * W + c;
            float v1, v2;
            if (helper) {
                const float v11 = in(index), v12 = in(index + 1);
                const float v21 = in(index + W), v22 = in(index + W + 1);
                const float w1 = inv * helper, w2 = (float)(1.0 - (double)w1);
                v1 = fma_(v21, w1, w2 * v11);
                v2 = fma_(v22, w1, w2 * v12);
            } else {
                v1 = in(index);
                v2 = in(index + 1);
            }
            float* o = &d.px[((size_t)W * R + c) * S];
            o[0] = v1;
            for (int i = 1; i < S; i++) {
                const float r2 = i * inv, r1 = 1.0f - r2;
                o[i] = fma_(v1, r1, v2 * r2);
            }
        }
    }
    return d;
}

// tex1Dfetch on linear memory: indices outside the bound allocation return 0 (CuTexImage
// allocations are exactly wa*h floats for reused-size pyramids).
inline float fetch(const Image& im, long idx) {
    if (idx < 0 || idx >= (long)im.px.size()) return 0.0f;
    return im.px[(size_t)idx];
}

// --- ComputeDOG_Kernel (ProgramCU.cu:485-517): dog = G[m] - G[m-1]; gradient of G[m] from
//     flat-index neighbours (row wrap at the left/right edge, 0 beyond the buffer).
void compute_dog(const Image& g, const Image& gp, Image* dog, std::vector<float>* grad) {
    const int W = g.w, H = g.h;
    dog->w = W;
    dog->h = H;
    dog->px.resize(g.px.size());
    if (grad) grad->resize(g.px.size() * 2);
    for (int r = 0; r < H; r++)
        for (int c = 0; c < W; c++) {
            long idx = (long)r * W + c;
            float vp = gp.px[idx], v = g.px[idx];
            dog->px[idx] = v - vp;
            if (!grad) continue;
            float vxn = fetch(g, idx + 1), vxp = fetch(g, idx - 1);
            float vyp = fetch(g, idx - W), vyn = fetch(g, idx + W);
            float dx = vxn - vxp, dy = vyn - vyp;
            float grd = 0.5f * sqrt_(fma_(dx, dx, dy * dy));
            float rot = (grd == 0.0f ? 0.0f : atan2_(dy, dx));
            (*grad)[idx * 2] = grd;
            (*grad)[idx * 2 + 1] = rot;
        }
}

struct Key4 { float x, y, z, w; };

// ORACLE_TIE_VARIANT (compile time; 0 = the reference's rules, what liboracle.so is built with):
// one tie rule flipped, for tests/test_structured_images.py, which shows that the structured
// images reach each rule (oracle/Makefile: liboracle_tie%.so).
//   1  READ_CMP_DOG_DATA's exits take equality (v <= nmax, v >= nmin)
//   2  the two-peak selection replaces on an equal weight (>=)
//   3  a peak may equal the bin before it (>=)
//   4  the one-orientation maximum moves to a later equal bin (>=)
//   6  the first test against the row neighbours is strict (<, >)
//   7  RowMatch_Kernel's equal maxima go to the lowest column mod 32 (not the reduction's order)
#ifndef ORACLE_TIE_VARIANT
#define ORACLE_TIE_VARIANT 0
#endif
constexpr int kTie = ORACLE_TIE_VARIANT;
static_assert(kTie == 0 || kTie == 1 || kTie == 2 || kTie == 3 || kTie == 4 || kTie == 6 ||
                  kTie == 7,
              "ORACLE_TIE_VARIANT");

// --- ComputeKEY_Kernel (ProgramCU.cu:553-671) with READ_CMP_DOG_DATA (:534-550).
//     Interior pixels only (row, col in [1, dim-2]); the comparison order and the early exits
//     are kept, because ties are resolved by that order.
void compute_key(const Image& dp, const Image& dc, const Image& dn, float t0, float t,
                 float edge, int subpixel, std::vector<Key4>* key) {
    const int W = dc.w, H = dc.h;
    key->assign((size_t)W * H, Key4{0, 0, 0, 0});
    for (int row = 1; row < H - 1; row++)
        for (int col = 1; col < W - 1; col++) {
            const long index = (long)row * W + col;
            const long idx[3] = {index - W, index, index + W};
            float data[3][3], datap[3][3], datan[3][3];
            float v, nmax, nmin, result = 0.0f, dx = 0, dy = 0, ds = 0;
            bool offset_ok = true;
            // READ_CMP_DOG_DATA as a lambda returning false on "goto key_finish"
            auto read_cmp = [&](float* d3, const Image& im, long i) {
                d3[0] = im.px[i - 1];
                d3[1] = im.px[i];
                d3[2] = im.px[i + 1];
                if (v > nmax) {
                    nmax = fmax_(nmax, d3[0]);
                    nmax = fmax_(nmax, d3[1]);
                    nmax = fmax_(nmax, d3[2]);
                    if (kTie == 1 ? v <= nmax : v < nmax) return false;
                } else {
                    nmin = fmin_(nmin, d3[0]);
                    nmin = fmin_(nmin, d3[1]);
                    nmin = fmin_(nmin, d3[2]);
                    if (kTie == 1 ? v >= nmin : v > nmin) return false;
                }
                return true;
            };
            data[1][1] = v = dc.px[idx[1]];
            if (fabs_(v) <= t0) goto finish;
            data[1][0] = dc.px[idx[1] - 1];
            data[1][2] = dc.px[idx[1] + 1];
            nmax = fmax_(data[1][0], data[1][2]);
            nmin = fmin_(data[1][0], data[1][2]);
            if (kTie == 6 ? (v < nmax && v > nmin) : (v <= nmax && v >= nmin)) goto finish;
            if (!read_cmp(data[0], dc, idx[0])) goto finish;
            if (!read_cmp(data[2], dc, idx[2])) goto finish;
            {
                float vx2 = v * 2.0f;
                float fxx = data[1][0] + data[1][2] - vx2;
                float fyy = data[0][1] + data[2][1] - vx2;
                float fxy = 0.25f * (data[2][2] + data[0][0] - data[2][0] - data[0][2]);
                float temp1 = fma_(fxx, fyy, -(fxy * fxy));
                float temp2 = (fxx + fyy) * (fxx + fyy);
                if (temp1 <= 0 || temp2 > edge * temp1) goto finish;
            }
            if (!read_cmp(datap[0], dp, idx[0])) goto finish;
            if (!read_cmp(datap[1], dp, idx[1])) goto finish;
            if (!read_cmp(datap[2], dp, idx[2])) goto finish;
            if (!read_cmp(datan[0], dn, idx[0])) goto finish;
            if (!read_cmp(datan[1], dn, idx[1])) goto finish;
            if (!read_cmp(datan[2], dn, idx[2])) goto finish;
            if (subpixel) {
                float vx2 = v * 2.0f;
                float fxx = data[1][0] + data[1][2] - vx2;
                float fyy = data[0][1] + data[2][1] - vx2;
                float fxy = 0.25f * (data[2][2] + data[0][0] - data[2][0] - data[0][2]);
                float fx = 0.5f * (data[1][2] - data[1][0]);
                float fy = 0.5f * (data[2][1] - data[0][1]);
                float fs = 0.5f * (datan[1][1] - datap[1][1]);
                float fss = (datan[1][1] + datap[1][1] - vx2);
                float fxs = 0.25f * (datan[1][2] + datap[1][0] - datan[1][0] - datap[1][2]);
                float fys = 0.25f * (datan[2][1] + datap[0][1] - datan[0][1] - datap[2][1]);
                // rows (a, b, c, rhs) with the sign flip of ProgramCU.cu:629-631
                float A0[4], A1[4], A2[4];
                auto setrow = [](float* A, float a, float b, float c, float r) {
                    if (a > 0) { A[0] = a; A[1] = b; A[2] = c; A[3] = -r; }
                    else { A[0] = -a; A[1] = -b; A[2] = -c; A[3] = r; }
                };
                setrow(A0, fxx, fxy, fxs, fx);
                setrow(A1, fxy, fyy, fys, fy);
                setrow(A2, fxs, fys, fss, fs);
                float maxa = fmax_(fmax_(A0[0], A1[0]), A2[0]);
                if (maxa >= 1e-10) {
                    if (maxa == A1[0]) { for (int q = 0; q < 4; q++) std::swap(A0[q], A1[q]); }
                    else if (maxa == A2[0]) { for (int q = 0; q < 4; q++) std::swap(A0[q], A2[q]); }
                    A0[1] /= A0[0]; A0[2] /= A0[0]; A0[3] /= A0[0];
                    A1[1] = fma_(-A1[0], A0[1], A1[1]);
                    A1[2] = fma_(-A1[0], A0[2], A1[2]);
                    A1[3] = fma_(-A1[0], A0[3], A1[3]);
                    A2[1] = fma_(-A2[0], A0[1], A2[1]);
                    A2[2] = fma_(-A2[0], A0[2], A2[2]);
                    A2[3] = fma_(-A2[0], A0[3], A2[3]);
                    if (fabs_(A2[1]) > fabs_(A1[1])) { for (int q = 0; q < 4; q++) std::swap(A1[q], A2[q]); }
                    if (fabs_(A1[1]) >= 1e-10) {
                        A1[2] /= A1[1]; A1[3] /= A1[1];
                        A2[2] = fma_(-A2[1], A1[2], A2[2]);
                        A2[3] = fma_(-A2[1], A1[3], A2[3]);
                        if (fabs_(A2[2]) >= 1e-10) {
                            ds = A2[3] / A2[2];
                            dy = fma_(-ds, A1[2], A1[3]);
                            dx = fma_(-dy, A0[1], fma_(-ds, A0[2], A0[3]));
                            float dot = fma_(ds, fs, fma_(dx, fx, dy * fy));
                            offset_ok = fabs_(fma_(0.5f, dot, data[1][1])) > t &&
                                        fabs_(ds) < 1.0f && fabs_(dx) < 1.0f && fabs_(dy) < 1.0f;
                        }
                    }
                }
            }
            if (offset_ok) result = v > nmax ? 1.0f : -1.0f;
        finish:
            (*key)[index] = Key4{result, dx, dy, ds};
        }
}

// --- histogram pyramid list generation, literal: InitHist_Kernel (ProgramCU.cu:698-721),
//     ReduceHist_Kernel (:739-757), FitHistogramPyramid (PyramidCU.cpp:1175-1193), the CPU seed
//     list (PyramidCU.cpp:781-811) and ListGen_Kernel (ProgramCU.cu:775-798).
std::vector<Candidate> histo_list(const std::vector<Key4>& key, int W, int H, int hp_levels) {
    struct I4 { int v[4]; };
    // level widths, finest (w = (W+2)>>2) first
    std::vector<int> widths;
    int w = (W + 2) >> 2;
    for (int k = 0; k < hp_levels; k++) {
        widths.push_back(w);
        if (w == 1) break;
        w = (w + 3) >> 2;
    }
    std::vector<std::vector<I4>> hist(widths.size());
    hist[0].resize((size_t)widths[0] * H);
    for (int row = 0; row < H; row++)
        for (int col = 0; col < widths[0]; col++) {
            I4 o{{0, 0, 0, 0}};
            if (row > 0 && row < H - 1)
                for (int i = 0; i < 4; i++) {
                    int scol = (col << 2) + i;
                    long sidx = (long)row * W + scol;
                    // texture fetch beyond the key buffer returns 0 (scol < W always here)
                    float kx = (scol < W) ? key[sidx].x : 0.0f;
                    o.v[i] = (scol < W - 1 && scol > 0 && kx != 0) ? 1 : 0;
                }
            hist[0][(size_t)row * widths[0] + col] = o;
        }
    for (size_t l = 1; l < widths.size(); l++) {
        int ws = widths[l - 1], wd = widths[l];
        hist[l].resize((size_t)wd * H);
        for (int row = 0; row < H; row++)
            for (int col = 0; col < wd; col++) {
                I4 o{{0, 0, 0, 0}};
                int scol = col << 2;
                for (int i = 0; i < 4 && scol < ws; ++i, ++scol) {
                    const I4& t = hist[l - 1][(size_t)row * ws + scol];
                    o.v[i] = t.v[0] + t.v[1] + t.v[2] + t.v[3];
                }
                hist[l][(size_t)row * wd + col] = o;
            }
    }
    // top level must be one int4 per row (PyramidCU.cpp:781 reads height*4 ints)
    const std::vector<I4>& top = hist.back();
    struct P { int x, y, z; };
    std::vector<P> list;
    for (int ii = 0; ii < H * 4; ++ii) {
        int cnt = top[ii / 4].v[ii % 4];
        if (!(cnt >= 0)) cnt = 0;
        for (int jj = 0; jj < cnt; ++jj) list.push_back(P{ii % 4, ii / 4, jj});
    }
    // descend: GenerateList against levels top-1 .. 0
    for (int l = (int)widths.size() - 2; l >= 0; --l) {
        int wl = widths[l];
        for (P& p : list) {
            const I4& t = hist[l][(size_t)p.y * wl + p.x];
            int sum1 = t.v[0] + t.v[1], sum2 = sum1 + t.v[2];
            p.x <<= 2;
            if (p.z >= sum2) { p.x += 3; p.z -= sum2; }
            else if (p.z >= sum1) { p.x += 2; p.z -= sum1; }
            else if (p.z >= t.v[0]) { p.x += 1; p.z -= t.v[0]; }
        }
    }
    std::vector<Candidate> out;
    out.reserve(list.size());
    for (const P& p : list) {
        const Key4& k = key[(size_t)p.y * W + p.x];
        out.push_back(Candidate{p.x, p.y, k.y, k.z, k.w});
    }
    return out;
}

inline uint32_t f2u(float f) { return as_uint(f); }

// float -> int as the GPU converts (cvt.rzi.s32.f32): NaN gives 0 (C++ leaves it undefined).
// Only a NaN pyramid (-fo -2, see extract) reaches it with NaN.
inline int cvt_rz(float f) { return f != f ? 0 : (int)f; }
inline float u2f(uint32_t u) { return as_float(u); }

// --- ComputeOrientation_Kernel (ProgramCU.cu:813-977) for one list entry.  grad is the
//     float2 gradient image of G[1+j] (texture point sampling at x = k + 0.5 -> texel k).
void orientation_key(Key4 key, const std::vector<float>& grad, int W, int H,
                     float gaussian_factor, float sample_factor, int num_orientation,
                     int existing, int circular, float* out);

void orientation(const Candidate& c, const std::vector<float>& grad, int W, int H, float sigma,
                 float sigma_step, float gaussian_factor, float sample_factor,
                 int num_orientation, int subpixel, int keepsign, int circular, float* out) {
    Key4 key;
    key.x = c.col + 0.5f;
    key.y = c.row + 0.5f;
    key.z = sigma;
    key.w = 0;
    if (subpixel) {
        key.x += c.dx;
        key.y += c.dy;
        key.z *= pow_(sigma_step, c.ds);
    }
    (void)keepsign;  // -sign multiplies by the extremum sign; handled by the caller
    orientation_key(key, grad, W, H, gaussian_factor, sample_factor, num_orientation, 0,
                    circular, out);
}

// The kernel body after the key is formed.  existing != 0: a caller-supplied keypoint list
// (texDataF4 input, ProgramCU.cu:830-833), which keeps only the strongest orientation
// (ProgramCU.cu:904: num_orientation == 1 || existing_keypoint).
void orientation_key(Key4 key, const std::vector<float>& grad, int W, int H,
                     float gaussian_factor, float sample_factor, int num_orientation,
                     int existing, int circular, float* out) {
    const float ten_degree_per_radius = (float)5.7295779513082320876798154814105;
    const float radius_per_ten_degrees = (float)(1.0 / 5.7295779513082320876798154814105);
    if (num_orientation == 0) {
        out[0] = key.x; out[1] = key.y; out[2] = key.z; out[3] = 0.0f;
        return;
    }
    float vote[37];
    float gsigma = key.z * gaussian_factor;
    float win = fabs_(key.z) * sample_factor;
    float dist_threshold = (float)(win * win + 0.5);
    float factor = -0.5f / (gsigma * gsigma);
    float xmin = fmax_(1.5f, floor_(key.x - win) + 0.5f);
    float ymin = fmax_(1.5f, floor_(key.y - win) + 0.5f);
    float xmax = fmin_(W - 1.5f, floor_(key.x + win) + 0.5f);
    float ymax = fmin_(H - 1.5f, floor_(key.y + win) + 0.5f);
    for (int i = 0; i < 36; ++i) vote[i] = 0.0f;
    for (float y = ymin; y <= ymax; y += 1.0f)
        for (float x = xmin; x <= xmax; x += 1.0f) {
            float dx = x - key.x, dy = y - key.y;
            float sq_dist = fma_(dx, dx, dy * dy);
            if (circular && sq_dist >= dist_threshold) continue;   // ProgramCU-0.cu:834
            size_t t = ((size_t)(int)y * W + (int)x) * 2;
            float gm = grad[t], ga = grad[t + 1];
            float weight = gm * exp_(sq_dist * factor);
            float fidx = floor_(ga * ten_degree_per_radius);
            int oidx = cvt_rz(fidx);
            if (oidx < 0) oidx += 36;
            vote[oidx] += weight;
        }
    const float one_third = (float)(1.0 / 3.0);
    for (int i = 0; i < 6; ++i) {
        vote[36] = vote[0];
        float pre = vote[35];
        for (int j = 0; j < 36; ++j) {
            float temp = one_third * (pre + vote[j] + vote[j + 1]);
            pre = vote[j];
            vote[j] = temp;
        }
    }
    vote[36] = vote[0];
    // __fdividef(a, b) is stated as a * (1/b) (two roundings) on both sides
    auto fdiv = [](float a, float b) { return a * (1.0f / b); };
    if (num_orientation == 1 || existing) {
        int index_max = 0;
        float max_vote = vote[0];
        for (int i = 1; i < 36; ++i) {
            index_max = (kTie == 4 ? vote[i] >= max_vote : vote[i] > max_vote) ? i : index_max;
            max_vote = fmax_(max_vote, vote[i]);
        }
        float pre = vote[index_max == 0 ? 35 : index_max - 1];
        float next = vote[index_max + 1];
        float weight = max_vote;
        float off = 0.5f * fdiv(next - pre, weight + weight - next - pre);
        key.w = radius_per_ten_degrees * (index_max + 0.5f + off);
        out[0] = key.x; out[1] = key.y; out[2] = key.z; out[3] = key.w;
        return;
    }
    float max_vote = vote[0];
    for (int i = 1; i < 36; ++i) max_vote = fmax_(max_vote, vote[i]);
    float vote_threshold = max_vote * 0.8f;
    float pre = vote[35];
    float max_rot[2] = {0, 0}, max_vot[2] = {0, 0};
    int ocount = 0;
    for (int i = 0; i < 36; ++i) {
        float next = vote[i + 1];
        if (vote[i] > vote_threshold && (kTie == 3 ? vote[i] >= pre : vote[i] > pre) &&
            vote[i] > next) {
            float di = 0.5f * fdiv(next - pre, vote[i] + vote[i] - next - pre);
            float rot = i + di + 0.5f;
            float weight = vote[i];
            if (kTie == 2 ? weight >= max_vot[1] : weight > max_vot[1]) {
                if (kTie == 2 ? weight >= max_vot[0] : weight > max_vot[0]) {
                    max_vot[1] = max_vot[0];
                    max_rot[1] = max_rot[0];
                    max_vot[0] = weight;
                    max_rot[0] = rot;
                } else {
                    max_vot[1] = weight;
                    max_rot[1] = rot;
                }
                ocount++;
            }
        }
        pre = vote[i];
    }
    float fr1 = max_rot[0] / 36.0f;
    if (fr1 < 0) fr1 += 1.0f;
    unsigned short us1 = ocount == 0 ? 65535 : (unsigned short)floor_(fr1 * 65535.0f);
    unsigned short us2 = 65535;
    if (ocount > 1) {
        float fr2 = max_rot[1] / 36.0f;
        if (fr2 < 0) fr2 += 1.0f;
        us2 = (unsigned short)floor_(fr2 * 65535.0f);
    }
    uint32_t uspack = ((uint32_t)us2 << 16) | us1;
    out[0] = key.x; out[1] = key.y; out[2] = key.z; out[3] = u2f(uspack);
}

// --- ComputeDescriptor_Kernel<false> (ProgramCU.cu:1013-1101) + NormalizeDescriptor_Kernel
//     (:1173-1208) for one feature (fx, fy, s, o) in octave coordinates.
// --- NormalizeDescriptor_Kernel (ProgramCU.cu:1173-1208): sums of the 32 float4 in order,
//     rsqrt, clip 0.2, renormalise.
void normalize_descriptor(float* des128, int normalize) {
    if (!normalize) return;
    auto sq4 = [](const float* p) {
        float t = p[0] * p[0];
        t = fma_(p[1], p[1], t);
        t = fma_(p[2], p[2], t);
        t = fma_(p[3], p[3], t);
        return t;
    };
    float norm1 = 0, norm2 = 0;
    for (int i = 0; i < 32; ++i) norm1 += sq4(des128 + 4 * i);
    norm1 = rsqrt_(norm1);
    for (int i = 0; i < 128; ++i) des128[i] = fmin_(0.2f, des128[i] * norm1);
    for (int i = 0; i < 32; ++i) norm2 += sq4(des128 + 4 * i);
    norm2 = rsqrt_(norm2);
    for (int i = 0; i < 128; ++i) des128[i] *= norm2;
}

void descriptor(const float* key, const std::vector<float>& grad, int W, int H,
                float window_factor, int normalize, float* des128) {
    const float rpi = (float)(4.0 / 3.14159265358979323846);
    for (int bidx = 0; bidx < 16; bidx++) {
        int ix = bidx & 3, iy = bidx >> 2;
        float spt = fabs_(key[2] * window_factor);
        float s, c;
        sincos_(key[3], &s, &c);
        float anglef = key[3] > 3.14159265358979323846
                           ? (float)(key[3] - (2.0 * 3.14159265358979323846)) : key[3];
        float cspt = c * spt, sspt = s * spt;
        float crspt = c / spt, srspt = s / spt;
        float ox = ix - 1.5f, oy = iy - 1.5f;
        float ptx = fma_(cspt, ox, -(sspt * oy)) + key[0];
        float pty = fma_(cspt, oy, sspt * ox) + key[1];
        float bsz = fabs_(cspt) + fabs_(sspt);
        float xmin = fmax_(1.5f, floor_(ptx - bsz) + 0.5f);
        float ymin = fmax_(1.5f, floor_(pty - bsz) + 0.5f);
        float xmax = fmin_(W - 1.5f, floor_(ptx + bsz) + 0.5f);
        float ymax = fmin_(H - 1.5f, floor_(pty + bsz) + 0.5f);
        float des[9];
        for (int i = 0; i < 9; ++i) des[i] = 0.0f;
        for (float y = ymin; y <= ymax; y += 1.0f)
            for (float x = xmin; x <= xmax; x += 1.0f) {
                float dx = x - ptx, dy = y - pty;
                float nx = fma_(crspt, dx, srspt * dy);
                float ny = fma_(crspt, dy, -(srspt * dx));
                float nxn = fabs_(nx), nyn = fabs_(ny);
                if (nxn < 1.0f && nyn < 1.0f) {
                    size_t t = ((size_t)(int)y * W + (int)x) * 2;
                    float gm = grad[t], ga = grad[t + 1];
                    float dnx = nx + ox, dny = ny + oy;
                    float ww = exp_(-0.125f * fma_(dnx, dnx, dny * dny));
                    float wx = (float)(1.0 - nxn), wy = (float)(1.0 - nyn);
                    float weight = ww * wx * wy * gm;
                    float theta = (anglef - ga) * rpi;
                    if (theta < 0) theta += 8.0f;
                    float fo = floor_(theta);
                    int fidx = cvt_rz(fo);
                    float weight1 = fo + 1.0f - theta;
                    float weight2 = theta - fo;
                    if (fidx >= 0 && fidx < 8) {   // the unrolled k == fidx test drops fidx == 8
                        des[fidx] = fma_(weight1, weight, des[fidx]);
                        des[fidx + 1] = fma_(weight2, weight, des[fidx + 1]);
                    }
                }
            }
        des[0] += des[8];
        for (int i = 0; i < 8; i++) des128[bidx * 8 + i] = des[i];
    }
    normalize_descriptor(des128, normalize);
}

// --- ComputeDescriptorRECT_Kernel<false> (ProgramCU.cu:1104-1171): keys passed with
//     keys_have_orientation == -1 (SIFT_RECT_DESCRIPTION, SiftPyramid.cpp:307-309) describe the
//     axis-aligned rectangle [x, x + z] x [y, y + w] (octave coordinates) as a 4 x 4 grid, with
//     bilinear cell weights, no Gaussian window and the gradient angle taken as is.
void descriptor_rect(const float* key, const std::vector<float>& grad, int W, int H,
                     int normalize, float* des128) {
    const float rpi = (float)(4.0 / 3.14159265358979323846);
    for (int bidx = 0; bidx < 16; bidx++) {
        const int ix = bidx & 3, iy = bidx >> 2;
        const float sptx = (float)(key[2] * 0.25), spty = (float)(key[3] * 0.25);
        const float ptx = fma_(sptx, ix + 0.5f, key[0]);
        const float pty = fma_(spty, iy + 0.5f, key[1]);
        const float xmin = fmax_(1.5f, floor_(ptx - sptx) + 0.5f);
        const float ymin = fmax_(1.5f, floor_(pty - spty) + 0.5f);
        const float xmax = fmin_(W - 1.5f, floor_(ptx + sptx) + 0.5f);
        const float ymax = fmin_(H - 1.5f, floor_(pty + spty) + 0.5f);
        float des[9];
        for (int i = 0; i < 9; ++i) des[i] = 0.0f;
        for (float y = ymin; y <= ymax; y += 1.0f)
            for (float x = xmin; x <= xmax; x += 1.0f) {
                const float nx = (x - ptx) / sptx, ny = (y - pty) / spty;
                const float nxn = fabs_(nx), nyn = fabs_(ny);
                if (nxn < 1.0f && nyn < 1.0f) {
                    const size_t t = ((size_t)(int)y * W + (int)x) * 2;
                    const float gm = grad[t], ga = grad[t + 1];
                    const float wx = (float)(1.0 - nxn), wy = (float)(1.0 - nyn);
                    const float weight = wx * wy * gm;
                    float theta = (-ga) * rpi;
                    if (theta < 0) theta += 8.0f;
                    const float fo = floor_(theta);
                    const int fidx = cvt_rz(fo);
                    const float weight1 = fo + 1.0f - theta, weight2 = theta - fo;
                    if (fidx >= 0 && fidx < 8) {
                        des[fidx] = fma_(weight1, weight, des[fidx]);
                        des[fidx + 1] = fma_(weight2, weight, des[fidx + 1]);
                    }
                }
            }
        des[0] += des[8];
        for (int i = 0; i < 8; i++) des128[bidx * 8 + i] = des[i];
    }
    normalize_descriptor(des128, normalize);
}

// --- GLTexInput::SetImageData with _down_sampled = ds > 0 (GLTexImage.cpp:928-1009,
//     DownSamplePixelDataI2F / DownSamplePixelDataF with skip): pixel (r << ds, c << ds) of the
//     full-width input for r < h >> ds, c < ((w >> ds) & ~3).
Image ingest_sampled(const uint8_t* img, const float* img_f32, int w, int h, int stride, int ds) {
    Image o;
    o.w = (w >> ds) & ~3;
    o.h = h >> ds;
    o.px.resize((size_t)o.w * o.h);
    for (int y = 0; y < o.h; y++)
        for (int x = 0; x < o.w; x++) {
            const size_t src = (size_t)(y << ds) * stride + (size_t)(x << ds);
            o.px[(size_t)y * o.w + x] = img_f32 ? img_f32[src] : img[src] / 255.0f;
        }
    return o;
}

// --- SiftPyramid::LimitFeatureCount (SiftPyramid.cpp:219-260), preceded for the keypoint
//     list by the level skip of PyramidCU::GenerateFeatureList (PyramidCU.cpp:829-853, with
//     FOR_EACH_OCTAVE / FOR_EACH_LEVEL reversed for -tc2, SiftPyramid.h:174-184).  A skipped
//     level has no features (the reference keeps the previous image's stale count there when
//     the pyramid is reused; a fresh pyramid has 0).
void limit_feature_count(std::vector<int>& cnt, int T, int method, bool list_stage) {
    const int nl = (int)cnt.size();
    if (list_stage && method != 0) {
        int feature_num = 0;
        for (int q = 0; q < nl; q++) {
            const int l = method == 1 ? nl - 1 - q : q;
            if (feature_num > T) { cnt[l] = 0; continue; }
            feature_num += cnt[l];
        }
    }
    int feature_num = 0;
    for (int c : cnt) feature_num += c;
    if (method == 2) {
        int i = 0, new_feature_num = 0;
        for (; new_feature_num < T && i < nl; ++i) new_feature_num += cnt[i];
        for (; i < nl; ++i) cnt[i] = 0;
    } else {
        int i = 0;
        while (i < nl && feature_num - cnt[i] > T) {
            feature_num -= cnt[i];
            cnt[i++] = 0;
        }
    }
}

}  // namespace

Result extract(const uint8_t* img, int w, int h, int stride, const sgpu_options& opt,
               bool keep, const float* img_f32, bool keep_stages) {
    // first octave: -fo, -prep and -maxd (sgp::plan_input restates GLTexImage.cpp:928-960 and
    // PyramidCU.cpp:89-135)
    const sgp::InputPlan plan = sgp::plan_input(w, h, std::max(-3, opt.octave_min),
                                                opt.max_dimension, opt.preprocess_on_cpu);
    sgp::Options po;
    po.filter_width_factor = opt.filter_width_factor;
    po.dog_level_num = opt.dog_level_num;
    po.dog_threshold = opt.dog_threshold;
    po.edge_threshold = opt.edge_threshold;
    po.octave_min = plan.octave_min + plan.ds;   // GetInitialSmoothSigma(_octave_min + ds)
    const sgp::Schedule S = sgp::make_schedule(po);
    const int d = S.dog_level_num, nlev = S.level_num;
    const int fo = plan.octave_min;
    Result R;
    R.octaves = sgp::make_octaves(plan.w, plan.h, opt.octave_num, fo);
    const int noct = (int)R.octaves.size();

    // ResizeFeatureStorage (PyramidCU.cpp:341-347): histopyramid depth from the base level
    int whmax = std::max(R.octaves[0].wa, R.octaves[0].h);
    int hp_levels = (int)std::ceil(std::log(double(whmax)) / std::log(4.0));

    Image input = plan.ds > 0 ? ingest_sampled(img, img_f32, w, h, stride, plan.ds)
                  : img_f32   ? ingest_f32(img_f32, w, h, stride)
                              : ingest(img, w, h, stride);
    float taps[sgp::kMaxFilterWidth];
    std::vector<Image> prev;  // previous octave's Gaussian levels
    const float sigma_step = powf(2.0f, 1.0f / d);  // PyramidCU.cpp:1200
    const float tdog1 = (opt.subpixel ? 0.8f : 1.0f) * S.dog_threshold;   // ProgramCU.cu:677
    const float tedge = (S.edge_threshold + 1) * (S.edge_threshold + 1) / S.edge_threshold;
    const int num_orientation = opt.fixed_orientation ? 0 : opt.max_orientation;
    const double twopi = 2.0 * 3.14159265358979323846;
    const float offset = opt.lowe_origin ? 0.0f : 0.5f;

    // ---- BuildPyramid + DetectKeypointsEX + GenerateFeatureList, octave by octave
    std::vector<std::vector<std::vector<float>>> grad(noct);   // [octave][j]: grad of G[1+j]
    std::vector<std::vector<float>> sign(noct * d);            // extremum sign per candidate
    for (int o = 0; o < noct; o++) {
        const sgp::Octave& oc = R.octaves[o];
        std::vector<Image> g(nlev);
        // BuildPyramid (PyramidCU.cpp:979-1044)
        if (o == 0) {
            int fw = sgp::make_filter(S.initial_smooth, opt.filter_width_factor, taps);
            if (fo == 0) g[0] = filter(input, taps, fw);
            else if (fo > 0) g[0] = filter(downsample_input(input, fo, oc.wa, oc.h), taps, fw);
            else g[0] = filter(upsample_input(input, -fo), taps, fw);
        } else {
            g[0] = downsample(prev[S.level_ds - S.level_min], oc.wa, oc.h);
            if (S.sigma_skip1 > 0) {
                int fw = sgp::make_filter(S.sigma_skip1, opt.filter_width_factor, taps);
                g[0] = filter(g[0], taps, fw);
            }
        }
        for (int k = 1; k < nlev; k++) {
            int fw = sgp::make_filter(S.sigma[k - 1], opt.filter_width_factor, taps);
            g[k] = filter(g[k - 1], taps, fw);
        }
        // DetectKeypointsEX (PyramidCU.cpp:1046-1114): dog 1..nlev-1, grad for 1..d
        std::vector<Image> dog(nlev);
        std::vector<std::vector<float>> gr(nlev);
        for (int m = 1; m < nlev; m++)
            compute_dog(g[m], g[m - 1], &dog[m], (m >= 1 && m < 1 + d) ? &gr[m] : nullptr);
        for (int j = 0; j < d; j++) {
            std::vector<Key4> key;
            compute_key(dog[1 + j], dog[2 + j], dog[3 + j], tdog1, S.dog_threshold, tedge,
                        opt.subpixel, &key);
            LevelResult L;
            L.octave = o;
            L.level = j;
            L.candidates = histo_list(key, oc.wa, oc.h, hp_levels);
            for (const Candidate& c : L.candidates)
                sign[o * d + j].push_back(key[(size_t)c.row * oc.wa + c.col].x);
            if (keep_stages) {
                L.tdog = S.dog_threshold;
                L.tedge = S.edge_threshold;
                for (int m = 1; m <= 3; m++)
                    L.dog.insert(L.dog.end(), dog[m + j].px.begin(), dog[m + j].px.end());
                L.grad = gr[1 + j];
                L.key.resize(key.size() * 4);
                memcpy(L.key.data(), key.data(), key.size() * sizeof(Key4));
            }
            R.levels.push_back(std::move(L));
        }
        for (int j = 0; j < d; j++) grad[o].push_back(std::move(gr[1 + j]));
        prev = std::move(g);
        if (keep) R.gauss.push_back(prev);
    }
    const int nl = noct * d;
    const int T = opt.feature_count_threshold;
    if (T > 0) {   // GenerateFeatureList level skip + LimitFeatureCount(0) (SiftPyramid.cpp:117)
        std::vector<int> cnt(nl);
        for (int l = 0; l < nl; l++) cnt[l] = (int)R.levels[l].candidates.size();
        limit_feature_count(cnt, T, opt.truncate_method, true);
        for (int l = 0; l < nl; l++)
            if (cnt[l] == 0) R.levels[l].candidates.clear();
    }

    // ---- GetFeatureOrientations (PyramidCU.cpp:1195-1222): grad of G[1+j], GetLevelSigma(j)
    for (int l = 0; l < nl; l++) {
        LevelResult& L = R.levels[l];
        const int o = L.octave, j = L.level;
        const sgp::Octave& oc = R.octaves[o];
        const float sigma = sgp::level_sigma(S, j + S.level_min + 1);
        L.sigma = sigma;
        L.sigma_step = sigma_step;
        L.oriented.resize(L.candidates.size() * 4);
        for (size_t f = 0; f < L.candidates.size(); f++) {
            orientation(L.candidates[f], grad[o][j], oc.wa, oc.h, sigma, sigma_step,
                        opt.orientation_gaussian_factor,
                        opt.orientation_gaussian_factor * opt.orientation_window_factor,
                        num_orientation, opt.subpixel, opt.keep_extremum_sign,
                        opt.circular_window, &L.oriented[f * 4]);
            if (opt.keep_extremum_sign)   // ProgramCU.cu:849: z *= sign of the extremum
                L.oriented[f * 4 + 2] *= sign[l][f];
        }
    }
    // ReshapeFeatureListCPU (PyramidCU.cpp:521-606): a keypoint becomes 0, 1 or 2 features
    auto n_oriented = [&](const float* src) -> int {
        if (num_orientation < 2) return 1;
        const uint32_t pk = f2u(src[3]);
        const unsigned o1 = pk & 0xffff, o2 = pk >> 16;
        if (o1 == 65535) return 0;
        return (o2 != 65535 && o2 != o1) ? 2 : 1;
    };
    std::vector<char> level_kept(nl, 1);
    if (T > 0 && num_orientation >= 2) {   // LimitFeatureCount(1) (SiftPyramid.cpp:152-160)
        std::vector<int> cnt(nl, 0);
        for (int l = 0; l < nl; l++)
            for (size_t f = 0; f < R.levels[l].candidates.size(); f++)
                cnt[l] += n_oriented(&R.levels[l].oriented[f * 4]);
        limit_feature_count(cnt, T, opt.truncate_method, false);
        for (int l = 0; l < nl; l++) level_kept[l] = cnt[l] != 0;
    }

    // ---- feature expansion, image coordinates (DownloadKeypoints / ReshapeFeatureListCPU)
    //      and GetFeatureDescriptors (PyramidCU.cpp:413-452)
    for (int l = 0; l < nl; l++) {
        if (!level_kept[l]) continue;
        const LevelResult& L = R.levels[l];
        const int o = L.octave, j = L.level;
        const sgp::Octave& oc = R.octaves[o];
        const float oss = ldexpf(1.0f, o + fo + plan.ds);   // os * 2^o, os = 2^(octave_min + ds)
        auto emit = [&](const float* src, float ang) {
            R.feat_oct.insert(R.feat_oct.end(), {src[0], src[1], src[2], ang});
            R.keys.push_back(oss * (src[0] - 0.5f) + offset);
            R.keys.push_back(oss * (src[1] - 0.5f) + offset);
            R.keys.push_back(oss * src[2]);
            R.keys.push_back((float)std::fmod(twopi - ang, twopi));
            R.feat_level.push_back(l);
        };
        const size_t first = R.feat_level.size();
        for (size_t f = 0; f < L.candidates.size(); f++) {
            const float* src = &L.oriented[f * 4];
            if (num_orientation >= 2) {
                const double factor = 2.0 * 3.14159265358979323846 / 65535.0;
                uint32_t pk = f2u(src[3]);
                unsigned short o1 = pk & 0xffff, o2 = pk >> 16;
                if (o1 != 65535) {
                    emit(src, float(factor * o1));
                    if (o2 != 65535 && o2 != o1) emit(src, float(factor * o2));
                }
            } else {
                emit(src, src[3]);
            }
        }
        if (opt.descriptors) {
            const size_t nf = R.feat_level.size();
            R.desc.resize(nf * 128);
            for (size_t f = first; f < nf; f++)
                descriptor(&R.feat_oct[f * 4], grad[o][j], oc.wa, oc.h,
                           opt.descriptor_window_factor, opt.normalized, &R.desc[f * 128]);
        }
    }
    return R;
}

// --- Caller-supplied keypoints: SiftPyramid::SetKeypointList / SiftGPU::RunSIFT(num, keys,
//     keys_have_orientation) (SiftPyramid.cpp:293-310, SiftGPU.cpp:287-291).  The pyramid of the
//     image is built as usual, then (SiftPyramid.cpp:83-89, 129-147, 167-177):
//       GenerateFeatureListTex (PyramidCU.cpp:454-504): each key goes to the level whose
//         [sigma / 2^(0.5/d), sigma * 2^(0.5/d)) holds its scale (below the first / above the
//         last level: the first / last level), in octave coordinates;
//       ComputeOrientation with existing_keypoint (strongest orientation only) unless the keys
//         carry orientations; DownloadKeypoints (PyramidCU.cpp:701-751) then rewrites the keys;
//       GetFeatureDescriptors (PyramidCU.cpp:413-450) per level, put back into input order.
std::vector<float> describe_keys(const uint8_t* img, int w, int h, int stride,
                                 const sgpu_options& opt, const float* keys, int num,
                                 int has_orientation, std::vector<float>* keys_out) {
    sgpu_options o2 = opt;
    o2.descriptors = 0;
    o2.feature_count_threshold = -1;   // LimitFeatureCount skips existing keypoints
    Result R = extract(img, w, h, stride, o2, true);
    const sgp::InputPlan plan = sgp::plan_input(w, h, std::max(-3, opt.octave_min),
                                                opt.max_dimension, opt.preprocess_on_cpu);
    const int oexp = plan.octave_min + plan.ds;   // coordinates scale by 2^(octave_min + ds)
    sgp::Options po;
    po.filter_width_factor = opt.filter_width_factor;
    po.dog_level_num = opt.dog_level_num;
    po.dog_threshold = opt.dog_threshold;
    po.edge_threshold = opt.edge_threshold;
    po.octave_min = oexp;
    const sgp::Schedule S = sgp::make_schedule(po);
    const int d = S.dog_level_num, noct = (int)R.octaves.size();
    const double twopi = 2.0 * 3.14159265358979323846;
    const float sigma_half_step = powf(2.0f, 0.5f / d);
    const float offset = opt.lowe_origin ? 0.0f : 0.5f;
    struct Entry { float k[4]; int index, octave, level; };
    std::vector<Entry> list;
    float octave_sigma = ldexpf(1.0f, oexp);   // PyramidCU.cpp:461-463
    for (int i = 0; i < noct; i++, octave_sigma *= 2.0f)
        for (int j = 0; j < d; j++) {
            const float level_sigma = sgp::level_sigma(S, j + S.level_min + 1) * octave_sigma;
            const float sigma_min = level_sigma / sigma_half_step;
            const float sigma_max = level_sigma * sigma_half_step;
            for (int k = 0; k < num; k++) {
                const float* key = keys + 4 * k;
                const bool rect = has_orientation == -1;   // SIFT_RECT_DESCRIPTION
                const float sigmak = rect ? fmin_(key[2], key[3]) / 12.0f : key[2];
                if ((sigmak >= sigma_min && sigmak < sigma_max) ||
                    (sigmak < sigma_min && i == 0 && j == 0) ||
                    (sigmak > sigma_max && i == noct - 1 && j == d - 1)) {
                    Entry e;
                    e.k[0] = (key[0] - offset) / octave_sigma + 0.5f;
                    e.k[1] = (key[1] - offset) / octave_sigma + 0.5f;
                    e.k[2] = key[2] / octave_sigma;
                    e.k[3] = rect ? key[3] / octave_sigma
                                  : (float)std::fmod(twopi - key[3], twopi);
                    e.index = k;
                    e.octave = i;
                    e.level = j;
                    list.push_back(e);
                }
            }
        }
    // gradients of G[1+j] of every octave
    std::vector<std::vector<std::vector<float>>> grad(noct, std::vector<std::vector<float>>(d));
    for (int o = 0; o < noct; o++)
        for (int j = 0; j < d; j++) {
            Image dog;
            compute_dog(R.gauss[o][1 + j], R.gauss[o][j], &dog, &grad[o][j]);
        }
    const int num_orientation = opt.fixed_orientation ? 0 : opt.max_orientation;
    if (!has_orientation) {
        for (Entry& e : list) {
            const sgp::Octave& oc = R.octaves[e.octave];
            Key4 key{e.k[0], e.k[1], e.k[2], e.k[3]};
            float out[4];
            orientation_key(key, grad[e.octave][e.level], oc.wa, oc.h,
                            opt.orientation_gaussian_factor,
                            opt.orientation_gaussian_factor * opt.orientation_window_factor,
                            num_orientation, 1, opt.circular_window, out);
            e.k[3] = out[3];
        }
    }
    // DownloadKeypoints + the descriptor re-ordering: list position i goes back to
    // keypoint_index[i] for i < _featureNum (= num)
    keys_out->assign(keys, keys + 4 * (size_t)num);
    std::vector<float> desc((size_t)num * 128, 0.0f);
    const int m = std::min<int>(num, (int)list.size());
    for (int i = 0; i < m; i++) {
        const Entry& e = list[i];
        const float os = ldexpf(1.0f, e.octave + oexp);
        if (!has_orientation) {
            float* kk = keys_out->data() + 4 * (size_t)e.index;
            kk[0] = os * (e.k[0] - 0.5f) + offset;
            kk[1] = os * (e.k[1] - 0.5f) + offset;
            kk[2] = os * e.k[2];
            kk[3] = (float)std::fmod(twopi - e.k[3], twopi);
        }
        if (opt.descriptors) {
            const sgp::Octave& oc = R.octaves[e.octave];
            if (has_orientation == -1)
                descriptor_rect(e.k, grad[e.octave][e.level], oc.wa, oc.h, opt.normalized,
                                &desc[(size_t)e.index * 128]);
            else
                descriptor(e.k, grad[e.octave][e.level], oc.wa, oc.h, opt.descriptor_window_factor,
                           opt.normalized, desc.data() + 128 * (size_t)e.index);
        }
    }
    return desc;
}

struct Top2 { int max = 0, idx = -1, second = 0; };

// RowMatch_Kernel (ProgramCU.cu:1785-1835): 32 threads, thread t scans columns t, t+32, ... with
// a running (max, second, idx) from (0, 0, -1) and strict '>'; a tree reduction (steps 16, 8, 4,
// 2, 1) then keeps the lower slot on equal maxima, and the second is the largest value except
// the winner.  Two threads with equal maxima meet at the step of their lowest differing bit, and
// the one with that bit clear is kept: among equal maxima the thread whose 5 bits, reversed,
// give the lowest number wins (threads 8 and 2 meet at step 2 in slots 0 and 2: 8 wins) -- not
// the lowest thread, which is what this function assumed until the reference's own kernel, run
// on the CPU, was compared (tests/test_ref_kernels.py; that rule is kept as tie variant 7).  In
// column order: a larger value wins; an equal value takes the index when its thread ranks
// lower (same thread: the first occurrence stays); the second collects every other value.
inline int row_tie_rank(int col) {
    if (kTie == 7) return col & 31;
    int r = 0;
    for (int b = 0; b < 5; b++) r |= ((col >> b) & 1) << (4 - b);
    return r;
}
inline void row_fold(Top2& t, int v, int col) {
    if (v > t.max) { t.second = t.max; t.max = v; t.idx = col; return; }
    t.second = std::max(t.second, v);
    if (v == t.max && t.idx >= 0 && row_tie_rank(col) < row_tie_rank(t.idx)) t.idx = col;
}

// MultiplyDescriptor(G)_Kernel's column partials + ColMatch_Kernel (ProgramCU.cu:1540-1552,
// 1874-1882): the same running top-2 in row order, ties keep the earlier row.
inline void col_fold(Top2& t, int v, int row) {
    if (v > t.max) { t.second = t.max; t.max = v; t.idx = row; }
    else t.second = std::max(t.second, v);
}

// --- Geometric test of MultiplyDescriptorG_Kernel (ProgramCU.cu:1648-1681) for one pair:
//     |H x1 - x2| (both coordinates) < hdistmax, then the Sampson error of x2' F x1 < fdistmax.
//     Contractions (nvcc's choice is not observable) are fixed as written out below on both
//     sides; FDIV(a, b) = a * (1 / b).
bool guided_pass(const float* H, const float* F, float x1, float y1, float x2, float y2,
                 float hdistmax, float fdistmax) {
    auto fdiv = [](float a, float b) { return a * (1.0f / b); };
    const float h0 = fma_(H[0], x1, fma_(H[1], y1, H[2]));
    const float h1 = fma_(H[3], x1, fma_(H[4], y1, H[5]));
    const float h2 = fma_(H[6], x1, fma_(H[7], y1, H[8]));
    const float d0 = fabs_(fdiv(h0, h2) - x2), d1 = fabs_(fdiv(h1, h2) - y2);
    if (!(d0 < hdistmax && d1 < hdistmax)) return false;
    const float f0 = fma_(F[0], x1, fma_(F[1], y1, F[2]));
    const float f1 = fma_(F[3], x1, fma_(F[4], y1, F[5]));
    const float f2 = fma_(F[6], x1, fma_(F[7], y1, F[8]));
    const float t0 = fma_(F[0], x2, fma_(F[3], y2, F[6]));
    const float t1 = fma_(F[1], x2, fma_(F[4], y2, F[7]));
    const float x2fx1 = fma_(x2, f0, fma_(y2, f1, f2));
    float den = f0 * f0;
    den = fma_(f1, f1, den);
    den = fma_(t0, t0, den);
    den = fma_(t1, t1, den);
    const float se = fdiv(x2fx1 * x2fx1, den);
    return se < fdistmax;
}

// SiftMatchCU::GetGuidedSiftMatch (SiftMatchCU.cpp:126-136) = MultiplyDescriptorG_Kernel
// (ProgramCU.cu:1607-1735) + the RowMatch / ColMatch decisions.  The guided dot of a pair is
// its dot when the pair passes the geometric test; otherwise -262144, plus the dot when any
// other row of its 8-row block (MULT_BLOCK_DIMY) passes at that column.  Rows: row_fold over
// max(v, 0); columns: the per-block (max, idx, second) of :1709-1721 merged over blocks as
// ColMatch_Kernel (:1874-1882).
std::vector<int> match_guided(const uint8_t* d1, int n1, const uint8_t* d2, int n2,
                              const float* loc1, const float* loc2, const float* H,
                              const float* F, float distmax, float ratiomax, float hdistmax,
                              float fdistmax, int mbm, int max_match) {
    std::vector<Top2> rows(n1), cols(n2);
    const int nblk = (n1 + 7) / 8;
    for (int j = 0; j < n2; j++) {
        Top2 colacc;
        for (int blk = 0; blk < nblk; blk++) {
            int res[8];
            int good = 0;
            for (int i = 0; i < 8; i++) {
                const int r = blk * 8 + i;
                res[i] = -262144;
                if (r < n1 && guided_pass(H, F, loc1[2 * r], loc1[2 * r + 1], loc2[2 * j],
                                          loc2[2 * j + 1], hdistmax, fdistmax))
                    res[i] = 0;
                good += res[i] >= 0;
            }
            if (good > 0)
                for (int i = 0; i < 8; i++) {
                    const int r = blk * 8 + i;
                    if (r >= n1) break;
                    int dot = 0;
                    for (int k = 0; k < 128; k++) dot += (int)d1[r * 128 + k] * (int)d2[j * 128 + k];
                    res[i] += dot;
                }
            Top2 cmp;   // (0, -1, 0)
            for (int i = 0; i < 8; i++) {
                const int r = blk * 8 + i;
                if (r >= n1) break;
                if (res[i] > cmp.max) { cmp.second = cmp.max; cmp.max = res[i]; cmp.idx = r; }
                else cmp.second = std::max(cmp.second, res[i]);
                row_fold(rows[r], std::max(res[i], 0), j);   // d_result = max(results, 0)
            }
            if (blk == 0) colacc = cmp;
            else if (colacc.max < cmp.max) colacc = Top2{cmp.max, cmp.idx, std::max(colacc.max, cmp.second)};
            else colacc.second = std::max(colacc.second, cmp.max);
        }
        cols[j] = colacc;
    }
    auto accept = [&](const Top2& t) {
        float dist = match_distance(std::min(t.max, 262144));
        float distn = match_distance(std::min(t.second, 262144));
        return (dist < distmax) && (dist < distn * ratiomax) ? t.idx : -1;
    };
    std::vector<int> out;
    for (int i = 0; i < n1 && (int)out.size() / 2 < max_match; ++i) {
        int j = accept(rows[i]);
        if (j >= 0 && (!mbm || accept(cols[j]) == i)) {
            out.push_back(i);
            out.push_back(j);
        }
    }
    return out;
}

// The same decisions as match() with the dot products computed by `threads` OpenMP threads:
// every row folds its columns in ascending order (row_fold) and every column its rows in
// ascending order (col_fold), exactly the sequences match() applies -- only the work is split
// (rows over threads, then columns over threads, each dot computed once per side).  Used at the
// benched C5 size (50k x 50k), where the single loop would take minutes.
std::vector<int> match_mt(const uint8_t* d1, int n1, const uint8_t* d2, int n2, float distmax,
                          float ratiomax, int mbm, int max_match, int threads) {
    std::vector<Top2> rows(n1), cols(n2);
    auto dot = [](const uint8_t* a, const uint8_t* b) {
        int s = 0;
        for (int k = 0; k < 128; k++) s += (int)a[k] * (int)b[k];
        return s;
    };
#pragma omp parallel for num_threads(threads) schedule(dynamic, 64)
    for (int i = 0; i < n1; i++)
        for (int j = 0; j < n2; j++) row_fold(rows[i], dot(d1 + (size_t)i * 128, d2 + (size_t)j * 128), j);
    if (mbm) {
#pragma omp parallel for num_threads(threads) schedule(dynamic, 64)
        for (int j = 0; j < n2; j++)
            for (int i = 0; i < n1; i++) col_fold(cols[j], dot(d1 + (size_t)i * 128, d2 + (size_t)j * 128), i);
    }
    auto accept = [&](const Top2& t) {
        float dist = match_distance(std::min(t.max, 262144));
        float distn = match_distance(std::min(t.second, 262144));
        return (dist < distmax) && (dist < distn * ratiomax) ? t.idx : -1;
    };
    std::vector<int> out;
    for (int i = 0; i < n1 && (int)out.size() / 2 < max_match; ++i) {
        int j = accept(rows[i]);
        if (j >= 0 && (!mbm || accept(cols[j]) == i)) {
            out.push_back(i);
            out.push_back(j);
        }
    }
    return out;
}

float match_distance(int dot) {
    // RowMatch_Kernel / ColMatch_Kernel (ProgramCU.cu:1838-1839, 1884-1885):
    // float product, min with 1.0 in double, acos in double, stored as float.
    return (float)std::acos(std::min((double)(dot * 0.000003814697265625f), 1.0));
}

std::vector<int> match(const uint8_t* d1, int n1, const uint8_t* d2, int n2, float distmax,
                       float ratiomax, int mbm, int max_match) {
    std::vector<Top2> rows(n1), cols(n2);
    // MultiplyDescriptor_Kernel (ProgramCU.cu:1466-1564): exact int dot products
    for (int i = 0; i < n1; i++)
        for (int j = 0; j < n2; j++) {
            int dot = 0;
            for (int k = 0; k < 128; k++) dot += (int)d1[i * 128 + k] * (int)d2[j * 128 + k];
            row_fold(rows[i], dot, j);
            col_fold(cols[j], dot, i);
        }
    auto accept = [&](const Top2& t) {
        float dist = match_distance(std::min(t.max, 262144));
        float distn = match_distance(std::min(t.second, 262144));
        return (dist < distmax) && (dist < distn * ratiomax) ? t.idx : -1;
    };
    std::vector<int> out;
    for (int i = 0; i < n1 && (int)out.size() / 2 < max_match; ++i) {
        int j = accept(rows[i]);
        if (j >= 0 && (!mbm || accept(cols[j]) == i)) {   // SiftMatchCU.cpp:166-176
            out.push_back(i);
            out.push_back(j);
        }
    }
    return out;
}

}  // namespace oracle

// ---------------------------------------------------------------------------------------------
// C entry points for ctypes (tests / bench cpu_baseline).
extern "C" {

// The first-octave plan (sgp::plan_input): out = {ds, w, h, octave_min}.
void oracle_plan(int w, int h, int fo, int max_dim, int prep, int* out) {
    const sgp::InputPlan p = sgp::plan_input(w, h, fo < -3 ? -3 : fo, max_dim, prep);
    out[0] = p.ds;
    out[1] = p.w;
    out[2] = p.h;
    out[3] = p.octave_min;
}

// SiftPyramid::SaveSIFT (SiftPyramid.cpp:311-387), restated with the same iostream formatting:
// binary (-b): n, dim, then per feature y, x, s, o (+ 128 floats); ASCII: "n 128" then per
// feature "y x s o" at fixed precision 2 2 3 3 and the 128 values (floor(0.5 + 512 d) when
// normalised, setprecision(8) floats with -unn), a newline after every 20; without descriptors
// (-sd) "n 0" and "y x s o" at the fixed default precision.
int oracle_save_sift(const char* path, const float* keys, const float* desc, int n, int binary,
                     int normalized, int has_desc) {
    if (n <= 0) return 0;
    const float* pk = keys;
    if (binary) {
        std::ofstream out(path, std::ios::binary);
        out.write((const char*)&n, sizeof(int));
        const int dim = has_desc ? 128 : 0;
        out.write((const char*)&dim, sizeof(int));
        const float* pd = desc;
        for (int i = 0; i < n; i++, pk += 4) {
            out.write((const char*)(pk + 1), sizeof(float));
            out.write((const char*)pk, sizeof(float));
            out.write((const char*)(pk + 2), 2 * sizeof(float));
            if (has_desc) {
                out.write((const char*)pd, 128 * sizeof(float));
                pd += 128;
            }
        }
        return 0;
    }
    std::ofstream out(path);
    out.flags(std::ios::fixed);
    if (has_desc) {
        const float* pd = desc;
        out << n << " 128" << std::endl;
        for (int i = 0; i < n; i++) {
            out << std::setprecision(2) << pk[1] << " " << std::setprecision(2) << pk[0] << " "
                << std::setprecision(3) << pk[2] << " " << std::setprecision(3) << pk[3]
                << std::endl;
            pk += 4;
            for (int k = 0; k < 128; k++, pd++) {
                if (normalized) out << ((unsigned int)floor(0.5 + 512.0f * (*pd))) << " ";
                else out << std::setprecision(8) << pd[0] << " ";
                if ((k + 1) % 20 == 0) out << std::endl;
            }
            out << std::endl;
        }
    } else {
        out << n << " 0" << std::endl;
        for (int i = 0; i < n; i++, pk += 4)
            out << pk[1] << " " << pk[0] << " " << pk[2] << " " << pk[3] << std::endl;
    }
    return 0;
}

int oracle_extract(const uint8_t* img, int w, int h, int stride, const sgpu_options* opt,
                   float* keys, float* desc, int cap, int* n_out) {
    try {
        oracle::Result R = oracle::extract(img, w, h, stride, *opt, false);
        int n = (int)R.feat_level.size();
        *n_out = n;
        if (n > cap) return -4;
        if (keys) memcpy(keys, R.keys.data(), sizeof(float) * 4 * n);
        if (desc && opt->descriptors) memcpy(desc, R.desc.data(), sizeof(float) * 128 * n);
        return 0;
    } catch (const std::invalid_argument&) {
        return -2;   // options the reference cannot run (see oracle::extract)
    }
}

// Gaussian level (octave o, level k) of the oracle pyramid.
int oracle_extract_f32(const float* img, int w, int h, int stride, const sgpu_options* opt,
                       float* keys, float* desc, int cap, int* n_out) {
    try {
        oracle::Result R = oracle::extract(nullptr, w, h, stride, *opt, false, img);
        int n = (int)R.feat_level.size();
        *n_out = n;
        if (n > cap) return -4;
        if (keys) memcpy(keys, R.keys.data(), sizeof(float) * 4 * n);
        if (desc && opt->descriptors) memcpy(desc, R.desc.data(), sizeof(float) * 128 * n);
        return 0;
    } catch (const std::invalid_argument&) {
        return -2;
    }
}

static int gaussian_of(const uint8_t* img, const float* img_f32, int w, int h, int stride,
                       const sgpu_options* opt, int octave, int level, float* out, int cap) {
    try {
        sgpu_options o2 = *opt;
        o2.descriptors = 0;
        oracle::Result R = oracle::extract(img, w, h, stride, o2, true, img_f32);
        if (octave >= (int)R.gauss.size()) return -1;
        const oracle::Image& g = R.gauss[octave][level];
        if ((int)g.px.size() > cap) return -4;
        memcpy(out, g.px.data(), g.px.size() * sizeof(float));
        return (int)g.px.size();
    } catch (const std::invalid_argument&) {
        return -2;   // options the reference cannot run (see oracle::extract)
    }
}

int oracle_gaussian(const uint8_t* img, int w, int h, int stride, const sgpu_options* opt,
                    int octave, int level, float* out, int cap) {
    return gaussian_of(img, nullptr, w, h, stride, opt, octave, level, out, cap);
}

// The same for float luminance input (oracle_extract_f32's pyramid).
int oracle_gaussian_f32(const float* img, int w, int h, int stride, const sgpu_options* opt,
                        int octave, int level, float* out, int cap) {
    return gaussian_of(nullptr, img, w, h, stride, opt, octave, level, out, cap);
}

// Candidates in reference order: ints {col,row,level_id,0}, floats {dx,dy,ds,0}.
static int candidates_of(const uint8_t* img, const float* img_f32, int w, int h, int stride,
                         const sgpu_options* opt, int* ints, float* floats, int cap, int* n_out) {
    try {
        sgpu_options o2 = *opt;
        o2.descriptors = 0;
        oracle::Result R = oracle::extract(img, w, h, stride, o2, false, img_f32);
        int n = 0, d = opt->dog_level_num;
        for (const auto& L : R.levels)
            for (const auto& c : L.candidates) {
                if (n < cap) {
                    int* p = ints + 4 * n;
                    p[0] = c.col; p[1] = c.row; p[2] = L.octave * d + L.level; p[3] = 0;
                    float* q = floats + 4 * n;
                    q[0] = c.dx; q[1] = c.dy; q[2] = c.ds; q[3] = 0;
                }
                n++;
            }
        *n_out = n;
        return n > cap ? -4 : 0;
    } catch (const std::invalid_argument&) {
        return -2;   // options the reference cannot run (see oracle::extract)
    }
}

int oracle_candidates(const uint8_t* img, int w, int h, int stride, const sgpu_options* opt,
                      int* ints, float* floats, int cap, int* n_out) {
    return candidates_of(img, nullptr, w, h, stride, opt, ints, floats, cap, n_out);
}

int oracle_candidates_f32(const float* img, int w, int h, int stride, const sgpu_options* opt,
                          int* ints, float* floats, int cap, int* n_out) {
    return candidates_of(nullptr, img, w, h, stride, opt, ints, floats, cap, n_out);
}

// Features in octave coordinates (x, y, s, o: the descriptor's input) with their level id
// (octave*d + j), in output order.  For the independent float64 cross-check (tests/ref_numpy.py).
int oracle_features_oct(const uint8_t* img, int w, int h, int stride, const sgpu_options* opt,
                        float* feat, int* level, int cap, int* n_out) {
    try {
        sgpu_options o2 = *opt;
        o2.descriptors = 0;
        oracle::Result R = oracle::extract(img, w, h, stride, o2, false);
        const int n = (int)R.feat_level.size();
        for (int i = 0; i < n && i < cap; i++) {
            memcpy(feat + 4 * i, &R.feat_oct[4 * (size_t)i], 4 * sizeof(float));
            level[i] = R.feat_level[i];
        }
        *n_out = n;
        return n > cap ? -4 : 0;
    } catch (const std::invalid_argument&) {
        return -2;   // options the reference cannot run (see oracle::extract)
    }
}

// SiftGPU::RunSIFT(num, keys, keys_have_orientation) on image img: keys_out [num][4],
// desc [num][128] in input order.
// The stages of level `level` of octave `octave` (Result::levels with keep_stages): dims =
// {wa, h, candidate count}, sig = {sigma, sigma_step, ComputeKEY's Tdog, Tedge}; dog 3 x wa x h, grad wa x h x 2, key
// wa x h x 4, list (col, row, 0, 0) and oriented 4 per candidate, up to cap.  Every output may
// be null.  Returns the candidate count, -1 for a level that does not exist.
int oracle_level_stages(const uint8_t* img, int w, int h, int stride, const sgpu_options* opt,
                        int octave, int level, int* dims, float* sig, float* dog, float* grad,
                        float* key, int* list, float* oriented, int cap) {
    oracle::Result R = oracle::extract(img, w, h, stride, *opt, false, nullptr, true);
    for (const oracle::LevelResult& L : R.levels) {
        if (L.octave != octave || L.level != level) continue;
        const int n = (int)L.candidates.size();
        if (dims) { dims[0] = R.octaves[octave].wa; dims[1] = R.octaves[octave].h; dims[2] = n; }
        if (sig) { sig[0] = L.sigma; sig[1] = L.sigma_step; sig[2] = L.tdog; sig[3] = L.tedge; }
        if (dog) memcpy(dog, L.dog.data(), L.dog.size() * sizeof(float));
        if (grad) memcpy(grad, L.grad.data(), L.grad.size() * sizeof(float));
        if (key) memcpy(key, L.key.data(), L.key.size() * sizeof(float));
        for (int i = 0; i < n && i < cap; i++) {
            if (list) { list[4 * i] = L.candidates[i].col; list[4 * i + 1] = L.candidates[i].row; list[4 * i + 2] = list[4 * i + 3] = 0; }
            if (oriented) memcpy(oriented + 4 * i, &L.oriented[4 * i], 4 * sizeof(float));
        }
        return n;
    }
    return -1;
}

// ---- single stages on caller-supplied inputs (tests/test_ref_kernels.py feeds the same arrays
//      to the reference's own kernels).  Images are row-major w x h.
static oracle::Image stage_image(const float* px, int w, int h) {
    oracle::Image im;
    im.w = w;
    im.h = h;
    im.px.assign(px, px + (size_t)w * h);
    return im;
}

// FilterImage(sigma): returns the filter width.
int oracle_stage_filter(const float* src, int w, int h, float sigma, float width_factor,
                        float* dst) {
    float taps[sgp::kMaxFilterWidth];
    const int fw = sgp::make_filter(sigma, width_factor, taps);
    const oracle::Image out = oracle::filter(stage_image(src, w, h), taps, fw);
    memcpy(dst, out.px.data(), out.px.size() * sizeof(float));
    return fw;
}

// ComputeDOG: dog = cur - prev and, unless grad is null, the float2 gradient of cur.
void oracle_stage_dog(const float* prev, const float* cur, int w, int h, float* dog, float* grad) {
    oracle::Image d;
    std::vector<float> g;
    oracle::compute_dog(stage_image(cur, w, h), stage_image(prev, w, h), &d, grad ? &g : nullptr);
    memcpy(dog, d.px.data(), d.px.size() * sizeof(float));
    if (grad) memcpy(grad, g.data(), g.size() * sizeof(float));
}

// ComputeKEY(dog, key, Tdog, Tedge) with the arguments ProgramCU::ComputeKEY takes.
void oracle_stage_key(const float* dp, const float* dc, const float* dn, int w, int h, float tdog,
                      float tedge, int subpixel, float* key) {
    std::vector<oracle::Key4> k;
    oracle::compute_key(stage_image(dp, w, h), stage_image(dc, w, h), stage_image(dn, w, h),
                        (subpixel ? 0.8f : 1.0f) * tdog, tdog, (tedge + 1) * (tedge + 1) / tedge,
                        subpixel, &k);
    memcpy(key, k.data(), k.size() * sizeof(oracle::Key4));
}

// The per-level list (col, row, 0, 0) of a key image inside a pyramid whose base level is
// base_w x base_h; returns the count (entries beyond cap are not written).
int oracle_stage_list(const float* key, int w, int h, int base_w, int base_h, int* list, int cap) {
    std::vector<oracle::Key4> k((size_t)w * h);
    memcpy(k.data(), key, k.size() * sizeof(oracle::Key4));
    const int levels = (int)std::ceil(std::log(double(std::max(base_w, base_h))) / std::log(4.0));
    const std::vector<oracle::Candidate> c = oracle::histo_list(k, w, h, levels);
    for (int i = 0; i < (int)c.size() && i < cap; i++) {
        list[4 * i] = c[i].col;
        list[4 * i + 1] = c[i].row;
        list[4 * i + 2] = list[4 * i + 3] = 0;
    }
    return (int)c.size();
}

// ComputeOrientation on list entries (col, row, ., .) with the key image's offsets: out 4 per
// entry (x, y, scale, packed orientations -- or the angle for num_orientation == 1).
void oracle_stage_orientation(const int* list, int n, const float* key, const float* grad, int w,
                              int h, float sigma, float sigma_step, float gaussian_factor,
                              float window_factor, int num_orientation, int subpixel, float* out) {
    const std::vector<float> g(grad, grad + (size_t)w * h * 2);
    for (int i = 0; i < n; i++) {
        const float* k = key + 4 * ((size_t)list[4 * i + 1] * w + list[4 * i]);
        const oracle::Candidate c{list[4 * i], list[4 * i + 1], k[1], k[2], k[3]};
        oracle::orientation(c, g, w, h, sigma, sigma_step, gaussian_factor,
                            gaussian_factor * window_factor, num_orientation, subpixel, 0, 0,
                            out + 4 * i);
    }
}

// ComputeDescriptor for n keys (x, y, scale, orientation) in octave coordinates; rect: the RECT
// kernel on (x, y, width, height).
void oracle_stage_descriptor(const float* keys, int n, const float* grad, int w, int h,
                             float window_factor, int normalized, int rect, float* out) {
    const std::vector<float> g(grad, grad + (size_t)w * h * 2);
    for (int i = 0; i < n; i++) {
        if (rect) oracle::descriptor_rect(keys + 4 * i, g, w, h, normalized, out + 128 * (size_t)i);
        else oracle::descriptor(keys + 4 * i, g, w, h, window_factor, normalized, out + 128 * (size_t)i);
    }
}

int oracle_describe_keys(const uint8_t* img, int w, int h, int stride, const sgpu_options* opt,
                         const float* keys, int num, int has_orientation, float* keys_out,
                         float* desc) {
    try {
        std::vector<float> ko;
        std::vector<float> d = oracle::describe_keys(img, w, h, stride, *opt, keys, num,
                                                     has_orientation, &ko);
        if (keys_out) memcpy(keys_out, ko.data(), ko.size() * sizeof(float));
        if (desc && opt->descriptors) memcpy(desc, d.data(), d.size() * sizeof(float));
        return 0;
    } catch (const std::invalid_argument&) {
        return -2;   // options the reference cannot run (see oracle::extract)
    }
}

int oracle_match(const uint8_t* d1, int n1, const uint8_t* d2, int n2, float distmax,
                 float ratiomax, int mbm, int max_match, int* out_pairs) {
    std::vector<int> m = oracle::match(d1, n1, d2, n2, distmax, ratiomax, mbm, max_match);
    memcpy(out_pairs, m.data(), m.size() * sizeof(int));
    return (int)m.size() / 2;
}

int oracle_match_mt(const uint8_t* d1, int n1, const uint8_t* d2, int n2, float distmax,
                    float ratiomax, int mbm, int max_match, int* out_pairs, int threads) {
    std::vector<int> m = oracle::match_mt(d1, n1, d2, n2, distmax, ratiomax, mbm, max_match,
                                          threads);
    memcpy(out_pairs, m.data(), m.size() * sizeof(int));
    return (int)m.size() / 2;
}

float oracle_match_distance(int dot) { return oracle::match_distance(dot); }

int oracle_match_guided(const uint8_t* d1, int n1, const uint8_t* d2, int n2, const float* loc1,
                        const float* loc2, const float* H, const float* F, float distmax,
                        float ratiomax, float hdistmax, float fdistmax, int mbm, int max_match,
                        int* out_pairs) {
    std::vector<int> m = oracle::match_guided(d1, n1, d2, n2, loc1, loc2, H, F, distmax, ratiomax,
                                              hdistmax, fdistmax, mbm, max_match);
    memcpy(out_pairs, m.data(), m.size() * sizeof(int));
    return (int)m.size() / 2;
}

int oracle_guided_pass(const float* H, const float* F, float x1, float y1, float x2, float y2,
                       float hdistmax, float fdistmax) {
    return oracle::guided_pass(H, F, x1, y1, x2, y2, hdistmax, fdistmax) ? 1 : 0;
}

void oracle_schedule(int dog_level_num, float* sigma0, float* sigma_skip0, float* sigmas,
                     int* widths) {
    sgp::Options po;
    po.dog_level_num = dog_level_num;
    sgp::Schedule S = sgp::make_schedule(po);
    *sigma0 = S.sigma0;
    *sigma_skip0 = S.sigma_skip0;
    float taps[sgp::kMaxFilterWidth];
    widths[0] = sgp::make_filter(S.initial_smooth, 4.0f, taps);
    for (int i = 0; i < S.level_num - 1; i++) {
        sigmas[i] = S.sigma[i];
        widths[i + 1] = sgp::make_filter(S.sigma[i], 4.0f, taps);
    }
}

// Every sigma FilterImage is called with for dog_level_num levels (first octave 0): the initial
// smoothing, the smoothing after an octave change (0 = none) and the level-to-level sigmas.
int oracle_filter_sigmas(int dog_level_num, float* out, int max) {
    sgp::Options po;
    po.dog_level_num = dog_level_num;
    const sgp::Schedule S = sgp::make_schedule(po);
    int n = 0;
    if (n < max) out[n++] = S.initial_smooth;
    if (n < max) out[n++] = S.sigma_skip1;
    for (int i = 0; i < S.level_num - 1 && n < max; i++) out[n++] = S.sigma[i];
    return n;
}

// Octave geometry (w, h, wa per octave) for an input of w x h (PyramidCU.cpp:89-271).
// The first octave's resampled input for -fo != 0 (before the initial smoothing): returns the
// element count, dims[0..1] = width, height.
int oracle_first_octave_input(const uint8_t* img, int w, int h, int stride, int fo, float* out,
                              int cap, int* dims) {
    oracle::Image in = oracle::ingest(img, w, h, stride);
    std::vector<sgp::Octave> oc = sgp::make_octaves(w, h, 1, fo);
    oracle::Image r = fo > 0 ? oracle::downsample_input(in, fo, oc[0].wa, oc[0].h)
                             : oracle::upsample_input(in, -fo);
    if ((int)r.px.size() > cap) return -4;
    memcpy(out, r.px.data(), r.px.size() * sizeof(float));
    dims[0] = r.w;
    dims[1] = r.h;
    return (int)r.px.size();
}

int oracle_geometry(int w, int h, int octave_num, int* dims, int max, int octave_min) {
    std::vector<sgp::Octave> oc = sgp::make_octaves(w, h, octave_num, octave_min);
    for (int o = 0; o < (int)oc.size() && o < max; o++) {
        dims[3 * o] = oc[o].w; dims[3 * o + 1] = oc[o].h; dims[3 * o + 2] = oc[o].wa;
    }
    return (int)oc.size();
}

// Histogram-pyramid level widths for a key image of width W inside a pyramid whose base level
// is base_w x base_h (FitHistogramPyramid PyramidCU.cpp:1175-1193 with the depth of
// ResizeFeatureStorage PyramidCU.cpp:341-347).
int oracle_hist_widths(int W, int base_w, int base_h, int* widths, int max) {
    int whmax = std::max(base_w, base_h);
    int levels = (int)std::ceil(std::log(double(whmax)) / std::log(4.0));
    int w = (W + 2) >> 2, n = 0;
    for (int k = 0; k < levels && n < max; k++) {
        widths[n++] = w;
        if (w == 1) break;
        w = (w + 3) >> 2;
    }
    return n;
}

// deterministic math probes (accuracy tests against libm)
float oracle_exp(float x) { return sgm::exp_(x); }
float oracle_atan2(float y, float x) { return sgm::atan2_(y, x); }
float oracle_log(float x) { return sgm::log_(x); }
void oracle_sincos(float x, float* s, float* c) { sgm::sincos_(x, s, c); }

}  // extern "C"
