// ref_driver.cpp -- C entry points over the reference's own ProgramCU:: stage functions, run on
// the CPU by the host execution layer (oracle/cuda_host).  TEST INFRASTRUCTURE ONLY.
//
// This file is compiled only where a checkout of the reference is present (oracle/Makefile),
// together with the reference's ProgramCU.cu (its launches rewritten by cuda_host/rewrite.py)
// and CuTexImage.cpp, into oracle/_ref/libref_kernels.so and libref_kernels_fast.so.  It calls
// the reference's functions by name on buffers the caller passes in, one stage per entry
// point, and holds none of the reference's code.  tests/ref_kernels.py loads it; with
// REF_DRIVER_MAIN it is a stand-alone program that runs every stage once (the sanitizer build).
//
// What the reference's GlobalUtil.cpp would define (it needs a window system) is defined here:
// the settings the stage functions read, with the reference's defaults, and a timer that does
// nothing.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "GL/glew.h"
#include "cuda_host.h"

#include "CuTexImage.h"
#include "GlobalUtil.h"
#include "ProgramCU.h"

int GlobalParam::_verbose = 0;
int GlobalParam::_timingS = 0;
int GlobalParam::_timingO = 0;
int GlobalParam::_MemCapGPU = 0;
int GlobalParam::_texMaxDimGL = 14096;
int GlobalParam::_UseDynamicIndexing = 0;
float GlobalParam::_FilterWidthFactor = 4.0f;
float GlobalParam::_OrientationWindowFactor = 2.0f;
float GlobalParam::_OrientationGaussianFactor = 1.5f;
float GlobalParam::_DescriptorWindowFactor = 3.0f;
int GlobalParam::_MaxOrientation = 2;
int GlobalParam::_SubpixelLocalization = 1;
int GlobalParam::_FixedOrientation = 0;
int GlobalParam::_NormalizedSIFT = 1;
int GlobalParam::_KeepExtremumSign = 0;
ClockTimer GlobalUtil::_globalTimer;
void ClockTimer::StartTimer(const char*, int) {}
void ClockTimer::StopTimer(int) {}
float ClockTimer::GetElapsedTime() { return 0.0f; }

namespace {

// A texture of w x h x nch floats holding `data` (nullptr: left as allocated).
void fill(CuTexImage& t, int w, int h, int nch, const void* data) {
    t.InitTexture(w, h, nch);
    if (data) t.CopyFromHost(data);
}

// Bytes as a one-channel texture of ceil(n / 4) floats.
void fill_bytes(CuTexImage& t, const void* data, size_t n) {
    std::vector<float> padded((n + 3) / 4, 0.0f);
    memcpy(padded.data(), data, n);
    fill(t, (int)padded.size(), 1, 1, padded.data());
}

// ReduceToSingleChannel and ConvertByteToFloat launch whole 128-thread blocks that store
// without a bound check: the destination gets room for the rounded-up count.
void fill_padded_dst(CuTexImage& t, int w, int h) {
    const int extra = (128 + w - 1) / w + 1;
    t.InitTexture(w, h + extra, 1);
    t.SetImageSize(w, h);
}

}  // namespace

extern "C" {

void ref_settings(int subpixel, int max_orientation, int fixed_orientation, int keep_sign,
                  float filter_width_factor, float orientation_gaussian_factor,
                  float orientation_window_factor, float descriptor_window_factor, int normalized,
                  int dynamic_indexing) {
    GlobalUtil::_SubpixelLocalization = subpixel;
    GlobalUtil::_MaxOrientation = max_orientation;
    GlobalUtil::_FixedOrientation = fixed_orientation;
    GlobalUtil::_KeepExtremumSign = keep_sign;
    GlobalUtil::_FilterWidthFactor = filter_width_factor;
    GlobalUtil::_OrientationGaussianFactor = orientation_gaussian_factor;
    GlobalUtil::_OrientationWindowFactor = orientation_window_factor;
    GlobalUtil::_DescriptorWindowFactor = descriptor_window_factor;
    GlobalUtil::_NormalizedSIFT = normalized;
    GlobalUtil::_UseDynamicIndexing = dynamic_indexing;
}

// out = {launches, blocks, out-of-range 1D fetches, clamped 2D fetches} since the last reset.
void ref_stats(long* out) {
    out[0] = cuda_host::stats.launches;
    out[1] = cuda_host::stats.blocks;
    out[2] = cuda_host::stats.oob_fetches;
    out[3] = cuda_host::stats.clamped_2d;
}
void ref_reset_stats() { cuda_host::reset_stats(); }

// CreateFilterKernel: kernel[33], returns the width.
int ref_filter_kernel(float sigma, float* kernel) {
    int width = 0;
    ProgramCU::CreateFilterKernel(sigma, kernel, width);
    return width;
}

// FilterImage(dst, src, buf, sigma) on a w x h float image; returns the filter width.
int ref_filter(const float* src, int w, int h, float sigma, float* dst) {
    CuTexImage s, d, b;
    fill(s, w, h, 1, src);
    fill(d, w, h, 1, nullptr);
    fill(b, w, h, 1, nullptr);
    ProgramCU::FilterImage(&d, &s, &b, sigma);
    d.CopyToHost(dst);
    float k[33];
    return ref_filter_kernel(sigma, k);
}

void ref_sample_d(const float* src, int sw, int sh, int log_scale, float* dst, int dw, int dh) {
    CuTexImage s, d;
    fill(s, sw, sh, 1, src);
    fill(d, dw, dh, 1, nullptr);
    ProgramCU::SampleImageD(&d, &s, log_scale);
    d.CopyToHost(dst);
}

// dst is (w << log_scale) x (h << log_scale).
void ref_sample_u(const float* src, int w, int h, int log_scale, float* dst) {
    CuTexImage s, d;
    fill(s, w, h, 1, src);
    fill(d, w << log_scale, h << log_scale, 1, nullptr);
    ProgramCU::SampleImageU(&d, &s, log_scale);
    d.CopyToHost(dst);
}

// src: w x h x 4 floats.
void ref_reduce_channel(const float* src, int w, int h, int convert_rgb, float* dst) {
    CuTexImage s, d;
    fill(s, w, h, 4, src);
    fill_padded_dst(d, w, h);
    ProgramCU::ReduceToSingleChannel(&d, &s, convert_rgb);
    d.CopyToHost(dst);
}

void ref_byte_to_float(const uint8_t* src, int w, int h, float* dst) {
    CuTexImage s, d;
    fill_bytes(s, src, (size_t)w * h);
    s.SetImageSize(w, h);
    fill_padded_dst(d, w, h);
    ProgramCU::ConvertByteToFloat(&s, &d);
    d.CopyToHost(dst);
}

// ComputeDOG(gus, dog, got): gus[-1] = prev, gus[0] = cur; got (w x h x 2) may be null.
void ref_dog(const float* prev, const float* cur, int w, int h, float* dog, float* got) {
    CuTexImage gus[2], d, g;
    fill(gus[0], w, h, 1, prev);
    fill(gus[1], w, h, 1, cur);
    fill(d, w, h, 1, nullptr);
    if (got) fill(g, w, h, 2, nullptr);
    ProgramCU::ComputeDOG(gus + 1, &d, &g);
    d.CopyToHost(dog);
    if (got) g.CopyToHost(got);
}

// ComputeKEY on three DoG levels; key: w x h x 4, zero where the kernel stores nothing.
void ref_key(const float* dp, const float* dc, const float* dn, int w, int h, float tdog,
             float tedge, float* key) {
    CuTexImage dog[3], k;
    fill(dog[0], w, h, 1, dp);
    fill(dog[1], w, h, 1, dc);
    fill(dog[2], w, h, 1, dn);
    std::vector<float> zero((size_t)w * h * 4, 0.0f);
    fill(k, w, h, 4, zero.data());
    ProgramCU::ComputeKEY(dog + 1, &k, tdog, tedge);
    k.CopyToHost(key);
}

void ref_init_hist(const float* key, int ws, int h, int wd, int* hist) {
    CuTexImage k, t;
    fill(k, ws, h, 4, key);
    fill(t, wd, h, 4, nullptr);
    ProgramCU::InitHistogram(&k, &t);
    t.CopyToHost(hist);
}

void ref_reduce_hist(const int* hist1, int ws, int h, int wd, int* hist2) {
    CuTexImage a, b;
    fill(a, ws, h, 4, hist1);
    fill(b, wd, h, 4, nullptr);
    ProgramCU::ReduceHistogram(&a, &b);
    b.CopyToHost(hist2);
}

// One GenerateList step, in place on list (len x int4) against a histogram level hw x hh x int4.
void ref_gen_list(int* list, int len, const int* hist, int hw, int hh) {
    // ListGen_Kernel stores for every thread of its 128-wide blocks: the list gets whole blocks.
    CuTexImage l, t;
    const int padded_len = (len + 127) / 128 * 128;
    std::vector<int> padded((size_t)padded_len * 4, 0);
    memcpy(padded.data(), list, (size_t)len * 16);
    fill(l, padded_len, 1, 4, padded.data());
    l.SetImageSize(len, 1);
    fill(t, hw, hh, 4, hist);
    ProgramCU::GenerateList(&l, &t);
    l.CopyToHost(list);
}

// ComputeOrientation in place on list (len x 4: the int4 list, or float4 keys when existing).
void ref_orientation(void* list, int len, const float* got, const float* key, int w, int h,
                     float sigma, float sigma_step, int existing) {
    CuTexImage l, g, k;
    fill(l, len, 1, 4, list);
    fill(g, w, h, 2, got);
    if (key) fill(k, w, h, 4, key);
    ProgramCU::ComputeOrientation(&l, &g, &k, sigma, sigma_step, existing);
    l.CopyToHost(list);
}

// ComputeDescriptor for num keys (x, y, s, o) in octave coordinates; desc: num x 128.
void ref_descriptor(const float* keys, int num, const float* got, int w, int h, int rect,
                    float* desc) {
    CuTexImage l, g, d;
    fill(l, num, 1, 4, keys);
    fill(g, w, h, 2, got);
    ProgramCU::ComputeDescriptor(&l, &g, &d, rect);
    d.CopyToHost(desc);
}

// MultiplyDescriptor (or, with loc1, MultiplyDescriptorG) -> GetRowMatch -> GetColMatch (mbm).
// row: n1 ints, col: n2 ints (untouched without mbm); dot (n1 x n2) may be null.
void ref_match_stages(const uint8_t* d1, int n1, const uint8_t* d2, int n2, const float* loc1,
                      const float* loc2, const float* H, const float* F, float hdistmax,
                      float fdistmax, float distmax, float ratiomax, int mbm, int* row, int* col,
                      int* dot) {
    CuTexImage des[2], loc[2], tdot, tcrt, tmatch[2];
    fill(des[0], 8 * n1, 1, 4, d1);
    fill(des[1], 8 * n2, 1, 4, d2);
    if (loc1) {
        fill(loc[0], n1, 1, 2, loc1);
        fill(loc[1], n2, 1, 2, loc2);
        float h[3][3], f[3][3];
        memcpy(h, H, sizeof(h));
        memcpy(f, F, sizeof(f));
        ProgramCU::MultiplyDescriptorG(des, des + 1, loc, loc + 1, &tdot, mbm ? &tcrt : nullptr,
                                       h, hdistmax, f, fdistmax);
    } else {
        ProgramCU::MultiplyDescriptor(des, des + 1, &tdot, mbm ? &tcrt : nullptr);
    }
    if (dot) tdot.CopyToHost(dot);
    tmatch[0].InitTexture(n1, 1);
    ProgramCU::GetRowMatch(&tdot, tmatch, distmax, ratiomax);
    tmatch[0].CopyToHost(row);
    if (mbm) {
        tmatch[1].InitTexture(n2, 1);
        ProgramCU::GetColMatch(&tcrt, tmatch + 1, distmax, ratiomax);
        tmatch[1].CopyToHost(col);
    }
}

}  // extern "C"

#ifdef REF_DRIVER_MAIN
// A short fixed sequence of every stage, for a build with -fsanitize=address,undefined.
int main() {
    const int w = 131, h = 37;
    std::vector<float> img((size_t)w * h), a(img.size()), b(img.size()), c(img.size()), e(img.size());
    unsigned s = 12345;
    auto rnd = [&] { s = s * 1664525u + 1013904223u; return (s >> 8) / 16777216.0f; };
    for (auto& v : img) v = rnd();
    long st[4];
    auto report = [&](const char* stage) {
        ref_stats(st);
        printf("%-22s launches %ld blocks %ld out-of-range fetches %ld clamped 2D fetches %ld\n",
               stage, st[0], st[1], st[2], st[3]);
        ref_reset_stats();
    };
    ref_reset_stats();
    std::vector<uint8_t> bytes((size_t)w * h);
    for (auto& v : bytes) v = (uint8_t)(rnd() * 256);
    ref_byte_to_float(bytes.data(), w, h, a.data());
    report("ConvertByteToFloat");
    std::vector<float> rgba((size_t)w * h * 4);
    for (auto& v : rgba) v = rnd();
    ref_reduce_channel(rgba.data(), w, h, 1, a.data());
    ref_reduce_channel(rgba.data(), w, h, 0, a.data());
    report("ReduceToSingleChannel");
    std::vector<float> up((size_t)w * h * 4);
    ref_sample_u(img.data(), w, h, 1, up.data());
    report("SampleImageU");
    std::vector<float> dn((size_t)(w / 2) * (h / 2));
    ref_sample_d(img.data(), w, h, 1, dn.data(), w / 2, h / 2);
    report("SampleImageD");
    ref_filter(img.data(), w, h, 1.6f, a.data());
    ref_filter(a.data(), w, h, 1.2f, b.data());
    ref_filter(b.data(), w, h, 1.5f, c.data());
    ref_filter(c.data(), w, h, 1.9f, e.data());
    ref_filter(e.data(), w, h, 8.0f, img.data());   // width 33
    report("FilterImage");
    std::vector<float> d0(a.size()), d1(a.size()), d2(a.size()), got(a.size() * 2);
    ref_dog(a.data(), b.data(), w, h, d0.data(), nullptr);
    ref_dog(b.data(), c.data(), w, h, d1.data(), got.data());
    ref_dog(c.data(), e.data(), w, h, d2.data(), nullptr);
    report("ComputeDOG");
    std::vector<float> key(a.size() * 4);
    ref_key(d0.data(), d1.data(), d2.data(), w, h, 0.0001f, 10.0f, key.data());
    report("ComputeKEY");
    const int w1 = (w + 3) / 4, w2 = (w1 + 3) / 4, w3 = (w2 + 3) / 4;
    std::vector<int> h1((size_t)w1 * h * 4), h2((size_t)w2 * h * 4), h3((size_t)w3 * h * 4);
    ref_init_hist(key.data(), w, h, w1, h1.data());
    report("InitHistogram");
    ref_reduce_hist(h1.data(), w1, h, w2, h2.data());
    ref_reduce_hist(h2.data(), w2, h, w3, h3.data());
    report("ReduceHistogram");
    std::vector<int> list;
    for (int i = 0; i < h * 4 * w3; i++)
        for (int j = 0; j < h3[i]; j++) {
            const int entry[4] = {i % (4 * w3), i / (4 * w3), j, 0};
            list.insert(list.end(), entry, entry + 4);
        }
    const int len = (int)list.size() / 4;
    printf("candidates %d\n", len);
    if (len > 0) {
        ref_gen_list(list.data(), len, h2.data(), w2, h);
        ref_gen_list(list.data(), len, h1.data(), w1, h);
        report("GenerateList");
        ref_orientation(list.data(), len, got.data(), key.data(), w, h, 2.0f, 1.26f, 0);
        report("ComputeOrientation");
        std::vector<float> keys(list.size());
        memcpy(keys.data(), list.data(), keys.size() * 4);
        for (int i = 0; i < len; i++) keys[4 * i + 3] = 0.1f * i;
        std::vector<float> desc((size_t)len * 128);
        ref_descriptor(keys.data(), len, got.data(), w, h, 0, desc.data());
        ref_settings(1, 2, 0, 0, 4.0f, 1.5f, 2.0f, 3.0f, 0, 0);
        ref_descriptor(keys.data(), len, got.data(), w, h, 0, desc.data());
        for (int i = 0; i < len; i++) keys[4 * i + 2] = keys[4 * i + 3] = 12.0f;
        ref_descriptor(keys.data(), len, got.data(), w, h, 1, desc.data());
        report("ComputeDescriptor");
    }
    const int n1 = 13, n2 = 150;
    std::vector<uint8_t> q1((size_t)n1 * 128), q2((size_t)n2 * 128);
    for (auto& v : q1) v = (uint8_t)(rnd() * 90);
    for (auto& v : q2) v = (uint8_t)(rnd() * 90);
    std::vector<int> row(n1), col(n2), dot((size_t)n1 * n2);
    ref_match_stages(q1.data(), n1, q2.data(), n2, nullptr, nullptr, nullptr, nullptr, 0, 0, 0.7f,
                     0.8f, 1, row.data(), col.data(), dot.data());
    report("match");
    std::vector<float> l1(n1 * 2), l2(n2 * 2);
    for (auto& v : l1) v = rnd() * 100;
    for (auto& v : l2) v = rnd() * 100;
    const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    ref_match_stages(q1.data(), n1, q2.data(), n2, l1.data(), l2.data(), I, I, 32.0f, 1e20f, 0.7f,
                     0.8f, 1, row.data(), col.data(), dot.data());
    report("guided match");
    return 0;
}
#endif
