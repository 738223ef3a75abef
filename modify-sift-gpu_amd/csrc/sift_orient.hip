// sift_orient.hip -- keypoint orientation and feature expansion (gfx950 / MI355X).
//
// Reference semantics: SiftGPU/ProgramCU.cu (ComputeOrientation_Kernel) and SiftGPU/PyramidCU.cpp
// (ReshapeFeatureListCPU, DownloadKeypoints).  MI355X-first, not a translation (sift_kernels.h):
// gradient images are never stored, the orientation kernels evaluate gradients from the Gaussian
// level on the fly, and a candidate finds its (image, octave, level, row, column) from the row
// scan and the keypoint mask (sift_keys.h) without a host round trip.
// Floating-point conventions are those of oracle/sift_oracle.cpp (fma contractions written
// out, transcendentals from sift_math.h); the build uses -ffp-contract=off.
#include <algorithm>

#include "sift_device.h"
#include "sift_keys.h"

namespace sgk {
namespace {

// Row-major walk of a window of ncols columns, advanced 4 samples at a time (one per quad lane).
struct Walk {
    int r, c;
    __device__ __forceinline__ void init(int i, int ncols) { r = i / ncols; c = i - r * ncols; }
    __device__ __forceinline__ void step(int ncols) {
        c += 4;
        while (c >= ncols) { c -= ncols; r++; }
    }
};

// ComputeOrientation_Kernel (ProgramCU.cu:813-977).  One quad (4 lanes) per keypoint: the
// lanes evaluate consecutive window samples (gradient, Gaussian weight, bin) in parallel and
// every lane then applies the quad's 4 votes in the reference's (y, x) order to the keypoint's
// 36-bin histogram in LDS, so each bin sees exactly the reference's sequence of float adds.
// Orientation histogram of ComputeOrientation_Kernel (ProgramCU.cu:857-903) for a keypoint
// (kx, ky, kz) of Gaussian level g (W x H): the quad's 4 lanes evaluate consecutive window
// samples and every lane applies the 4 votes in the reference's (y, x) order to the 36-bin LDS
// histogram; returns the 6-times smoothed histogram in vote[0..36] (vote[36] = vote[0]).
__device__ __forceinline__ void orientation_hist(const float* __restrict__ g, int W, int H,
                                                 float kx, float ky, float kz,
                                                 const FeatureParams& fp, int sub, float* vote_l,
                                                 float (&vote)[37]) {
    const float ten_degree_per_radius = (float)5.7295779513082320876798154814105;
    const float gsigma = kz * fp.gaussian_factor;
    const float win = fabs_(kz) * fp.sample_factor;
    const float dist_threshold = (float)((double)(win * win) + 0.5);
    const float factor = -0.5f / (gsigma * gsigma);
    const float xmin = fmax_(1.5f, floor_(kx - win) + 0.5f);
    const float ymin = fmax_(1.5f, floor_(ky - win) + 0.5f);
    const float xmax = fmin_(W - 1.5f, floor_(kx + win) + 0.5f);
    const float ymax = fmin_(H - 1.5f, floor_(ky + win) + 0.5f);
    for (int i = sub; i < 36; i += 4) vote_l[i] = 0.0f;
    const int ncols = xmax >= xmin ? (int)(xmax - xmin) + 1 : 0;
    const int nrows = ymax >= ymin ? (int)(ymax - ymin) + 1 : 0;
    const int total = ncols * nrows;
    // The 4 gradient neighbours of this lane's next sample are loaded one iteration ahead
    // (unconditionally: past the window's end a lane reads the window's first pixel), so a
    // sample's gathers overlap the previous sample's votes instead of starting after them.
    // Same values and the same arithmetic as grad_at.
    Walk wk;
    float nl = 0.f, nr = 0.f, nu = 0.f, nd = 0.f;
    const int x_safe = (int)xmin, y_safe = (int)ymin;
    auto fetch = [&](const Walk& w, bool ok) {
        const int x = ok ? (int)(xmin + (float)w.c) : x_safe;
        const int y = ok ? (int)(ymin + (float)w.r) : y_safe;
        const float* p = g + (long long)y * W + x;
        nl = p[-1];
        nr = p[1];
        nu = p[-W];
        nd = p[W];
    };
    if (total > 0) {
        wk.init(sub, ncols);
        fetch(wk, sub < total);
    }
    for (int base = 0; base < total; base += 4) {
        // this lane's sample: index base + sub
        const bool valid = base + sub < total;
        const float pl = nl, pr = nr, pu = nu, pd = nd;
        const float x = xmin + (float)wk.c, y = ymin + (float)wk.r;
        if (valid) wk.step(ncols);
        fetch(wk, base + 4 + sub < total);
        int bin = -1;
        float weight = 0.0f;
        if (valid) {
            const float dx = x - kx, dy = y - ky;
            const float sq = fma_(dx, dx, dy * dy);
            if (!(fp.circular && sq >= dist_threshold)) {
                const float gdx = pr - pl, gdy = pd - pu;   // grad_at (ProgramCU.cu:495-502)
                const float grd = 0.5f * sqrt_(fma_(gdx, gdx, gdy * gdy));
                const float rot = grd == 0.0f ? 0.0f : atan2_(gdy, gdx);
                weight = grd * exp_(sq * factor);
                bin = (int)floor_(rot * ten_degree_per_radius);
                if (bin < 0) bin += 36;
            }
        }
        // apply the 4 votes in sample order: lane 0 of the quad issues them as LDS float adds
        // (ds_add_f32, IEEE round-to-nearest like the VALU add), which the LDS performs in issue
        // order -- each bin sees the reference's sequence of adds, and no read-modify-write
        // round trip sits between one group of samples and the next
        const int b0 = qbcast<0>(bin), b1 = qbcast<1>(bin), b2 = qbcast<2>(bin), b3 = qbcast<3>(bin);
        const float w0 = qbcastf<0>(weight), w1 = qbcastf<1>(weight), w2 = qbcastf<2>(weight),
                    w3 = qbcastf<3>(weight);
        if (sub == 0) {
            auto add = [&](int bb, float ww) {
                __hip_atomic_fetch_add(&vote_l[bb], ww, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
            };
            if (b0 >= 0) add(b0, w0);
            if (b1 >= 0) add(b1, w1);
            if (b2 >= 0) add(b2, w2);
            if (b3 >= 0) add(b3, w3);
        }
    }
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < 36; ++i) vote[i] = vote_l[i];
    const float one_third = (float)(1.0 / 3.0);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        vote[36] = vote[0];
        float pre = vote[35];
#pragma unroll
        for (int j = 0; j < 36; ++j) {
            const float temp = one_third * (pre + vote[j] + vote[j + 1]);
            pre = vote[j];
            vote[j] = temp;
        }
    }
    vote[36] = vote[0];
}

// The strongest orientation (ProgramCU.cu:904-919: num_orientation == 1 or a caller-supplied
// keypoint list), in radians of the reference's internal convention.
__device__ __forceinline__ float strongest_orientation(const float (&vote)[37]) {
    const float radius_per_ten_degrees = (float)(1.0 / 5.7295779513082320876798154814105);
    int index_max = 0;
    float max_vote = vote[0];
#pragma unroll
    for (int i = 1; i < 36; ++i) {
        index_max = vote[i] > max_vote ? i : index_max;
        max_vote = fmax_(max_vote, vote[i]);
    }
    float pre = vote[35], next = vote[1];
#pragma unroll
    for (int i = 1; i < 36; ++i)
        if (i == index_max) { pre = vote[i - 1]; next = vote[i + 1]; }
    const float off = 0.5f * ((next - pre) * (1.0f / (max_vote + max_vote - next - pre)));
    return radius_per_ten_degrees * (index_max + 0.5f + off);
}

// Keypoint of candidate f in octave coordinates (ComputeOrientation_Kernel's key, ProgramCU.cu:
// 838-851) and its info record; false when no orientation is computed (num_orientation == 0:
// the keypoint is written with orientation 0 here).
struct OriKey { float kx, ky, kz; const float* g; int W, H; };
// locate() by a whole wave (the one-wave-per-candidate orientation form): the same (image,
// octave, level, row, column) from 3 dependent loads instead of ~13 binary-search steps plus a
// serial scan over the mask row's words (up to 60 for a 1080p row) -- the latency chain of a
// single image's orientation launch.
//   * row: a 64-ary search for the last row whose scanned base is <= f -- the lanes probe 64
//     evenly spaced rows of the remaining range, the highest lane whose probe passes narrows it;
//   * column: lane l loads mask word l (64 at a time), a wave prefix sum of their popcounts picks
//     the word holding the k-th set bit, that lane finds the bit.
__device__ __forceinline__ KeyLoc locate_wave(uint32_t f, int lane, const uint32_t* __restrict__ row_base,
                                              int total_rows, const uint32_t* __restrict__ mask,
                                              const FeatureParams& fp) {
    int lo = 0, n = total_rows;   // the answer lies in [lo, lo + n); row_base[lo] <= f
    uint32_t base_lo = 0;         // row_base[lo] (row_base[0] = 0)
    while (n > 1) {
        const int step = (n + 63) / 64;
        const int i = lo + lane * step;
        const bool in = lane * step < n;
        const uint32_t v = in ? row_base[i] : 0xffffffffu;
        const unsigned long long bal = __ballot(in && v <= f);   // lane 0 always passes
        const int k = 63 - __clzll(bal);
        base_lo = (uint32_t)__builtin_amdgcn_readlane((int)v, k);
        const int end = lo + n;
        lo += k * step;
        n = min(step, end - lo);
    }
    KeyLoc L = row_loc(lo, fp);
    uint32_t k = f - base_lo;
    const OctaveDesc& od = fp.oct[L.o];
    const uint32_t* mrow = mask + od.mask_off + L.j * od.mask_level_stride +
                           ((long long)L.b * od.h + L.row) * od.nwords;
    int col = 0;
    for (int w0 = 0; w0 < od.nwords; w0 += 64) {
        const int w = w0 + lane;
        uint32_t m = w < od.nwords ? mrow[w] : 0u;
        const int c = __popc(m);
        int incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(incl, d, 64);
            if (lane >= d) incl += u;
        }
        const int excl = incl - c;
        const unsigned long long hit = __ballot((uint32_t)excl <= k && k < (uint32_t)incl);
        if (hit) {
            const int hl = __ffsll((long long)hit) - 1;
            for (uint32_t q = 0; q < k - (uint32_t)excl && lane == hl; q++) m &= m - 1;
            col = __builtin_amdgcn_readlane(w * 32 + (__ffs(m) - 1), hl);
            break;
        }
        k -= (uint32_t)__builtin_amdgcn_readlane(incl, 63);
    }
    L.col = col;
    return L;
}

__device__ __forceinline__ bool orientation_key(uint32_t f, bool writer,
                                                const float* __restrict__ pyr,
                                                const uint32_t* __restrict__ mask,
                                                const uint32_t* __restrict__ row_base,
                                                int total_rows, const FeatureParams& fp,
                                                float4* __restrict__ out4,
                                                int2* __restrict__ info,
                                                uint32_t* __restrict__ ocount, OriKey& K,
                                                int wave_lane = -1) {
    // wave_lane >= 0: called by a whole wave for one candidate (locate_wave), else per lane
    const KeyLoc L = wave_lane >= 0 ? locate_wave(f, wave_lane, row_base, total_rows, mask, fp)
                                    : locate(f, row_base, total_rows, mask, fp);
    const KeyOut kv = key_at(pyr, fp, L);
    const OctaveDesc& od = fp.oct[L.o];

    float kx = L.col + 0.5f, ky = L.row + 0.5f, kz = fp.level_sigma[L.j];
    if (fp.subpixel) {
        kx += kv.dx;
        ky += kv.dy;
        kz *= pow_(fp.sigma_step, kv.ds);
    }
    if (fp.keep_sign) kz *= kv.result;
    if (writer) info[f] = make_int2(L.b, L.o * fp.d + L.j);
    if (fp.num_orientation == 0) {
        if (writer) {
            out4[f] = make_float4(kx, ky, kz, 0.0f);
            ocount[f] = 1;
        }
        return false;
    }
    // gradient of Gaussian level 1 + j (PyramidCU.cpp:1204)
    K.g = pyr + od.gauss_off + (long long)(1 + L.j) * od.level_stride + (long long)L.b * od.wa * od.h;
    K.W = od.wa;
    K.H = od.h;
    K.kx = kx;
    K.ky = ky;
    K.kz = kz;
    return true;
}

// Peaks of the smoothed histogram (ProgramCU.cu:904-977) -> the keypoint with its one or two
// orientations packed as u16 fractions of 2 pi, and the feature count it expands to
// (ReshapeFeatureListCPU, PyramidCU.cpp:560-578: drop "no orientation", keep a distinct second).
__device__ __forceinline__ void orientation_finish(uint32_t f, const float (&vote)[37],
                                                   const OriKey& K, const FeatureParams& fp,
                                                   float4* __restrict__ out4,
                                                   uint32_t* __restrict__ ocount) {
    if (fp.num_orientation == 1) {
        out4[f] = make_float4(K.kx, K.ky, K.kz, strongest_orientation(vote));
        ocount[f] = 1;
        return;
    }
    float max_vote = vote[0];
#pragma unroll
    for (int i = 1; i < 36; ++i) max_vote = fmax_(max_vote, vote[i]);
    const float vote_threshold = max_vote * 0.8f;
    float pre = vote[35];
    float rot0 = 0.f, rot1 = 0.f, vot0 = 0.f, vot1 = 0.f;
    int ocnt = 0;
#pragma unroll
    for (int i = 0; i < 36; ++i) {
        const float next = vote[i + 1];
        const float vi = vote[i];
        if (vi > vote_threshold && vi > pre && vi > next) {
            const float di = 0.5f * ((next - pre) * (1.0f / (vi + vi - next - pre)));
            const float rot = i + di + 0.5f;
            if (vi > vot1) {
                if (vi > vot0) { vot1 = vot0; rot1 = rot0; vot0 = vi; rot0 = rot; }
                else { vot1 = vi; rot1 = rot; }
                ocnt++;
            }
        }
        pre = vi;
    }
    float fr1 = rot0 / 36.0f;
    if (fr1 < 0) fr1 += 1.0f;
    const uint32_t us1 = ocnt == 0 ? 65535u : (uint32_t)(unsigned short)floor_(fr1 * 65535.0f);
    uint32_t us2 = 65535u;
    if (ocnt > 1) {
        float fr2 = rot1 / 36.0f;
        if (fr2 < 0) fr2 += 1.0f;
        us2 = (uint32_t)(unsigned short)floor_(fr2 * 65535.0f);
    }
    out4[f] = make_float4(K.kx, K.ky, K.kz, as_float((us2 << 16) | us1));
    ocount[f] = us1 == 65535u ? 0u : (1u + ((us2 != 65535u && us2 != us1) ? 1u : 0u));
}

__device__ __forceinline__ void orientation_one(uint32_t f, int sub, float* vote_l,
                                                const float* __restrict__ pyr,
                                                const uint32_t* __restrict__ mask,
                                                const uint32_t* __restrict__ row_base,
                                                int total_rows, const FeatureParams& fp,
                                                float4* __restrict__ out4,
                                                int2* __restrict__ info,
                                                uint32_t* __restrict__ ocount) {
    OriKey K;
    if (!orientation_key(f, sub == 0, pyr, mask, row_base, total_rows, fp, out4, info, ocount, K))
        return;
    float vote[37];
    orientation_hist(K.g, K.W, K.H, K.kx, K.ky, K.kz, fp, sub, vote_l, vote);
    if (sub != 0) return;
    orientation_finish(f, vote, K, fp, out4, ocount);
}

// The histogram of orientation_hist evaluated by a whole wave, for few candidates (a single
// image: ~1,500 candidates leave most SIMDs idle under the quad form, and each quad walks its
// window serially): 64 window samples at a time are evaluated in parallel, then lane b < 36
// adds the batch's votes for bin b in sample order.  Each bin sees the reference's sequence of
// float adds (the other samples add nothing: acc + 0.0f = acc, acc >= +0), so the histogram is
// orientation_hist's bit for bit.  Same window, sample arithmetic and smoothing.
__device__ __forceinline__ void orientation_hist_wave(const OriKey& K, const FeatureParams& fp,
                                                      int lane, float* s_v, float2* s_bw,
                                                      float (&vote)[37]) {
    const float ten_degree_per_radius = (float)5.7295779513082320876798154814105;
    const float gsigma = K.kz * fp.gaussian_factor;
    const float win = fabs_(K.kz) * fp.sample_factor;
    const float dist_threshold = (float)((double)(win * win) + 0.5);
    const float factor = -0.5f / (gsigma * gsigma);
    const float xmin = fmax_(1.5f, floor_(K.kx - win) + 0.5f);
    const float ymin = fmax_(1.5f, floor_(K.ky - win) + 0.5f);
    const float xmax = fmin_(K.W - 1.5f, floor_(K.kx + win) + 0.5f);
    const float ymax = fmin_(K.H - 1.5f, floor_(K.ky + win) + 0.5f);
    const int ncols = xmax >= xmin ? (int)(xmax - xmin) + 1 : 0;
    const int nrows = ymax >= ymin ? (int)(ymax - ymin) + 1 : 0;
    const int total = ncols * nrows;
    float acc = 0.0f;   // bin `lane`
    // sample base + lane: its pixel and the 4 gradient neighbours, fetched one batch ahead (the
    // loads are unconditional, at a clamped in-plane pixel, so the compiler waits only for the
    // batch it uses); `in` = inside the window and the circle
    struct Smp { float x, y, sq, a, b, c, d; bool in; };
    auto fetch = [&](int base, Smp& q) {
        const int sidx = base + lane;
        const bool valid = sidx < total;
        const int si = valid ? sidx : 0;
        const int r = si / max(ncols, 1), c = si - r * max(ncols, 1);
        q.x = xmin + (float)c;
        q.y = ymin + (float)r;
        const float dx = q.x - K.kx, dy = q.y - K.ky;
        q.sq = fma_(dx, dx, dy * dy);
        q.in = valid && total > 0 && !(fp.circular && q.sq >= dist_threshold);
        const int px = q.in ? (int)q.x : 1, py = q.in ? (int)q.y : 1;   // (1, 1): in-plane
        const float* p = K.g + (long long)py * K.W + px;
        q.a = p[1];
        q.b = p[-1];
        q.c = p[K.W];
        q.d = p[-K.W];
    };
    Smp cur, nxt;
    fetch(0, cur);
    for (int base = 0; base < total; base += 64) {
        fetch(base + 64, nxt);
        int bin = -1;
        float weight = 0.0f;
        if (cur.in) {
            const float gdx = cur.a - cur.b, gdy = cur.c - cur.d;   // grad_at
            const float grd = 0.5f * sqrt_(fma_(gdx, gdx, gdy * gdy));
            const float rot = grd == 0.0f ? 0.0f : atan2_(gdy, gdx);
            weight = grd * exp_(cur.sq * factor);
            bin = (int)floor_(rot * ten_degree_per_radius);
            if (bin < 0) bin += 36;
        }
        // the batch's (bin, weight) pairs through the wave's LDS (every lane writes one: samples
        // past the window have bin -1), read back as broadcasts of 4 pairs; lane b adds the
        // weights of bin b in sample order (the others add +0, which leaves acc >= +0 unchanged)
        const int nb = min(64, total - base);   // uniform
        s_bw[lane] = make_float2(__int_as_float(bin), weight);
        asm volatile("" ::: "memory");   // one wave: its LDS writes complete before its reads
        for (int k = 0; k < nb; k += 4) {
            const float4 q0 = *reinterpret_cast<const float4*>(&s_bw[k]);
            const float4 q1 = *reinterpret_cast<const float4*>(&s_bw[k + 2]);
            acc += __float_as_int(q0.x) == lane ? q0.y : 0.0f;
            acc += __float_as_int(q0.z) == lane ? q0.w : 0.0f;
            acc += __float_as_int(q1.x) == lane ? q1.y : 0.0f;
            acc += __float_as_int(q1.z) == lane ? q1.w : 0.0f;
        }
        asm volatile("" ::: "memory");   // read before the next batch overwrites them
        cur = nxt;
    }
    // the 6 smoothing passes, a bin per lane: each pass is a stencil over the previous pass's
    // values, (pre + vote[j]) + vote[j + 1] as the serial form, the ring through the wave's LDS
    const float one_third = (float)(1.0 / 3.0);
    const int jm = lane == 0 ? 35 : lane - 1, jp = lane == 35 ? 0 : lane + 1;
    float v = acc;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        if (lane < 36) s_v[lane] = v;
        asm volatile("" ::: "memory");   // one wave: its LDS writes complete before its reads
        const float pre = s_v[min(jm, 35)], nx = s_v[min(jp, 35)];
        asm volatile("" ::: "memory");
        v = one_third * (pre + v + nx);
    }
    if (lane < 36) s_v[lane] = v;
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < 36; ++i) vote[i] = s_v[i];
    asm volatile("" ::: "memory");
    vote[36] = vote[0];
}

// One wave per candidate, grid-stride (the few-candidates form of k_orientation; same outputs).
__global__ __launch_bounds__(256) void k_orientation_wave(const float* __restrict__ pyr,
                                                          const uint32_t* __restrict__ mask,
                                                          const uint32_t* __restrict__ row_base,
                                                          int total_rows,
                                                          const uint32_t* __restrict__ n_cand_dev,
                                                          uint32_t cap, const FeatureParams fp,
                                                          float4* __restrict__ out4,
                                                          int2* __restrict__ info,
                                                          uint32_t* __restrict__ ocount) {
    __shared__ float s_vote[4][64];
    __shared__ __attribute__((aligned(16))) float2 s_pair[4][64];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t n = min(*n_cand_dev, cap);
    for (uint32_t f = blockIdx.x * 4 + wave; f < n; f += gridDim.x * 4) {   // uniform per wave
        OriKey K;
        if (!orientation_key(f, lane == 0, pyr, mask, row_base, total_rows, fp, out4, info,
                             ocount, K, lane))
            continue;
        float vote[37];
        orientation_hist_wave(K, fp, lane, s_vote[wave], s_pair[wave], vote);
        if (lane == 0) orientation_finish(f, vote, K, fp, out4, ocount);
        asm volatile("" ::: "memory");   // the next candidate's votes overwrite s_vote after
    }
}

// Grid-stride over the candidates (the grid is sized from the buffer capacity, the count is
// read on the device, so no host round trip sits between detection and orientation).
__global__ __launch_bounds__(256) void k_orientation(const float* __restrict__ pyr,
                                                     const uint32_t* __restrict__ mask,
                                                     const uint32_t* __restrict__ row_base,
                                                     int total_rows,
                                                     const uint32_t* __restrict__ n_cand_dev,
                                                     uint32_t cap, const FeatureParams fp,
                                                     float4* __restrict__ out4,
                                                     int2* __restrict__ info,
                                                     uint32_t* __restrict__ ocount) {
    __shared__ float s_vote[64 * 37];
    const int sub = threadIdx.x & 3, slot = threadIdx.x >> 2;
    const uint32_t n = min(*n_cand_dev, cap);
    float* vote_l = s_vote + slot * 37;
    for (uint32_t f = blockIdx.x * 64 + slot; f < n; f += gridDim.x * 64)   // uniform per quad
        orientation_one(f, sub, vote_l, pyr, mask, row_base, total_rows, fp, out4, info, ocount);
}

// k_orientation as resident one-wave workgroups fed from work counters: the
// grid is the number of waves the device holds at once, and each wave takes groups of 16
// candidates (a quad each, as above) until the candidates are used up, so a wave slot is
// refilled as soon as its own 16 candidates are done.  Candidate f is computed by the same code
// and written to the same slot as above.  The counters are zero at the launch; a surplus
// workgroup finds nothing to do and exits (no workgroup waits for another).
__global__ __launch_bounds__(64) void k_orientation_queue(const float* __restrict__ pyr,
                                                          const uint32_t* __restrict__ mask,
                                                          const uint32_t* __restrict__ row_base,
                                                          int total_rows,
                                                          const uint32_t* __restrict__ n_cand_dev,
                                                          uint32_t cap, const FeatureParams fp,
                                                          float4* __restrict__ out4,
                                                          int2* __restrict__ info,
                                                          uint32_t* __restrict__ ocount,
                                                          uint32_t* __restrict__ next) {
    __shared__ float s_vote[16 * 37];
    const int sub = threadIdx.x & 3, slot = threadIdx.x >> 2;
    const uint32_t n = min(*n_cand_dev, cap);
    const uint32_t groups = (n + 15) / 16;
    float* vote_l = s_vote + slot * 37;
    for (uint32_t g = blockIdx.x; g < groups;
         g = queue_unit(queue_ask(next, blockIdx.x), blockIdx.x, gridDim.x)) {
        const uint32_t f = 16 * g + slot;   // uniform per quad
        if (f < n)
            orientation_one(f, sub, vote_l, pyr, mask, row_base, total_rows, fp, out4, info, ocount);
    }
}

// ------------------------------------------------------------------------------------------
// Feature expansion + image coordinates (PyramidCU.cpp:521-606 / 701-751).
// (io.off != nullptr: the grid's last block writes the readback record instead -- off[0] = the
// candidate count, off[1 + b] = image b's first feature for b in [0, batch] -- which one more
// launch after the descriptors wrote before; a single image's extract pays per launch)
// Candidate f's 0, 1 or 2 features at slots e0 .. e0 + n - 1 (ReshapeFeatureListCPU,
// PyramidCU.cpp:560-578): the orientations unpacked, the image-coordinate keys
// (PyramidCU.cpp:701-751).
__device__ __forceinline__ void expand_one(uint32_t f, uint32_t e0, uint32_t n,
                                           const float4* __restrict__ cand,
                                           const int2* __restrict__ info, const FeatureParams& fp,
                                           float4* __restrict__ feat, int2* __restrict__ feat_info,
                                           float4* __restrict__ keys) {
    const float4 c = cand[f];
    const int2 in = info[f];
    const int o = in.y / fp.d;
    const float oss = ldexpf(1.0f, o + fp.octave_min);   // os * 2^o, os = 2^octave_min
    const double twopi = 2.0 * 3.14159265358979323846;
    float ang[2];
    if (fp.num_orientation >= 2) {
        const double factor = 2.0 * 3.14159265358979323846 / 65535.0;
        const uint32_t pk = as_uint(c.w);
        ang[0] = (float)(factor * (double)(pk & 0xffffu));
        ang[1] = (float)(factor * (double)(pk >> 16));
    } else {
        ang[0] = ang[1] = c.w;
    }
    for (uint32_t q = 0; q < n; q++) {
        const uint32_t e = e0 + q;
        feat[e] = make_float4(c.x, c.y, c.z, ang[q]);
        feat_info[e] = in;
        keys[e] = make_float4(oss * (c.x - 0.5f) + fp.origin_offset,
                              oss * (c.y - 0.5f) + fp.origin_offset, oss * c.z,
                              (float)fmod(twopi - (double)ang[q], twopi));
    }
}

__global__ __launch_bounds__(256) void k_expand(const float4* __restrict__ cand,
                                                const int2* __restrict__ info,
                                                const uint32_t* __restrict__ eoff,
                                                const uint32_t* __restrict__ n_cand_dev,
                                                const FeatureParams fp, float4* __restrict__ feat,
                                                int2* __restrict__ feat_info,
                                                float4* __restrict__ keys, uint32_t cap,
                                                const ImageOffsetsArgs io) {
    int nblk = (int)gridDim.x;
    if (io.off) {
        nblk--;
        if ((int)blockIdx.x == nblk) {
            for (int b = threadIdx.x; b <= io.batch + 1; b += 256) {
                if (b == 0) {
                    io.off[0] = (int64_t)io.row_base[io.total_rows];
                } else {
                    const int r = b - 1 == io.batch ? io.total_rows : (b - 1) * io.rows_per_image;
                    io.off[b] = (int64_t)eoff[min(io.row_base[r], cap)];
                }
            }
            return;
        }
    }
    const uint32_t ncand = min(*n_cand_dev, cap);
    for (uint32_t f = blockIdx.x * 256 + threadIdx.x; f < ncand; f += (uint32_t)nblk * 256) {
        const uint32_t e0 = eoff[f], n = eoff[f + 1] - e0;
        if (n != 0) expand_one(f, e0, n, cand, info, fp, feat, feat_info, keys);
    }
}

// Caller-supplied keypoints (SiftGPU::RunSIFT(num, keys, keys_have_orientation),
// SiftPyramid.cpp:83-89, 129-147, 167-177): feat holds the keypoint list in octave coordinates,
// grouped by level as GenerateFeatureListTex (PyramidCU.cpp:454-504) builds it.  The strongest
// orientation (ComputeOrientation_Kernel with existing_keypoint, ProgramCU.cu:830-833, 904)
// replaces feat.w, and the keys are rewritten in image coordinates at keys_out[index[e]]
// (DownloadKeypoints, PyramidCU.cpp:701-751).
__global__ __launch_bounds__(256) void k_orient_keys(const float* __restrict__ pyr,
                                                     float4* __restrict__ feat,
                                                     const int2* __restrict__ feat_info,
                                                     const int* __restrict__ index, int n,
                                                     const FeatureParams fp,
                                                     float4* __restrict__ keys_out) {
    __shared__ float s_vote[64 * 37];
    const int sub = threadIdx.x & 3, slot = threadIdx.x >> 2;
    float* vote_l = s_vote + slot * 37;
    const double twopi = 2.0 * 3.14159265358979323846;
    for (int e = blockIdx.x * 64 + slot; e < n; e += gridDim.x * 64) {   // uniform per quad
        const float4 k = feat[e];
        const int2 in = feat_info[e];
        const int o = in.y / fp.d, j = in.y - o * fp.d;
        const OctaveDesc& od = fp.oct[o];
        float angle = 0.0f;
        if (fp.num_orientation != 0) {
            const float* g = pyr + od.gauss_off + (long long)(1 + j) * od.level_stride +
                             (long long)in.x * od.wa * od.h;
            float vote[37];
            orientation_hist(g, od.wa, od.h, k.x, k.y, k.z, fp, sub, vote_l, vote);
            angle = strongest_orientation(vote);
        }
        if (sub == 0) {
            feat[e].w = angle;
            const float os = ldexpf(1.0f, o + fp.octave_min);
            keys_out[index[e]] = make_float4(os * (k.x - 0.5f) + fp.origin_offset,
                                             os * (k.y - 0.5f) + fp.origin_offset, os * k.z,
                                             (float)fmod(twopi - (double)angle, twopi));
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------
hipError_t orientation_queue_occupancy(int* blocks) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, k_orientation_queue, 64, 0);
}

hipError_t feature_queue_grids(FeatureQueue* q) {
    int dev = 0, cus = 0, ori = 0, d1 = 0, d2 = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess) e = orientation_queue_occupancy(&ori);
    if (e == hipSuccess) e = descriptor_queue_occupancy(&d1, &d2);
    if (e != hipSuccess) return e;
    if (cus <= 0 || ori <= 0 || d1 <= 0 || d2 <= 0) return hipErrorInvalidValue;
    // the descriptor in two-wave workgroups only where a compute unit holds more waves that way
    // (a limit on its workgroups, or the LDS allocation's granularity)
    q->desc_waves = 2 * d2 > d1 ? 2 : 1;
    q->ori_grid = ori * cus;
    q->desc_grid = (q->desc_waves == 2 ? d2 : d1) * cus;
    return hipSuccess;
}

hipError_t launch_orientation(const float* pyr, const uint32_t* mask, const uint32_t* row_base,
                              int total_rows, const uint32_t* n_cand_dev, int n_cand_cap,
                              int grid_hint, const FeatureParams& fp, float4* out4, int2* info,
                              uint32_t* ocount, hipStream_t stream, bool wave_per_candidate,
                              const FeatureQueue* queue) {
    if (n_cand_cap <= 0) return hipSuccess;
    if (queue && !wave_per_candidate) {
        if (!queue->next || queue->ori_grid <= 0) return hipErrorInvalidValue;
        // no more workgroups than groups of 16 the capacity holds (the rest would only exit), and
        // at least one wave per counter (a counter's units are taken by its own waves only)
        const long long groups = ((long long)n_cand_cap + 15) / 16;
        const unsigned grid = (unsigned)std::max<long long>(kQueueCounters, std::min<long long>(groups, queue->ori_grid));
        hipLaunchKernelGGL(k_orientation_queue, dim3(grid), dim3(64), 0, stream, pyr, mask,
                           row_base, total_rows, n_cand_dev, (uint32_t)n_cand_cap, fp, out4, info,
                           ocount, queue->next);
        return hipGetLastError();
    }
    if (wave_per_candidate) {
        const unsigned grid = (unsigned)std::max(1LL, std::min(((long long)grid_hint + 3) / 4, 8192LL));
        hipLaunchKernelGGL(k_orientation_wave, dim3(grid), dim3(256), 0, stream, pyr, mask,
                           row_base, total_rows, n_cand_dev, (uint32_t)n_cand_cap, fp, out4, info,
                           ocount);
        return hipGetLastError();
    }
    const unsigned grid = (unsigned)std::max(1LL, std::min(((long long)grid_hint + 63) / 64, 4096LL));
    hipLaunchKernelGGL(k_orientation, dim3(grid), dim3(256), 0, stream, pyr, mask, row_base,
                       total_rows, n_cand_dev, (uint32_t)n_cand_cap, fp, out4, info, ocount);
    return hipGetLastError();
}

hipError_t launch_expand(const float4* cand, const int2* info, const uint32_t* eoff,
                         const uint32_t* n_cand_dev, int n_cand_cap, const FeatureParams& fp,
                         float4* feat, int2* feat_info, float4* keys, hipStream_t stream,
                         const ImageOffsetsArgs* io) {
    if (n_cand_cap <= 0) return hipSuccess;
    const ImageOffsetsArgs none{};
    const unsigned grid = (unsigned)std::min(((long long)n_cand_cap + 255) / 256, 1024LL) +
                          (io && io->off ? 1u : 0u);
    hipLaunchKernelGGL(k_expand, dim3(grid), dim3(256), 0, stream, cand, info, eoff, n_cand_dev,
                       fp, feat, feat_info, keys, (uint32_t)n_cand_cap, io ? *io : none);
    return hipGetLastError();
}

hipError_t launch_orient_keys(const float* pyr, float4* feat, const int2* feat_info,
                              const int* index, int n, const FeatureParams& fp, float4* keys_out,
                              hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min((n + 63) / 64, 4096);
    hipLaunchKernelGGL(k_orient_keys, dim3(grid), dim3(256), 0, stream, pyr, feat, feat_info,
                       index, n, fp, keys_out);
    return hipGetLastError();
}

}  // namespace sgk
