// sift_select.h -- the selection rule of preemptive matching (sgpu_select_top_scale_*,
// sgpu_prematch_*): which rows of a feature set are its `top` largest-scale ones.
// Plain C++, no HIP: SGSEL_HD is `__host__ __device__` under hipcc and nothing under g++, so that
// the kernel (sift_select.hip) and a host-only program (tests/abi/select_check.cpp) share it.
//
// Rule.  A set has n rows with scales s[i]; m = min(n, top) rows are selected.  Rows are ordered by
// order_key(bits of s[i]), the monotone map of float bits to unsigned, largest first; equal keys
// resolve to the lower row index.  The selection is the first m rows of that order, reported as
// their row indices in ascending index order.  With T the m-th largest key and g the number of
// keys above T, that is: every row with key > T, plus the first m - g rows with key == T in index
// order.  order_key is a total order of all bit patterns, so the rule has no special case: for
// positive finite scales (every extracted key) it is the numeric order; for caller data -0 sorts
// below +0, negatives below both, +inf above every finite value and a NaN where its bits put it.
#ifndef SIFT_SELECT_H
#define SIFT_SELECT_H
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define SGSEL_HD __host__ __device__ inline
#else
#define SGSEL_HD inline
#endif

namespace sgsel {

// float bits -> unsigned, monotone: a set sign bit flips every bit, a clear one sets the sign bit
SGSEL_HD uint32_t order_key(uint32_t bits) {
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

// rows selected of a set of n
SGSEL_HD int selected(int64_t n, int top) { return (int)(n < (int64_t)top ? n : (int64_t)top); }

// The cut of a set: T and the number of rows with key == T that are taken (m - g).
struct Cut {
    uint32_t T;
    int quota;
};
// Does a row with this key belong to the selection?  eq_before = rows with key == T at lower
// indices.
SGSEL_HD bool takes(const Cut& c, uint32_t key, int eq_before) {
    return key > c.T || (key == c.T && eq_before < c.quota);
}

// One step of the most-significant-byte-first radix select, shared by the kernel and the host loop:
// hist[b] = rows whose key matches the prefix found so far and has byte b at `shift`; want = the
// rank still looked for among them (1 = the largest).  Returns the byte whose bin holds that rank
// and lowers *want by the rows in the bins above it.
inline int radix_bin(const int* hist, int* want) {
    int above = 0;
    for (int b = 255; b > 0; b--) {
        if (above + hist[b] >= *want) {
            *want -= above;
            return b;
        }
        above += hist[b];
    }
    *want -= above;
    return 0;
}

inline uint32_t scale_key(const float* scale, int stride, int64_t i) {
    uint32_t bits;
    memcpy(&bits, scale + i * (int64_t)stride, sizeof(bits));
    return order_key(bits);
}

// The cut of rows scale[0], scale[stride], ... (n > top >= 1), by the four radix passes the kernel
// runs.
inline Cut cut_host(const float* scale, int stride, int n, int top) {
    uint32_t prefix = 0, mask = 0;
    int want = top;
    for (int shift = 24; shift >= 0; shift -= 8) {
        int hist[256] = {};
        for (int i = 0; i < n; i++) {
            const uint32_t k = scale_key(scale, stride, i);
            if ((k & mask) == prefix) hist[(k >> shift) & 255]++;
        }
        const int b = radix_bin(hist, &want);
        prefix |= (uint32_t)b << shift;
        mask |= 255u << shift;
    }
    return Cut{prefix, want};
}

// The reference loop of the rule: out[0 .. m) = the selected row indices of a set of n rows,
// ascending; returns m = min(n, top) (0 for n <= 0 or top <= 0).
inline int select_host(const float* scale, int stride, int n, int top, int* out) {
    if (n <= 0 || top <= 0) return 0;
    if (n <= top) {
        for (int i = 0; i < n; i++) out[i] = i;
        return n;
    }
    const Cut c = cut_host(scale, stride, n, top);
    int eq = 0, m = 0;
    for (int i = 0; i < n; i++) {
        const uint32_t k = scale_key(scale, stride, i);
        if (takes(c, k, eq)) out[m++] = i;
        eq += k == c.T;
    }
    return m;
}

// sub[0 .. nsets] = the scan of min(n_s, top): where set s's selection starts in the compact
// buffers.  off must be validated (non-negative, non-decreasing).
inline void subset_offsets(const int64_t* off, int nsets, int top, std::vector<int64_t>& sub) {
    sub.assign((size_t)nsets + 1, 0);
    for (int s = 0; s < nsets; s++) sub[s + 1] = sub[s] + selected(off[s + 1] - off[s], top);
}

}  // namespace sgsel
#endif  // SIFT_SELECT_H
