// sift_device.h -- device-side helpers that more than one of the stage files (sift_level.hip,
// sift_detect.hip, sift_orient.hip, sift_kernels.hip) use, and the two occupancy queries that
// feature_queue_grids puts together.  Internal: a helper that one stage alone uses lives in that
// stage's file.
#pragma once
#include "sift_kernels.h"
#include "sift_math.h"

using namespace sgm;

namespace sgk {

// Resident workgroups per compute unit of the work-counter kernels, each asked
// of the file that holds the kernel: k_orientation_queue (sift_orient.hip), and
// k_descriptor_queue<1> / <2> (sift_kernels.hip).
hipError_t orientation_queue_occupancy(int* blocks);
hipError_t descriptor_queue_occupancy(int* blocks_one_wave, int* blocks_two_waves);

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// a float pair: its fma is one v_pk_fma_f32 (gfx950 issues packed FP32 at twice the scalar rate)
typedef float f2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f2v pk_fma(f2v a, float b, f2v c) {
    return __builtin_elementwise_fma(a, f2v{b, b}, c);
}

// XCD-aware block order: blocks are dealt round-robin over the 8 XCDs (observed placement,
// MI355X_MICROARCH.md; speed only, never correctness), so logical block xcd * q + k runs on XCD
// xcd and a run of consecutive logical blocks -- neighbouring image regions -- shares one L2.
__device__ __forceinline__ int xcd_block(int bid, int nb) {
    const int q = nb / 8, r = nb % 8, xcd = bid % 8, k = bid / 8;
    return xcd < r ? xcd * (q + 1) + k : r * (q + 1) + (xcd - r) * q + k;
}

// Grouped XCD order: G logically consecutive workgroups on one XCD, dispatched within 8 G slots
// of each other (workgroup b runs on XCD b % 8), the groups in dispatch order -- locality for
// neighbours without xcd_block's partition of the whole grid into 8 contiguous ranges (which
// leaves XCDs idle when the work per workgroup changes along the grid).  The last partial round
// of 8 G keeps the identity.
template <int G>
__device__ __forceinline__ int xcd_group(int bid, int nb) {
    const int full = nb / (8 * G) * (8 * G);
    if (bid >= full) return bid;
    const int m = bid / (8 * G), r = bid % (8 * G);
    return m * (8 * G) + (r % 8) * G + r / 8;
}

// words 4 q .. 4 q + 3 of the n-word buffer p to zero (one 16-byte store; the tail word by word)
__device__ __forceinline__ void zero_words(uint32_t* p, size_t n, size_t q) {
    if (q * 4 + 4 <= n) {
        *reinterpret_cast<uint4*>(p + q * 4) = make_uint4(0, 0, 0, 0);
    } else {
        for (size_t i = q * 4; i < n; i++) p[i] = 0;
    }
}

// Quad (4-lane) broadcast of lane S through DPP quad_perm [S,S,S,S]: no LDS traffic.
template <int S>
__device__ __forceinline__ int qbcast(int v) {
    return __builtin_amdgcn_mov_dpp(v, S * 0x55, 0xF, 0xF, false);
}
template <int S>
__device__ __forceinline__ float qbcastf(float v) {
    return as_float((uint32_t)qbcast<S>((int)as_uint(v)));
}

// A wave's walk over the units of a feature stage.  The wave's first unit is its
// own index in the grid, without a counter access (a whole grid asking a counter at the launch is
// served one wave after the other: 60-90 us for a resident grid); every further one comes from a
// work counter.  kQueueCounters counters, kQueueStride words apart, share the units past the
// grid's first ones: counter k hands out units nwaves + k, nwaves + k + kQueueCounters, ... to
// the waves whose index is k mod kQueueCounters (same-address atomics are served one at a time
// by the memory side, ~11.5 ns each: one counter for 2 x 10^5 features takes longer than the
// features; interleaved, the counters hold equal shares of the work, so no wave needs another's
// counter).  In two steps, so that a kernel can ask for its next unit before the end of the
// current one and have the counter's round trip run beside the rest of it: queue_ask returns
// lane 0's ticket, queue_unit turns it into the wave's next unit.
// (Relaxed: the counters order nothing, every unit is computed from buffers that earlier
// launches finished.)
__device__ __forceinline__ uint32_t queue_ask(uint32_t* next, uint32_t wave) {
    uint32_t i = 0;
    if ((threadIdx.x & 63) == 0)
        i = __hip_atomic_fetch_add(next + (wave % kQueueCounters) * kQueueStride, 1u,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return i;
}
__device__ __forceinline__ uint32_t queue_unit(uint32_t ticket, uint32_t wave, uint32_t nwaves) {
    return nwaves + __builtin_amdgcn_readfirstlane(ticket) * kQueueCounters + wave % kQueueCounters;
}

}  // namespace

}  // namespace sgk
