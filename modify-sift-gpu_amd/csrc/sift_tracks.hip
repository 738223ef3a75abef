// sift_tracks.hip -- feature tracks from a pair list's matches (sgpu_tracks_*):
// the connected components of the match graph by a concurrent union-find, their grouping into
// row-ordered segments, the consistency test and the compaction into CSR.  The rule is
// sift_tracks.h's; the result is a pure function of the inputs although the union's and the
// scatter's orders are not: a component's root is its smallest row whatever the order of the
// hooks, sizes are integer sums, and every segment is ordered by row before anything reads it.
//
// k_tracks_init     parent[r] = r, size = fill = 0, the header's counters = 0.
// k_tracks_union    one work item per match: both rows' roots by path halving, the larger root
//                   hooked under the smaller by a compare-and-swap on its parent slot.
// k_tracks_label    label[r] = root of r (read only), size[label]++.
// k_tracks_mark     the roots' verdict from their size (sgtrk::classify): val[r] = the size of a
//                   candidate root, else 0; the statistics.  A scan of val gives the segments.
// k_tracks_scatter  every row of a candidate into its segment, in any order; out_track = -1 / -2
//                   for every other row.
// k_tracks_order    a wave per candidate: rank of every row among the segment's (<= nsets) rows,
//                   64 rows per step, and the row's successor; the segment is inconsistent when a
//                   successor lies in the row's own set.  Scans of the consistent candidates' sizes
//                   and flags give out_offsets and the track ids.
// k_tracks_finish   a wave per candidate: out_rows, out_offsets, out_track.
//
// Visibility.  The eight XCDs' L2 caches are not coherent within a kernel and a CU's L1 is not
// refreshed by another CU's stores, so in k_tracks_union every access to parent[] is an agent-scope
// atomic (loads and the halving's fetch-min bypass L1 and meet at the memory side; the CAS too).
// Every later kernel starts after the union's end and reads plain.
//
// Termination.  parent[x] <= x always (init; a hook writes the smaller root; halving writes an
// ancestor, and only ever lowers a slot).  A find steps from x to parent[x] < x, a retry of the hook
// continues from the value the CAS returned, below the root it failed on: every loop moves to a
// strictly smaller index or ends.  A step that would not is an invariant broken: it raises the
// call's error flag (hdr[kTracksHdrErr]) and leaves the loop.  No loop waits on another work item.
#include <algorithm>

#include "sift_kernels.h"
#include "sift_tracks.h"

namespace sgk {
namespace {

constexpr int kTrkThreads = 256;

#define SGK_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ int parent_load(int* parent, int x) {
    return __hip_atomic_load(parent + x, SGK_RLX_AGENT);
}

__device__ __forceinline__ void raise_error(int* hdr) { atomicOr(hdr + kTracksHdrErr, 1); }

// the root of x, halving the path on the way.  x strictly decreases from step to step.
__device__ int find_halving(int* parent, int x, int* hdr) {
    for (;;) {
        const int p = parent_load(parent, x);
        if (p == x) return x;
        if (p > x) {
            raise_error(hdr);
            return x;
        }
        const int g = parent_load(parent, p);
        if (g > p) {
            raise_error(hdr);
            return p;
        }
        if (g != p) __hip_atomic_fetch_min(parent + x, g, SGK_RLX_AGENT);   // an ancestor, lower than p
        x = g;   // g <= p < x
    }
}

__global__ __launch_bounds__(kTrkThreads) void k_tracks_init(int* __restrict__ parent,
                                                             uint32_t* __restrict__ size,
                                                             uint32_t* __restrict__ fill,
                                                             int* __restrict__ hdr, long long rows) {
    const long long r = (long long)blockIdx.x * kTrkThreads + threadIdx.x;
    if (r < kTracksHdrWords) hdr[r] = 0;
    if (r >= rows) return;
    parent[r] = (int)r;
    size[r] = 0u;
    fill[r] = 0u;
}

__global__ __launch_bounds__(kTrkThreads) void k_tracks_union(const long long* __restrict__ pair_start,
                                                              const int* __restrict__ pair_base,
                                                              int npairs,
                                                              const int* __restrict__ matches,
                                                              long long total, int* parent,
                                                              int* __restrict__ hdr) {
    const long long step = (long long)gridDim.x * kTrkThreads;
    for (long long e = (long long)blockIdx.x * kTrkThreads + threadIdx.x; e < total; e += step) {
        const int p = sgtrk::pair_of_match(pair_start, npairs, e);
        const int u = pair_base[2 * p] + matches[2 * e], v = pair_base[2 * p + 1] + matches[2 * e + 1];
        int ru = find_halving(parent, u, hdr), rv = find_halving(parent, v, hdr);
        // max(ru, rv) strictly decreases from turn to turn
        while (ru != rv) {
            const int hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
            int seen = hi;
            if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED,
                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                break;   // hooked: hi was a root
            if (seen >= hi) {   // a root's slot holds the root; anything else lies below it
                raise_error(hdr);
                break;
            }
            ru = find_halving(parent, seen, hdr);   // <= seen < hi
            rv = find_halving(parent, lo, hdr);     // <= lo < hi
        }
    }
}

__global__ __launch_bounds__(kTrkThreads) void k_tracks_label(const int* __restrict__ parent,
                                                              int* __restrict__ label,
                                                              uint32_t* __restrict__ size,
                                                              int* __restrict__ hdr, long long rows) {
    const long long r = (long long)blockIdx.x * kTrkThreads + threadIdx.x;
    if (r >= rows) return;
    int x = (int)r;
    for (;;) {   // x strictly decreases
        const int p = parent[x];
        if (p == x) break;
        if (p > x) {
            raise_error(hdr);
            break;
        }
        x = p;
    }
    label[r] = x;
    atomicAdd(size + x, 1u);   // integer adds: the sum does not depend on their order
}

// one add per wave and counter
__device__ __forceinline__ void count_wave(int* counter, bool flag) {
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(counter, (int)__popcll(m));
}

__global__ __launch_bounds__(kTrkThreads) void k_tracks_mark(const int* __restrict__ label,
                                                             const uint32_t* __restrict__ size,
                                                             uint32_t* __restrict__ val,
                                                             int* __restrict__ hdr, long long rows,
                                                             int min_length, int nsets) {
    const long long r = (long long)blockIdx.x * kTrkThreads + threadIdx.x;
    const bool root = r < rows && label[r] == (int)r;
    const uint32_t n = root ? size[r] : 0u;
    const int kind = sgtrk::classify(n, min_length, nsets);
    const bool cand = n >= 2u && kind == sgtrk::kCandidate;
    if (r < rows) val[r] = cand ? n : 0u;
    count_wave(hdr + kTracksHdrComponents, n >= 2u);
    count_wave(hdr + kTracksHdrOversize, n >= 2u && kind == sgtrk::kOversize);
    count_wave(hdr + kTracksHdrShort, n >= 2u && kind == sgtrk::kShort);
    count_wave(hdr + kTracksHdrCandidates, cand);
}

__global__ __launch_bounds__(kTrkThreads) void k_tracks_scatter(const int* __restrict__ label,
                                                                const uint32_t* __restrict__ size,
                                                                const uint32_t* __restrict__ val,
                                                                const uint32_t* __restrict__ seg_start,
                                                                uint32_t* __restrict__ fill,
                                                                int* __restrict__ seg,
                                                                int* __restrict__ out_track,
                                                                int* __restrict__ hdr, long long rows,
                                                                int min_length, int nsets) {
    const long long r = (long long)blockIdx.x * kTrkThreads + threadIdx.x;
    if (r >= rows) return;
    const int L = label[r];
    const uint32_t n = val[L];
    if (n == 0u) {
        const uint32_t all = size[L];
        out_track[r] = all >= 2u && sgtrk::classify(all, min_length, nsets) == sgtrk::kOversize
                           ? sgtrk::kTrackInconsistent : sgtrk::kTrackNone;
        return;
    }
    const uint32_t k = atomicAdd(fill + L, 1u);
    if (k < n) seg[seg_start[L] + k] = (int)r;   // (seg_start[L] + n <= rows: the scan of val)
    else raise_error(hdr);
}

// The wave's 64 rows; each candidate root among them is handled by the whole wave in turn.
__global__ __launch_bounds__(kTrkThreads) void k_tracks_order(const long long* __restrict__ set_off,
                                                              int nsets,
                                                              const uint32_t* __restrict__ val,
                                                              const uint32_t* __restrict__ seg_start,
                                                              const int* __restrict__ seg,
                                                              int* __restrict__ sorted,
                                                              uint32_t* __restrict__ tval,
                                                              uint32_t* __restrict__ tflag,
                                                              long long rows) {
    const long long r = (long long)blockIdx.x * kTrkThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = r < rows;
    const int my_n = in ? (int)val[r] : 0;
    const uint32_t my_base = my_n ? seg_start[r] : 0u;
    unsigned long long todo = __ballot(my_n != 0);
    uint32_t mine = 0u;
    while (todo) {   // one bit fewer per turn
        const int b = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int n = __shfl(my_n, b, 64);
        const uint32_t base = __shfl(my_base, b, 64);
        bool bad = false;
        for (int k0 = 0; k0 < n; k0 += 64) {
            const bool have = k0 + lane < n;
            const int x = have ? seg[base + k0 + lane] : 0x7fffffff;
            int rank = 0, next = 0x7fffffff;   // rows below x; the lowest row above x
            for (int y = 0; y < n; y++) {
                const int v = seg[base + y];
                rank += v < x;
                next = v > x && v < next ? v : next;
            }
            if (have) {
                if (rank < n) sorted[base + rank] = x;   // (rows differ, so rank < n)
                if (next != 0x7fffffff)
                    bad |= next < set_off[sgtrk::set_of_row(set_off, nsets, x) + 1];
            }
        }
        const bool any_bad = __ballot(bad) != 0ull;
        if (lane == b) mine = any_bad ? 0u : (uint32_t)n;
    }
    if (in) {
        tval[r] = mine;
        tflag[r] = mine != 0u;
    }
}

__global__ __launch_bounds__(kTrkThreads) void k_tracks_finish(const uint32_t* __restrict__ val,
                                                               const uint32_t* __restrict__ seg_start,
                                                               const int* __restrict__ sorted,
                                                               const uint32_t* __restrict__ tval,
                                                               const uint32_t* __restrict__ toff,
                                                               const uint32_t* __restrict__ tid,
                                                               int* __restrict__ out_track,
                                                               long long* __restrict__ out_offsets,
                                                               int* __restrict__ out_rows,
                                                               int* __restrict__ hdr, long long rows) {
    const long long r = (long long)blockIdx.x * kTrkThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = r < rows;
    const int my_n = in ? (int)val[r] : 0;
    const uint32_t my_base = my_n ? seg_start[r] : 0u;
    const bool my_good = my_n && tval[r] != 0u;
    const uint32_t my_off = my_n ? toff[r] : 0u, my_id = my_n ? tid[r] : 0u;
    if (r == 0) {   // the totals: toff[rows] rows in tid[rows] tracks
        out_offsets[tid[rows]] = (long long)toff[rows];
        hdr[kTracksHdrTracks] = (int)tid[rows];
        hdr[kTracksHdrTrackRows] = (int)toff[rows];
    }
    unsigned long long todo = __ballot(my_n != 0);
    while (todo) {   // one bit fewer per turn
        const int b = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int n = __shfl(my_n, b, 64);
        const uint32_t base = __shfl(my_base, b, 64), o = __shfl(my_off, b, 64);
        const int t = (int)__shfl(my_id, b, 64);
        const bool good = __shfl((int)my_good, b, 64) != 0;
        for (int k = lane; k < n; k += 64) {
            const int x = sorted[base + k];
            if ((unsigned)x >= (unsigned long long)rows) continue;   // (never: the scatter filled it)
            out_track[x] = good ? t : sgtrk::kTrackInconsistent;
            if (good) out_rows[o + k] = x;
        }
        if (good && lane == 0) out_offsets[t] = (long long)o;
    }
}

unsigned row_blocks(long long rows) { return (unsigned)((rows + kTrkThreads - 1) / kTrkThreads); }

}  // namespace

hipError_t launch_tracks(const TracksTables& tab, const TracksWork& w, long long rows, int nsets,
                         int npairs, long long total, int min_length, int* out_track,
                         long long* out_offsets, int* out_rows, hipStream_t stream) {
    if (rows <= 0 || rows > 0x7fffffffLL || nsets <= 0) return hipErrorInvalidValue;
    const dim3 grid(row_blocks(rows)), block(kTrkThreads);
    hipLaunchKernelGGL(k_tracks_init, grid, block, 0, stream, w.parent, w.size, w.fill, w.hdr, rows);
    if (total > 0) {
        const unsigned ublocks = (unsigned)std::min<long long>((total + kTrkThreads - 1) / kTrkThreads,
                                                               1 << 20);
        hipLaunchKernelGGL(k_tracks_union, dim3(ublocks), block, 0, stream, tab.pair_start,
                           tab.pair_base, npairs, tab.matches, total, w.parent, w.hdr);
    }
    hipLaunchKernelGGL(k_tracks_label, grid, block, 0, stream, w.parent, w.label, w.size, w.hdr, rows);
    hipLaunchKernelGGL(k_tracks_mark, grid, block, 0, stream, w.label, w.size, w.val, w.hdr, rows,
                       min_length, nsets);
    hipError_t e = launch_scan(w.val, w.seg_start, (size_t)rows, w.scan_tmp, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tracks_scatter, grid, block, 0, stream, w.label, w.size, w.val, w.seg_start,
                       w.fill, w.seg, out_track, w.hdr, rows, min_length, nsets);
    hipLaunchKernelGGL(k_tracks_order, grid, block, 0, stream, tab.set_off, nsets, w.val, w.seg_start,
                       w.seg, w.sorted, w.tval, w.tflag, rows);
    if ((e = launch_scan(w.tval, w.toff, (size_t)rows, w.scan_tmp, stream)) != hipSuccess) return e;
    if ((e = launch_scan(w.tflag, w.tid, (size_t)rows, w.scan_tmp, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_tracks_finish, grid, block, 0, stream, w.val, w.seg_start, w.sorted, w.tval,
                       w.toff, w.tid, out_track, out_offsets, out_rows, w.hdr, rows);
    return hipGetLastError();
}

}  // namespace sgk
