// sgpu_tracks.cpp -- host side of the track builder (sgpu_tracks_batch, sgpu_tracks_images;
// DESIGN.md 4.20): sift_tracks.h is the rule, sift_tracks.hip the kernels.  Everything is checked
// here before anything is queued, so the kernels never meet an index they would have to refuse.
// One upload ([set offsets][pair starts][pair bases][matches]), the kernel sequence, the header's
// download and one synchronisation; then the outputs at their exact sizes and a second one.
#include <cstring>

#include "sgpu_ctx.h"
#include "sift_tracks.h"

using namespace sgh;

namespace {

size_t slot_words(int64_t rows) { return ((size_t)rows + 1 + 3) & ~(size_t)3; }

int tracks_impl(sgpu_ctx* ctx, const int64_t* off, int nsets, const int* set_pairs, int npairs,
                const int* matches, const int* counts, int min_length, int* out_track,
                int64_t* out_offsets, int* out_rows, long long* out_stats) {
    const char* why = "";
    int64_t rows = 0, total = 0;
    if (sgtrk::check_args(off, nsets, set_pairs, npairs, matches, counts, min_length, &why, &rows,
                          &total) != sgtrk::kArgsOk)
        return ctx->fail(SGPU_EINVAL, why);
    if (!out_track) return ctx->fail(SGPU_EINVAL, "null out_track");
    if (!out_offsets != !out_rows) return ctx->fail(SGPU_EINVAL, "out_offsets and out_rows go together");
    ctx->timing[T_TRACKS] = 0.f;
    long long stats[4] = {0, 0, 0, 0};
    if (rows == 0 || total == 0) {   // no edge: no component of two rows
        for (int64_t r = 0; r < rows; r++) out_track[r] = SGPU_TRACK_NONE;
        if (out_offsets) out_offsets[0] = 0;
        if (out_stats) memcpy(out_stats, stats, sizeof(stats));
        return 0;
    }

    // ---- the tables, one block: [set offsets nsets + 1][pair starts npairs + 1] (64-bit), [pair
    // bases npairs x 2][matches total x 2] (int)
    hipStream_t st = ctx->stream;
    const size_t b_off = ((size_t)nsets + 1) * sizeof(long long);
    const size_t b_start = ((size_t)npairs + 1) * sizeof(long long);
    const size_t b_base = (size_t)npairs * 2 * sizeof(int);
    const size_t b_matches = (size_t)total * 2 * sizeof(int);
    ctx->t_tables.resize(b_off + b_start + b_base + b_matches);
    unsigned char* tb = ctx->t_tables.data();
    auto* h_off = reinterpret_cast<long long*>(tb);
    auto* h_start = reinterpret_cast<long long*>(tb + b_off);
    auto* h_base = reinterpret_cast<int*>(tb + b_off + b_start);
    for (int s = 0; s <= nsets; s++) h_off[s] = off[s];
    long long at = 0;
    for (int p = 0; p < npairs; p++) {
        h_start[p] = at;
        at += counts[p];
        h_base[2 * p] = (int)off[set_pairs[2 * p]];
        h_base[2 * p + 1] = (int)off[set_pairs[2 * p + 1]];
    }
    h_start[npairs] = at;
    memcpy(tb + b_off + b_start + b_base, matches, b_matches);

    // ---- buffers: twelve work arrays and the scans' scratch; [out_offsets][out_track][out_rows][hdr]
    const size_t slot = slot_words(rows);
    const size_t b_work = (12 * slot + sgk::scan_tmp_words((size_t)rows)) * sizeof(uint32_t);
    const size_t b_ooff = ((size_t)rows / 2 + 1) * sizeof(long long);
    const size_t b_rows = (size_t)rows * sizeof(int);
    ALLOCCHK(ctx, ctx->t_tab.ensure(ctx->t_tables.size()));
    ALLOCCHK(ctx, ctx->t_work.ensure(b_work));
    ALLOCCHK(ctx, ctx->t_out.ensure(b_ooff + 2 * b_rows + sgk::kTracksHdrWords * sizeof(int)));
    HIPCHK(ctx, hipMemcpyAsync(ctx->t_tab.p, tb, ctx->t_tables.size(), hipMemcpyHostToDevice, st));
    const unsigned char* dt = ctx->t_tab.as<unsigned char>();
    sgk::TracksTables tab;
    tab.set_off = reinterpret_cast<const long long*>(dt);
    tab.pair_start = reinterpret_cast<const long long*>(dt + b_off);
    tab.pair_base = reinterpret_cast<const int*>(dt + b_off + b_start);
    tab.matches = reinterpret_cast<const int*>(dt + b_off + b_start + b_base);
    uint32_t* wk = ctx->t_work.as<uint32_t>();
    auto* d_ooff = ctx->t_out.as<long long>();
    int* d_track = reinterpret_cast<int*>(ctx->t_out.as<unsigned char>() + b_ooff);
    int* d_rows = d_track + rows;
    int* d_hdr = d_rows + rows;
    sgk::TracksWork w;
    w.parent = reinterpret_cast<int*>(wk);
    w.label = reinterpret_cast<int*>(wk + slot);
    w.seg = reinterpret_cast<int*>(wk + 2 * slot);
    w.sorted = reinterpret_cast<int*>(wk + 3 * slot);
    w.size = wk + 4 * slot;
    w.fill = wk + 5 * slot;
    w.val = wk + 6 * slot;
    w.seg_start = wk + 7 * slot;
    w.tval = wk + 8 * slot;
    w.tflag = wk + 9 * slot;
    w.toff = wk + 10 * slot;
    w.tid = wk + 11 * slot;
    w.scan_tmp = wk + 12 * slot;
    w.hdr = d_hdr;

    // ---- the queue
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, sgk::launch_tracks(tab, w, rows, nsets, npairs, total, min_length, d_track, d_ooff,
                                   d_rows, st));
    HIPCHK(ctx, hipEventRecord(ctx->ev[2], st));
    int hdr[sgk::kTracksHdrWords] = {};
    HIPCHK(ctx, hipMemcpyAsync(hdr, d_hdr, sizeof(hdr), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&ctx->timing[T_TRACKS], ctx->ev[1], ctx->ev[2]);
    const int T = hdr[sgk::kTracksHdrTracks], track_rows = hdr[sgk::kTracksHdrTrackRows];
    if (hdr[sgk::kTracksHdrErr] || T < 0 || T > rows / 2 || track_rows < 0 || track_rows > rows)
        return ctx->fail(SGPU_ENODEV, "tracks: a union-find step did not move to a smaller row");
    HIPCHK(ctx, hipMemcpyAsync(out_track, d_track, b_rows, hipMemcpyDeviceToHost, st));
    if (out_offsets) {
        static_assert(sizeof(int64_t) == sizeof(long long), "out_offsets is copied as it is");
        HIPCHK(ctx, hipMemcpyAsync(out_offsets, d_ooff, ((size_t)T + 1) * sizeof(long long),
                                   hipMemcpyDeviceToHost, st));
        if (track_rows > 0)
            HIPCHK(ctx, hipMemcpyAsync(out_rows, d_rows, (size_t)track_rows * sizeof(int),
                                       hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (out_stats) {
        stats[0] = hdr[sgk::kTracksHdrComponents];
        stats[1] = T;
        stats[2] = hdr[sgk::kTracksHdrOversize] + (hdr[sgk::kTracksHdrCandidates] - T);
        stats[3] = hdr[sgk::kTracksHdrShort];
        memcpy(out_stats, stats, sizeof(stats));
    }
    return T;
}

}  // namespace

extern "C" {

int sgpu_tracks_batch(sgpu_ctx* ctx, const int64_t* set_offsets, int nsets, const int* set_pairs,
                      int npairs, const int* matches, const int* match_counts, int min_length,
                      int* out_track, int64_t* out_offsets, int* out_rows, long long* out_stats) {
    if (!ctx) return SGPU_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return tracks_impl(ctx, set_offsets, nsets, set_pairs, npairs, matches, match_counts, min_length,
                       out_track, out_offsets, out_rows, out_stats);
}

int sgpu_tracks_images(sgpu_ctx* ctx, const int* image_pairs, int npairs, const int* matches,
                       const int* match_counts, int min_length, int* out_track,
                       int64_t* out_offsets, int* out_rows, long long* out_stats) {
    if (!ctx) return SGPU_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = check_batch(ctx, "build tracks on")) return rc;
    return tracks_impl(ctx, ctx->img_off.data(), ctx->batch, image_pairs, npairs, matches,
                       match_counts, min_length, out_track, out_offsets, out_rows, out_stats);
}

}  // extern "C"
