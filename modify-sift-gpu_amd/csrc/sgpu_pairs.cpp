// sgpu_pairs.cpp -- the host path that the callers of the grouped pair matcher share
// (sgpu_match_batch.cpp, sgpu_verify.cpp, sgpu_prematch.cpp): where the sets come
// from, the plan-sized buffers, one matching pass, and the download of the matches that fit.
#include <string>

#include "sgpu_ctx.h"

namespace sgh {

int check_batch(sgpu_ctx* ctx, const char* what) {
    if (ctx->batch <= 0 || ctx->img_off.empty())
        return ctx->fail(SGPU_EINVAL, (std::string("no extracted batch to ") + what).c_str());
    if (!ctx->opt.descriptors) return ctx->fail(SGPU_EINVAL, "descriptors disabled (-sd)");
    return SGPU_OK;
}

int probe_offsets(const int64_t* off, int nsets) {
    sgplan::Plan probe;
    return sgplan::build_plan(off, nsets, nullptr, 0, false, 0, probe);
}

static int upload(sgpu_ctx* ctx, DevBuf& buf, const void* src, size_t bytes) {
    ALLOCCHK(ctx, buf.ensure(bytes));
    HIPCHK(ctx, hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return SGPU_OK;
}

int resolve_sets(sgpu_ctx* ctx, const SetSource& src, int64_t rows, int need, DeviceSets& sets) {
    sets = DeviceSets{};
    if (src.images) {
        if (need & SET_DESC) {
            // a quantisation this call has to make counts into its device time; it is queued on
            // the matcher's stream, with no wait in between
            sets.timing_started = !ctx->f_ready;
            if (sets.timing_started) HIPCHK(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
            if (const int rc = feature_u8(ctx)) return rc;
            sets.u8 = ctx->f_u8.as<uint8_t>();
            sets.s8 = ctx->f_s8.as<uint8_t>();
            sets.sums = ctx->f_sums.as<int>();
        }
        if (need & (SET_LOC | SET_SCALE)) {
            // the batch's device keys [x, y, scale, orientation] (gathers a multi-part batch)
            const float* keys = nullptr;
            if (const int rc = sgpu_device_features(ctx, &keys, nullptr, nullptr)) return rc;
            sets.loc = keys;
            sets.scale = keys ? keys + 2 : nullptr;
            sets.loc_stride = sets.scale_stride = 4;
        }
        return SGPU_OK;
    }
    sets.u8 = src.desc;
    sets.loc = src.loc;
    sets.scale = src.scale;
    sets.scale_stride = src.scale_stride;
    if (src.device) return SGPU_OK;
    if (need & SET_DESC) {
        if (const int rc = upload(ctx, ctx->b_desc, src.desc, (size_t)rows * 128)) return rc;
        sets.u8 = ctx->b_desc.as<uint8_t>();
    }
    if (need & SET_LOC) {
        if (const int rc = upload(ctx, ctx->b_loc, src.loc, (size_t)rows * 2 * sizeof(float))) return rc;
        sets.loc = ctx->b_loc.as<float>();
    }
    if (need & SET_SCALE) {   // the floats that the rows of [0, rows) read
        const size_t floats = (size_t)(rows - 1) * src.scale_stride + 1;
        if (const int rc = upload(ctx, ctx->p_scale, src.scale, floats * sizeof(float))) return rc;
        sets.scale = ctx->p_scale.as<float>();
    }
    return SGPU_OK;
}

int ensure_pair_buffers(sgpu_ctx* ctx, const sgplan::Plan& plan, size_t table_bytes,
                        int64_t out_rows, int cnt_pairs, int64_t s8_rows) {
    ALLOCCHK(ctx, ctx->b_plan.ensure(table_bytes));
    ALLOCCHK(ctx, ctx->b_part.ensure((size_t)plan.part_total * sizeof(sgk::Top2)));
    ALLOCCHK(ctx, ctx->b_dec.ensure((size_t)plan.dec_total * sizeof(int)));
    // [offsets npairs + 1 (64-bit)][counts npairs]
    if (cnt_pairs > 0)
        ALLOCCHK(ctx, ctx->b_cnt.ensure((size_t)(cnt_pairs + 1) * sizeof(long long) +
                                        (size_t)cnt_pairs * sizeof(int)));
    ALLOCCHK(ctx, ctx->b_out.ensure((size_t)std::max<int64_t>(out_rows, 1) * 2 * sizeof(int)));
    if (s8_rows > 0) {
        ALLOCCHK(ctx, ctx->b_s8.ensure((size_t)s8_rows * 128));
        ALLOCCHK(ctx, ctx->b_sums.ensure((size_t)s8_rows * sizeof(int)));
    }
    return SGPU_OK;
}

int derive_s8(sgpu_ctx* ctx, DeviceSets& sets, int64_t rows) {
    if (sets.s8 && sets.sums) return SGPU_OK;
    sgk::PrepSet prep{sets.u8, (int)rows, ctx->b_s8.as<uint8_t>()};
    prep.sums = ctx->b_sums.as<int>();
    HIPCHK(ctx, sgk::launch_prep_set(prep, ctx->stream));
    sets.s8 = ctx->b_s8.as<uint8_t>();
    sets.sums = ctx->b_sums.as<int>();
    return SGPU_OK;
}

int queue_match_pass(sgpu_ctx* ctx, const MatchPass& m) {
    hipStream_t st = ctx->stream;
    sgk::Top2* d_part = ctx->b_part.as<sgk::Top2>();
    int* d_dec = ctx->b_dec.as<int>();
    const int nitems = (int)m.plan.items.size();
    if (m.d_geom)
        HIPCHK(ctx, sgk::launch_match_pairs_guided(m.s8, m.tab.items, nitems, d_part, m.loc,
                                                   m.loc_stride, m.d_geom, st));
    else
        HIPCHK(ctx, sgk::launch_match_pairs(m.s8, m.tab.items, nitems, d_part, st));
    HIPCHK(ctx, sgk::launch_match_pairs_finish(d_part, m.tab.sides, m.tab.fpanels,
                                               (int)m.plan.fpanels.size(), m.sums,
                                               ctx->m_dist.as<float>(), m.distmax, m.ratiomax,
                                               d_dec, st));
    HIPCHK(ctx, sgk::launch_match_pairs_compact(d_dec, m.tab.pairs, (int)m.plan.pairs.size(),
                                                m.max_match, m.out_rows, m.d_counts, m.d_offs,
                                                m.d_out, st));
    return SGPU_OK;
}

int download_fitting(sgpu_ctx* ctx, const int* counts, int npairs, const int* d_out, int* out_pairs,
                     int64_t cap, bool want_matches) {
    // the pairs that fit form a prefix (the offsets only grow): copy their matches
    int64_t total = 0, fit = 0;
    bool fits = true;
    for (int p = 0; p < npairs; p++) {
        total += counts[p];
        fits = fits && total <= cap;
        if (fits) fit = total;
    }
    if (total > INT_MAX) return ctx->fail(SGPU_ERANGE, "match total exceeds the return type");
    if (!want_matches) return (int)total;
    if (fit > 0) {
        HIPCHK(ctx, hipMemcpyAsync(out_pairs, d_out, (size_t)fit * 2 * sizeof(int),
                                   hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (total > cap) return ctx->fail(SGPU_ERANGE, "matches exceed cap (counts are complete)");
    return (int)total;
}

}  // namespace sgh
