// sgpu_match.cpp -- host side of the two-set matcher: sgpu_match, sgpu_match_guided and the
// sharded form (sgpu_match_shard_begin / _end, sgpu_match_sharded) run one host sequence
// (run_match), driven by a description of the call (describe_match).
#include <cmath>
#include <cstring>

#include "sgpu_ctx.h"

using namespace sgh;

// float(acos(min(v * 2^-18, 1.0))) -- the expression of RowMatch_Kernel (ProgramCU.cu:1838),
// evaluated on the host; the oracle's bit-exactness rests on it
float sgh::match_dist(int v) {
    v = std::min(std::max(v, 0), sgk::kDistTable - 1);
    return (float)std::acos(std::min((double)(v * 0.000003814697265625f), 1.0));
}

int sgh::ensure_dist_table(sgpu_ctx* ctx) {
    if (ctx->dist_ready) return SGPU_OK;
    std::vector<float> t(sgk::kDistTable);
    for (int v = 0; v < sgk::kDistTable; v++) t[v] = match_dist(v);
    ALLOCCHK(ctx, ctx->m_dist.ensure(t.size() * sizeof(float)));
    HIPCHK(ctx, hipMemcpy(ctx->m_dist.p, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
    ctx->dist_ready = true;
    return SGPU_OK;
}

namespace {

// What a two-set call computes and through which kernels; every flag has its one rule in
// describe_match.
struct MatchCall {
    const uint8_t* d1;   // set 1 (a shard: its rows of it) and set 2, host or device (flags)
    int n1;
    const uint8_t* d2;
    int n2;
    float distmax, ratiomax;
    bool mbm;
    int flags;                                  // SGPU_INPUT_DEVICE
    const float* loc1 = nullptr;                // guided: the sets' locations and the geometry
    const float* loc2 = nullptr;
    const sgk::GuidedParams* guided = nullptr;
    bool best2 = false, fused = false, raw = false, dma = false, compact = false, prune = false;
};

// Where run_match left its results on the device: the row decisions [n1], the column decisions
// [n2] right behind them (mbm), and every column's (max, row, second) (best2).
struct MatchResult {
    int *match1, *match2;
    sgk::Top2* best2;
};

// shard: the rows of set 1 are one rank's share (sgpu_match_shard_begin).  The column decision of
// a set-2 row then needs the (max, row, second) of every rank, merged on the host
// (sgpu_match_shard_end): the column side returns that state for every column (best2).
void describe_match(const sgpu_ctx* ctx, bool shard, MatchCall& c) {
    const int dbg = ctx->debug_flags;
    const bool guided = c.guided != nullptr;
    c.best2 = shard && c.mbm;
    // Mutual matching: guided (or SGPU_DEBUG_FUSED_MATCH) computes the dots once and derives
    // both decisions from them (k_match_rows<.., COLS>); plain matching runs the row kernel a
    // second time with the sets swapped, which measured faster (1.07 vs 1.15 ms at 50k x 50k,
    // DESIGN.md section 10) because the fused epilogue halves the kernel's occupancy.
    c.fused = c.mbm && (guided || (dbg & SGPU_DEBUG_FUSED_MATCH));
    // keyless folding (k_match_raw / k_match_rows<..., RAW>): exact whenever a tied maximum
    // cannot pass the ratio test, i.e. ratiomax <= 1 (the reference's default 0.8);
    // SGPU_DEBUG_KEYED_MATCH keeps the keyed epilogue.  A shard's column side is merged over the
    // ranks by row index, so it needs every column's row and stays keyed (run_match).
    c.raw = !guided && !(c.ratiomax > 1.0f) && !(dbg & SGPU_DEBUG_KEYED_MATCH);
    // dma: through the LDS-DMA kernel k_match_raw (its own chunk split), unless
    // SGPU_DEBUG_MATCH_REGSTAGE.  Shards stay on the register-staged kernels: k_match_raw has no
    // keyed form for their column side, and their row side follows it (chunks without dma).
    c.dma = c.raw && !shard && !(dbg & SGPU_DEBUG_MATCH_REGSTAGE);
    // plain mutual matching decides only the columns some row matched (run_match); a shard cannot:
    // a column unmatched by this rank's rows may be matched by another's
    c.compact = c.mbm && !c.fused && !shard && !(dbg & SGPU_DEBUG_FULL_COLUMNS);
    // ... over the rows of set 1 that can change a listed column's decision (the LDS-DMA kernel
    // only: its B count may live on the device)
    c.prune = c.compact && c.dma && ctx->match_prune;
}

// SiftMatchGPU::SetDescriptors + GetSiftMatch (SiftMatchCU.cpp:71-179); with c.guided,
// SetFeautreLocation + GetGuidedSiftMatch (SiftMatchCU.cpp:104-136).  Everything from the uploads
// to the last kernel, queued on the context's stream; the caller queues its readback and waits
// (match_wait).  n1, n2 > 0.
int run_match(sgpu_ctx* ctx, const MatchCall& c, MatchResult& res) {
    const int n1 = c.n1, n2 = c.n2;
    const bool mbm = c.mbm, fused = c.fused, raw = c.raw, dma = c.dma, compact = c.compact, prune = c.prune;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (const int rc = ensure_dist_table(ctx)) return rc;
    const float* dist = ctx->m_dist.as<float>();
    const uint8_t *a = c.d1, *b = c.d2;
    // (no event before the uploads: nothing reads it, and each record costs ~4.5 us of GPU time)
    if (!(c.flags & SGPU_INPUT_DEVICE)) {
        ALLOCCHK(ctx, ctx->m_d1.ensure((size_t)n1 * 128));
        ALLOCCHK(ctx, ctx->m_d2.ensure((size_t)n2 * 128));
        HIPCHK(ctx, hipMemcpyAsync(ctx->m_d1.p, c.d1, (size_t)n1 * 128, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->m_d2.p, c.d2, (size_t)n2 * 128, hipMemcpyHostToDevice, st));
        a = ctx->m_d1.as<uint8_t>();
        b = ctx->m_d2.as<uint8_t>();
    }
    // guided: locations (float2 per feature) and the row side's geometric mask (the fused GEMM
    // derives the column side from the same values)
    const float *l1 = c.loc1, *l2 = c.loc2;
    if (c.guided) {
        ALLOCCHK(ctx, ctx->m_mask.ensure(sgk::guided_mask_bytes(n1, n2)));
        if (!(c.flags & SGPU_INPUT_DEVICE)) {
            ALLOCCHK(ctx, ctx->m_loc.ensure((size_t)(n1 + n2) * 2 * sizeof(float)));
            float* dl = ctx->m_loc.as<float>();
            HIPCHK(ctx, hipMemcpyAsync(dl, c.loc1, (size_t)n1 * 2 * sizeof(float), hipMemcpyHostToDevice, st));
            HIPCHK(ctx, hipMemcpyAsync(dl + 2 * n1, c.loc2, (size_t)n2 * 2 * sizeof(float),
                                       hipMemcpyHostToDevice, st));
            l1 = dl;
            l2 = dl + 2 * n1;
        }
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    const int ca = sgk::match_chunks(n1, n2, dma && !fused), panels = sgk::match_panels(n1);
    const int cb = mbm && !fused ? sgk::match_chunks(n2, n1, dma) : 0;
    // the matched columns' count is known on the device only, so the partials are sized for any
    const size_t part_b = compact ? sgk::match_part_bound(n2, n1, dma) : (size_t)cb * n2;
    const size_t part_n = std::max((size_t)ca * n1, part_b);
    ALLOCCHK(ctx, ctx->m_part.ensure((part_n + (c.best2 ? n2 : 0)) * sizeof(sgk::Top2)));
    if (fused) ALLOCCHK(ctx, ctx->m_colpart.ensure((size_t)panels * n2 * sizeof(sgk::Top2)));
    if (compact) ALLOCCHK(ctx, ctx->m_cols.ensure((size_t)(2 * n2 + 3) * sizeof(int)));
    if (prune) {
        ALLOCCHK(ctx, ctx->m_prune.ensure(((size_t)3 * n1 + sgk::match_ct_pad()) * sizeof(int)));
        ALLOCCHK(ctx, ctx->m_s1c.ensure((size_t)n1 * 128));
    }
    ALLOCCHK(ctx, ctx->m_terms.ensure(((size_t)2 * (n1 + n2) + 2 * sgk::match_ct_pad()) * sizeof(int)));
    ALLOCCHK(ctx, ctx->m_match.ensure((size_t)(n1 + n2) * sizeof(int)));
    int* row1 = ctx->m_terms.as<int>();          // row terms 128 * sum(d1), column terms
    int* col2 = row1 + n1;                       // 128 * sum(d2) - 2^21
    int* ct1 = col2 + n2;                        // k_match_raw's column terms of each set
    int* ct2 = ct1 + n1 + sgk::match_ct_pad();
    int* match1 = ctx->m_match.as<int>();
    int* match2 = match1 + n1;
    sgk::Top2* part = ctx->m_part.as<sgk::Top2>();
    sgk::Top2* best2 = c.best2 ? part + part_n : nullptr;
    sgk::Top2* colpart = fused ? ctx->m_colpart.as<sgk::Top2>() : nullptr;
    uint8_t* rmask = c.guided ? ctx->m_mask.as<uint8_t>() : nullptr;
    if (c.guided)
        HIPCHK(ctx, sgk::launch_guided_mask(l1, n1, l2, n2, *c.guided, rmask, nullptr, st));
    // s8 forms of both sets: the operands of the i8 MFMA
    ALLOCCHK(ctx, ctx->m_s1.ensure((size_t)n1 * 128));
    ALLOCCHK(ctx, ctx->m_s2.ensure((size_t)n2 * 128));
    uint8_t* s1 = ctx->m_s1.as<uint8_t>();
    uint8_t* s2 = ctx->m_s2.as<uint8_t>();
    uint8_t* s1c = prune ? ctx->m_s1c.as<uint8_t>() : nullptr;
    // ... with the row terms 128 * sum(d1) and, for mutual matching, the column side's terms
    // (two GEMMs: 128 * sum(d2), the row terms of the swapped launch; fused: the column terms
    // 128 * sum(d2) - 2^21, guided: 0) and the matched-column flags cleared
    // [flag n2][count][ntau][pruned count][list n2]
    int* cw = compact ? ctx->m_cols.as<int>() : nullptr;
    int* rmax1 = prune ? ctx->m_prune.as<int>() : nullptr;   // pruning: row maxima of set 1,
    int* map1c = prune ? rmax1 + n1 : nullptr;                // the kept rows' indices,
    int* ct1c = prune ? map1c + n1 : nullptr;                 // their column terms
    sgk::PrepSet p1{a, n1, s1};
    p1.sums = row1;
    p1.ctp = dma && mbm && !fused ? ct1 : nullptr;
    p1.ctfill = ct1c;
    HIPCHK(ctx, sgk::launch_prep_set(p1, st));
    if (mbm || dma) {
        sgk::PrepSet p2{b, n2, s2};
        p2.sums = mbm ? col2 : nullptr;
        p2.scale = c.guided && fused ? 0 : 128;
        p2.bias = fused && !c.guided ? -2097152 : 0;
        p2.zero = cw;
        p2.nzero = compact ? n2 + 3 : 0;
        p2.ctp = dma ? ct2 : nullptr;
        HIPCHK(ctx, sgk::launch_prep_set(p2, st));
    } else {
        HIPCHK(ctx, sgk::launch_to_s8(b, n2, s2, st));
    }
    // The mutual check reads the column decision match2[j] only for j = match1[i] >= 0, so the
    // column GEMM of a compact call runs over those columns alone: the row finish appends each
    // matched column once to a list (flags and count zeroed with the s8 conversion), and the
    // column launches take their rows from it, their count from the device.  Every listed column
    // still scans all of set 1, so its decision is the reference's (SGPU_DEBUG_FULL_COLUMNS:
    // every column, as ColMatch_Kernel does).
    //
    // Pruning (plain mutual matching with ratiomax <= 1): a listed column's decision depends
    // only on rows of set 1 with some dot >= tau, the smallest second value that fails the
    // ratio test against the weakest passing row maximum (k_match_finish).
    // The row finish records every row's maximum and that bound, k_prune_set compacts the
    // rows at or above it, and the column GEMM runs over them (count on the device): the
    // same decisions, the same pairs.
    sgk::ColumnList claim, cols;
    if (compact) {
        claim.flag = cw;
        claim.count = cw + n2;
        claim.list = cw + n2 + 3;
        cols.count = claim.count;
        cols.map = claim.list;
        cols.dma = dma ? 1 : 0;
    }
    if (prune) {
        claim.rmax = rmax1;
        claim.ntau = cw + n2 + 1;
        cols.bmap = map1c;
        cols.bn = cw + n2 + 2;
    }
    // ---- the row side.  fused: one GEMM for both decisions (MultiplyDescriptor_Kernel's row
    // results + column partials, ProgramCU.cu:1466-1564); guided: the column values already hold
    // the column term (col_term 0)
    sgk::MatchRows r{s1, n1, s2, n2, ca, part};
    r.mask = rmask;
    sgk::MatchFinish f{part, n1, ca, row1, dist, c.distmax, c.ratiomax, match1};
    if (fused) {
        r.row_term = row1;
        r.colpart = colpart;
    } else {
        r.raw = raw;
        r.ctp = dma ? ct2 : nullptr;
        f.raw_A = raw ? a : nullptr;
        f.raw_B = raw ? b : nullptr;
        f.nB = n2;
        f.cl = claim;
    }
    HIPCHK(ctx, sgk::launch_match_rows(r, st));
    HIPCHK(ctx, sgk::launch_match_finish(f, st));
    // ---- the column side: from the fused launch's panels, or the row kernel with the sets
    // swapped.  A call that wants best2 merges its columns' rows with other ranks': keyed.
    if (fused) {
        HIPCHK(ctx, sgk::launch_match_cols(colpart, n2, panels, col2, dist, c.distmax, c.ratiomax,
                                           match2, best2, st));
    } else if (mbm) {
        const bool craw = raw && !c.best2;
        if (prune)
            HIPCHK(ctx, sgk::launch_prune_set(rmax1, claim.ntau, n1, s1, ct1, s1c, ct1c, map1c,
                                              cw + n2 + 2, st));
        sgk::MatchRows cr{s2, n2, prune ? s1c : s1, n1, cb, part};
        cr.row_side = false;
        cr.raw = craw;
        cr.amap = cols.map;
        cr.an = cols.count;
        cr.ctp = prune ? ct1c : dma ? ct1 : nullptr;
        cr.bn = cols.bn;
        HIPCHK(ctx, sgk::launch_match_rows(cr, st));
        sgk::MatchFinish cf{part, n2, cb, col2, dist, c.distmax, c.ratiomax, match2};
        cf.row_side = false;
        cf.best = best2;
        cf.raw_A = craw ? b : nullptr;
        cf.raw_B = craw ? a : nullptr;
        cf.nB = n1;
        cf.cl = cols;
        HIPCHK(ctx, sgk::launch_match_finish(cf, st));
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[2], st));
    res = MatchResult{match1, match2, best2};
    return SGPU_OK;
}

// after the caller's readback copies: wait for the stream, time the kernels
int match_wait(sgpu_ctx* ctx) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    (void)hipEventElapsedTime(&ctx->timing[T_MATCH], ctx->ev[1], ctx->ev[2]);
    return SGPU_OK;
}

int match_impl(sgpu_ctx* ctx, const uint8_t* d1, int n1, const uint8_t* d2, int n2,
               float distmax, float ratiomax, int mbm, int max_match, int* out_pairs, int flags,
               const float* loc1, const float* loc2, const sgk::GuidedParams* guided) {
    if (!ctx) return SGPU_EINVAL;
    if (n1 <= 0 || n2 <= 0) return 0;   // SiftMatchCU.cpp:142
    if (!d1 || !d2 || (max_match > 0 && !out_pairs)) return ctx->fail(SGPU_EINVAL, "bad match arguments");
    if (guided && (!loc1 || !loc2)) return ctx->fail(SGPU_EINVAL, "guided match needs locations");
    MatchCall c{d1, n1, d2, n2, distmax, ratiomax, mbm != 0, flags, loc1, loc2, guided};
    describe_match(ctx, false, c);
    MatchResult res;
    if (const int rc = run_match(ctx, c, res)) return rc;
    ctx->h_match.resize((size_t)n1 + n2);
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_match.data(), res.match1, (size_t)(mbm ? n1 + n2 : n1) * sizeof(int),
                               hipMemcpyDeviceToHost, ctx->stream));
    if (const int rc = match_wait(ctx)) return rc;
    // mutual check in ascending i (SiftMatchCU.cpp:166-176)
    const int* bufr = ctx->h_match.data();
    const int* bufc = bufr + n1;
    int nmatch = 0;
    for (int i = 0; i < n1 && nmatch < max_match; ++i) {
        const int j = bufr[i];
        if (j >= 0 && (!mbm || bufc[j] == i)) {
            out_pairs[2 * nmatch] = i;
            out_pairs[2 * nmatch + 1] = j;
            nmatch++;
        }
    }
    return nmatch;
}

}  // namespace

extern "C" {

int sgpu_match(sgpu_ctx* ctx, const uint8_t* d1, int n1, const uint8_t* d2, int n2,
               float distmax, float ratiomax, int mbm, int max_match, int* out_pairs,
               int flags) {
    return match_impl(ctx, d1, n1, d2, n2, distmax, ratiomax, mbm, max_match, out_pairs, flags,
                      nullptr, nullptr, nullptr);
}

// ---- sharded matcher: rows of set 1 split over ranks, set 2 replicated ----
// The row decision of a set-1 row needs only its own dots, so it stays local.  The column
// decision of a set-2 row j needs the best / second-best over ALL set-1 rows: every rank
// reduces its shard to the clamped running state (max, argmax, second) that
// RowMatch_Kernel / ColMatch_Kernel keep (ProgramCU.cu:1803, 1850: running maxima start at 0
// with index -1), the ranks exchange those n2 x 3 ints, and the merge -- max, the column
// side's tie order (lowest set-1 row first), second = max(min of the maxima, seconds) -- gives
// exactly the single-device state, because clamping at 0 commutes with max.

int sgpu_match_shard_begin(sgpu_ctx* ctx, const uint8_t* d1, int ns, int row_begin,
                           const uint8_t* d2, int n2, float distmax, float ratiomax, int mbm,
                           int* row_match, int* col_best, int flags) {
    if (!ctx) return SGPU_EINVAL;
    if (ns < 0 || n2 < 0 || row_begin < 0 || (ns > 0 && (!d1 || !row_match)) ||
        (n2 > 0 && !d2) || (mbm && n2 > 0 && !col_best))
        return ctx->fail(SGPU_EINVAL, "bad shard-match arguments");
    if (mbm)   // an empty shard contributes the initial state (0, -1, 0) to every column
        for (int j = 0; j < n2; j++) {
            col_best[3 * j] = 0;
            col_best[3 * j + 1] = -1;
            col_best[3 * j + 2] = 0;
        }
    if (ns == 0 || n2 == 0) {
        for (int i = 0; i < ns; i++) row_match[i] = -1;
        return SGPU_OK;
    }
    MatchCall c{d1, ns, d2, n2, distmax, ratiomax, mbm != 0, flags};
    describe_match(ctx, true, c);
    MatchResult res;
    if (const int rc = run_match(ctx, c, res)) return rc;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(row_match, res.match1, (size_t)ns * sizeof(int), hipMemcpyDeviceToHost, st));
    if (mbm) {
        static_assert(sizeof(sgk::Top2) == 3 * sizeof(int), "Top2 = 3 ints");
        HIPCHK(ctx, hipMemcpyAsync(col_best, res.best2, (size_t)n2 * sizeof(sgk::Top2),
                                   hipMemcpyDeviceToHost, st));
    }
    if (const int rc = match_wait(ctx)) return rc;
    if (mbm)   // Top2 is (max, idx, second); the shard's row index becomes the global one
        for (int j = 0; j < n2; j++)
            if (col_best[3 * j + 1] >= 0) col_best[3 * j + 1] += row_begin;
    return SGPU_OK;
}

int sgpu_match_shard_end(const int* col_best_all, int nshards, int n2, const int* row_match,
                         int ns, int row_begin, float distmax, float ratiomax, int mbm,
                         int max_match, int* out_pairs) {
    if (ns < 0 || n2 < 0 || (ns > 0 && !row_match) || (max_match > 0 && !out_pairs) ||
        (mbm && (nshards < 1 || (n2 > 0 && !col_best_all))))
        return SGPU_EINVAL;
    std::vector<int> col_match;
    if (mbm) {
        col_match.assign((size_t)n2, -1);
        for (int j = 0; j < n2; j++) {
            // shards in rank order: rank r's rows precede rank r+1's (lowest row wins ties)
            int m = col_best_all[3 * j], idx = col_best_all[3 * j + 1], sc = col_best_all[3 * j + 2];
            for (int r = 1; r < nshards; r++) {
                const int* u = col_best_all + ((size_t)r * n2 + j) * 3;
                const bool later = u[0] > m || (u[0] == m && u[1] >= 0 && (idx < 0 || u[1] < idx));
                sc = std::max(std::min(m, u[0]), std::max(sc, u[2]));
                if (later) idx = u[1];
                m = std::max(m, u[0]);
            }
            const float d1 = match_dist(m), d2 = match_dist(sc);
            col_match[j] = (d1 < distmax) && (d1 < d2 * ratiomax) ? idx : -1;
        }
    }
    int nmatch = 0;
    for (int i = 0; i < ns && nmatch < max_match; ++i) {
        const int j = row_match[i];
        if (j >= 0 && j < n2 && (!mbm || col_match[j] == row_begin + i)) {
            out_pairs[2 * nmatch] = row_begin + i;
            out_pairs[2 * nmatch + 1] = j;
            nmatch++;
        }
    }
    return nmatch;
}

int sgpu_match_sharded(sgpu_ctx* ctx, const uint8_t* d1, int ns, int row_begin,
                       const uint8_t* d2, int n2, float distmax, float ratiomax, int mbm,
                       int max_match, int* out_pairs, int flags) {
    if (!ctx) return SGPU_EINVAL;
    const int ranks = ctx->comm ? ctx->comm_ranks : 1;
    std::vector<int> rows((size_t)std::max(ns, 1)), mine((size_t)3 * std::max(n2, 1));
    int rc = sgpu_match_shard_begin(ctx, d1, ns, row_begin, d2, n2, distmax, ratiomax, mbm,
                                    rows.data(), mine.data(), flags);
    const bool collective = mbm && ctx->comm && n2 > 0;
    if (collective) {
        // every rank learns whether any rank failed locally before the data collective, so a
        // local failure never leaves the peers waiting inside ncclAllGather
        double failed = rc != SGPU_OK ? 1.0 : 0.0;
        const int rs = sgpu_comm_allreduce_f64(ctx, &failed, 1, 1);
        if (rs != SGPU_OK) return rs;
        if (failed != 0.0)
            return rc != SGPU_OK ? rc : ctx->fail(SGPU_ENODEV, "sgpu_match_sharded: a peer rank failed");
    } else if (rc != SGPU_OK) {
        return rc;
    }
    std::vector<int> all;
    if (collective) {   // RCCL all-gather of the n2 x 3 column states
        all.resize((size_t)3 * n2 * ranks);
        rc = sgpu_comm_allgather_i32(ctx, mine.data(), 3 * n2, all.data());
        if (rc != SGPU_OK) return rc;
    } else {
        all = mine;
    }
    return sgpu_match_shard_end(all.data(), ranks, n2, rows.data(), ns, row_begin, distmax,
                                ratiomax, mbm, max_match, out_pairs);
}

// SiftMatchGPU::GetGuidedSiftMatch (SiftMatch.cpp:663-677 defaults, SiftMatchCU.cpp:126-136).
int sgpu_match_guided(sgpu_ctx* ctx, const uint8_t* d1, int n1, const uint8_t* d2, int n2,
                      const float* loc1, const float* loc2, const float* H, const float* F,
                      float distmax, float ratiomax, float hdistmax, float fdistmax, int mbm,
                      int max_match, int* out_pairs, int flags) {
    if (!ctx) return SGPU_EINVAL;
    if (!H && !F)
        return match_impl(ctx, d1, n1, d2, n2, distmax, ratiomax, mbm, max_match, out_pairs,
                          flags, nullptr, nullptr, nullptr);
    // a missing matrix is the identity with its threshold at 1e20 (SiftMatch.cpp:667-675)
    static const float kIdentity[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    sgk::GuidedParams gp;
    memcpy(gp.H, H ? H : kIdentity, sizeof(gp.H));
    memcpy(gp.F, F ? F : kIdentity, sizeof(gp.F));
    gp.hdistmax = H ? hdistmax : 1.0e+20f;
    gp.fdistmax = F ? fdistmax : 1.0e+20f;
    return match_impl(ctx, d1, n1, d2, n2, distmax, ratiomax, mbm, max_match, out_pairs, flags,
                      loc1, loc2, &gp);
}

}  // extern "C"
