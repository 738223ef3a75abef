// sgpu_extract.cpp -- host side of extraction: the batch pipeline, caller-supplied keypoints,
// feature access and the device quantiser.
//
// Host orchestration of one batch (replaces SiftPyramid::RunSIFT, SiftPyramid.cpp:58-216, and
// the PyramidCU stage methods).  A batch can be split into parts of consecutive images, each
// with its own HIP streams and buffers; part p+1 starts its pyramid when part p has finished
// detection, so that the HBM-bound pyramid/extremum kernels of one part can run beside the
// VALU-bound orientation/descriptor kernels of the previous one (one part by default, see
// extract_impl).  Inside a part everything is queued
// without host round trips (keypoint counts stay on the device; launch grids come from buffer
// capacities); the host waits once per batch, reads the per-image offsets and, if a part's
// candidates overflowed its capacity, grows the buffers and re-runs that part.  (The reference
// does four host round trips per DoG level, PyramidCU.cpp:783-813.)
#include <cmath>
#include <cstring>

#include "sgpu_ctx.h"

using namespace sgh;

extern "C" {

// Layout of one part of the planned batch (plan_batch): feature parameters, buffer offsets,
// capacities, and every device and pinned buffer the part's pipeline needs, allocated (grow-only).
// enqueue_part runs it first; sgpu_reserve (SiftGPU::AllocatePyramid) runs it alone.
static int layout_part(sgpu_ctx* ctx, Part& pt) {
    const sgpu_options& O = ctx->opt;
    const sgp::Schedule& S = ctx->sched;
    const int d = S.dog_level_num, nlev = S.level_num;
    const int noct = (int)ctx->oct.size();
    const int n = pt.n;

    // ---- layout: pyramid [octave][level][image][h][wa]; mask [octave][dog level][image][h][words]
    sgk::FeatureParams& fp = pt.fp;
    fp = sgk::FeatureParams{};
    fp.batch = n;
    fp.n_octaves = noct;
    fp.d = d;
    long long goff = 0, moff = 0;
    int rows = 0;
    for (int o = 0; o < noct; o++) {
        const sgp::Octave& oc = ctx->oct[o];
        sgk::OctaveDesc& od = fp.oct[o];
        od.w = oc.w;
        od.h = oc.h;
        od.wa = oc.wa;
        od.nwords = (oc.wa + 31) / 32;
        od.gauss_off = goff;
        od.level_stride = (long long)n * oc.wa * oc.h;
        goff += od.level_stride * nlev;
        od.mask_off = moff;
        od.mask_level_stride = (long long)n * oc.h * od.nwords;
        moff += od.mask_level_stride * d;
        fp.row_off[o] = rows;
        rows += d * oc.h;
    }
    fp.rows_per_image = rows;
    pt.total_rows = rows * n;
    pt.mask_words = moff;
    for (int j = 0; j < d; j++) fp.level_sigma[j] = sgp::level_sigma(S, j + S.level_min + 1);
    fp.sigma_step = powf(2.0f, 1.0f / d);
    fp.t0 = (O.subpixel ? 0.8f : 1.0f) * S.dog_threshold;
    fp.t = S.dog_threshold;
    fp.edge = (S.edge_threshold + 1) * (S.edge_threshold + 1) / S.edge_threshold;
    fp.gaussian_factor = O.orientation_gaussian_factor;
    fp.sample_factor = O.orientation_gaussian_factor * O.orientation_window_factor;
    fp.window_factor = O.descriptor_window_factor;
    fp.subpixel = O.subpixel ? 1 : 0;
    fp.num_orientation = O.fixed_orientation ? 0 : std::min(O.max_orientation, 2);
    fp.keep_sign = O.keep_extremum_sign;
    fp.circular = O.circular_window;
    fp.normalize = O.normalized;
    fp.unit_input = ctx->unit_input ? 1 : 0;
    fp.origin_offset = O.lowe_origin ? 0.0f : 0.5f;
    fp.octave_min = ctx->plan.octave_min + ctx->plan.ds;   // coordinate scale 2^(om + ds)

    // candidate capacity: grow-only, first guess one per 256 octave pixels
    const size_t sum_px = (size_t)goff / (size_t)std::max(1, nlev) / (size_t)n;
    pt.cand_cap = (ctx->debug_flags & SGPU_DEBUG_TINY_CAP)
                      ? std::max<size_t>(pt.cand_cap, 64)
                      : std::max(pt.cand_cap, std::max<size_t>(1024, sum_px / 256 * n));
    const size_t nc = pt.cand_cap, ne_cap = 2 * nc;
    // + 256 B: the descriptor's 16-byte strip loads may read up to 4 floats past the end of a
    // row (k_descriptor_fast).  Invariant: every strip it loads starts at a sample of the
    // feature's box, which is clamped to columns 1 .. W-2 and rows 1 .. H-2 of the plane for any
    // keypoint (detected or caller-supplied), and an empty box loads at row 1, column 1; so the
    // overshoot past the last plane is at most 5 floats, whatever the keypoint.
    ALLOCCHK(ctx, pt.pyr.ensure((size_t)goff * sizeof(float) + 256));
    ALLOCCHK(ctx, pt.mask.ensure((size_t)moff * sizeof(uint32_t)));
    ALLOCCHK(ctx, pt.row_count.ensure((size_t)pt.total_rows * sizeof(uint32_t)));
    ALLOCCHK(ctx, pt.row_base.ensure(((size_t)pt.total_rows + 1) * sizeof(uint32_t)));
    ALLOCCHK(ctx, pt.img_off_dev.ensure((size_t)(n + 2) * sizeof(int64_t)));
    ALLOCCHK(ctx, pt.cand.ensure(nc * sizeof(float4)));
    ALLOCCHK(ctx, pt.info.ensure(nc * sizeof(int2)));
    // (+ the feature queue's work counters after the counts, from the next 128-byte line on,
    // zeroed with them)
    ALLOCCHK(ctx, pt.ocount.ensure((sgk::feature_queue_base(nc) + sgk::kFeatureQueueWords) * sizeof(uint32_t)));
    ALLOCCHK(ctx, pt.eoff.ensure((nc + 1) * sizeof(uint32_t)));
    ALLOCCHK(ctx, pt.feat.ensure(ne_cap * sizeof(float4)));
    ALLOCCHK(ctx, pt.feat_info.ensure(ne_cap * sizeof(int2)));
    ALLOCCHK(ctx, pt.keys.ensure(ne_cap * sizeof(float4)));
    if (O.descriptors) ALLOCCHK(ctx, pt.desc.ensure(ne_cap * 128 * sizeof(float)));
    ALLOCCHK(ctx, pt.scan_tmp.ensure((sgk::scan_tmp_words(std::max<size_t>(nc, pt.total_rows)) + 16) * 4));
    if (pt.h_read_n < (size_t)n + 2) {
        if (pt.h_read) (void)hipHostFree(pt.h_read);
        pt.h_read = nullptr;
        g_allocs++;
        ALLOCCHK(ctx, hipHostMalloc((void**)&pt.h_read, ((size_t)n + 2) * sizeof(int64_t)));
        pt.h_read_n = (size_t)n + 2;
    }
    return SGPU_OK;
}

// The level filters of every octave of a part's pyramid into pt.ops, and what the planner reads
// of them into pt.levels: op (o, k) filters level k-1 into level k (op (0, 0) smooths the input
// into level 0); level kds = level_ds - level_min of octave o also writes its 2x decimation as
// level 0 of octave o+1 (PyramidCU.cpp:1024).  With -fo != 0 it first queues the input's
// resampling on st.  The filter of every octave's last level is also kept in pt.top_ops; with
// `lazy` it is left out of the list (nothing but the last DoG plane reads that
// level, and the extremum pass evaluates it where a candidate needs it).
static int build_level_ops(sgpu_ctx* ctx, Part& pt, const uint8_t* src8, const float* srcf,
                           int stride, hipStream_t st, bool lazy) {
    const sgpu_options& O = ctx->opt;
    const sgp::Schedule& S = ctx->sched;
    const sgk::FeatureParams& fp = pt.fp;
    const int nlev = S.level_num, noct = (int)ctx->oct.size(), n = pt.n, h = ctx->h;
    const size_t img_elems = (size_t)stride * h;
    float* pyr = pt.pyr.as<float>();
    sgk::Taps ltaps[sgk::kMaxLevels], taps0;
    int lfw[sgk::kMaxLevels] = {0};
    for (int k = 1; k < nlev; k++)
        lfw[k] = sgp::make_filter(S.sigma[k - 1], O.filter_width_factor, ltaps[k].k);
    const int fw0 = sgp::make_filter(S.initial_smooth, O.filter_width_factor, taps0.k);
    const int kds = S.level_ds - S.level_min;
    pt.ops.clear();
    pt.levels.clear();
    pt.ops.reserve((size_t)noct * nlev);
    pt.levels.reserve((size_t)noct * nlev);
    pt.top_ops.resize((size_t)noct);
    for (int o = 0; o < noct; o++) {
        const sgk::OctaveDesc& od = fp.oct[o];
        const long long npx = (long long)od.wa * od.h;
        float* lvl0 = pyr + od.gauss_off;
        float* ds = nullptr;
        int dsw = 0, dsh = 0;
        long long ds_stride = 0;
        if (o + 1 < noct) {
            const sgk::OctaveDesc& nd = fp.oct[o + 1];
            ds = pyr + nd.gauss_off;
            dsw = nd.wa;
            dsh = nd.h;
            ds_stride = (long long)nd.wa * nd.h;
        }
        const float* in_f = srcf;
        const uint8_t* in_8 = src8;
        int in_stride = stride;
        long long in_img = (long long)img_elems;
        if (o == 0 && ctx->plan.octave_min != 0) {
            // -fo != 0: resample the input into level 1's storage (free until level 1 is
            // filtered), then the initial smoothing as for a float input
            float* tmp = lvl0 + od.level_stride;
            HIPCHK(ctx, sgk::launch_first_octave_input(srcf, src8, stride, (long long)img_elems,
                                                       ctx->w & ~3, h, ctx->plan.octave_min, tmp,
                                                       od.wa, od.h, npx, n, st));
            in_f = tmp;
            in_8 = nullptr;
            in_stride = od.wa;
            in_img = npx;
        }
        for (int k = (o == 0 ? 0 : 1); k < nlev; k++) {
            pt.ops.emplace_back();
            sgk::LevelOp& op = pt.ops.back();
            op.fw = k == 0 ? fw0 : lfw[k];
            const float* tk = k == 0 ? taps0.k : ltaps[k].k;
            for (int i = 0; i < op.fw; i++) op.taps.k[i] = tk[i];
            const bool dk = ds && kds == k;
            op.src = k == 0 ? in_f : lvl0 + (k - 1) * od.level_stride;
            op.src_u8 = k == 0 ? in_8 : nullptr;
            op.src_stride = k == 0 ? in_stride : od.wa;
            op.src_img_stride = k == 0 ? in_img : npx;
            op.dst = lvl0 + k * od.level_stride;
            op.dst_img_stride = npx;
            op.w = od.wa;
            op.h = od.h;
            op.batch = n;
            op.ds_dst = dk ? ds : nullptr;
            op.ds_w = dk ? dsw : 0;
            op.ds_h = dk ? dsh : 0;
            op.ds_img_stride = dk ? ds_stride : 0;
            if (o == 0 && k == 0 && pt.one_stream) {
                // the first level launch also zeroes the extremum kernel's mask and row counts
                // and the orientation counts (one launch fewer than launch_zero)
                op.zero.p[0] = pt.row_count.as<uint32_t>();
                op.zero.n[0] = (size_t)pt.total_rows;
                op.zero.p[1] = pt.mask.as<uint32_t>();
                op.zero.n[1] = (size_t)pt.mask_words;
                op.zero.p[2] = pt.ocount.as<uint32_t>();
                op.zero.n[2] = sgk::feature_queue_base(pt.cand_cap) + sgk::kFeatureQueueWords;   // + the work counters
            }
            if (k == nlev - 1) {
                pt.top_ops[o] = op;
                if (lazy) {
                    pt.ops.pop_back();
                    continue;
                }
            }
            pt.levels.push_back(sgpyr::LevelDesc{o, k, op.fw, op.w, op.h, op.batch, dk,
                                                 op.src_u8 != nullptr,
                                                 (op.zero.n[0] | op.zero.n[1] | op.zero.n[2]) != 0});
        }
    }
    pt.gauss_filters = (int)pt.ops.size();
    return SGPU_OK;
}

// The planner's support queries, answered from the real level filters.
struct OpSupport {
    const sgk::LevelOp* op;
    bool tile(int i) const { return sgk::gauss_tile_supported(op[i]); }
    bool tile_duo(int i, int j) const { return sgk::gauss_tile_duo_supported(op[i], op[j]); }
    bool duo(int i, int j) const { return sgk::gauss_duo_supported(op[i], op[j]); }
    bool trio(int i, int j, int l) const { return sgk::gauss_trio_supported(op[i], op[j], op[l]); }
};

// The planner's rules from the context's switches and debug flags.
// Stream layout (SGPU_STREAMS=multi, not the default: extract_body): octaves >= 1 run on a second
// stream, which starts as soon as octave 0's level kds has written octave 1's base (level 0), so
// their small launches run beside octave 0's last levels (pyramid 3.64 vs 3.69-3.74 ms per 128 x
// 1080p), and the main stream waits for them before the extremum kernel.
// SGPU_DEBUG_PYR_SERIAL: one stream for the pyramid only.
static sgpyr::Rules pyramid_rules(const sgpu_ctx* ctx, const Part& pt) {
    const int f = ctx->debug_flags;
    sgpyr::Rules R;
    R.kds = ctx->sched.level_ds - ctx->sched.level_min;
    R.side_stream = !pt.one_stream;
    R.serial = (f & SGPU_DEBUG_PYR_SERIAL) != 0;
    R.wave_rows = (f & SGPU_DEBUG_GAUSS_BLOCK) ? -1 : ((f >> SGPU_DEBUG_BAND_SHIFT) & 0x7ff);
    R.long_bands = (f & SGPU_DEBUG_GAUSS_LONG_BANDS) != 0;
    R.tiles_off = (f & SGPU_DEBUG_GAUSS_TILE_OFF) != 0;
    R.tiles_always = (f & SGPU_DEBUG_GAUSS_TILE_ALWAYS) != 0;
    R.tile_mb = ctx->tile_mb;
    R.tile_duo = ctx->tile_duo;
    R.duo_off = (f & SGPU_DEBUG_DUO_OFF) != 0;
    R.duo_always = (f & SGPU_DEBUG_DUO_ALWAYS) != 0;
    R.duo_on = ctx->duo_on;
    R.duo_wide = ctx->duo_wide;
    R.duo_u8 = ctx->duo_u8;
    R.trio_mode = ctx->trio_mode;
    R.duo_plan = ctx->duo_plan;
    return R;
}
static_assert(SGPU_TRIO_OFF == sgpyr::kTrioOff && SGPU_TRIO_ON == sgpyr::kTrioOn &&
              SGPU_TRIO_ALWAYS == sgpyr::kTrioAlways && SGPU_PAIRS_FRONT == sgpyr::kPairsFront &&
              SGPU_PAIRS_END == sgpyr::kPairsEnd, "sgpu.h and sift_pyramid_plan.h agree");

// k_gauss_duo's / k_gauss_trio's scratch stores (grow-only, shared by the context's parts)
static int ensure_gauss_trash(sgpu_ctx* ctx) {
    ALLOCCHK(ctx, ctx->duo_trash.ensure(std::max(sgk::kGaussDuoTrashBytes, sgk::kGaussTrioTrashBytes)));
    return SGPU_OK;
}

// Queue the whole pipeline of one part on its stream.  `wait` (may be null) is an event the
// part's pyramid must wait for.  No host synchronisation.
static int enqueue_part(sgpu_ctx* ctx, Part& pt, const void* src_in, bool is_f32, int stride,
                        hipEvent_t wait, hipEvent_t wait_lo = nullptr) {
    hipStream_t st = pt.stream;   // reassigned per stage below
    const sgpu_options& O = ctx->opt;
    const int n = pt.n, h = ctx->h;
    const int rc_layout = layout_part(ctx, pt);
    if (rc_layout != SGPU_OK) return rc_layout;
    const sgk::FeatureParams& fp = pt.fp;
    const long long moff = pt.mask_words;
    const size_t nc = pt.cand_cap, ne_cap = 2 * nc;

    if (wait) HIPCHK(ctx, hipStreamWaitEvent(st, wait, 0));
    // stage events: always where a stream waits on them (the multi-stream layouts, the
    // host-in / host-out stream), else only when the context times its stages
    pt.events = ctx->stage_timing || !pt.one_stream || ctx->nparts > 1 || ctx->streaming;
    auto rec = [&](int i, hipStream_t s_) -> hipError_t {
        return pt.events ? hipEventRecord(pt.ev[i], s_) : hipSuccess;
    };
    HIPCHK(ctx, rec(0, st));
    const size_t img_elems = (size_t)stride * h;
    const uint8_t* src8 = is_f32 ? nullptr : (const uint8_t*)src_in + (size_t)pt.img0 * img_elems;
    const float* srcf = is_f32 ? (const float*)src_in + (size_t)pt.img0 * img_elems : nullptr;

    // ---- Gaussian pyramid (BuildPyramid, PyramidCU.cpp:979-1044) for the whole part: the level
    // filters, the planner's launch list for them (sift_pyramid_plan.h: every schedule decision
    // is made there), and one launch per entry.
    float* pyr = pt.pyr.as<float>();
    // a cache-resident pyramid (the same size rule as the level tiles): the tile extremum kernel
    const bool ext_small = 4ll * fp.oct[0].wa * fp.oct[0].h * n <= ((long long)ctx->tile_mb << 20);
    const bool ext_tiles = !(ctx->debug_flags & SGPU_DEBUG_EXTREMA_TILE_OFF) &&
                           ((ctx->debug_flags & SGPU_DEBUG_GAUSS_TILE_ALWAYS) || ext_small);
    // The octaves' last level is left out where the wave-streaming extremum kernel
    // runs because the size rule chose it (SGPU_TOP_LEVEL_RULE, shipped), or wherever it runs
    // (SGPU_TOP_LEVEL_LAZY); the tile extremum kernel always gets the dense pyramid.
    pt.lazy = !ext_tiles && ctx->top_level != SGPU_TOP_LEVEL_DENSE &&
              (ctx->top_level == SGPU_TOP_LEVEL_LAZY || !ext_small);
    pt.top_dense.assign(ctx->oct.size(), pt.lazy ? 0 : 1);
    const int rc_ops = build_level_ops(ctx, pt, src8, srcf, stride, st, pt.lazy);
    if (rc_ops != SGPU_OK) return rc_ops;
    const sgpyr::Rules R = pyramid_rules(ctx, pt);
    sgpyr::plan_pyramid(pt.levels.data(), (int)pt.levels.size(), R, OpSupport{pt.ops.data()}, pt.plan);
    const int rc_trash = pt.plan.trash ? ensure_gauss_trash(ctx) : SGPU_OK;
    if (rc_trash != SGPU_OK) return rc_trash;
    const bool side = pt.plan.side;
    float* const trash = ctx->duo_trash.as<float>();
    pt.gauss_launches = 0;   // kernel launches of the level filters (sgpu_last_pyramid_launches)
    for (const sgpyr::Launch& l : pt.plan.launches) {
        const hipStream_t s_ = l.side ? pt.stream_oct : st;
        const sgk::LevelOp& a = pt.ops[l.op[0]];
        const sgk::LevelOp& b = pt.ops[std::max(l.op[1], 0)];   // (a again where the kind has no b, c)
        const sgk::LevelOp& c = pt.ops[std::max(l.op[2], 0)];
        int nl = 1;   // the two-job launchers report 1 or 2
        if (l.wait_ds) HIPCHK(ctx, hipStreamWaitEvent(s_, pt.ev_ds, 0));
        switch (l.kind) {
            case sgpyr::kLevel: HIPCHK(ctx, sgk::launch_gauss_op(a, s_, R.wave_rows, R.long_bands)); break;
            case sgpyr::kTile: HIPCHK(ctx, sgk::launch_gauss_tile(a, s_)); break;
            case sgpyr::kTwo: HIPCHK(ctx, sgk::launch_gauss_two(a, b, s_, R.wave_rows, R.long_bands, &nl)); break;
            case sgpyr::kTileTwo: HIPCHK(ctx, sgk::launch_gauss_tile_two(a, b, s_, &nl)); break;
            case sgpyr::kTileDuo: HIPCHK(ctx, sgk::launch_gauss_tile_duo(a, b, s_)); break;
            case sgpyr::kTileDuoOne: HIPCHK(ctx, sgk::launch_gauss_tile_duo_one(a, b, c, s_, &nl)); break;
            case sgpyr::kDuo:
                HIPCHK(ctx, sgk::launch_gauss_duo(a, b, s_, R.wave_rows, trash, ctx->duo_strips));
                break;
            case sgpyr::kTrio: HIPCHK(ctx, sgk::launch_gauss_trio(a, b, c, s_, R.wave_rows, trash)); break;
            default: return ctx->fail(SGPU_EINVAL, "unknown pyramid launch kind");
        }
        pt.gauss_launches += nl;
        if (l.rec_ds) HIPCHK(ctx, hipEventRecord(pt.ev_ds, st));
    }
    if (side) {
        HIPCHK(ctx, hipEventRecord(pt.ev_oct, pt.stream_oct));
        HIPCHK(ctx, hipStreamWaitEvent(st, pt.ev_oct, 0));
    }
    HIPCHK(ctx, rec(1, st));

    // ---- extrema + row scan (the strip extremum kernel only sets the bits it accepts)
    // (the row counts and the mask start zeroed: on one stream the first level launch zeroed
    // them and the orientation counts; otherwise one launch here, and the orientation counts
    // are zeroed on the feature stream after its waits)
    if (!pt.one_stream)
        HIPCHK(ctx, sgk::launch_zero(pt.row_count.as<uint32_t>(), (size_t)pt.total_rows,
                                     pt.mask.as<uint32_t>(), (size_t)moff, nullptr, 0, st));
    HIPCHK(ctx, sgk::launch_extrema(pyr, pt.mask.as<uint32_t>(), pt.row_count.as<uint32_t>(),
                                    fp, st, ext_tiles, pt.lazy));
    if (pt.lazy) {   // the pending pixels of the top DoG level: evaluate, test, count or clear
        sgk::TopLevelFilter tf;
        tf.fw = pt.top_ops[0].fw;
        tf.taps = pt.top_ops[0].taps;
        HIPCHK(ctx, sgk::launch_extrema_top(pyr, pt.mask.as<uint32_t>(), pt.row_count.as<uint32_t>(),
                                            fp, tf, st));
    }
    if (O.feature_count_threshold > 0)   // -tc: GenerateFeatureList skip + LimitFeatureCount(0)
        HIPCHK(ctx, sgk::launch_limit_rows(pt.row_count.as<uint32_t>(), fp,
                                           O.feature_count_threshold, O.truncate_method, st));
    HIPCHK(ctx, rec(7, st));
    HIPCHK(ctx, sgk::launch_scan(pt.row_count.as<uint32_t>(), pt.row_base.as<uint32_t>(),
                                 pt.total_rows, pt.scan_tmp.as<uint32_t>(), st));
    HIPCHK(ctx, rec(2, st));

    // ---- orientation (+ keypoint refinement), expansion, descriptors on the low-priority
    // stream: counts stay on the device, grids come from the previous call's counts (the
    // kernels grid-stride over whatever the device count is)
    if (!pt.one_stream) {
        st = pt.stream_lo;
        HIPCHK(ctx, hipStreamWaitEvent(st, pt.ev[2], 0));
    }
    if (wait_lo) HIPCHK(ctx, hipStreamWaitEvent(st, wait_lo, 0));   // previous features read out
    const uint32_t* n_cand_dev = pt.row_base.as<uint32_t>() + pt.total_rows;
    if (!pt.one_stream)
        HIPCHK(ctx, sgk::launch_zero(pt.ocount.as<uint32_t>(), sgk::feature_queue_base(nc) + sgk::kFeatureQueueWords,
                                     nullptr, 0, nullptr, 0, st));
    // the persistent form of the quad orientation and the one-wave descriptor kernels: this
    // part's own work counters, behind its orientation counts and zeroed with them (the parts of
    // a batch and the batches of sgpu_extract_stream run side by side)
    sgk::FeatureQueue fq = ctx->fq;
    fq.next = pt.ocount.as<uint32_t>() + sgk::feature_queue_base(nc);
    const int cand_grid = (int)std::min(nc, pt.cand_hint ? pt.cand_hint : nc);
    // few candidates (a single image): one wave per candidate instead of a quad, so that the
    // SIMDs are filled and each window is walked 64 samples at a time (same bits)
    const bool ori_wave = (ctx->debug_flags & SGPU_DEBUG_ORIENT_WAVE) ||
                          (pt.cand_hint > 0 && pt.cand_hint <= ctx->wave_orient_max);
    const int feat_grid = (int)std::min(ne_cap, pt.feat_hint ? pt.feat_hint : ne_cap);
    // few features (a single image): a workgroup of 4 waves per feature instead of one wave
    // (k_descriptor_wide, same bits)
    const bool desc_wide = !(ctx->debug_flags & SGPU_DEBUG_DESC_WIDE_OFF) &&
                           ((ctx->debug_flags & SGPU_DEBUG_DESC_WIDE_ALWAYS) ||
                            (pt.feat_hint > 0 && pt.feat_hint <= ctx->wide_desc_max));
    HIPCHK(ctx, sgk::launch_orientation(pyr, pt.mask.as<uint32_t>(), pt.row_base.as<uint32_t>(),
                                        pt.total_rows, n_cand_dev, (int)nc, cand_grid, fp,
                                        pt.cand.as<float4>(), pt.info.as<int2>(),
                                        pt.ocount.as<uint32_t>(), st, ori_wave,
                                        ctx->queue_ori ? &fq : nullptr));
    if (O.feature_count_threshold > 0 && fp.num_orientation >= 2)   // LimitFeatureCount(1)
        HIPCHK(ctx, sgk::launch_limit_oriented(pt.ocount.as<uint32_t>(), pt.row_base.as<uint32_t>(),
                                               fp, O.feature_count_threshold, O.truncate_method,
                                               (uint32_t)nc, st));
    HIPCHK(ctx, rec(3, st));
    const uint32_t* n_feat_dev = pt.eoff.as<uint32_t>() + nc;
    // (the expansion launch also writes the readback record: candidate count + per-image offsets)
    sgk::ImageOffsetsArgs io;
    io.row_base = pt.row_base.as<uint32_t>();
    io.batch = n;
    io.rows_per_image = fp.rows_per_image;
    io.total_rows = pt.total_rows;
    io.off = pt.img_off_dev.as<int64_t>();
    // (the scan and the expansion in one single-workgroup launch measured slower for one image:
    // 17.0-17.5 against ~13.5 us for the two launches)
    HIPCHK(ctx, sgk::launch_scan(pt.ocount.as<uint32_t>(), pt.eoff.as<uint32_t>(), nc,
                                 pt.scan_tmp.as<uint32_t>(), st));
    HIPCHK(ctx, sgk::launch_expand(pt.cand.as<float4>(), pt.info.as<int2>(),
                                   pt.eoff.as<uint32_t>(), n_cand_dev, (int)nc, fp,
                                   pt.feat.as<float4>(), pt.feat_info.as<int2>(),
                                   pt.keys.as<float4>(), st, &io));
    HIPCHK(ctx, rec(4, st));
    // one image with registered host buffers: its keys, descriptors and count record go straight
    // to the host (enqueue_readback then copies nothing) -- from the workgroup-per-feature
    // descriptor kernel itself when it runs (written over the host link while it computes), else
    // by k_copy_out after it
    pt.copied_out = ctx->host_out.active && pt.one_stream && n == 1 && ctx->nparts == 1;
    const bool exact_desc = ctx->debug_flags & SGPU_DEBUG_EXACT_DESCRIPTOR;
    const bool dual_desc = ctx->debug_flags & SGPU_DEBUG_DESC_DUAL;
    const bool host_in_desc = pt.copied_out && O.descriptors && desc_wide && !exact_desc && !dual_desc;
    sgk::HostCopy hcopy;
    if (host_in_desc) {
        hcopy.keys = pt.keys.as<float4>();
        hcopy.rec = pt.img_off_dev.as<int64_t>();
        hcopy.rec_n = n + 2;
        hcopy.cap = (uint32_t)ctx->host_out.cap;
        hcopy.hkeys = reinterpret_cast<float4*>(ctx->host_out.keys);
        hcopy.hdesc = ctx->host_out.desc;
        hcopy.hrec = pt.h_read;
    }
    if (O.descriptors) {
        sgk::DescriptorForm form;
        form.exact = exact_desc;
        form.dual = dual_desc;
        form.wide = desc_wide;
        form.host = host_in_desc ? &hcopy : nullptr;
        form.queue = ctx->queue_desc ? &fq : nullptr;
        HIPCHK(ctx, sgk::launch_descriptor(pyr, pt.feat.as<float4>(), pt.feat_info.as<int2>(),
                                           n_feat_dev, feat_grid, fp, pt.desc.as<float>(), form, st));
    }
    HIPCHK(ctx, rec(5, st));
    if (pt.copied_out && !host_in_desc)
        HIPCHK(ctx, sgk::launch_copy_out(pt.keys.as<float4>(), O.descriptors ? pt.desc.as<float>() : nullptr,
                                         n_feat_dev, ctx->host_out.cap, pt.img_off_dev.as<int64_t>(),
                                         n + 2, ctx->host_out.keys,
                                         O.descriptors ? ctx->host_out.desc : nullptr, pt.h_read, st));
    return SGPU_OK;
}

// Queue the (pinned) readback of a part's counts and offsets.
static int enqueue_readback(sgpu_ctx* ctx, Part& pt) {
    hipStream_t st = pt.one_stream ? pt.stream : pt.stream_lo;
    // one copy: [0] = the candidate count, [1 .. n + 1] = the per-image feature offsets (the
    // record k_expand writes); none when k_copy_out wrote it with the features
    if (!pt.copied_out)
        HIPCHK(ctx, hipMemcpyAsync(pt.h_read, pt.img_off_dev.p, (size_t)(pt.n + 2) * sizeof(int64_t),
                                   hipMemcpyDeviceToHost, st));
    if (pt.events) HIPCHK(ctx, hipEventRecord(pt.ev[6], st));
    return SGPU_OK;
}

// Geometry of a batch of n images of w x h (first octave: GLTexInput::SetImageData +
// PyramidCU::InitPyramid with -fo, -prep, -maxd; octaves; sigma schedule) into the context.
static int plan_batch(sgpu_ctx* ctx, int n, int w, int h) {
    const sgpu_options& O = ctx->opt;
    const sgp::InputPlan plan = sgp::plan_input(w, h, O.octave_min, O.max_dimension, O.preprocess_on_cpu);
    if (plan.w < 8 || plan.h < 8) return ctx->fail(SGPU_EINVAL, "image too small for the first octave");
    {
        sgp::Options po;
        po.filter_width_factor = O.filter_width_factor;
        po.dog_level_num = O.dog_level_num;
        po.dog_threshold = O.dog_threshold;
        po.edge_threshold = O.edge_threshold;
        po.octave_min = plan.octave_min + plan.ds;   // GetInitialSmoothSigma(_octave_min + ds)
        ctx->sched = sgp::make_schedule(po);
    }
    ctx->plan = plan;
    ctx->oct = sgp::make_octaves(plan.w, plan.h, O.octave_num, plan.octave_min);
    const int noct = (int)ctx->oct.size();
    if (noct > sgk::kMaxOctaves) return ctx->fail(SGPU_EINVAL, "too many octaves");
    for (const auto& oc : ctx->oct)
        if (oc.w < 4 || oc.h < 4) return ctx->fail(SGPU_EINVAL, "image too small for the octave count");
    ctx->batch = n;
    ctx->w = plan.ds ? plan.w : w;
    ctx->h = plan.h;
    ctx->gathered = false;
    ctx->f_ready = false;
    return SGPU_OK;
}

// After a failed extract nothing may still be queued that reads the caller's input or writes
// the caller's outputs, and no per-image query may read the previous extract's offsets (the
// batch geometry was already replaced): wait for every stream of the context, then forget the
// batch.
static int abandon_batch(sgpu_ctx* ctx, int rc) {
    ctx->host_out.done = false;
    for (hipStream_t st : {ctx->stream, ctx->h2d, ctx->d2h})
        if (st) (void)hipStreamSynchronize(st);
    for (Part& pt : ctx->part) {
        if (pt.stream) (void)hipStreamSynchronize(pt.stream);
        if (pt.stream_lo) (void)hipStreamSynchronize(pt.stream_lo);
        if (pt.stream_oct) (void)hipStreamSynchronize(pt.stream_oct);
        pt.img_off.clear();
    }
    ctx->batch = 0;
    ctx->img_off.clear();
    ctx->gathered = false;
    ctx->f_ready = false;
    return rc;
}

// Argument checks of sgpu_extract*: a rejected call queues nothing and leaves the previous
// extract's results readable.
static int check_extract_args(sgpu_ctx* ctx, const void* images, bool is_f32, int n, int w, int h,
                              int stride, int flags, int color) {
    const bool staged = (flags & SGPU_INPUT_STAGED) != 0;
    const int channels = color == SGPU_RGB || color == SGPU_BGR ? 3 : color ? 4 : 1;
    if ((!images && !staged) || n <= 0 || w < 8 || h < 8 || stride < w * channels)
        return ctx->fail(SGPU_EINVAL, "bad image arguments");
    if (color && (staged || is_f32 || color > SGPU_BGRA))
        return ctx->fail(SGPU_EINVAL, "bad color input");
    if (staged && (is_f32 || ctx->staged_bytes < (size_t)n * h * stride))
        return ctx->fail(SGPU_EINVAL, "staged input does not match the batch");
    return SGPU_OK;
}

static int extract_body(sgpu_ctx* ctx, const void* images, bool is_f32, int n, int w, int h,
                        int stride, int flags, int color) {
    // a caller's float image may hold any range; u8, colour and the library's own conversions of
    // them lie in [0, 1] (FeatureParams::unit_input; the shipped 64-bit descriptor sums hold for both)
    ctx->unit_input = !is_f32;
    const bool staged = (flags & SGPU_INPUT_STAGED) != 0;
    const int channels = color == SGPU_RGB || color == SGPU_BGR ? 3 : color ? 4 : 1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc0 = plan_batch(ctx, n, w, h);
    if (rc0 != SGPU_OK) return rc0;
    const sgp::InputPlan plan = ctx->plan;

    // parts: one by default.  Measured on MI355X (profiles/): a second
    // part's pyramid starves beside the previous part's descriptor kernel (the dispatcher keeps
    // filling the CUs with descriptor workgroups despite the stream priorities), so splitting
    // does not pay yet.  Test hook: SGPU_DEBUG_PARTS2 / SGPU_DEBUG_PARTS4.
    int np = 1;
    if ((ctx->debug_flags & SGPU_DEBUG_PARTS2) && n >= 2) np = 2;
    if ((ctx->debug_flags & SGPU_DEBUG_PARTS4) && n >= 4) np = 4;
    ctx->nparts = np;
    for (int p = 0; p < np; p++)
        if (part_streams(ctx->part[p]) != SGPU_OK)
            return ctx->fail(SGPU_ENODEV, "stream creation failed");
    for (int p = 0, i0 = 0; p < np; p++) {
        const int cnt = n / np + (p < n % np ? 1 : 0);
        ctx->part[p].img0 = i0;
        ctx->part[p].n = cnt;
        ctx->part[p].one_stream = false;
        i0 += cnt;
    }
    // A single-part batch runs upload, pyramid and feature stages on one stream.  Measured
    // (alternating processes): the octave stream and the feature stream, each
    // joined by a cross-stream event wait, cost more than their overlap gains -- C2 (one image
    // through SiftGPU::RunSIFT) 0.50 vs 0.56-0.61 ms per image, the 128 x 1080p batch 15.26-15.33k
    // vs 14.50-14.75k images/s (extrema 1.72 vs 1.92 ms, orientation 0.50 vs 0.55 ms after the
    // waits).  SGPU_STREAMS=multi keeps the stream layout (A/B hook).
    const bool one = np == 1 && !ctx->multi_stream;
    ctx->part[0].one_stream = one;
    const hipStream_t up = one ? ctx->part[0].stream : ctx->stream;

    // input: host batches are uploaded first on the context stream.  The upload's events are
    // recorded only when there is input work to time or a stream to join: every event record
    // in a stream costs ~4.5 us of GPU time between the commands around it, whatever its flags
    // (tests/microbench/event_gap.hip: 2.2 vs 6.7 us per short kernel), and a staged or device
    // batch on one stream has neither (C2, the bench's batches)
    const size_t in_bytes = (size_t)n * h * stride * (is_f32 ? sizeof(float) : 1);
    const bool up_events = !one || ((color || plan.ds > 0 ||
                                     !(flags & (SGPU_INPUT_DEVICE | SGPU_INPUT_STAGED))) &&
                                    ctx->stage_timing);
    if (up_events) HIPCHK(ctx, hipEventRecord(ctx->ev[0], up));
    const void* src_in = staged ? ctx->input.p : images;
    if (!(flags & (SGPU_INPUT_DEVICE | SGPU_INPUT_STAGED))) {
        ctx->staged_bytes = 0;
        ALLOCCHK(ctx, ctx->input.ensure(in_bytes));
        HIPCHK(ctx, hipMemcpyAsync(ctx->input.p, images, in_bytes, hipMemcpyHostToDevice, up));
        src_in = ctx->input.p;
    }
    if (color) {
        // luminance on the device; the pipeline then takes it as float input, tw floats a row
        const int tw = w & ~3;
        ALLOCCHK(ctx, ctx->gray.ensure((size_t)n * h * tw * sizeof(float)));
        HIPCHK(ctx, sgk::launch_color_to_gray((const uint8_t*)src_in, n, w, h, stride, channels,
                                              color == SGPU_BGR || color == SGPU_BGRA,
                                              ctx->gray.as<float>(), up));
        src_in = ctx->gray.p;
        is_f32 = true;
        stride = tw;
    }
    if (plan.ds > 0) {
        // -fo > 0 with -prep (GLTexInput::SetImageData -> DownSamplePixelDataI2F/F,
        // GLTexImage.cpp:928-1009): pixel (r << ds, c << ds) of the input, plan.w x plan.h
        // (the sampled columns never reach the truncated-away ones)
        const size_t px = (size_t)plan.w * plan.h;
        ALLOCCHK(ctx, ctx->pre.ensure((size_t)n * px * sizeof(float)));
        HIPCHK(ctx, sgk::launch_first_octave_input(is_f32 ? (const float*)src_in : nullptr,
                                                   is_f32 ? nullptr : (const uint8_t*)src_in,
                                                   stride, (long long)stride * h, w & ~3, h, plan.ds,
                                                   ctx->pre.as<float>(), plan.w, plan.h,
                                                   (long long)px, n, up));
        src_in = ctx->pre.p;
        is_f32 = true;
        stride = plan.w;
    }
    if (up_events) HIPCHK(ctx, hipEventRecord(ctx->ev[1], up));

    // part p's pyramid starts when part p-1 has finished detection
    for (int p = 0; p < np; p++) {
        hipEvent_t wait = p == 0 ? (one ? nullptr : ctx->ev[1]) : ctx->part[p - 1].ev[2];
        int rc = enqueue_part(ctx, ctx->part[p], src_in, is_f32, stride, wait);
        if (rc != SGPU_OK) return rc;
    }
    for (int p = 0; p < np; p++) {
        int rc = enqueue_readback(ctx, ctx->part[p]);
        if (rc != SGPU_OK) return rc;
    }
    for (int p = 0; p < np; p++) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->part[p].stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->part[p].stream_lo));
    }

    // capacity check: a part whose candidates overflowed is re-run with larger buffers
    for (int p = 0; p < np; p++) {
        Part& pt = ctx->part[p];
        uint32_t nc = (uint32_t)pt.h_read[0];
        if (nc > pt.cand_cap) {
            pt.cand_cap = (size_t)nc + nc / 4 + 1024;
            int rc = enqueue_part(ctx, pt, src_in, is_f32, stride, nullptr);
            if (rc == SGPU_OK) rc = enqueue_readback(ctx, pt);
            if (rc != SGPU_OK) return rc;
            HIPCHK(ctx, hipStreamSynchronize(pt.one_stream ? pt.stream : pt.stream_lo));
            nc = (uint32_t)pt.h_read[0];
            if (nc > pt.cand_cap) return ctx->fail(SGPU_ERANGE, "keypoint capacity overflow");
        }
        pt.n_cand = nc;
        pt.img_off.assign(pt.h_read + 1, pt.h_read + 2 + pt.n);
        pt.cand_hint = (size_t)nc + nc / 16 + 64;
        pt.feat_hint = (size_t)pt.img_off[pt.n] + pt.img_off[pt.n] / 16 + 64;
    }
    ctx->img_off.assign(n + 1, 0);
    int64_t base = 0;
    for (int p = 0; p < np; p++) {
        const Part& pt = ctx->part[p];
        for (int i = 0; i <= pt.n; i++) ctx->img_off[pt.img0 + i] = base + pt.img_off[i];
        base += pt.img_off[pt.n];
    }

    // timings: stages of part 0 (its pyramid and detection run alone), total over all parts
    Part& p0 = ctx->part[0];
    ctx->timing[T_UPLOAD] = 0.0f;
    if (!p0.events) {   // sgpu_set_stage_timing(ctx, 0): no stage events were recorded
        for (int i = T_UPLOAD; i <= T_DOWNLOAD; i++) ctx->timing[i] = 0.0f;
        ctx->timing[T_TOTAL] = ctx->timing[T_LIST] = 0.0f;
        return SGPU_OK;
    }
    if (up_events) (void)hipEventElapsedTime(&ctx->timing[T_UPLOAD], ctx->ev[0], ctx->ev[1]);
    (void)hipEventElapsedTime(&ctx->timing[T_PYRAMID], p0.ev[0], p0.ev[1]);
    (void)hipEventElapsedTime(&ctx->timing[T_DETECT], p0.ev[1], p0.ev[2]);
    (void)hipEventElapsedTime(&ctx->timing[T_LIST], p0.ev[7], p0.ev[2]);
    (void)hipEventElapsedTime(&ctx->timing[T_ORIENT], p0.ev[2], p0.ev[3]);
    (void)hipEventElapsedTime(&ctx->timing[T_EXPAND], p0.ev[3], p0.ev[4]);
    (void)hipEventElapsedTime(&ctx->timing[T_DESC], p0.ev[4], p0.ev[5]);
    (void)hipEventElapsedTime(&ctx->timing[T_DOWNLOAD], p0.ev[5], p0.ev[6]);
    (void)hipEventElapsedTime(&ctx->timing[T_TOTAL], up_events ? ctx->ev[0] : p0.ev[0], ctx->part[np - 1].ev[6]);
    return SGPU_OK;
}

static int extract_impl(sgpu_ctx* ctx, const void* images, bool is_f32, int n, int w, int h,
                        int stride, int flags, int color = 0) {
    if (!ctx) return SGPU_EINVAL;
    // a registered host output serves this extract only (consumed even when the extract is
    // rejected: ADVICE r05), and only one image
    const bool armed = ctx->host_out.armed;
    ctx->host_out.armed = false;
    ctx->host_out.done = false;
    const int rc_args = check_extract_args(ctx, images, is_f32, n, w, h, stride, flags, color);
    if (rc_args != SGPU_OK) return rc_args;
    ctx->host_out.active = armed && n == 1;
    const int rc = extract_body(ctx, images, is_f32, n, w, h, stride, flags, color);
    ctx->host_out.done = rc == SGPU_OK && ctx->host_out.active && ctx->nparts == 1 &&
                         ctx->part[0].copied_out;
    ctx->host_out.active = false;
    ctx->part[0].copied_out = ctx->part[1].copied_out = false;
    return rc == SGPU_OK ? rc : abandon_batch(ctx, rc);
}

// Host-in / host-out extraction of a stream of batches: SiftGPU::RunSIFT(w, h, data) per image
// followed by GetFeatureVector, i.e. with the reference's input upload (PyramidCU.cpp:949-976)
// and descriptor download (PyramidCU.cpp:434) in the measured work.  Two slots -- parts 0 and 1
// with their own buffers, two device input buffers -- alternate between batches: the upload of
// batch k+1 (host-to-device copy engine) and the download of batch k-1's keys and descriptors
// (device-to-host copy engine) run while batch k computes.  Kernels of consecutive batches stay
// in order (batch k+1's pyramid waits for batch k's last kernel), so every batch sees the whole
// GPU as in sgpu_extract.  One host wait per batch: the small count readback of batch k-1, needed
// to size its download, happens after batch k is queued.
static int extract_stream_body(sgpu_ctx* ctx, const uint8_t* const* batches, int nbatches,
                               int batch, int w, int h, int stride, float* keys, float* desc,
                               int64_t cap, int32_t* counts) {
    if (!batches || nbatches <= 0 || batch <= 0 || w < 8 || h < 8 || stride < w || !counts ||
        cap < 0)
        return ctx->fail(SGPU_EINVAL, "bad stream arguments");
    for (int k = 0; k < nbatches; k++)
        if (!batches[k]) return ctx->fail(SGPU_EINVAL, "null batch pointer");
    if (desc && !ctx->opt.descriptors) return ctx->fail(SGPU_EINVAL, "descriptors disabled (-sd)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = plan_batch(ctx, batch, w, h);
    if (rc != SGPU_OK) return rc;
    int64_t out_base = 0;
    int result = SGPU_OK;
    auto emit_counts = [&](int k, const std::vector<int64_t>& off, int n) {
        for (int i = 0; i < n; i++) counts[(size_t)k * batch + i] = (int32_t)(off[i + 1] - off[i]);
    };
    if (ctx->plan.ds > 0) {
        // -fo > 0 with -prep samples the input on the device first (extract_impl): no overlap,
        // batch by batch
        for (int k = 0; k < nbatches; k++) {
            rc = extract_impl(ctx, batches[k], false, batch, w, h, stride, SGPU_INPUT_HOST);
            if (rc != SGPU_OK) return rc;
            emit_counts(k, ctx->img_off, batch);
            const int64_t nf = ctx->img_off[batch];
            if (out_base + nf > cap) {
                result = ctx->fail(SGPU_ERANGE, "features exceed the output capacity");
            } else if (nf > 0) {
                const Part& pt = ctx->part[0];
                if (keys)
                    HIPCHK(ctx, hipMemcpy(keys + out_base * 4, pt.keys.p, nf * sizeof(float4),
                                          hipMemcpyDeviceToHost));
                if (desc)
                    HIPCHK(ctx, hipMemcpy(desc + out_base * 128, pt.desc.p,
                                          nf * 128 * sizeof(float), hipMemcpyDeviceToHost));
            }
            out_base += nf;
        }
        return result;
    }
    if (part_streams(ctx->part[1]) != SGPU_OK)
        return ctx->fail(SGPU_ENODEV, "stream creation failed");
    if (!ctx->h2d) {   // created with the context; kept for a context whose creation order changes
        HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->h2d, hipStreamNonBlocking));
        HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->d2h, hipStreamNonBlocking));
        for (int i = 0; i < 2; i++) {
            HIPCHK(ctx, hipEventCreateWithFlags(&ctx->up_ev[i], hipEventDisableTiming));
            HIPCHK(ctx, hipEventCreateWithFlags(&ctx->down_ev[i], hipEventDisableTiming));
        }
    }
    const size_t in_bytes = (size_t)batch * h * stride;
    // each slot's kernels on its own stream (extract_body's measurement); slots and copies overlap
    ctx->part[0].one_stream = ctx->part[1].one_stream = !ctx->multi_stream;
    ctx->staged_bytes = 0;
    ALLOCCHK(ctx, ctx->input.ensure(in_bytes));
    ALLOCCHK(ctx, ctx->input2.ensure(in_bytes));
    void* din[2] = {ctx->input.p, ctx->input2.p};
    ctx->nparts = 1;
    // batch k's results: wait for its counts, re-run it on overflow, queue its download
    auto finish = [&](int k) -> int {
        Part& pt = ctx->part[k & 1];
        HIPCHK(ctx, hipEventSynchronize(pt.ev[6]));
        uint32_t nc = (uint32_t)pt.h_read[0];
        if (nc > pt.cand_cap) {
            pt.cand_cap = (size_t)nc + nc / 4 + 1024;
            int r = enqueue_part(ctx, pt, din[k & 1], false, stride, nullptr, nullptr);
            if (r == SGPU_OK) r = enqueue_readback(ctx, pt);
            if (r != SGPU_OK) return r;
            HIPCHK(ctx, hipStreamSynchronize(pt.one_stream ? pt.stream : pt.stream_lo));
            nc = (uint32_t)pt.h_read[0];
            if (nc > pt.cand_cap) return ctx->fail(SGPU_ERANGE, "keypoint capacity overflow");
        }
        pt.n_cand = nc;
        pt.img_off.assign(pt.h_read + 1, pt.h_read + 2 + pt.n);
        pt.cand_hint = (size_t)nc + nc / 16 + 64;
        pt.feat_hint = (size_t)pt.img_off[pt.n] + pt.img_off[pt.n] / 16 + 64;
        emit_counts(k, pt.img_off, pt.n);
        const int64_t nf = pt.img_off[pt.n];
        if (out_base + nf > cap) {
            result = ctx->fail(SGPU_ERANGE, "features exceed the output capacity");
        } else if (nf > 0) {
            HIPCHK(ctx, hipStreamWaitEvent(ctx->d2h, pt.ev[6], 0));
            if (keys)
                HIPCHK(ctx, hipMemcpyAsync(keys + out_base * 4, pt.keys.p, nf * sizeof(float4),
                                           hipMemcpyDeviceToHost, ctx->d2h));
            if (desc)
                HIPCHK(ctx, hipMemcpyAsync(desc + out_base * 128, pt.desc.p,
                                           nf * 128 * sizeof(float), hipMemcpyDeviceToHost,
                                           ctx->d2h));
        }
        HIPCHK(ctx, hipEventRecord(ctx->down_ev[k & 1], ctx->d2h));
        out_base += nf;
        return SGPU_OK;
    };
    for (int k = 0; k < nbatches; k++) {
        const int slot = k & 1;
        Part& pt = ctx->part[slot];
        pt.img0 = 0;
        pt.n = batch;
        // upload k into its slot once batch k-2's pyramid (the slot's last reader) is done
        if (k >= 2) HIPCHK(ctx, hipStreamWaitEvent(ctx->h2d, pt.ev[1], 0));
        HIPCHK(ctx, hipMemcpyAsync(din[slot], batches[k], in_bytes, hipMemcpyHostToDevice,
                                   ctx->h2d));
        HIPCHK(ctx, hipEventRecord(ctx->up_ev[slot], ctx->h2d));
        // compute k after batch k-1's last kernel; its features overwrite the slot only after
        // batch k-2's download
        if (k >= 1) HIPCHK(ctx, hipStreamWaitEvent(pt.stream, ctx->part[slot ^ 1].ev[5], 0));
        rc = enqueue_part(ctx, pt, din[slot], false, stride, ctx->up_ev[slot],
                          k >= 2 ? ctx->down_ev[slot] : nullptr);
        if (rc == SGPU_OK) rc = enqueue_readback(ctx, pt);
        if (rc == SGPU_OK && k >= 1) rc = finish(k - 1);
        if (rc != SGPU_OK) return rc;
    }
    rc = finish(nbatches - 1);
    if (rc != SGPU_OK) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->d2h));
    return result;
}

int sgpu_extract_stream(sgpu_ctx* ctx, const uint8_t* const* batches, int nbatches, int batch,
                        int w, int h, int stride, float* keys, float* desc, int64_t cap,
                        int32_t* counts) {
    if (!ctx) return SGPU_EINVAL;
    ctx->streaming = true;   // its waits use the slots' stage events
    ctx->host_out.done = false;
    const int rc = extract_stream_body(ctx, batches, nbatches, batch, w, h, stride, keys, desc,
                                       cap, counts);
    ctx->streaming = false;
    // on success as on failure: every copy from the caller's batches and into the caller's
    // outputs has completed, and the per-image queries (sgpu_copy_features, ...) have no "last
    // batch" after a stream
    return abandon_batch(ctx, rc);
}

void* sgpu_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void sgpu_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

// SiftGPU::RunSIFT(num, keys, keys_have_orientation) on image `image` of the last extract
// (SiftPyramid::SetKeypointList with run_on_current, SiftPyramid.cpp:293-310): the keys are
// assigned to levels as GenerateFeatureListTex does (PyramidCU.cpp:454-504, host side: a few
// float ops per key), then the device computes the strongest orientation when the keys have
// none and the descriptors, both written back in input order.  The results replace the
// context's features: image `image` has `num` features, every other image none.
int sgpu_extract_keypoints(sgpu_ctx* ctx, int image, const float* keys, int num,
                           int has_orientation) {
    if (!ctx || !keys || num <= 0) return SGPU_EINVAL;
    ctx->host_out.done = false;   // the features it writes replace what k_copy_out delivered
    if (ctx->batch <= 0 || image < 0 || image >= ctx->batch)
        return ctx->fail(SGPU_EINVAL, "no extracted image to describe keypoints on");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int p = ctx->part_of(image);
    Part& pt = ctx->part[p];
    const int b = image - pt.img0;
    const sgpu_options& O = ctx->opt;
    const sgp::Schedule& S = ctx->sched;
    const int d = S.dog_level_num, noct = (int)ctx->oct.size();
    const double twopi = 2.0 * 3.14159265358979323846;
    const float sigma_half_step = powf(2.0f, 0.5f / d);
    const float offset = O.lowe_origin ? 0.0f : 0.5f;
    const bool rect = has_orientation == -1;
    std::vector<float4> lf;
    std::vector<int2> li;
    std::vector<int> lidx;
    float octave_sigma = ldexpf(1.0f, ctx->plan.octave_min + ctx->plan.ds);   // PyramidCU.cpp:461-463
    for (int i = 0; i < noct; i++, octave_sigma *= 2.0f)
        for (int j = 0; j < d; j++) {
            const float level_sigma = sgp::level_sigma(S, j + S.level_min + 1) * octave_sigma;
            const float sigma_min = level_sigma / sigma_half_step;
            const float sigma_max = level_sigma * sigma_half_step;
            for (int k = 0; k < num; k++) {
                const float* key = keys + 4 * (size_t)k;
                // RECT (keys_have_orientation == -1, SiftPyramid.cpp:308-309): (x, y, width,
                // height) rectangles, levelled by min(width, height) / 12 (PyramidCU.cpp:480)
                const float sigmak = rect ? std::min(key[2], key[3]) / 12.0f : key[2];
                if ((sigmak >= sigma_min && sigmak < sigma_max) ||
                    (sigmak < sigma_min && i == 0 && j == 0) ||
                    (sigmak > sigma_max && i == noct - 1 && j == d - 1)) {
                    lf.push_back(make_float4((key[0] - offset) / octave_sigma + 0.5f,
                                             (key[1] - offset) / octave_sigma + 0.5f,
                                             key[2] / octave_sigma,
                                             rect ? key[3] / octave_sigma
                                                  : (float)std::fmod(twopi - key[3], twopi)));
                    li.push_back(make_int2(b, i * d + j));
                    lidx.push_back(k);
                }
            }
        }
    // the reference re-orders list entries i < num (_featureNum) only
    const int m = std::min<int>(num, (int)lf.size());
    hipStream_t st = ctx->stream;
    const size_t cap = std::max<size_t>(lf.size(), (size_t)num);
    ALLOCCHK(ctx, pt.feat.ensure(cap * sizeof(float4)));
    ALLOCCHK(ctx, pt.feat_info.ensure(cap * sizeof(int2)));
    ALLOCCHK(ctx, pt.keys.ensure((size_t)num * sizeof(float4)));
    ALLOCCHK(ctx, pt.ocount.ensure((cap + 1) * sizeof(int)));   // list -> input index, count
    if (O.descriptors) ALLOCCHK(ctx, pt.desc.ensure((size_t)num * 128 * sizeof(float)));
    int* d_index = pt.ocount.as<int>();
    uint32_t* d_m = pt.ocount.as<uint32_t>() + cap;
    if (m > 0) {
        HIPCHK(ctx, hipMemcpyAsync(pt.feat.p, lf.data(), m * sizeof(float4), hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(pt.feat_info.p, li.data(), m * sizeof(int2), hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(d_index, lidx.data(), m * sizeof(int), hipMemcpyHostToDevice, st));
    }
    const uint32_t mm = (uint32_t)m;
    HIPCHK(ctx, hipMemcpyAsync(d_m, &mm, sizeof(uint32_t), hipMemcpyHostToDevice, st));
    // keys come back unchanged when they carry orientations (no DownloadKeypoints)
    HIPCHK(ctx, hipMemcpyAsync(pt.keys.p, keys, (size_t)num * sizeof(float4), hipMemcpyHostToDevice, st));
    if (!has_orientation)
        HIPCHK(ctx, sgk::launch_orient_keys(pt.pyr.as<float>(), pt.feat.as<float4>(),
                                            pt.feat_info.as<int2>(), d_index, m, pt.fp,
                                            pt.keys.as<float4>(), st));
    if (O.descriptors) {
        HIPCHK(ctx, hipMemsetAsync(pt.desc.p, 0, (size_t)num * 128 * sizeof(float), st));
        sgk::DescriptorForm form;
        form.out_index = d_index;
        form.rect = rect;
        form.exact = (ctx->debug_flags & SGPU_DEBUG_EXACT_DESCRIPTOR) != 0;
        form.dual = (ctx->debug_flags & SGPU_DEBUG_DESC_DUAL) != 0;
        HIPCHK(ctx, sgk::launch_descriptor(pt.pyr.as<float>(), pt.feat.as<float4>(),
                                           pt.feat_info.as<int2>(), d_m, std::max(m, 1), pt.fp,
                                           pt.desc.as<float>(), form, st));
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    // the described image now owns the context's feature list
    for (int q = 0; q < ctx->nparts; q++) {
        Part& pq = ctx->part[q];
        for (int i = 0; i <= pq.n; i++)
            pq.img_off[i] = (q == p && pq.img0 + i > image) ? num : 0;
    }
    for (int i = 0; i <= ctx->batch; i++) ctx->img_off[i] = i > image ? num : 0;
    ctx->gathered = false;
    ctx->f_ready = false;
    return SGPU_OK;
}

int sgpu_stage_input(sgpu_ctx* ctx, const uint8_t* images, int n, int w, int h, int stride) {
    if (!ctx || !images || n <= 0 || stride < w) return SGPU_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)n * h * stride;
    ALLOCCHK(ctx, ctx->input.ensure(bytes));
    HIPCHK(ctx, hipMemcpy(ctx->input.p, images, bytes, hipMemcpyHostToDevice));
    ctx->staged_bytes = bytes;
    return SGPU_OK;
}

// SiftGPU::AllocatePyramid (SiftGPU.cpp:1435-1460: PyramidCU::ResizePyramid for the first
// octave of a width x height input): every device and pinned buffer an extract of n images of
// w x h u8 pixels (rows `stride` bytes apart) needs -- the staged input, the pyramid, the mask,
// the row and candidate arrays at their first-guess capacity -- allocated now, so that the next
// sgpu_stage_input + sgpu_extract of that geometry allocates nothing (unless its keypoints
// exceed the first-guess capacity).  Like an extract it replaces the batch: the previous
// results are gone.
int sgpu_reserve(sgpu_ctx* ctx, int n, int w, int h, int stride) {
    if (!ctx) return SGPU_EINVAL;
    if (n <= 0 || w < 8 || h < 8 || stride < w) return ctx->fail(SGPU_EINVAL, "bad reserve arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = abandon_batch(ctx, SGPU_OK);   // nothing queued may still use the buffers
    ctx->staged_bytes = 0;                  // the input buffer may be reallocated
    if (rc == SGPU_OK) rc = plan_batch(ctx, n, w, h);
    if (rc == SGPU_OK && part_streams(ctx->part[0]) != SGPU_OK)
        rc = ctx->fail(SGPU_ENODEV, "stream creation failed");
    if (rc == SGPU_OK) {
        ctx->nparts = 1;
        Part& pt = ctx->part[0];
        pt.img0 = 0;
        pt.n = n;
        rc = layout_part(ctx, pt);
    }
    if (rc == SGPU_OK && ctx->input.ensure((size_t)n * h * stride) != hipSuccess)
        rc = ctx->fail(SGPU_ENOMEM, "device allocation failed");
    return abandon_batch(ctx, rc);
}

int sgpu_set_host_output(sgpu_ctx* ctx, float* keys, float* descriptors, int capacity) {
    if (!ctx || capacity < 0) return SGPU_EINVAL;
    ctx->host_out.keys = keys;
    ctx->host_out.desc = descriptors;
    ctx->host_out.cap = capacity;
    ctx->host_out.armed = keys != nullptr && capacity > 0;
    ctx->host_out.done = false;
    return SGPU_OK;
}

int sgpu_extract(sgpu_ctx* ctx, const uint8_t* images, int n, int w, int h, int stride,
                 int flags) {
    return extract_impl(ctx, images, false, n, w, h, stride, flags);
}

int sgpu_extract_f32(sgpu_ctx* ctx, const float* images, int n, int w, int h, int stride,
                     int flags) {
    return extract_impl(ctx, images, true, n, w, h, stride, flags);
}

int sgpu_extract_color(sgpu_ctx* ctx, const uint8_t* images, int n, int w, int h, int stride,
                       int format, int flags) {
    if (!ctx) return SGPU_EINVAL;
    if (format < SGPU_RGB || format > SGPU_BGRA) return ctx->fail(SGPU_EINVAL, "bad color format");
    return extract_impl(ctx, images, false, n, w, h, stride, flags, format);
}

int sgpu_feature_count(const sgpu_ctx* ctx, int image) {
    if (!ctx || image < 0 || image >= ctx->batch || ctx->img_off.empty()) return 0;
    return (int)(ctx->img_off[image + 1] - ctx->img_off[image]);
}

int64_t sgpu_feature_total(const sgpu_ctx* ctx) {
    if (!ctx || ctx->img_off.empty()) return 0;
    return ctx->img_off[ctx->batch];
}

int sgpu_copy_features(sgpu_ctx* ctx, int image, float* keys, float* descriptors) {
    if (!ctx || image < 0 || image >= ctx->batch || ctx->img_off.empty()) return SGPU_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const Part& pt = ctx->part[ctx->part_of(image)];
    const int li = image - pt.img0;
    const int64_t a = pt.img_off[li], nf = pt.img_off[li + 1] - a;
    if (nf <= 0) {   // nothing copied: the copy slots read 0, not the previous call's times
        ctx->timing[T_COPY_KEYS] = 0.f;
        ctx->timing[T_COPY_DESC] = 0.f;
        return SGPU_OK;
    }
    if (descriptors && !ctx->opt.descriptors) return ctx->fail(SGPU_EINVAL, "descriptors disabled (-sd)");
    const auto& ho = ctx->host_out;
    if (ho.done && image == 0 && a == 0 && keys == ho.keys && (!descriptors || descriptors == ho.desc) &&
        nf <= ho.cap) {
        // the extract already wrote them there (sgpu_set_host_output)
        ctx->timing[T_COPY_KEYS] = ctx->timing[T_COPY_DESC] = 0.f;
        return SGPU_OK;
    }
    // both copies, then one synchronisation; events split the time between them
    // (sgpu_last_timing slots 10, 11) when the context times its stages
    const bool tm = ctx->stage_timing;
    if (tm) HIPCHK(ctx, hipEventRecord(ctx->ev[T_COPY_KEYS], ctx->stream));
    if (keys)
        HIPCHK(ctx, hipMemcpyAsync(keys, pt.keys.as<float4>() + a, nf * sizeof(float4),
                                   hipMemcpyDeviceToHost, ctx->stream));
    if (tm) HIPCHK(ctx, hipEventRecord(ctx->ev[T_COPY_DESC], ctx->stream));
    if (descriptors)
        HIPCHK(ctx, hipMemcpyAsync(descriptors, pt.desc.as<float>() + a * 128,
                                   nf * 128 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (tm) HIPCHK(ctx, hipEventRecord(ctx->ev[T_N], ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->timing[T_COPY_KEYS] = ctx->timing[T_COPY_DESC] = 0.f;
    if (tm) {
        (void)hipEventElapsedTime(&ctx->timing[T_COPY_KEYS], ctx->ev[T_COPY_KEYS], ctx->ev[T_COPY_DESC]);
        (void)hipEventElapsedTime(&ctx->timing[T_COPY_DESC], ctx->ev[T_COPY_DESC], ctx->ev[T_N]);
    }
    return SGPU_OK;
}

int sgpu_device_features(sgpu_ctx* ctx, const float** keys, const float** descriptors,
                         const int64_t** image_offsets) {
    if (!ctx) return SGPU_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const float* k = nullptr;
    const float* dsc = nullptr;
    if (ctx->nparts == 1) {
        k = ctx->part[0].keys.as<float>();
        dsc = ctx->part[0].desc.as<float>();
    } else if (ctx->nparts > 1) {
        // one contiguous copy of the batch's features, gathered on first request
        const int64_t total = ctx->img_off.empty() ? 0 : ctx->img_off[ctx->batch];
        if (!ctx->gathered) {
            ALLOCCHK(ctx, ctx->all_keys.ensure((size_t)std::max<int64_t>(total, 1) * sizeof(float4)));
            if (ctx->opt.descriptors)
                ALLOCCHK(ctx, ctx->all_desc.ensure((size_t)std::max<int64_t>(total, 1) * 128 * sizeof(float)));
            for (int p = 0; p < ctx->nparts; p++) {
                const Part& pt = ctx->part[p];
                const int64_t base = ctx->img_off[pt.img0], nf = pt.img_off[pt.n];
                if (nf <= 0) continue;
                HIPCHK(ctx, hipMemcpyAsync(ctx->all_keys.as<float4>() + base, pt.keys.p,
                                           nf * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream));
                if (ctx->opt.descriptors)
                    HIPCHK(ctx, hipMemcpyAsync(ctx->all_desc.as<float>() + base * 128, pt.desc.p,
                                               nf * 128 * sizeof(float), hipMemcpyDeviceToDevice,
                                               ctx->stream));
            }
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            ctx->gathered = true;
        }
        k = ctx->all_keys.as<float>();
        dsc = ctx->all_desc.as<float>();
    }
    if (keys) *keys = k;
    if (descriptors) *descriptors = ctx->opt.descriptors ? dsc : nullptr;
    if (image_offsets) *image_offsets = ctx->img_off.data();
    return SGPU_OK;
}

void sgpu_quantize_descriptors(const float* d, size_t count, uint8_t* out) {
    for (size_t i = 0; i < count; ++i) out[i] = (uint8_t)(int)(512 * d[i] + 0.5);
}

int sgpu_quantize_descriptors_gpu(sgpu_ctx* ctx, const float* d, size_t ndesc, uint8_t* out,
                                  int flags) {
    if (!ctx) return SGPU_EINVAL;
    if (ndesc == 0) return SGPU_OK;
    if (!d || !out) return ctx->fail(SGPU_EINVAL, "bad quantize arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (flags & SGPU_INPUT_DEVICE) {
        HIPCHK(ctx, sgk::launch_quantize_desc(d, ndesc, out, nullptr, nullptr, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        return SGPU_OK;
    }
    ALLOCCHK(ctx, ctx->q_in.ensure(ndesc * 128 * sizeof(float)));
    ALLOCCHK(ctx, ctx->q_out.ensure(ndesc * 128));
    HIPCHK(ctx, hipMemcpyAsync(ctx->q_in.p, d, ndesc * 128 * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, sgk::launch_quantize_desc(ctx->q_in.as<float>(), ndesc, ctx->q_out.as<uint8_t>(),
                                          nullptr, nullptr, st));
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->q_out.p, ndesc * 128, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return SGPU_OK;
}

// The last extract's descriptors as u8 (and, for the matcher, s8 and row sums): one
// k_quantize_desc launch over the batch's float descriptors on first request, kept until the
// batch or the options change (f_ready).
}  // extern "C"
int sgh::feature_u8(sgpu_ctx* ctx) {
    if (ctx->batch <= 0 || ctx->img_off.empty())
        return ctx->fail(SGPU_EINVAL, "no extracted batch to quantise");
    if (!ctx->opt.descriptors) return ctx->fail(SGPU_EINVAL, "descriptors disabled (-sd)");
    if (ctx->f_ready) return SGPU_OK;
    const float* dsc = nullptr;
    const int rc = sgpu_device_features(ctx, nullptr, &dsc, nullptr);   // (gathers a multi-part batch)
    if (rc != SGPU_OK) return rc;
    const size_t total = (size_t)ctx->img_off[ctx->batch];
    ALLOCCHK(ctx, ctx->f_u8.ensure(std::max<size_t>(total, 1) * 128));
    ALLOCCHK(ctx, ctx->f_s8.ensure(std::max<size_t>(total, 1) * 128));
    ALLOCCHK(ctx, ctx->f_sums.ensure(std::max<size_t>(total, 1) * sizeof(int)));
    if (total > 0) {
        if (!dsc) return ctx->fail(SGPU_EINVAL, "the batch has no descriptors");
        HIPCHK(ctx, sgk::launch_quantize_desc(dsc, total, ctx->f_u8.as<uint8_t>(),
                                              ctx->f_s8.as<uint8_t>(), ctx->f_sums.as<int>(),
                                              ctx->stream));
    }
    ctx->f_ready = true;
    return SGPU_OK;
}
extern "C" {

int sgpu_feature_descriptors_u8(sgpu_ctx* ctx, const uint8_t** desc_u8) {
    if (!ctx || !desc_u8) return SGPU_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int rc = feature_u8(ctx);
    if (rc != SGPU_OK) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // readable from any stream of the caller
    *desc_u8 = ctx->f_u8.as<uint8_t>();
    return SGPU_OK;
}

int sgpu_copy_features_u8(sgpu_ctx* ctx, int image, uint8_t* desc) {
    if (!ctx) return SGPU_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int rc = feature_u8(ctx);
    if (rc != SGPU_OK) return rc;
    if (image < 0 || image >= ctx->batch) return ctx->fail(SGPU_EINVAL, "no such image");
    const int64_t a = ctx->img_off[image], nf = ctx->img_off[image + 1] - a;
    if (nf <= 0) return SGPU_OK;
    if (!desc) return ctx->fail(SGPU_EINVAL, "null output");
    HIPCHK(ctx, hipMemcpyAsync(desc, ctx->f_u8.as<uint8_t>() + a * 128, (size_t)nf * 128,
                               hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return SGPU_OK;
}

}  // extern "C"
