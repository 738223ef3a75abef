// sgpu_capi.cpp -- the C ABI (include/sgpu.h) over the gfx950 kernels: options, the context's
// life, timing and the debug hooks.  The subsystems' host code is in sgpu_extract.cpp,
// sgpu_match.cpp, sgpu_comm.cpp and sgpu_match_batch.cpp.
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sgpu_ctx.h"

using namespace sgh;

std::atomic<long long> sgh::g_allocs{0};   // (sgpu_ctx.h; sgpu_debug_alloc_count)

// A part's streams and events, created when the part is first used: the pyramid/detection
// stream gets the dispatch priority over the orientation/descriptor stream (of the previous
// part, when a batch runs in parts); octaves >= 1 of the pyramid run on a third stream.
int sgh::part_streams(Part& pt, int which) {
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    if ((which & PS_MAIN) && !pt.stream &&
        hipStreamCreateWithPriority(&pt.stream, hipStreamNonBlocking, prio_hi) != hipSuccess)
        return SGPU_ENODEV;
    if ((which & PS_LO) && !pt.stream_lo &&
        hipStreamCreateWithPriority(&pt.stream_lo, hipStreamNonBlocking, prio_lo) != hipSuccess)
        return SGPU_ENODEV;
    if ((which & PS_OCT) && !pt.stream_oct &&
        hipStreamCreateWithPriority(&pt.stream_oct, hipStreamNonBlocking, prio_hi) != hipSuccess)
        return SGPU_ENODEV;
    if (!pt.ev_ds) {
        // stage events.  Each record leaves the GPU idle ~4.5 us between the kernels around it
        // (C2 kernel trace; tests/microbench/event_gap.hip), whatever its flags: a device-scope
        // release or no timing at all measured the same
        for (hipEvent_t& e : pt.ev)
            if (hipEventCreate(&e) != hipSuccess) return SGPU_ENODEV;
        if (hipEventCreateWithFlags(&pt.ev_ds, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&pt.ev_oct, hipEventDisableTiming) != hipSuccess)
            return SGPU_ENODEV;
    }
    return SGPU_OK;
}

// The environment hooks read at creation: test modes and the A/B switches of bench / probe runs.
static void apply_env_hooks(sgpu_ctx* ctx) {
    // test mode for the C++ replicas, which only see SiftGPU.h: the bit-exact descriptor
    if (const char* ev = getenv("SGPU_EXACT_DESCRIPTOR"))
        if (ev[0] == '1') ctx->debug_flags |= SGPU_DEBUG_EXACT_DESCRIPTOR;
    // A/B hook for the Gaussian kernels (bench / probe runs in one process tree)
    if (const char* ev = getenv("SGPU_GAUSS")) {
        if (!strcmp(ev, "block")) ctx->debug_flags |= SGPU_DEBUG_GAUSS_BLOCK;
    }
    if (const char* ev = getenv("SGPU_DUO")) {   // A/B hook of the paired-level kernel
        if (!strcmp(ev, "off")) ctx->debug_flags |= SGPU_DEBUG_DUO_OFF;
        if (!strcmp(ev, "always")) ctx->debug_flags |= SGPU_DEBUG_DUO_ALWAYS;
        if (!strcmp(ev, "on")) ctx->duo_on = true;
    }
    if (const char* ev = getenv("SGPU_DUO_WIDE")) {
        if (ev[0] == '1') ctx->duo_wide = true;
    }
    if (const char* ev = getenv("SGPU_DUO_U8")) {
        if (ev[0] == '1') ctx->duo_u8 = true;
    }
    if (const char* ev = getenv("SGPU_DUO_PLAN")) {   // A/B hook of the octave pairing
        if (!strcmp(ev, "end")) ctx->duo_plan = SGPU_PAIRS_END;
        if (!strcmp(ev, "front")) ctx->duo_plan = SGPU_PAIRS_FRONT;
    }
    if (const char* ev = getenv("SGPU_TOP_LEVEL")) {   // A/B hook of the lazy top level
        if (!strcmp(ev, "dense")) ctx->top_level = SGPU_TOP_LEVEL_DENSE;
        if (!strcmp(ev, "lazy")) ctx->top_level = SGPU_TOP_LEVEL_LAZY;
    }
    if (const char* ev = getenv("SGPU_TRIO")) {   // A/B hook of the three-level kernel
        if (!strcmp(ev, "off")) ctx->trio_mode = SGPU_TRIO_OFF;
        if (!strcmp(ev, "always")) ctx->trio_mode = SGPU_TRIO_ALWAYS;
        if (!strcmp(ev, "on")) ctx->trio_mode = SGPU_TRIO_ON;
    }
    if (const char* ev = getenv("SGPU_GAUSS_BANDS"))
        if (!strcmp(ev, "long")) ctx->debug_flags |= SGPU_DEBUG_GAUSS_LONG_BANDS;
    if (const char* ev = getenv("SGPU_PYR")) {
        if (!strcmp(ev, "serial")) ctx->debug_flags |= SGPU_DEBUG_PYR_SERIAL;
    }
    if (const char* ev = getenv("SGPU_STREAMS")) ctx->multi_stream = !strcmp(ev, "multi");
    if (const char* ev = getenv("SGPU_MATCH"))
        if (!strcmp(ev, "reg")) ctx->debug_flags |= SGPU_DEBUG_MATCH_REGSTAGE;
    if (const char* ev = getenv("SGPU_DESC")) {
        if (!strcmp(ev, "dual")) ctx->debug_flags |= SGPU_DEBUG_DESC_DUAL;
        if (!strcmp(ev, "narrow")) ctx->debug_flags |= SGPU_DEBUG_DESC_WIDE_OFF;
        if (!strcmp(ev, "wide")) ctx->debug_flags |= SGPU_DEBUG_DESC_WIDE_ALWAYS;
    }
    if (const char* ev = getenv("SGPU_GAUSS_TILE")) {   // A/B hook of the tile kernel
        if (!strcmp(ev, "off")) ctx->debug_flags |= SGPU_DEBUG_GAUSS_TILE_OFF;
        if (!strcmp(ev, "always")) ctx->debug_flags |= SGPU_DEBUG_GAUSS_TILE_ALWAYS;
    }
    if (const char* ev = getenv("SGPU_WIDE_DESC_MAX"))
        if (atoll(ev) >= 0) ctx->wide_desc_max = (size_t)atoll(ev);
    if (const char* ev = getenv("SGPU_WAVE_ORIENT_MAX"))
        if (atoll(ev) >= 0) ctx->wave_orient_max = (size_t)atoll(ev);
    if (const char* ev = getenv("SGPU_EXTREMA")) {   // A/B hook of the tile extremum kernel
        if (!strcmp(ev, "wave")) ctx->debug_flags |= SGPU_DEBUG_EXTREMA_TILE_OFF;
    }
    if (const char* ev = getenv("SGPU_FEATURE_QUEUE")) {   // A/B hook of the persistent feature kernels
        // (any other value leaves the shipped forms)
        if (!strcmp(ev, "on") || !strcmp(ev, "ori") || !strcmp(ev, "desc") || !strcmp(ev, "off")) {
            ctx->queue_ori = !strcmp(ev, "on") || !strcmp(ev, "ori");
            ctx->queue_desc = !strcmp(ev, "on") || !strcmp(ev, "desc");
        }
    }
    // test hook: at most this many resident workgroups per feature kernel, so that small batches
    // take most of their units from the work counters (the launchers keep one wave per counter)
    if (const char* ev = getenv("SGPU_FEATURE_QUEUE_GRID"))
        if (atoi(ev) >= 1) {
            ctx->fq.ori_grid = std::min(ctx->fq.ori_grid, atoi(ev));
            ctx->fq.desc_grid = std::min(ctx->fq.desc_grid, atoi(ev));
        }
    if (const char* ev = getenv("SGPU_TILE_DUO"))
        ctx->tile_duo = !strcmp(ev, "on");
    if (const char* ev = getenv("SGPU_MATCH_PRUNE"))   // A/B hook of the pruned column side
        ctx->match_prune = strcmp(ev, "off") != 0;
    if (const char* ev = getenv("SGPU_GAUSS_TILE_MB"))
        if (atoi(ev) >= 0) ctx->tile_mb = atoi(ev);
}

extern "C" {

void sgpu_default_options(sgpu_options* o) {
    o->filter_width_factor = 4.0f;
    o->descriptor_window_factor = 3.0f;
    o->orientation_window_factor = 2.0f;
    o->orientation_gaussian_factor = 1.5f;
    o->dog_threshold = 0.0f;
    o->edge_threshold = 0.0f;
    o->subpixel = 1;
    o->max_orientation = 2;
    o->fixed_orientation = 0;
    o->octave_min = 0;
    o->octave_num = -1;
    o->dog_level_num = 3;
    o->lowe_origin = 0;
    o->normalized = 1;
    o->descriptors = 1;
    o->keep_extremum_sign = 0;
    o->circular_window = 0;
    o->verbose = 0;
    o->max_dimension = 13200;
    o->preprocess_on_cpu = 1;
    o->feature_count_threshold = -1;
    o->truncate_method = 0;
}

// SiftGPU::ParseParam (SiftGPU.cpp:801-1246): options are matched on their first four
// characters, case-insensitively; numeric arguments are consumed only when they parse and
// pass the same range checks as the reference.
int sgpu_parse_args(sgpu_options* o, int argc, const char* const* argv, int* device) {
    if (!o) return SGPU_EINVAL;
    auto key = [](const char* s) {
        std::string k;
        for (int i = 0; i < 4 && s[i]; i++) k += (char)((s[i] >= 'A' && s[i] <= 'Z') ? s[i] + 32 : s[i]);
        return k;
    };
    for (int i = 0; i < argc; i++) {
        const char* arg = argv[i];
        if (!arg || arg[0] != '-' || !arg[1]) continue;
        const std::string k = key(arg + 1);
        const char* param = (i + 1 < argc) ? argv[i + 1] : nullptr;
        float fv = 0.f;
        int iv = 0;
        if (k == "cuda") {
            int dev = -1;
            if (param && sscanf(param, "%d", &dev) == 1 && dev >= 0) {
                if (device) *device = dev;
                i++;
            }
        } else if (k == "sd") o->descriptors = 0;
        else if (k == "unn") o->normalized = 0;
        else if (k == "ndes") o->normalized = 1;
        else if (k == "m" || k == "mo") {
            int mo = 2;
            if (param) sscanf(param, "%d", &mo);
            o->max_orientation = std::min(std::max(1, mo), 4);
        } else if (k == "m2p") o->max_orientation = 2;
        else if (k == "s") {
            int sp = 1;
            if (param) sscanf(param, "%d", &sp);
            o->subpixel = std::min(std::max(0, sp), 5);
        } else if (k == "ofix") o->fixed_orientation = (strcmp(arg + 1, "ofix") == 0);
        else if (k == "lowe") o->lowe_origin = 1;
        else if (k == "sign") o->keep_extremum_sign = 1;
        else if (k == "prep") o->preprocess_on_cpu = 1;
        else if (k == "nopr") o->preprocess_on_cpu = 0;
        else if (!param) continue;
        else if (k == "tc" || k == "tc1" || k == "tc2" || k == "tc3") {
            // SiftGPU.cpp:1185-1203: the method is set even when no count follows
            o->truncate_method = k == "tc2" ? 1 : k == "tc3" ? 2 : 0;
            if (sscanf(param, "%d", &iv) == 1 && iv > 0) { o->feature_count_threshold = iv; i++; }
        } else if (k == "maxd") {   // SiftGPU.cpp:1213-1222
            if (sscanf(param, "%d", &iv) == 1 && iv > 0) { o->max_dimension = iv; i++; }
        }
        else if (k == "f") { if (sscanf(param, "%f", &fv) == 1 && fv > 0) { o->filter_width_factor = fv; i++; } }
        else if (k == "w") { if (sscanf(param, "%f", &fv) == 1 && fv > 0) { o->orientation_window_factor = fv; i++; } }
        else if (k == "dw") { if (sscanf(param, "%f", &fv) == 1 && fv > 0) { o->descriptor_window_factor = fv; i++; } }
        else if (k == "fo") { iv = -3; if (sscanf(param, "%d", &iv) == 1 && iv >= -2) { o->octave_min = iv; i++; } }
        else if (k == "no") {
            iv = -1;
            if (sscanf(param, "%d", &iv) == 1) {
                iv = std::max(-1, iv);
                if (iv == -1 || iv >= 1) { o->octave_num = iv; i++; }
            }
        } else if (k == "t") { if (sscanf(param, "%f", &fv) == 1 && fv > 0 && fv < 0.5f) { o->dog_threshold = fv; i++; } }
        else if (k == "e") { if (sscanf(param, "%f", &fv) == 1 && fv > 0) { o->edge_threshold = fv; i++; } }
        else if (k == "d") { if (sscanf(param, "%d", &iv) == 1 && iv >= 1 && iv <= 6) { o->dog_level_num = iv; i++; } }
        else if (k == "v") { if (sscanf(param, "%d", &iv) == 1 && iv >= 0 && iv <= 4) o->verbose = iv; }
    }
    return SGPU_OK;
}

int sgpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int sgpu_ctx_set_options(sgpu_ctx* ctx, const sgpu_options* opt) {
    if (!ctx) return SGPU_EINVAL;
    sgpu_options o;
    if (opt) o = *opt; else sgpu_default_options(&o);
    // -fo -2 runs as in the reference: its initial smoothing sigma is 0 (sqrt only when
    // 1.6 > 0.5 * 4 + 0.001, SiftGPU.cpp:446-452), CreateFilterKernel(0) yields NaN taps
    // (ProgramCU.cu:391-398) and the NaN pyramid has no keypoint with an orientation: the call
    // succeeds with 0 features.  -fo below -3 is clamped to -3
    // (PyramidCU.cpp:106-107).
    if (o.octave_min < -3) o.octave_min = -3;
    if (o.dog_level_num < 1 || o.dog_level_num > 6) return ctx->fail(SGPU_EINVAL, "dog_level_num must be 1..6");
    if (o.max_dimension < 8) return ctx->fail(SGPU_EINVAL, "max_dimension must be >= 8");
    ctx->opt = o;
    ctx->f_ready = false;   // the cached u8 descriptors belong to the previous options
    sgp::Options po;
    po.filter_width_factor = o.filter_width_factor;
    po.dog_level_num = o.dog_level_num;
    po.dog_threshold = o.dog_threshold;
    po.edge_threshold = o.edge_threshold;
    po.octave_min = o.octave_min;
    ctx->sched = sgp::make_schedule(po);
    return SGPU_OK;
}

int sgpu_ctx_create(int device, const sgpu_options* opt, sgpu_ctx** out) {
    if (!out) return SGPU_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return SGPU_ENODEV;
    if (device < 0 || device >= n) return SGPU_EINVAL;
    sgpu_ctx* ctx = new sgpu_ctx();
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return SGPU_ENODEV;
    }
    for (int i = 0; i <= T_N; i++) (void)hipEventCreate(&ctx->ev[i]);
    // Streams in an order that puts the concurrently busy ones on distinct hardware queues: the
    // runtime hands a process's streams the hardware queues in turn (4 on the GPU box), so the
    // i-th stream created here shares a queue with the (i+4)-th.  Busy together: a part's
    // pyramid stream and its octave stream (extract), and in sgpu_extract_stream also the copy
    // streams h2d / d2h (a batch's orientation / descriptor stream runs beside the copies
    // only).  Order (queue = index mod 4): 0 context stream, 1 part 0 main, 2 part 0 octaves,
    // 3 h2d, 4 d2h, 5 part 0 low, 6 part 1 octaves, 7-8 part 2 main / low (idle unless
    // SGPU_DEBUG_PARTS4), 9 part 1 main, 10 part 1 low: the main and octave streams on queues
    // 1 and 2, the copies on 3 and 0.  Measured: the same streams created part by part put a
    // copy stream beside a pyramid stream and cost the host-in / host-out stream 13 % (DESIGN.md
    // 4.3).  The rest are created when first used (part_streams).
    {
        Part* p = ctx->part;
        bool ok = part_streams(p[0], PS_MAIN) == SGPU_OK && part_streams(p[0], PS_OCT) == SGPU_OK &&
                  hipStreamCreateWithFlags(&ctx->h2d, hipStreamNonBlocking) == hipSuccess &&
                  hipStreamCreateWithFlags(&ctx->d2h, hipStreamNonBlocking) == hipSuccess &&
                  part_streams(p[0], PS_LO) == SGPU_OK && part_streams(p[1], PS_OCT) == SGPU_OK &&
                  part_streams(p[2], PS_MAIN) == SGPU_OK && part_streams(p[2], PS_LO) == SGPU_OK &&
                  part_streams(p[1], PS_MAIN) == SGPU_OK && part_streams(p[1], PS_LO) == SGPU_OK;
        ok = ok && sgk::feature_queue_grids(&ctx->fq) == hipSuccess;
        for (int i = 0; ok && i < 2; i++)
            ok = hipEventCreateWithFlags(&ctx->up_ev[i], hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&ctx->down_ev[i], hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            sgpu_ctx_destroy(ctx);
            return SGPU_ENODEV;
        }
    }
    apply_env_hooks(ctx);
    ctx->env_flags = ctx->debug_flags;   // kept by sgpu_debug_set_flags (A/B runs of the probes)
    int rc = sgpu_ctx_set_options(ctx, opt);
    if (rc != SGPU_OK) {
        sgpu_ctx_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return SGPU_OK;
}

int sgpu_ctx_destroy(sgpu_ctx* ctx) {
    if (!ctx) return SGPU_EINVAL;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (Part& pt : ctx->part) {
        if (pt.stream) (void)hipStreamSynchronize(pt.stream);
        if (pt.stream_lo) (void)hipStreamSynchronize(pt.stream_lo);
        if (pt.stream_oct) (void)hipStreamSynchronize(pt.stream_oct);
        pt.release();
    }
    comm_release(ctx);
    for (hipStream_t st : {ctx->h2d, ctx->d2h})
        if (st) (void)hipStreamSynchronize(st);
    for (int i = 0; i < 2; i++) {
        if (ctx->up_ev[i]) (void)hipEventDestroy(ctx->up_ev[i]);
        if (ctx->down_ev[i]) (void)hipEventDestroy(ctx->down_ev[i]);
    }
    if (ctx->h2d) (void)hipStreamDestroy(ctx->h2d);
    if (ctx->d2h) (void)hipStreamDestroy(ctx->d2h);
    DevBuf* bufs[] = {&ctx->input, &ctx->input2, &ctx->duo_trash, &ctx->all_keys, &ctx->all_desc, &ctx->gray, &ctx->pre, &ctx->m_d1, &ctx->m_d2, &ctx->m_s1, &ctx->m_s2,
                      &ctx->m_part, &ctx->m_terms, &ctx->m_match, &ctx->m_dist, &ctx->m_mask, &ctx->m_loc,
                      &ctx->m_colpart, &ctx->m_cols, &ctx->m_prune, &ctx->m_s1c,
                      &ctx->b_desc, &ctx->b_s8, &ctx->b_sums, &ctx->b_plan, &ctx->b_part, &ctx->b_dec,
                      &ctx->b_cnt, &ctx->b_out, &ctx->b_loc, &ctx->q_in, &ctx->q_out, &ctx->f_u8, &ctx->f_s8,
                      &ctx->f_sums, &ctx->c_buf, &ctx->e_loc, &ctx->e_plan, &ctx->e_pts, &ctx->e_slots,
                      &ctx->e_out, &ctx->e_mask, &ctx->v_buf, &ctx->p_scale, &ctx->p_index, &ctx->p_u8,
                      &ctx->t_tab, &ctx->t_work, &ctx->t_out, &ctx->o_tab, &ctx->o_out};
    for (DevBuf* b : bufs) b->release();
    for (int i = 0; i <= T_N; i++)
        if (ctx->ev[i]) (void)hipEventDestroy(ctx->ev[i]);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return SGPU_OK;
}

const char* sgpu_last_error(const sgpu_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

long long sgpu_debug_alloc_count(void) { return g_allocs.load(); }

int sgpu_set_stage_timing(sgpu_ctx* ctx, int on) {
    if (!ctx) return SGPU_EINVAL;
    ctx->stage_timing = on != 0;
    return SGPU_OK;
}

int sgpu_last_pyramid_launches(const sgpu_ctx* ctx, int* filters) {
    if (!ctx || ctx->batch <= 0) return SGPU_EINVAL;
    if (filters) *filters = ctx->part[0].gauss_filters;
    return ctx->part[0].gauss_launches;
}

int sgpu_last_timing(const sgpu_ctx* ctx, float* times, int n) {
    if (!ctx || !times) return SGPU_EINVAL;
    for (int i = 0; i < n && i < T_N; i++) times[i] = ctx->timing[i];
    return SGPU_OK;
}

int sgpu_debug_set_flags(sgpu_ctx* ctx, int flags) {
    if (!ctx) return SGPU_EINVAL;
    ctx->debug_flags = flags | ctx->env_flags;
    return SGPU_OK;
}

int sgpu_debug_set_match_prune(sgpu_ctx* ctx, int on) {
    if (!ctx) return SGPU_EINVAL;
    ctx->match_prune = on != 0;
    return SGPU_OK;
}

int sgpu_debug_match_plan_stats(const sgpu_ctx* ctx, long long out[4]) {
    if (!ctx || !out || !ctx->b_planned) return SGPU_EINVAL;
    const sgplan::Plan& plan = ctx->b_hplan;
    long long tiles = 0, chunks = 0;
    for (const sgplan::Item& it : plan.items)
        tiles = std::max<long long>(tiles, (it.c_end - it.c_begin + sgplan::kTileCols - 1) / sgplan::kTileCols);
    for (const sgplan::Side& sd : plan.sides) chunks = std::max<long long>(chunks, sd.chunks);
    out[0] = (long long)plan.items.size();
    out[1] = (long long)plan.sides.size();
    out[2] = tiles;
    out[3] = chunks;
    return SGPU_OK;
}

static_assert(SGPU_PLAN_KINDS == sgpyr::kKinds && SGPU_PLAN_TRIO == sgpyr::kTrio &&
              SGPU_PLAN_TILE_DUO_ONE == sgpyr::kTileDuoOne, "sgpu.h and sift_pyramid_plan.h agree");
int sgpu_debug_pyramid_plan(const sgpu_ctx* ctx, int* out, int cap) {
    if (!ctx || ctx->batch <= 0 || cap < 0 || (cap > 0 && !out)) return SGPU_EINVAL;
    const Part& pt = ctx->part[0];
    const int n = (int)pt.plan.launches.size();
    for (int e = 0; e < n && (e + 1) * SGPU_PLAN_ENTRY_INTS <= cap; e++) {
        const sgpyr::Launch& l = pt.plan.launches[e];
        int* p = out + e * SGPU_PLAN_ENTRY_INTS;
        p[0] = l.kind;
        for (int j = 0; j < 3; j++) {
            p[1 + 2 * j] = l.op[j] < 0 ? -1 : pt.levels[l.op[j]].o;
            p[2 + 2 * j] = l.op[j] < 0 ? -1 : pt.levels[l.op[j]].k;
        }
    }
    return n;
}

static_assert(SGPU_DUO_STRIPS_RULE == sgk::kDuoStripsRule && SGPU_DUO_STRIPS_WAVE == sgk::kDuoStripsWave &&
              SGPU_DUO_STRIPS_COOP == sgk::kDuoStripsCoop, "sgpu.h and sift_kernels.h agree");
int sgpu_debug_set_duo_strips(sgpu_ctx* ctx, int mode) {
    if (!ctx || mode < SGPU_DUO_STRIPS_RULE || mode > SGPU_DUO_STRIPS_COOP) return SGPU_EINVAL;
    ctx->duo_strips = mode;
    return SGPU_OK;
}

int sgpu_debug_set_feature_queue(sgpu_ctx* ctx, int mode) {
    if (!ctx || mode < SGPU_FEATURES_QUEUE || mode > SGPU_FEATURES_STATIC) return SGPU_EINVAL;
    ctx->queue_ori = !(mode & SGPU_FEATURES_STATIC_ORIENTATION);
    ctx->queue_desc = !(mode & SGPU_FEATURES_STATIC_DESCRIPTOR);
    return SGPU_OK;
}

int sgpu_debug_set_schedule(sgpu_ctx* ctx, int trio, int pairs) {
    if (!ctx || trio < SGPU_TRIO_OFF || trio > SGPU_TRIO_ALWAYS || pairs < SGPU_PAIRS_FRONT ||
        pairs > SGPU_PAIRS_END)
        return SGPU_EINVAL;
    ctx->trio_mode = trio;
    ctx->duo_plan = pairs;
    return SGPU_OK;
}

int sgpu_debug_set_top_level(sgpu_ctx* ctx, int mode) {
    if (!ctx || mode < SGPU_TOP_LEVEL_RULE || mode > SGPU_TOP_LEVEL_LAZY) return SGPU_EINVAL;
    ctx->top_level = mode;
    return SGPU_OK;
}

int sgpu_debug_geometry(const sgpu_ctx* ctx, int* n_octaves, int* dims, int max) {
    if (!ctx || !n_octaves) return SGPU_EINVAL;
    *n_octaves = (int)ctx->oct.size();
    for (int o = 0; o < (int)ctx->oct.size() && o < max; o++) {
        dims[3 * o] = ctx->oct[o].w;
        dims[3 * o + 1] = ctx->oct[o].h;
        dims[3 * o + 2] = ctx->oct[o].wa;
    }
    return SGPU_OK;
}

int sgpu_debug_gaussian(sgpu_ctx* ctx, int image, int octave, int level, float* out) {
    if (!ctx || image < 0 || image >= ctx->batch || octave < 0 ||
        octave >= (int)ctx->oct.size() || level < 0 || level >= ctx->sched.level_num)
        return SGPU_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Part& pt = ctx->part[ctx->part_of(image)];
    const sgk::OctaveDesc& od = pt.fp.oct[octave];
    const long long npx = (long long)od.wa * od.h;
    if (level == ctx->sched.level_num - 1 && (size_t)octave < pt.top_dense.size() &&
        !pt.top_dense[octave]) {
        // a lazy pyramid holds this level only around its DoG candidates: filter it now (the
        // sparse values are the same bits), dense until the next extract
        HIPCHK(ctx, sgk::launch_gauss_op(pt.top_ops[octave], ctx->stream, 0));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        pt.top_dense[octave] = 1;
    }
    const float* src = pt.pyr.as<float>() + od.gauss_off + level * od.level_stride +
                       (image - pt.img0) * npx;
    HIPCHK(ctx, hipMemcpy(out, src, npx * sizeof(float), hipMemcpyDeviceToHost));
    return SGPU_OK;
}

// The test-hook library beside this one (lib/libsiftgpu_debug.so, csrc/sgpu_debug.hip), loaded on
// first use: the candidate dump's kernel is not part of the product library.
static void* debug_library() {
    static void* lib = []() -> void* {
        Dl_info info{};
        if (!dladdr(reinterpret_cast<void*>(&sgpu_debug_candidates), &info) || !info.dli_fname)
            return nullptr;
        std::string path(info.dli_fname);
        const size_t slash = path.rfind('/');
        path = (slash == std::string::npos ? std::string(".") : path.substr(0, slash)) +
               "/libsiftgpu_debug.so";
        return dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    }();
    return lib;
}
static void* debug_symbol(const char* name) {
    void* h = debug_library();
    return h ? dlsym(h, name) : nullptr;
}
static sgk::DebugCandidatesFn debug_candidates_hook() {
    static sgk::DebugCandidatesFn fn =
        reinterpret_cast<sgk::DebugCandidatesFn>(debug_symbol("sgpu_testhook_candidates"));
    return fn;
}

int sgpu_debug_top_level_at(sgpu_ctx* ctx, int image, int octave, int x, int y, float out[9]) {
    if (!ctx || !out || image < 0 || image >= ctx->batch || ctx->img_off.empty() || octave < 0 ||
        octave >= (int)ctx->oct.size())
        return SGPU_EINVAL;
    const Part& pt = ctx->part[ctx->part_of(image)];
    const sgk::OctaveDesc& od = pt.fp.oct[octave];
    if (x < 1 || x > od.wa - 2 || y < 1 || y > od.h - 2 || (size_t)octave >= pt.top_ops.size())
        return ctx->fail(SGPU_EINVAL, "point outside the octave's interior");
    const sgk::DebugTopLevelFn hook = reinterpret_cast<sgk::DebugTopLevelFn>(debug_symbol("sgpu_testhook_top_level"));
    if (!hook) return ctx->fail(SGPU_EINVAL, "test-hook library lib/libsiftgpu_debug.so not found");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf d;
    ALLOCCHK(ctx, d.ensure(9 * sizeof(float)));
    sgk::TopLevelFilter tf;
    tf.fw = pt.top_ops[octave].fw;
    tf.taps = pt.top_ops[octave].taps;
    hipError_t e = hook(pt.pyr.as<float>(), &pt.fp, &tf, image - pt.img0, octave, x, y,
                        d.as<float>(), ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(out, d.p, 9 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    d.release();
    HIPCHK(ctx, e);
    return SGPU_OK;
}

int sgpu_debug_candidates(sgpu_ctx* ctx, int* ints, float* floats, int cap, int* n) {
    if (!ctx || !n) return SGPU_EINVAL;
    uint32_t total = 0;
    for (int p = 0; p < ctx->nparts; p++) total += ctx->part[p].n_cand;
    *n = (int)total;
    if (!ints || !floats || cap < (int)total) return total ? SGPU_ERANGE : SGPU_OK;
    if (total == 0) return SGPU_OK;
    const sgk::DebugCandidatesFn hook = debug_candidates_hook();
    if (!hook) return ctx->fail(SGPU_EINVAL, "test-hook library lib/libsiftgpu_debug.so not found");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf a, b;
    ALLOCCHK(ctx, a.ensure(total * sizeof(int4)));
    ALLOCCHK(ctx, b.ensure(total * sizeof(float4)));
    uint32_t at = 0;
    for (int p = 0; p < ctx->nparts; p++) {
        const Part& pt = ctx->part[p];
        if (!pt.n_cand) continue;
        HIPCHK(ctx, hook(pt.pyr.as<float>(), pt.mask.as<uint32_t>(), pt.row_base.as<uint32_t>(),
                         pt.total_rows, pt.row_base.as<uint32_t>() + pt.total_rows,
                         (int)pt.n_cand, &pt.fp, a.as<int4>() + at, b.as<float4>() + at,
                         ctx->stream));
        at += pt.n_cand;
    }
    HIPCHK(ctx, hipMemcpyAsync(ints, a.p, total * sizeof(int4), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(floats, b.p, total * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // the kernel reports part-local image indices
    at = 0;
    for (int p = 0; p < ctx->nparts; p++) {
        const Part& pt = ctx->part[p];
        for (uint32_t i = 0; i < pt.n_cand; i++) ints[4 * (at + i) + 3] += pt.img0;
        at += pt.n_cand;
    }
    a.release();
    b.release();
    return SGPU_OK;
}

}  // extern "C"
