// sgpu_ctx.h -- what the C ABI's host files share (internal: not installed, not under include/):
// the context behind include/sgpu.h's opaque sgpu_ctx, its buffers and batch parts, the error
// macros, and the few helpers that cross files.  File map: DESIGN.md 4.15.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sgpu.h"
#include "sift_geom.h"
#include "sift_kernels.h"
#include "sift_match_plan.h"
#include "sift_params.h"
#include "sift_pyramid_plan.h"
#include "sift_select.h"

// RCCL's communicator handle as rccl.h declares it (sgpu_comm.cpp alone includes rccl.h)
typedef struct ncclComm* ncclComm_t;

// The types live in a named namespace: sgpu_ctx has members of them and is one type across the
// translation units only if they have external linkage.
namespace sgh {

// feature counts (of the previous call) up to which each descriptor gets a workgroup of 4 waves
// (k_descriptor_wide): ~1,500 features of one 1080p image are ~1.5 waves per SIMD under one wave
// each
#ifndef SGK_WIDE_DESC_MAX
#define SGK_WIDE_DESC_MAX 8192
#endif

// device and pinned-host allocations made by the library (sgpu_debug_alloc_count): a test hook
// for sgpu_reserve, whose point is that the extract after it allocates nothing
extern std::atomic<long long> g_allocs;   // one object, defined in sgpu_capi.cpp

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t n) {
        if (n <= bytes) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        n = std::max<size_t>(n, 256);
        g_allocs++;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// stage timings (sgpu_last_timing): T_DETECT spans the extremum kernel and the row scan (the
// reference's "Detection" and "Feature List" stages, SiftPyramid.cpp:107,123); T_LIST is the
// row-scan part of it
enum { T_UPLOAD, T_PYRAMID, T_DETECT, T_ORIENT, T_EXPAND, T_DESC, T_DOWNLOAD, T_TOTAL, T_MATCH,
       T_LIST, T_COPY_KEYS, T_COPY_DESC, T_ESTIMATE, T_VERIFY, T_PREMATCH, T_TRACKS, T_POSE,
       T_N };

// One part of a batch: consecutive images [img0, img0 + n) with their own stream and buffers.
struct Part {
    hipStream_t stream = nullptr;      // high priority: pyramid + detection
    hipStream_t stream_lo = nullptr;   // low priority: orientation, descriptors, readback
    // a small batch (one image through SiftGPU::RunSIFT) runs every stage on `stream`: the
    // cross-stream event waits cost more than the overlap gains there (extract_body)
    bool one_stream = false;
    hipStream_t stream_oct = nullptr;  // high priority: pyramid octaves >= 1 (enqueue_part)
    hipEvent_t ev_ds = nullptr;        // octave 0's decimating level done
    hipEvent_t ev_oct = nullptr;       // octaves >= 1 done
    size_t cand_hint = 0, feat_hint = 0;   // counts of the previous call (launch-grid sizing)
    int gauss_launches = 0, gauss_filters = 0;   // the last pyramid: launches, level filters
    // the last pyramid's level filters (build_level_ops), what the planner reads of them, and its
    // launch list (sift_pyramid_plan.h; sgpu_debug_pyramid_plan); kept across calls for their storage
    std::vector<sgk::LevelOp> ops;
    std::vector<sgpyr::LevelDesc> levels;
    sgpyr::Plan plan;
    // the octaves' last level: its filter per octave, kept beside the list; lazy =
    // the last pyramid left it out (the extremum pass evaluated it at the pending pixels only);
    // top_dense[o] = octave o's plane holds the whole level (always unless lazy; in a lazy part
    // once sgpu_debug_gaussian has filled it in)
    std::vector<sgk::LevelOp> top_ops;
    std::vector<char> top_dense;
    bool lazy = false;
    bool events = true;                    // the last enqueue recorded its stage events
    bool copied_out = false;               // the last enqueue copied its results to host_out
    hipEvent_t ev[10] = {};  // start, pyramid, detect, orientation, expand, descriptor, end,
                             // extrema done (before the row scan), (spare), (spare)
    int img0 = 0, n = 0;
    sgk::FeatureParams fp{};
    int total_rows = 0;
    long long mask_words = 0;
    size_t cand_cap = 0;     // candidate capacity of cand/info/ocount (features: 2x)
    uint32_t n_cand = 0;
    std::vector<int64_t> img_off;          // local per-image offsets [n + 1]
    int64_t* h_read = nullptr;             // pinned readback: [0] = n_cand, [1..n+1] = offsets
    size_t h_read_n = 0;
    DevBuf pyr, mask, row_count, row_base, scan_tmp, cand, info, ocount, eoff, feat, feat_info,
        keys, desc, img_off_dev;
    float timing[T_N] = {};

    void release() {
        DevBuf* bufs[] = {&pyr, &mask, &row_count, &row_base, &scan_tmp, &cand, &info, &ocount,
                          &eoff, &feat, &feat_info, &keys, &desc, &img_off_dev};
        for (DevBuf* b : bufs) b->release();
        if (h_read) (void)hipHostFree(h_read);
        h_read = nullptr;
        for (hipEvent_t& e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
        if (stream_lo) (void)hipStreamDestroy(stream_lo);
        if (ev_ds) (void)hipEventDestroy(ev_ds);
        if (ev_oct) (void)hipEventDestroy(ev_oct);
        ev_ds = ev_oct = nullptr;
        if (stream_oct) (void)hipStreamDestroy(stream_oct);
        stream = stream_lo = stream_oct = nullptr;
    }
};

constexpr int kMaxParts = 4;
// candidate counts (of the previous call) up to which orientation runs one wave per candidate
#ifndef SGPU_WAVE_ORIENT_MAX
#define SGPU_WAVE_ORIENT_MAX 16384
#endif
constexpr size_t kWaveOrientationMax = SGPU_WAVE_ORIENT_MAX;

}  // namespace sgh

struct sgpu_ctx {
    int device = 0;
    hipStream_t stream = nullptr;   // matcher, uploads, gathers
    sgpu_options opt{};
    sgp::Schedule sched{};
    sgp::InputPlan plan{};                 // first octave of the last extract (plan_input)
    int debug_flags = 0;                   // SGPU_DEBUG_* test hooks
    bool multi_stream = false;             // SGPU_STREAMS=multi: octave and feature streams
    bool duo_on = false;                   // SGPU_DUO=on: paired-level launches (size rule)
    bool duo_wide = false;                 // SGPU_DUO_WIDE=1: also the (21, 25) pairs
    bool duo_u8 = false;                   // SGPU_DUO_U8=1: the u8 ingest pair (13, 11)
    int trio_mode = SGPU_TRIO_OFF;         // three-level launches: SGPU_TRIO_* (SGPU_TRIO=off / on /
                                           // always; sgpu_debug_set_schedule)
    int duo_plan = SGK_DUO_PLAN;           // SGPU_PAIRS_END: pairs from the octave's end
                                           // (SGPU_DUO_PLAN=end), SGPU_PAIRS_FRONT: from its front
    int top_level = SGPU_TOP_LEVEL_RULE;   // the octaves' last Gaussian level: dense, or only around
                                           // its DoG candidates (SGPU_TOP_LEVEL=dense|lazy;
                                           // sgpu_debug_set_top_level)
    int duo_strips = SGPU_DUO_STRIPS_RULE; // strip geometry of the paired-level launches
                                           // (sgpu_debug_set_duo_strips)
    size_t wide_desc_max = SGK_WIDE_DESC_MAX;   // feature counts (of the previous call) up to which
                                           // descriptors run a workgroup per feature
                                           // (SGPU_WIDE_DESC_MAX)
    size_t wave_orient_max = sgh::kWaveOrientationMax;   // candidate counts (of the previous call) up to
                                           // which orientation runs a wave per candidate
                                           // (SGPU_WAVE_ORIENT_MAX; a test hook: 0 keeps the quad
                                           // forms for small batches)
    bool unit_input = true;                // the last extract's input lies in [0, 1] (not a caller's f32)
    bool tile_duo = false;                 // tile duos when every level is tiled (SGPU_TILE_DUO=on;
                                           // measured slower)
    int tile_mb = SGK_TILE_MB;             // levels of at most this many MB: 2-D tile launches
                                           // (SGPU_GAUSS_TILE_MB; k_gauss_tile)
    int env_flags = 0;                     // debug flags set from the environment at creation
    // the feature stages' persistent form: the resident grids of this device,
    // and which of the two kernels take it (sgpu_debug_set_feature_queue; SGPU_FEATURE_QUEUE=off
    // / ori / desc / on at creation, an A/B hook)
    sgk::FeatureQueue fq{};
    bool queue_ori = true, queue_desc = true;
    // sgpu_set_host_output: page-locked host buffers the next one-image extract fills in its own
    // stream (armed until that extract); done = the last extract filled them
    struct HostOut {
        float* keys = nullptr;
        float* desc = nullptr;
        int cap = 0;
        bool armed = false, active = false, done = false;
    } host_out;
    // per-stage HIP events of an extract (sgpu_last_timing's stage slots).  Each event record
    // costs ~4.5 us of GPU time between the commands around it (tests/microbench/event_gap.hip),
    // ~40 us per single-image extract; sgpu_set_stage_timing(ctx, 0) drops them where they only
    // time (one-stream extracts; the multi-stream layouts need some to synchronise)
    bool stage_timing = true;
    bool streaming = false;                // inside sgpu_extract_stream (its waits use events)
    std::string err;
    // last extract
    int batch = 0, w = 0, h = 0, nparts = 0;
    std::vector<sgp::Octave> oct;
    size_t staged_bytes = 0;
    std::vector<int64_t> img_off;          // global per-image offsets [batch + 1]
    sgh::Part part[sgh::kMaxParts];
    sgh::DevBuf input, all_keys, all_desc, gray, pre;  // all_*: lazily gathered multi-part outputs;
                                                  // pre: the 2^ds-sampled input (-fo > 0)
    // sgpu_extract_stream: second input slot, copy-engine streams, slot events
    sgh::DevBuf input2;
    sgh::DevBuf duo_trash;                      // k_gauss_duo's / k_gauss_trio's scratch stores
    hipStream_t h2d = nullptr, d2h = nullptr;
    hipEvent_t up_ev[2] = {}, down_ev[2] = {};
    bool gathered = false;
    hipEvent_t ev[sgh::T_N + 1] = {};
    float timing[sgh::T_N] = {};
    // matcher
    sgh::DevBuf m_d1, m_d2, m_s1, m_s2, m_part, m_terms, m_match, m_dist, m_mask, m_loc, m_colpart, m_cols;
    sgh::DevBuf m_prune, m_s1c;                 // pruned column side: [rmax n1][map n1][ct n1 + pad], s8 rows
    bool match_prune = true;               // plain mutual matching prunes set 1 for the column side
                                           // (sgpu_debug_set_match_prune; SGPU_MATCH_PRUNE=off)
    std::vector<int> h_match;
    bool dist_ready = false;
    // grouped pair matcher (sgpu_match_batch): uploaded descriptors and their s8 form / row sums,
    // the planner's tables, chunk partials, decisions, [offsets npairs + 1 (64-bit)][counts npairs],
    // pairs
    sgh::DevBuf b_desc, b_s8, b_sums, b_plan, b_part, b_dec, b_cnt, b_out;
    sgh::DevBuf b_loc;                          // sgpu_match_batch_guided: uploaded locations [rows][2]
    sgplan::Plan b_hplan;
    bool b_planned = false;                // b_hplan is a call's plan (sgpu_debug_match_plan_stats)
    std::vector<unsigned char> b_tables;   // the tables as uploaded (alive until the call's sync)
    // geometry estimator (sgpu_estimate_batch): uploaded locations, [pairs][items][matches] in one
    // upload, the matches' float4 rows, [slots npairs (64-bit)][error flag], [models][inliers], mask
    sgh::DevBuf e_loc, e_plan, e_pts, e_slots, e_out, e_mask;
    sgeo::Plan e_hplan;
    std::vector<unsigned char> e_tables, e_result;
    // verify chain (sgpu_verify_batch; the matcher's and the estimator's buffers above carry its
    // tables, partials, decisions, matches and float4 rows): everything the stages hand each other
    // on the device and the one block that comes down (layout: sgpu_verify.cpp), its host copy
    sgh::DevBuf v_buf;
    std::vector<unsigned char> v_result;
    // preemptive matching (sgpu_prematch_batch, sgpu_select_top_scale_batch; the matcher's b_*
    // buffers above carry its tables, the subsets' matcher forms, partials, decisions and matches):
    // uploaded scales, the selected rows' indices, the gathered u8 rows of a caller's descriptors;
    // its plan over the subset offsets, those offsets and the all-pairs list
    sgh::DevBuf p_scale, p_index, p_u8;
    sgplan::Plan p_hplan;
    std::vector<int64_t> p_sub;
    std::vector<int> p_pairs;
    // track builder (sgpu_tracks_batch): the uploaded tables [set offsets][pair starts][pair bases]
    // [matches], the work arrays and the scans' scratch, [out_offsets][out_track][out_rows][header];
    // the tables as uploaded (alive until the call's first sync)
    sgh::DevBuf t_tab, t_work, t_out;
    std::vector<unsigned char> t_tables;
    // relative pose (sgpu_pose_batch; the estimator's e_loc, e_pts and e_hplan above carry its
    // uploaded locations, float4 rows and pair records): the uploaded tables [pairs][matches][set
    // pairs][F][intrinsics], [R][t][counts][points][mask]; the tables as uploaded (alive until the
    // call's sync) and the result block's host copy
    sgh::DevBuf o_tab, o_out;
    std::vector<unsigned char> o_tables, o_result;
    // device quantiser: staging of a host-pointer sgpu_quantize_descriptors_gpu, and the last
    // extract's descriptors as u8 / s8 / row sums (sgpu_feature_descriptors_u8; valid while f_ready)
    sgh::DevBuf q_in, q_out, f_u8, f_s8, f_sums;
    bool f_ready = false;
    // multi-GPU: RCCL communicator of this context's device (sgpu_comm_*)
    ncclComm_t comm = nullptr;
    int comm_ranks = 0, comm_rank = 0;
    sgh::DevBuf c_buf;

    int fail(int code, const char* what, hipError_t e = hipSuccess) {
        err = what;
        if (e != hipSuccess) {
            err += ": ";
            err += hipGetErrorString(e);
        }
        return code;
    }
    // part holding image i of the last batch
    int part_of(int i) const {
        for (int p = 0; p < nparts; p++)
            if (i < part[p].img0 + part[p].n) return p;
        return nparts - 1;
    }
};

#define HIPCHK(ctx, call)                                                \
    do {                                                                 \
        hipError_t _e = (call);                                          \
        if (_e != hipSuccess) return (ctx)->fail(SGPU_ENODEV, #call, _e); \
    } while (0)
#define ALLOCCHK(ctx, call)                                              \
    do {                                                                 \
        hipError_t _e = (call);                                          \
        if (_e != hipSuccess) return (ctx)->fail(SGPU_ENOMEM, #call, _e); \
    } while (0)

// ---- helpers that cross files ----
namespace sgh {
// sgpu_capi.cpp: a part's streams and events, created when the part is first used
enum { PS_MAIN = 1, PS_LO = 2, PS_OCT = 4, PS_ALL = 7 };
int part_streams(Part& pt, int which = PS_ALL);
// sgpu_match.cpp: dist[v] = float(acos(min(v * 2^-18, 1.0))), the expression of RowMatch_Kernel
// (ProgramCU.cu:1838), and the device table of it that every matcher reads (uploaded once)
float match_dist(int v);
int ensure_dist_table(sgpu_ctx* ctx);
// sgpu_extract.cpp: the last extract's descriptors as u8 / s8 / row sums (ctx->f_*)
int feature_u8(sgpu_ctx* ctx);
// sgpu_comm.cpp: destroys the context's communicator, if any
void comm_release(sgpu_ctx* ctx);

// ---- sgpu_pairs.cpp: what the callers of the grouped pair matcher share ----
// Where a call's sets come from: the last extract (images), or the caller's desc / loc / scale,
// host memory (uploaded by resolve_sets) or device memory (device).
struct SetSource {
    bool images = false, device = false;
    const uint8_t* desc = nullptr;
    const float* loc = nullptr;     // [rows][2]
    const float* scale = nullptr;   // row r's scale at scale[r * scale_stride]
    int scale_stride = 1;
};
// The sets on the device.  s8 / sums are set where the matcher's forms exist (the last extract's).
struct DeviceSets {
    const uint8_t* u8 = nullptr;
    const uint8_t* s8 = nullptr;
    const int* sums = nullptr;
    const float* loc = nullptr;     // x, y of row r at loc[r * loc_stride]
    int loc_stride = 2;
    const float* scale = nullptr;
    int scale_stride = 1;
    bool timing_started = false;    // ev[1] is recorded: the call had to quantise the batch
};
enum { SET_DESC = 1, SET_LOC = 2, SET_SCALE = 4 };
// `need` (SET_*) of the rows [0, rows) on the device: the batch's buffers (SET_DESC quantises them
// if need be, after recording ev[1]), uploads into b_desc / b_loc / p_scale, or the caller's
// device pointers as they are.  Queues on ctx->stream, waits for nothing.
int resolve_sets(sgpu_ctx* ctx, const SetSource& src, int64_t rows, int need, DeviceSets& sets);
// the states feature_u8 refuses, before anything is queued: "no extracted batch to <what>"
int check_batch(sgpu_ctx* ctx, const char* what);
// sgplan's verdict on the set offsets alone, before any size is taken from them
int probe_offsets(const int64_t* off, int nsets);
// a trailer's next 8-byte boundary
inline size_t round8(size_t n) { return (n + 7) & ~(size_t)7; }
// The plan-sized buffers: b_plan (table_bytes), b_part, b_dec, b_out (out_rows), b_cnt for
// cnt_pairs pairs (0: the caller keeps its counts elsewhere), b_s8 / b_sums for s8_rows rows (0:
// the matcher's forms exist).
int ensure_pair_buffers(sgpu_ctx* ctx, const sgplan::Plan& plan, size_t table_bytes,
                        int64_t out_rows, int cnt_pairs, int64_t s8_rows);
// s8 / sums of sets.u8's rows into b_s8 / b_sums, one launch, if sets has none
int derive_s8(sgpu_ctx* ctx, DeviceSets& sets, int64_t rows);
// One pass of the matcher over a plan's tables: k_match_pairs (guided: loc and geom set), finish,
// compact.  Partials and decisions go through b_part / b_dec.
struct MatchPass {
    const uint8_t* s8;
    const int* sums;
    const sgplan::Plan& plan;       // the counts of what tab points to
    sgplan::TableView tab;          // device
    float distmax, ratiomax;
    int max_match;
    int64_t out_rows;               // rows of d_out that may be written
    int* d_counts;
    long long* d_offs;
    int* d_out;
    const float* loc = nullptr;
    int loc_stride = 2;
    const sgk::GuidedParams* d_geom = nullptr;
};
int queue_match_pass(sgpu_ctx* ctx, const MatchPass& m);
// The host has the pairs' counts: the pairs that fit cap form a prefix, whose matches come down
// from d_out (want_matches false: counts only, cap is not looked at).  Returns the total, or
// SGPU_ERANGE when it exceeds cap (counts are complete) or the return type.
int download_fitting(sgpu_ctx* ctx, const int* counts, int npairs, const int* d_out, int* out_pairs,
                     int64_t cap, bool want_matches = true);
}  // namespace sgh
