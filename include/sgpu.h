/* sgpu.h -- C ABI of the MI355X SIFT hot path (libsiftgpu.so).
 *
 * Plain C types only (no torch, no C++): this is the boundary a cgo/ctypes/JNI binding or the
 * C++ SiftGPU/SiftMatchGPU classes (include/SiftGPU.h) call.  Each entry point names the
 * reference interface it replaces (paths relative to the reference repo root).
 *
 * Errors: every function returns SGPU_OK (0) or a negative SGPU_E* code; sgpu_last_error()
 * returns a message.  There is no CPU fallback: when no gfx950 device is usable the context
 * cannot be created and every compute call fails with SGPU_ENODEV.
 */
#ifndef SGPU_H
#define SGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGPU_OK 0
#define SGPU_EINVAL (-1)   /* bad argument */
#define SGPU_ENODEV (-2)   /* no usable GPU / HIP runtime error */
#define SGPU_ENOMEM (-3)   /* device or host allocation failed */
#define SGPU_ERANGE (-4)   /* capacity exceeded (e.g. more matches than max_match) */

/* Extraction / matching options.  Field meaning and defaults follow the reference's global
 * parameters (SiftGPU/GlobalUtil.cpp:50-135) and ParseParam (SiftGPU/SiftGPU.cpp:801-1246). */
typedef struct sgpu_options {
    float filter_width_factor;         /* -f   (4.0)                                        */
    float descriptor_window_factor;    /* -dw  (3.0)                                        */
    float orientation_window_factor;   /* -w   (2.0)                                        */
    float orientation_gaussian_factor; /*      (1.5)                                        */
    float dog_threshold;               /* -t   (0 -> 0.02/dog_level_num)                    */
    float edge_threshold;              /* -e   (0 -> 10)                                    */
    int subpixel;                      /* -s   (1)                                          */
    int max_orientation;               /* -m   (2)                                          */
    int fixed_orientation;             /* -ofix (0)                                         */
    int octave_min;                    /* -fo  first octave, >= -2 (0)                       */
    int octave_num;                    /* -no  (-1 = floor(log2(min(w,h)))-3)                */
    int dog_level_num;                 /* -d   (3)                                          */
    int lowe_origin;                   /* -loweo (0)                                        */
    int normalized;                    /* -unn clears (1)                                   */
    int descriptors;                   /* -sd clears (1)                                    */
    int keep_extremum_sign;            /* -sign (0)                                         */
    int circular_window;               /* 0: square orientation window of the active
                                          ProgramCU.cu:869-884; 1: circular window of
                                          ProgramCU-0.cu:834 / the GLSL path                */
    int verbose;                       /* -v   (0 here; the library prints nothing at 0)     */
    int max_dimension;                 /* -maxd (13200, GlobalUtil.cpp:86; SiftGPU::SetMaxDimension):
                                          while the first octave is wider or taller, octave_min
                                          is raised by one (PyramidCU::InitPyramid,
                                          PyramidCU.cpp:129-135)                              */
    int preprocess_on_cpu;             /* -prep / -noprep (1, GlobalUtil.cpp:81): with -fo > 0
                                          the input is first sampled by 2^fo and its width
                                          truncated (GLTexInput::SetImageData,
                                          GLTexImage.cpp:928-1009), then run from octave 0;
                                          0: the first octave is SampleImageD of the full input  */
    int feature_count_threshold;       /* -tc[1|2|3] <n> (-1 = off, GlobalUtil.cpp:135)         */
    int truncate_method;               /* 0: -tc / -tc1, 1: -tc2, 2: -tc3 (SiftGPU.cpp:1185-1203;
                                          SiftPyramid::LimitFeatureCount, SiftPyramid.cpp:219-260,
                                          and the level skip of PyramidCU::GenerateFeatureList,
                                          PyramidCU.cpp:829-853)                              */
} sgpu_options;

/* Defaults of GlobalUtil.cpp:50-135. */
void sgpu_default_options(sgpu_options* opt);

/* Parse reference command-line options into *opt (SiftGPU::ParseParam, SiftGPU.cpp:801-1246:
 * first-4-character case-insensitive option hashing, same argument rules).  Options the MI355X
 * path has no use for (-cuda, -winpos, -display, -pack, ...) are accepted and ignored; -cuda <n>
 * sets *device when device != NULL.  Returns SGPU_OK. */
int sgpu_parse_args(sgpu_options* opt, int argc, const char* const* argv, int* device);

typedef struct sgpu_ctx sgpu_ctx;

/* Create a context bound to HIP device `device` (replaces ProgramCU::CheckCudaDevice,
 * ProgramCU.cu:1414-1448, + PyramidCU construction).  The context owns all device buffers. */
int sgpu_ctx_create(int device, const sgpu_options* opt, sgpu_ctx** out);
int sgpu_ctx_destroy(sgpu_ctx* ctx);
int sgpu_ctx_set_options(sgpu_ctx* ctx, const sgpu_options* opt);
const char* sgpu_last_error(const sgpu_ctx* ctx);
/* Number of visible HIP devices (0 when the runtime is unusable). */
int sgpu_device_count(void);

/* Input flags. */
#define SGPU_INPUT_HOST   0   /* `images` is a host pointer                                */
#define SGPU_INPUT_DEVICE 1   /* `images` is a device pointer on the context's device      */
#define SGPU_INPUT_STAGED 2   /* use the batch staged in HBM by sgpu_stage_input (images
                                 may be NULL); the input stays resident across calls       */

/* Copy a batch of u8 images (same layout as sgpu_extract) into the context's device input
 * buffer, so that later extract calls with SGPU_INPUT_STAGED start from HBM-resident input. */
int sgpu_stage_input(sgpu_ctx* ctx, const uint8_t* images, int n, int w, int h, int stride);

/* Allocate now every device and pinned buffer that an extract of n gray u8 images of w x h
 * pixels (rows `stride` bytes apart, staged or uploaded) needs, so that the next
 * sgpu_stage_input + sgpu_extract of that geometry allocates nothing unless its keypoints exceed
 * the first-guess capacity.  Replaces SiftGPU::AllocatePyramid (SiftGPU.h:193,
 * SiftGPU.cpp:1435-1460 -> PyramidCU::ResizePyramid, PyramidCU.cpp:178-271).  Like an extract
 * it replaces the batch: the previous results and the staged input are gone. */
int sgpu_reserve(sgpu_ctx* ctx, int n, int w, int h, int stride);
/* The last extract's Gaussian pyramid (part 0): returns the number of kernel launches that
 * filtered its levels and stores the number of level filters in *filters (the reference's
 * FilterImage calls, PyramidCU.cpp:979-1044; several run in one launch under the diagonal and
 * paired-level schedules).  bench.py divides the pyramid's bytes and time by it. */
int sgpu_last_pyramid_launches(const sgpu_ctx* ctx, int* filters);
/* Test hook: number of device and pinned-host allocations the library has made so far. */
long long sgpu_debug_alloc_count(void);

/* Extract SIFT features from n gray u8 images of w x h pixels, row stride `stride` bytes,
 * image i at images + i*stride*h.  Replaces SiftGPU::RunSIFT(w, h, data, GL_LUMINANCE,
 * GL_UNSIGNED_BYTE) (SiftGPU.h:176, SiftGPU.cpp:233-268 -> SiftPyramid::RunSIFT,
 * SiftPyramid.cpp:58-216), batched.  Results stay valid until the next extract call.
 * What is read (this and every extract entry below, stride in its own unit): a host buffer is
 * copied as n * h * stride elements, so the last row's padding must exist; of each row only the
 * first w & ~3 columns are ever used (a device buffer's padding is never read). */
int sgpu_extract(sgpu_ctx* ctx, const uint8_t* images, int n, int w, int h, int stride,
                 int flags);

/* Host-in / host-out extraction of a stream of batches: nbatches batches of `batch` u8 gray
 * images (batches[k] -> batch images of w x h, rows `stride` bytes apart, in host memory).  The
 * keys (x, y, scale, orientation) and descriptors of all images go to keys[cap][4] and
 * desc[cap][128] (either may be NULL) in image order, counts[nbatches * batch] the per-image
 * feature counts.  Replaces a loop of SiftGPU::RunSIFT(w, h, data, GL_LUMINANCE,
 * GL_UNSIGNED_BYTE) + GetFeatureVector (SiftGPU.cpp:233-268, SiftPyramid.cpp:287-291) with the
 * reference's upload (PyramidCU.cpp:949-976) and descriptor download (PyramidCU.cpp:434) in the
 * pipeline: the upload of batch k+1 and the download of batch k-1 overlap batch k's kernels.
 * The copies overlap only from page-locked memory (sgpu_host_alloc).  Returns SGPU_ERANGE when
 * the features exceed cap (counts are complete, the features stop at the last batch that fit).
 * Afterwards the context holds no "last batch" for the per-image queries. */
int sgpu_extract_stream(sgpu_ctx* ctx, const uint8_t* const* batches, int nbatches, int batch,
                        int w, int h, int stride, float* keys, float* desc, int64_t cap,
                        int32_t* counts);
/* Page-locked host memory for sgpu_extract_stream's input and output (hipHostMalloc). */
void* sgpu_host_alloc(size_t bytes);
void sgpu_host_free(void* p);

/* Same with float luminance input in [0, 1] (stride in floats): the GL_FLOAT / converted-RGB
 * input path of GLTexInput::SetImageData (GLTexImage.cpp:981-1006). */
int sgpu_extract_f32(sgpu_ctx* ctx, const float* images, int n, int w, int h, int stride,
                     int flags);

/* Color input, converted to luminance on the device with the reference's formula
 * (GLTexInput::SetImageData -> DownSamplePixelDataI2F<u8>, GLTexImage.cpp:834-858:
 * (19595 r + 38470 g + 7471 b) / (65535 * 255); BGR swaps r and b; alpha ignored).  `format`
 * is one of SGPU_RGB, SGPU_BGR, SGPU_RGBA, SGPU_BGRA; `stride` in bytes.  Replaces
 * RunSIFT(w, h, data, GL_RGB | GL_BGR | GL_RGBA | GL_BGRA, GL_UNSIGNED_BYTE), batched. */
#define SGPU_RGB  1
#define SGPU_BGR  2
#define SGPU_RGBA 3
#define SGPU_BGRA 4
int sgpu_extract_color(sgpu_ctx* ctx, const uint8_t* images, int n, int w, int h, int stride,
                       int format, int flags);

/* Feature count of image i of the last extract (SiftGPU::GetFeatureNum, SiftGPU.cpp:1411). */
int sgpu_feature_count(const sgpu_ctx* ctx, int image);
/* Total over the batch. */
int64_t sgpu_feature_total(const sgpu_ctx* ctx);

/* Copy image i's keypoints (x, y, scale, orientation: 4 floats each) and descriptors (128
 * floats each) to host memory; either pointer may be NULL (SiftGPU::GetFeatureVector,
 * SiftGPU.cpp:1416-1428, SiftPyramid::CopyFeatureVector, SiftPyramid.cpp:287-291). */
int sgpu_copy_features(sgpu_ctx* ctx, int image, float* keys, float* descriptors);

/* Device pointers to the whole batch's keypoints [total][4] / descriptors [total][128] and the
 * per-image start offsets [n+1] (host array).  Zero-copy access for batch consumers. */
int sgpu_device_features(sgpu_ctx* ctx, const float** keys, const float** descriptors,
                         const int64_t** image_offsets);

/* Descriptors of caller-supplied keypoints on image `image` of the last extract (its pyramid is
 * reused): SiftGPU::RunSIFT(num, keys, keys_have_orientation) (SiftGPU.cpp:287-291,
 * SiftPyramid::SetKeypointList SiftPyramid.cpp:293-310, GenerateFeatureListTex
 * PyramidCU.cpp:454-504).  keys: num x (x, y, scale, orientation) in image coordinates.  With
 * has_orientation == 0 the strongest orientation is computed (ComputeOrientation_Kernel with
 * existing_keypoint) and the keys are rewritten as DownloadKeypoints does.  has_orientation ==
 * -1 is the rectangle mode (SIFT_RECT_DESCRIPTION, SiftPyramid.cpp:308-309): keys are
 * (x, y, width, height) and ComputeDescriptorRECT_Kernel (ProgramCU.cu:1104-1171) describes the
 * rectangle; keys come back unchanged.  Results (input order)
 * replace the context's features: image `image` reports num features (sgpu_copy_features),
 * every other image none. */
int sgpu_extract_keypoints(sgpu_ctx* ctx, int image, const float* keys, int num,
                           int has_orientation);

/* Matcher.  d1 [n1][128], d2 [n2][128] u8 descriptors (the reference quantizes float
 * descriptors as (unsigned char)int(512*d+0.5), SiftMatchCU.cpp:87-101: see
 * sgpu_quantize_descriptors).  Replaces SiftMatchGPU::SetDescriptors + GetSiftMatch
 * (SiftGPU.h:300-311; SiftMatchCU.cpp:139-179; kernels ProgramCU.cu:1466-1900).
 * Writes pairs {i, j} in ascending i into out_pairs (max_match entries) and returns the match
 * count (>= 0) or an error. */
int sgpu_match(sgpu_ctx* ctx, const uint8_t* d1, int n1, const uint8_t* d2, int n2,
               float distmax, float ratiomax, int mutual_best_match, int max_match,
               int* out_pairs, int flags);

/* Guided matcher: SiftMatchGPU::SetFeautreLocation + GetGuidedSiftMatch (SiftGPU.h:313-321;
 * SiftMatch.cpp:663-677; SiftMatchCU.cpp:104-136; kernel MultiplyDescriptorG_Kernel
 * ProgramCU.cu:1607-1777).  loc1 [n1][2], loc2 [n2][2] feature (x, y) (packed: the reference's
 * `gap` is applied by the caller); H, F row-major 3x3.  A pair passes when
 * |H x1 - x2| < hdistmax in both coordinates and its Sampson error under F is < fdistmax; the
 * dot of every pair of an 8-row block with a passing row enters the row/column decisions as
 * MultiplyDescriptorG_Kernel defines them.  H == NULL and F == NULL: plain sgpu_match; one of
 * them NULL: the identity with threshold 1e20.  SGPU_INPUT_DEVICE covers the locations too. */
int sgpu_match_guided(sgpu_ctx* ctx, const uint8_t* d1, int n1, const uint8_t* d2, int n2,
                      const float* loc1, const float* loc2, const float* H, const float* F,
                      float distmax, float ratiomax, float hdistmax, float fdistmax,
                      int mutual_best_match, int max_match, int* out_pairs, int flags);

/* Sharded matcher (multi-GPU extension of SiftMatchGPU::GetSiftMatch):
 * this rank holds rows [row_begin, row_begin + ns) of set 1 (d1 = those rows) and all n2 rows
 * of set 2.  The result over all ranks equals sgpu_match on the whole of set 1.
 * sgpu_match_shard_begin: row_match[ns] = the row decision of each local row (matched set-2
 * row or -1; RowMatch_Kernel, ProgramCU.cu:1785-1841) and, with mutual_best_match, col_best
 * [n2][3] = this shard's clamped column state (max dot, global set-1 row, second dot) of
 * ColMatch_Kernel (ProgramCU.cu:1844-1900).
 * sgpu_match_shard_end (host only, no device): merges the nshards column states (rank order),
 * applies the column decision and the mutual check (SiftMatchCU.cpp:166-176) and writes this
 * shard's pairs {global i, j} in ascending i; returns their count.  Concatenated in rank order
 * the shards' pairs are sgpu_match's (max_match applies per call).
 * sgpu_match_sharded: both, with the exchange as an RCCL all-gather over the context's
 * communicator (sgpu_comm_init; without one it is a single shard). */
int sgpu_match_shard_begin(sgpu_ctx* ctx, const uint8_t* d1, int ns, int row_begin,
                           const uint8_t* d2, int n2, float distmax, float ratiomax,
                           int mutual_best_match, int* row_match, int* col_best, int flags);
int sgpu_match_shard_end(const int* col_best_all, int nshards, int n2, const int* row_match,
                         int ns, int row_begin, float distmax, float ratiomax,
                         int mutual_best_match, int max_match, int* out_pairs);
int sgpu_match_sharded(sgpu_ctx* ctx, const uint8_t* d1, int ns, int row_begin,
                       const uint8_t* d2, int n2, float distmax, float ratiomax,
                       int mutual_best_match, int max_match, int* out_pairs, int flags);

/* float -> u8 quantization of SiftMatchCU::SetDescriptors (SiftMatchCU.cpp:94-99), host side. */
void sgpu_quantize_descriptors(const float* d, size_t count, uint8_t* out);
/* The same quantization on the device: d [ndesc][128] floats -> out [ndesc][128] u8, byte for
 * byte what sgpu_quantize_descriptors writes (the add in double).  SGPU_INPUT_HOST: both are host
 * pointers (upload, one kernel, download); SGPU_INPUT_DEVICE: both are device pointers. */
int sgpu_quantize_descriptors_gpu(sgpu_ctx* ctx, const float* d, size_t ndesc, uint8_t* out,
                                  int flags);
/* Device pointer to the last extract's descriptors as u8 [total][128], in the order of
 * sgpu_device_features (a multi-part batch goes through the same gathered buffer).  Quantized on
 * first request, in one launch that also prepares the matcher's forms of the sets, and kept until
 * the next extract, sgpu_extract_keypoints or options change.  SGPU_EINVAL when the context holds
 * no last batch (e.g. after sgpu_extract_stream) or descriptors are off. */
int sgpu_feature_descriptors_u8(sgpu_ctx* ctx, const uint8_t** desc_u8);
/* Copy image i's u8 descriptors (128 bytes each) to host memory: a quarter of the float
 * download of sgpu_copy_features.  Same error conditions as sgpu_feature_descriptors_u8. */
int sgpu_copy_features_u8(sgpu_ctx* ctx, int image, uint8_t* desc);

/* Grouped pair matcher: many set pairs of one descriptor buffer in one call.  desc is u8
 * [set_offsets[nsets]][128] (host, or device with SGPU_INPUT_DEVICE; exactly that many bytes are
 * read), set s = rows [set_offsets[s], set_offsets[s + 1]); set_offsets and set_pairs are host
 * arrays.  Pair p = (a, b) gives exactly sgpu_match(set a, set b, distmax, ratiomax,
 * mutual_best_match, max_match): {i, j} in ascending i, at most max_match per pair.  The pairs'
 * results are concatenated in pair order into out_pairs [cap][2], out_counts[p] = pair p's count;
 * returns the total.  More than cap matches: SGPU_ERANGE, all counts complete, the matches of
 * the leading pairs that fit written (sgpu_extract_stream's convention).  Empty sets give count
 * 0; (a, a), repeated pairs and both orders are legal; an index outside [0, nsets) or decreasing
 * offsets give SGPU_EINVAL.  No reference counterpart: SiftMatchGPU matches one pair per
 * SetDescriptors + GetSiftMatch (SiftGPU.h:300-311).  The number of kernel launches, copies and
 * synchronisations does not depend on npairs; sgpu_last_timing's times[8] is its device time. */
int sgpu_match_batch(sgpu_ctx* ctx, const uint8_t* desc, const int64_t* set_offsets, int nsets,
                     const int* set_pairs /* [npairs][2] */, int npairs,
                     float distmax, float ratiomax, int mutual_best_match, int max_match,
                     int* out_pairs /* [cap][2] */, int64_t cap, int* out_counts /* [npairs] */,
                     int flags);
/* sgpu_match_batch over the last extract: the sets are the batch's images, their descriptors
 * sgpu_feature_descriptors_u8's, so no descriptor crosses PCIe.  SGPU_EINVAL under the same
 * conditions as sgpu_feature_descriptors_u8. */
int sgpu_match_images(sgpu_ctx* ctx, const int* image_pairs, int npairs, float distmax,
                      float ratiomax, int mutual_best_match, int max_match,
                      int* out_pairs, int64_t cap, int* out_counts);

/* Guided matching of many set pairs in one call, each pair under its own matrices: pair p =
 * (a, b) gives exactly sgpu_match_guided(set a, set b, loc a, loc b, H + 9 p, F + 9 p, ...), set
 * a being the reference's set 1 (H x1 is compared with x2; the 8-row block rule of
 * MultiplyDescriptorG_Kernel counts set a's rows from the set's first row).  loc is
 * [set_offsets[nsets]][2] floats (x, y), packed, host or device memory together with desc
 * (SGPU_INPUT_DEVICE covers both); H and F are host arrays [npairs][9], row-major 3x3, or NULL:
 * a missing array is the identity with its threshold at 1e20 for every pair.  Both NULL: the call
 * is sgpu_match_batch and loc may be NULL.  Outputs, cap / SGPU_ERANGE, max_match, the legal
 * pair lists, SGPU_EINVAL and times[8] are sgpu_match_batch's; SGPU_EINVAL also for a NULL loc
 * with a matrix.  The geometric test runs inside the matching kernel: no mask is stored, and the
 * number of launches, copies and synchronisations does not depend on npairs (the matrices go up
 * with the plan's tables). */
int sgpu_match_batch_guided(sgpu_ctx* ctx, const uint8_t* desc, const float* loc,
                            const int64_t* set_offsets, int nsets,
                            const int* set_pairs /* [npairs][2] */, int npairs,
                            const float* H /* [npairs][9] or NULL */,
                            const float* F /* [npairs][9] or NULL */,
                            float distmax, float ratiomax, float hdistmax, float fdistmax,
                            int mutual_best_match, int max_match,
                            int* out_pairs /* [cap][2] */, int64_t cap,
                            int* out_counts /* [npairs] */, int flags);
/* sgpu_match_batch_guided over the last extract: descriptors as sgpu_match_images, locations =
 * x, y of the batch's device keys (the two floats SetFeatureLocation takes with gap = 2), so
 * neither a key nor a descriptor crosses PCIe.  Error conditions of sgpu_match_images. */
int sgpu_match_images_guided(sgpu_ctx* ctx, const int* image_pairs, int npairs,
                             const float* H, const float* F,
                             float distmax, float ratiomax, float hdistmax, float fdistmax,
                             int mutual_best_match, int max_match,
                             int* out_pairs, int64_t cap, int* out_counts);

/* Geometry of matched pairs: one homography or fundamental matrix per pair of a pair list, by a
 * fixed budget of RANSAC hypotheses, on the device, in one call -- the step between
 * sgpu_match_batch / sgpu_match_images and their guided forms.  No reference counterpart:
 * SiftMatchGPU::GetGuidedSiftMatch takes H and F from the caller (SiftGPU.h:313-321).
 *
 * loc, set_offsets, set_pairs: as sgpu_match_batch_guided (loc host memory, or device memory with
 * SGPU_INPUT_DEVICE).  matches / match_counts: the out_pairs / out_counts of sgpu_match_batch,
 * host arrays, set-local {i, j}, concatenated in pair order.  out_models[p] is a row-major 3x3 at
 * unit Frobenius norm that goes unchanged into sgpu_match_*_guided as H + 9 p or F + 9 p; set a is
 * the reference's set 1 (H x1 is compared with x2; the Sampson error of x2' F x1).  out_inliers[p]
 * = its inlier count, out_mask (or NULL) = one byte per match, 1 for an inlier.
 *
 * What is computed (csrc/sift_geom.h defines the arithmetic):
 *  - the inlier test is the guided matcher's own, in its float operation order: homography
 *    |H x1 - x2| < threshold in both coordinates; fundamental: Sampson error < threshold (squared
 *    pixels, as fdistmax).  The mask is exactly what the guided test says about the returned
 *    float matrix, so a guided pass at the same threshold keeps every inlier's geometry;
 *  - hypothesis t of pair position p draws its minimal sample (4 / 8 matches, without
 *    replacement) by a counter-based hash of (seed, p, t, draw), solves it in double (H: the
 *    four-point closed form; F: the eight-point null vector after isotropic normalisation,
 *    complete pivoting) and rounds to float.  Degenerate samples (a repeated point, three
 *    collinear points for H, a vanishing pivot for F) are never chosen;
 *  - the winner has the most inliers, then the lowest t.  `iterations` hypotheses are always
 *    run: the result is a pure function of the inputs and the seed;
 *  - a pair with fewer matches than the minimal sample, or without a valid hypothesis, has no
 *    model: zeros, 0 inliers, a zero mask; fed to a guided call it yields no matches;
 *  - F is the minimal-sample solution WITHOUT rank-2 enforcement (the Sampson test does not need
 *    it; a caller that wants epipoles enforces rank 2 itself).  No local refinement: the
 *    _refined forms below add it.
 * The number of launches, copies and synchronisations does not depend on npairs;
 * sgpu_last_timing's times[12] is the call's device time.
 * SGPU_EINVAL: a pair index outside [0, nsets), decreasing offsets, a negative count, a match
 * index outside its set (all checked on the host before anything is launched), iterations outside
 * [1, 65536], an unknown model, NULL out_models / out_inliers (or NULL inputs that are needed). */
#define SGPU_MODEL_HOMOGRAPHY  0   /* minimal sample 4 */
#define SGPU_MODEL_FUNDAMENTAL 1   /* minimal sample 8 */
int sgpu_estimate_batch(sgpu_ctx* ctx, const float* loc /* [set_offsets[nsets]][2] */,
                        const int64_t* set_offsets, int nsets,
                        const int* set_pairs /* [npairs][2] */, int npairs,
                        const int* matches /* [sum counts][2], set-local {i, j} */,
                        const int* match_counts /* [npairs] */,
                        int model, float threshold, int iterations, uint32_t seed,
                        float* out_models /* [npairs][9] */, int* out_inliers /* [npairs] */,
                        uint8_t* out_mask /* [sum counts] or NULL */, int flags);
/* sgpu_estimate_batch over the last extract: the sets are the batch's images, the locations x, y
 * of its device keys (a multi-part batch: the gathered key buffer), so no key crosses PCIe.
 * Error conditions of sgpu_match_images_guided. */
int sgpu_estimate_images(sgpu_ctx* ctx, const int* image_pairs, int npairs,
                         const int* matches, const int* match_counts,
                         int model, float threshold, int iterations, uint32_t seed,
                         float* out_models, int* out_inliers, uint8_t* out_mask);
/* The estimator followed by local refinement, still one call on the device: the winner of every
 * pair is refitted by least squares on its own inliers, up to refine_rounds times (0 .. 16;
 * outside: SGPU_EINVAL; 0 returns the bits of the unrefined call).  One round (csrc/sift_geom.h
 * defines the arithmetic):
 *  - both images' inlier points are normalised (centroid to the origin, mean absolute deviation
 *    per coordinate to 1), the 9 x 9 normal matrix of the DLT rows (H: two per inlier) or of the
 *    eight-point rows (F) is summed in double, and the eigenvector of its smallest eigenvalue,
 *    by cyclic Jacobi, is denormalised, scaled to unit Frobenius norm and rounded to float.  F
 *    stays without rank-2 enforcement; there is no sign convention;
 *  - the refit is scored with the same inlier test over all matches of the pair.  Fewer inliers
 *    than before: the round is rejected and the loop ends with the model it had.  Otherwise the
 *    refit, its mask and its count replace the model's, and the loop ends early when the mask
 *    did not change (the next refit would be the same) or a refit is degenerate.
 * So out_inliers[p] is never below the unrefined call's, out_mask is still exactly the guided test
 * of out_models[p], a pair without a model stays without one, and the result is a pure function of
 * the inputs and the seed.  out_rounds (or NULL) [npairs] = the accepted rounds of every pair.  The
 * launches, copies and synchronisations depend neither on npairs nor on refine_rounds (one more
 * launch than the unrefined call, none more for 0); times[12] covers it.  All other arguments,
 * flags, outputs and error conditions are those of sgpu_estimate_batch / sgpu_estimate_images. */
int sgpu_estimate_batch_refined(sgpu_ctx* ctx, const float* loc, const int64_t* set_offsets,
                                int nsets, const int* set_pairs, int npairs, const int* matches,
                                const int* match_counts, int model, float threshold,
                                int iterations, uint32_t seed, int refine_rounds,
                                float* out_models, int* out_inliers, uint8_t* out_mask,
                                int* out_rounds /* [npairs] or NULL */, int flags);
int sgpu_estimate_images_refined(sgpu_ctx* ctx, const int* image_pairs, int npairs,
                                 const int* matches, const int* match_counts,
                                 int model, float threshold, int iterations, uint32_t seed,
                                 int refine_rounds, float* out_models, int* out_inliers,
                                 uint8_t* out_mask, int* out_rounds /* [npairs] or NULL */);

/* Timing of the last call: stage times in milliseconds measured with HIP events
 * (SiftGPU::_timing, SiftPyramid.cpp:48-56).  times[0..7] =
 * {upload, pyramid, detect, orientation, expand, descriptor, download, total} of the last
 * extract; times[8] = the last sgpu_match call; times[9] = the feature-list (row scan) part of
 * detect; times[10], [11] = the key and descriptor copies of the last sgpu_copy_features;
 * times[12] = the last sgpu_estimate_* call; times[13] = the last sgpu_verify_* call; times[14] =
 * the last sgpu_prematch_* call; times[15] = the last sgpu_tracks_* call; times[16] = the last
 * sgpu_pose_* call.
 * SiftGPU::_timing[2..8] map them to the reference's slots (siftgpu_api.cpp).  Slots 0-7 and
 * 9-11 read 0 after a one-stream extract / copy made with the stage timing off. */
int sgpu_last_timing(const sgpu_ctx* ctx, float* times, int n);
/* Register page-locked host buffers (sgpu_host_alloc) for the NEXT extract of one image
 * (sgpu_extract / _f32 / _color with n == 1): it writes image 0's keys (4 floats each) and
 * descriptors (128 floats each; descriptors may be NULL) for up to `capacity` features into them
 * from the GPU, in its own stream before its one synchronisation, in place of the count copy and
 * the two downloads of sgpu_copy_features.  sgpu_copy_features(ctx, 0, keys, descriptors) with
 * the same pointers then returns at once when the image's features fit (otherwise it copies as
 * usual).  The registration is consumed by that extract.  No reference counterpart: the
 * reference's RunSIFT downloads keys and descriptors after the pyramid (PyramidCU.cpp:434). */
int sgpu_set_host_output(sgpu_ctx* ctx, float* keys, float* descriptors, int capacity);
/* Stage timing on (default) or off.  Replaces the reference's GlobalUtil::_timingS (GlobalUtil.cpp:51,
 * set by SiftGPU::SetVerbose, SiftGPU.cpp:401-429; 0 skips the per-stage finish calls,
 * PyramidCU.cpp:439,873,1041).  Off, a one-stream extract records none of its ~10 stage events
 * (each ~4.5 us of GPU time between two kernels); the multi-stream layouts and
 * sgpu_extract_stream keep the events they synchronise on. */
int sgpu_set_stage_timing(sgpu_ctx* ctx, int on);

/* ---- multi-GPU batch driver (no reference counterpart: the reference
 * runs one SiftGPU per device thread, TestWin/MultiThreadSIFT.cpp:141-155).  One process per
 * GPU, each with its own context; images are sharded and the only exchange is an RCCL
 * all-gather (over xGMI) of the per-image feature counts.  Rendezvous: rank 0 creates the id,
 * the launcher distributes it (bench.py uses torch.distributed on the host). */
#define SGPU_COMM_ID_BYTES 128
/* Create a communicator id (ncclGetUniqueId) into id[bytes], bytes >= SGPU_COMM_ID_BYTES. */
int sgpu_comm_unique_id(uint8_t* id, int bytes);
/* Join the communicator of nranks contexts (ncclCommInitRank, collective over the ranks). */
int sgpu_comm_init(sgpu_ctx* ctx, int nranks, int rank, const uint8_t* id, int bytes);
/* recv[r*n + i] = send of rank r, element i (host arrays; device staging + ncclAllGather). */
int sgpu_comm_allgather_i32(sgpu_ctx* ctx, const int32_t* send, int n, int32_t* recv);
/* In-place all-reduce of n doubles (op_max != 0: max, else sum). */
int sgpu_comm_allreduce_f64(sgpu_ctx* ctx, double* v, int n, int op_max);

/* ---- test hooks (parity tests read intermediate stages; not part of the drop-in surface) ---- */
/* Per-context debug flags (0 = shipped configuration). */
#define SGPU_DEBUG_PARTS2   1   /* split a batch into 2 parts on separate streams              */
#define SGPU_DEBUG_PARTS4   2   /* ... into 4 parts                                            */
#define SGPU_DEBUG_TINY_CAP 4   /* start the keypoint capacity at 64 per part, so that the
                                   capacity-overflow re-run of a part is exercised             */
#define SGPU_DEBUG_FUSED_MATCH 8 /* plain mutual matching through the fused one-GEMM kernel
                                   (the guided matcher always uses it)                         */
#define SGPU_DEBUG_EXACT_DESCRIPTOR 16 /* descriptors in the reference's per-bin fma order with the
                                   oracle's transcendentals: bit-identical to the oracle.  The
                                   shipped kernel sums in any order with hardware sqrt/rcp/exp
                                   (descriptor L2 ~1e-6 from the oracle).  Also set at context
                                   creation by the environment variable SGPU_EXACT_DESCRIPTOR=1 */
#define SGPU_DEBUG_GAUSS_BLOCK 32 /* Gaussian levels through the workgroup strip kernel
                                   (k_gauss_pk2) instead of the shipped wave-streaming one
                                   (k_gauss_lean); both are bit-identical.  Bits
                                   SGPU_DEBUG_BAND_SHIFT.. of the flags, when not 0, force the
                                   wave kernel's band height in rows (test / tuning hook) */
#define SGPU_DEBUG_BAND_SHIFT 20  /* band height field: (flags >> 20) & 0x7ff rows (< 2048); the flag bits
                                     below it never reach it (DESC_DUAL at 1 << 16
                                     used to share its bit with the band field) */
#define SGPU_DEBUG_KEYED_MATCH 64 /* plain matching through the keyed epilogue (every value
                                   folded with its column's tie-order bits) even when
                                   ratiomax <= 1, where the keyless one is exact and used     */
#define SGPU_DEBUG_FULL_COLUMNS 128 /* plain mutual matching decides every column of set 2, not
                                   only the columns some row of set 1 matched                 */
#define SGPU_DEBUG_DESC_DUAL 256 /* detected features' descriptors through the round-4 dual-cell
                                    kernel instead of the pixel-parallel k_descriptor_flat */
#define SGPU_DEBUG_ORIENT_WAVE 512 /* orientation one wave per candidate for any count (the shipped
                                     path picks it for few candidates only): same bits */
#define SGPU_DEBUG_GAUSS_TILE_ALWAYS 1024 /* every level through the 2-D tile kernel
                                             (k_gauss_tile) and the extremum detection through
                                             k_extrema_tile, whatever the size (the shipped path
                                             tiles levels of at most SGPU_GAUSS_TILE_MB, default
                                             16 MB: a single image's): same levels and keys */
#define SGPU_DEBUG_MATCH_REGSTAGE 2048 /* keyless plain matching through the register-staged
                                          k_match_rows<..., RAW> instead of the LDS-DMA
                                          k_match_raw: same pairs */
#define SGPU_DEBUG_PYR_SERIAL 4096 /* the pyramid octave by octave, one level per launch (the
                                      shipped path runs octave o+1's first levels in the same
                                      launches as octave o's last ones; the stream layout runs
                                      octaves >= 1 on a second stream): same levels */
#define SGPU_DEBUG_GAUSS_LONG_BANDS 8192 /* Gaussian bands of >= 4 chunks on every level (round
                                            2's band rule; the shipped rule lets cache-resident
                                            levels use 1-chunk bands): same levels.  Also set at
                                            context creation by SGPU_GAUSS_BANDS=long */
#define SGPU_DEBUG_DUO_ALWAYS 16384 /* paired-level Gaussian launches (k_gauss_duo) for every
                                        eligible level pair, whatever its size (the shipped path
                                        pairs only levels of >= 128 MB): same levels */
#define SGPU_DEBUG_DUO_OFF 32768 /* no paired-level launches (one level per launch, the round-4
                                    schedule): same levels */
#define SGPU_DEBUG_GAUSS_TILE_OFF 65536 /* no 2-D tile launches: every level through the
                                           wave-streaming kernels (round 5): same levels */
#define SGPU_DEBUG_DESC_WIDE_OFF 131072 /* descriptors one wave per feature for every count (the
                                           shipped path gives few features a workgroup each):
                                           same bits */
#define SGPU_DEBUG_DESC_WIDE_ALWAYS 262144 /* descriptors one workgroup per feature for every
                                              count: same bits */
#define SGPU_DEBUG_EXTREMA_TILE_OFF 524288 /* extremum detection always through the
                                              wave-streaming k_extrema_wave2 (the shipped path
                                              tiles cache-resident pyramids, k_extrema_tile;
                                              SGPU_DEBUG_GAUSS_TILE_ALWAYS tiles every one) */

int sgpu_debug_set_flags(sgpu_ctx* ctx, int flags);
/* How a batch's orientation and descriptor kernels get their work, a test / A-B
 * hook -- the same bits in every form.  (A setter of its own: every flag bit below the band
 * height field is taken.)  QUEUE (shipped): resident one-wave workgroups fed from the extract's
 * work counters (k_orientation_queue, k_descriptor_queue); STATIC_ORIENTATION, STATIC_DESCRIPTOR:
 * that kernel through a grid that covers the work (k_orientation, k_descriptor_flat); STATIC:
 * both.  SGPU_FEATURE_QUEUE=on / ori / desc / off at context creation sets the same. */
#define SGPU_FEATURES_QUEUE 0
#define SGPU_FEATURES_STATIC_ORIENTATION 1
#define SGPU_FEATURES_STATIC_DESCRIPTOR 2
#define SGPU_FEATURES_STATIC 3
int sgpu_debug_set_feature_queue(sgpu_ctx* ctx, int mode);
/* The batch pyramid's launch plan, a test / A-B hook -- the levels are the same
 * bits in every plan.  trio: three-level launches (k_gauss_trio): none (shipped), on levels of
 * >= 512 MB, or wherever the widths and the decimation allow (SGPU_TRIO=off / on / always at
 * context creation).  pairs: the octave's paired-level launches taken from its end, (4, 5),
 * (2, 3) with the decimation, (0, 1) (shipped), or from its front (SGPU_DUO_PLAN=end / front). */
#define SGPU_TRIO_OFF 0
#define SGPU_TRIO_ON 1
#define SGPU_TRIO_ALWAYS 2
#define SGPU_PAIRS_FRONT 0
#define SGPU_PAIRS_END 1
int sgpu_debug_set_schedule(sgpu_ctx* ctx, int trio, int pairs);
/* Strip geometry of the paired-level launches (k_gauss_duo), a test / A-B hook --
 * the levels are the same bits in every form.  RULE (shipped): a workgroup's four waves share one
 * strip of 480 columns where that issues fewer lane-columns than a strip of 96 columns per wave
 * (1920, 960 and 480 columns, not 240; levels of at most 1920 columns) and measured faster; WAVE: a strip per wave on
 * every level; COOP: the shared strip wherever it is compiled, at any width. */
#define SGPU_DUO_STRIPS_RULE 0
#define SGPU_DUO_STRIPS_WAVE 1
#define SGPU_DUO_STRIPS_COOP 2
int sgpu_debug_set_duo_strips(sgpu_ctx* ctx, int mode);
/* The last Gaussian level of every octave, a test / A-B hook -- the same features
 * in every mode.  Only the last DoG plane reads that level, and ComputeKEY reads that plane only
 * around a candidate of the top DoG level.  LAZY: the pyramid leaves the level out; the
 * wave-streaming extremum kernel marks the top DoG level's undecided pixels in the keypoint mask,
 * and k_extrema_top evaluates the level at their 3 x 3 neighbourhoods (the dense filter's bits),
 * stores those values and decides them; the rest of the level's plane holds stale data.  DENSE:
 * every level filtered for every pixel.  RULE (shipped): lazy where the batch is too large for the
 * tile extremum kernel, dense otherwise.  Whatever the mode, a batch whose extremum pass is the tile
 * kernel is dense.  SGPU_TOP_LEVEL=dense / lazy at context creation sets the same.
 * sgpu_last_pyramid_launches reports the filters that ran; sgpu_debug_gaussian returns the dense
 * level in every mode (it filters a lazy octave's last level on first request). */
#define SGPU_TOP_LEVEL_RULE 0
#define SGPU_TOP_LEVEL_DENSE 1
#define SGPU_TOP_LEVEL_LAZY 2
int sgpu_debug_set_top_level(sgpu_ctx* ctx, int mode);
/* Plain mutual matching (ratiomax <= 1) decides the listed columns over the rows of set 1 that can
 * change a decision -- those with some dot at or above the smallest second value that fails the
 * ratio test against the weakest passing row maximum -- instead of all of set 1 (on != 0, the
 * shipped default; SGPU_MATCH_PRUNE=off at context creation turns it off): the same pairs
 * (DESIGN.md 4.8), a test / A-B hook. */
int sgpu_debug_set_match_prune(sgpu_ctx* ctx, int on);
/* The plan of the last sgpu_match_batch / sgpu_match_images call, read-only:
 * out[0] = work items, out[1] = sides, out[2] = the most 128-column tiles of any item,
 * ceil((c_end - c_begin) / 128), out[3] = the most column chunks of any side (all 0 for a call
 * with no pair of two non-empty sets).  SGPU_EINVAL before the first such call and after one whose
 * offsets or pair indices were rejected.  Tests use it to prove which plan regime they ran in. */
int sgpu_debug_match_plan_stats(const sgpu_ctx* ctx, long long out[4]);
/* The launch list of the last extract's Gaussian pyramid (part 0) as its planner made it
 * (csrc/sift_pyramid_plan.h), read-only, in issue order.  Returns the number of
 * entries and writes the first cap / SGPU_PLAN_ENTRY_INTS of them to out (cap ints; 0 with out
 * NULL just counts): per entry {kind, o0, k0, o1, k1, o2, k2} -- kind one of SGPU_PLAN_*, then the
 * (octave, level written) of each level filter of the launch, (-1, -1) where the kind has fewer.
 * An entry of a "two" kind can take one or two kernel launches (sgpu_last_pyramid_launches counts
 * those).  SGPU_EINVAL before the first extract.  Tests use it to prove which launches ran. */
#define SGPU_PLAN_ENTRY_INTS 7
#define SGPU_PLAN_LEVEL 0        /* one level, wave kernels (k_gauss_lean / k_gauss_pk2)        */
#define SGPU_PLAN_TILE 1         /* one level in 2-D tiles (k_gauss_tile)                       */
#define SGPU_PLAN_TWO 2          /* two independent levels, wave kernels                        */
#define SGPU_PLAN_TILE_TWO 3     /* two independent tiled levels                                */
#define SGPU_PLAN_TILE_DUO 4     /* two consecutive levels per tile (k_gauss_tile_duo)          */
#define SGPU_PLAN_TILE_DUO_ONE 5 /* a tile duo beside an independent tiled level                */
#define SGPU_PLAN_DUO 6          /* paired levels (k_gauss_duo)                                 */
#define SGPU_PLAN_TRIO 7         /* three levels (k_gauss_trio)                                 */
#define SGPU_PLAN_KINDS 8
int sgpu_debug_pyramid_plan(const sgpu_ctx* ctx, int* out, int cap);
/* Octave geometry of the last extract: n_octaves, and (w, h, wa) per octave. */
int sgpu_debug_geometry(const sgpu_ctx* ctx, int* n_octaves, int* dims /* 3*max */, int max);
/* Gaussian level (image, octave, level 0..level_num-1) as wa*h floats. */
int sgpu_debug_gaussian(sgpu_ctx* ctx, int image, int octave, int level, float* out);
/* Detected (pre-orientation) keypoints of the batch in reference order: per entry
 * {col, row, level_id, image} ints and {dx, dy, ds, pad} floats.  Returns count via *n. */
int sgpu_debug_candidates(sgpu_ctx* ctx, int* ints, float* floats, int cap, int* n);
/* The sparse evaluation of the last Gaussian level (k_extrema_top's) at one point
 * of the last extract: out[3 r + c] = the level at (x + c - 1, y + r - 1) of (image, octave),
 * computed from the level below it; 1 <= x <= wa - 2, 1 <= y <= h - 2.  Stores nothing into the
 * pyramid.  From the test-hook library, like sgpu_debug_candidates. */
int sgpu_debug_top_level_at(sgpu_ctx* ctx, int image, int octave, int x, int y, float out[9]);

/* Verified matches of many set pairs in one call: putative matching, one H and / or F per pair
 * with local refinement, and guided matching under those matrices, queued back to back on the
 * device.  Neither a match nor a matrix crosses PCIe between the stages, and the host validates
 * and plans once.  No reference counterpart (SiftMatchGPU::GetGuidedSiftMatch takes H and F from
 * the caller, SiftGPU.h:313-321).
 *
 * Contract: the results are the bits of the chain of the separate calls.  Let
 *   1  P = sgpu_match_batch(desc, ..., distmax, ratiomax, mutual_best_match, max_match) with a
 *      cap that holds everything;
 *   2  for each requested model X: sgpu_estimate_batch_refined(loc, ..., matches = P, model X,
 *      X_threshold, iterations, seed, refine_rounds) -- the same seed for both models, the same
 *      pair positions;
 *   3  sgpu_match_batch_guided(desc, loc, ..., H, F, distmax, ratiomax, hdistmax, fdistmax,
 *      mutual_best_match, max_match, cap).
 * Then out_putative (or NULL) [npairs] = P's counts; out_H / out_F [npairs][9] and
 * out_inliers_H / out_inliers_F (or NULL) [npairs] = step 2's bytes; out_pairs, out_counts and
 * the return value = step 3's, with its cap / SGPU_ERANGE convention (the putative pass has no
 * cap) and its legal pair lists.  out_H == NULL: no H is estimated and the guided pass runs under
 * the identity with threshold 1e20 for H, as a NULL H does there; the same for F.  A pair with
 * fewer putative matches than a requested model's minimal sample, or without a valid hypothesis,
 * gets a zero matrix and therefore no verified match, exactly as the chain gives.
 *
 * desc, loc, set_offsets, set_pairs and flags: as sgpu_match_batch_guided (SGPU_INPUT_DEVICE
 * covers desc and loc).  SGPU_EINVAL, all checked on the host before anything is queued: every
 * argument error of the three calls, NULL params, iterations outside [1, 65536], refine_rounds
 * outside [0, 16], out_H and out_F both NULL (that call is sgpu_match_batch), a NULL loc or desc
 * with rows to read.
 * One table upload, at most two synchronisations, and no device-to-host copy or host wait before
 * the last kernel is queued; the number of launches, copies and synchronisations depends neither
 * on npairs nor on refine_rounds.  sgpu_last_timing's times[13] is the call's device time, from
 * before its first kernel to after its last; the call leaves times[8] and times[12] as they were. */
typedef struct sgpu_verify_params {
    float distmax, ratiomax;        /* both matching passes (sgpu_match_batch's)            */
    int   mutual_best_match;
    int   max_match;                /* per pair, both passes                                */
    float h_threshold, f_threshold; /* estimator thresholds (sgpu_estimate_batch's)         */
    float hdistmax, fdistmax;       /* guided pass thresholds (sgpu_match_batch_guided's)   */
    int   iterations;               /* 1 .. 65536                                           */
    uint32_t seed;
    int   refine_rounds;            /* 0 .. 16                                              */
} sgpu_verify_params;
/* distmax 0.7, ratiomax 0.8, mutual_best_match 1, max_match 4096; h_threshold 2.0, f_threshold
 * 4.0; hdistmax 2.0, fdistmax 4.0; iterations 512, seed 0, refine_rounds 3 -- the values this
 * project's tests and timing scripts run the separate calls with.  Needs no device. */
void sgpu_default_verify_params(sgpu_verify_params* p);
int sgpu_verify_batch(sgpu_ctx* ctx, const uint8_t* desc, const float* loc,
                      const int64_t* set_offsets, int nsets,
                      const int* set_pairs /* [npairs][2] */, int npairs,
                      const sgpu_verify_params* params,
                      float* out_H /* [npairs][9] or NULL */, int* out_inliers_H /* or NULL */,
                      float* out_F /* [npairs][9] or NULL */, int* out_inliers_F /* or NULL */,
                      int* out_putative /* [npairs] or NULL */,
                      int* out_pairs /* [cap][2] */, int64_t cap, int* out_counts /* [npairs] */,
                      int flags);
/* sgpu_verify_batch over the last extract: sets, descriptors and locations as
 * sgpu_match_images_guided takes them (the device u8 descriptors, x, y of the device keys; a
 * multi-part batch: its gathered buffers).  Error conditions of sgpu_match_images_guided and
 * sgpu_verify_batch. */
int sgpu_verify_images(sgpu_ctx* ctx, const int* image_pairs, int npairs,
                       const sgpu_verify_params* params,
                       float* out_H, int* out_inliers_H, float* out_F, int* out_inliers_F,
                       int* out_putative, int* out_pairs, int64_t cap, int* out_counts);

/* Preemptive matching: which pairs of a batch are worth matching, from every set's `top`
 * largest-scale rows alone (Wu, "Towards Linear-time Incremental Structure from Motion", 3DV 2013,
 * section 3: h = 100 features, pairs with at least 4 subset matches are kept).  No reference
 * counterpart in SiftMatchGPU.  The selection, the gather of the selected rows and the matching of
 * the subsets run on the device; the thresholding of the counts is the caller's.
 *
 * Selection rule (csrc/sift_select.h): of a set of n rows, m = min(n, top) are
 * selected: the rows with the largest scales, compared as the monotone unsigned image of their
 * float bits (a total order of every bit pattern; the numeric order for the positive finite scales
 * of extracted keys), equal values resolving to the lower row index.  The selection is reported as
 * set-local row indices in ascending order.
 *
 * sgpu_select_top_scale_batch: the scale of buffer row r is scale[r * scale_stride] (host memory,
 * or device memory with SGPU_INPUT_DEVICE; the floats up to the last row's scale are read), set s =
 * rows [set_offsets[s], set_offsets[s + 1]).  out_offsets[0 .. nsets] = the scan of min(n_s, top),
 * out_index[out_offsets[s] ..) = set s's selection.  sgpu_select_top_scale_images: the sets are the
 * last extract's images, the scale column 2 of its device keys. */
int sgpu_select_top_scale_batch(sgpu_ctx* ctx, const float* scale, int scale_stride /* floats */,
                                const int64_t* set_offsets, int nsets, int top,
                                int* out_index /* [sum min(n_s, top)] */,
                                int64_t* out_offsets /* [nsets + 1] */, int flags);
int sgpu_select_top_scale_images(sgpu_ctx* ctx, int top, int* out_index, int64_t* out_offsets);
/* sgpu_prematch_batch -- contract: the bits of the chain.  With idx_s the selection of set s, pair
 * (a, b) gives exactly sgpu_match_batch on the two gathered subsets (rows idx_a and idx_b, in that
 * ascending order) with max_match = top, and every match {i, j} is reported as {idx_a[i],
 * idx_b[j]}: set-local rows, still in ascending first index.  top >= every n returns the bits of
 * sgpu_match_batch with max_match = top.
 * desc, set_offsets and the legal pair lists are sgpu_match_batch's (a device desc is 16-byte
 * aligned); scale as above, host or device memory together with desc.  set_pairs == NULL: all pairs
 * a < b in lexicographic order, and npairs must be nsets (nsets - 1) / 2.  out_counts [npairs] is
 * always complete and the return value is its total.  out_pairs == NULL: counts only, cap is
 * ignored and no match is downloaded; otherwise sgpu_match_batch's cap / SGPU_ERANGE convention.
 * SGPU_EINVAL, checked on the host before anything is queued: top < 1, scale_stride < 1, a NULL
 * scale or desc with rows to read, NULL out_counts (NULL out_index / out_offsets for the select
 * calls), bad offsets or pair indices, the all-pairs count mismatch.
 * The number of launches, copies and synchronisations depends neither on nsets nor on npairs (one
 * table upload; the host plans from set_offsets and top alone).  sgpu_last_timing's times[14] is
 * the call's device time, from before the selection to after the last kernel; every other slot is
 * left as it was.
 * The _images forms run over the last extract (scales: column 2 of the device keys; descriptors:
 * the matcher's forms behind sgpu_feature_descriptors_u8, gathered in place of a new preparation;
 * a multi-part batch: its gathered buffers), with the error conditions of sgpu_match_images. */
int sgpu_prematch_batch(sgpu_ctx* ctx, const uint8_t* desc, const float* scale, int scale_stride,
                        const int64_t* set_offsets, int nsets,
                        const int* set_pairs /* [npairs][2] or NULL */, int npairs, int top,
                        float distmax, float ratiomax, int mutual_best_match,
                        int* out_counts /* [npairs] */,
                        int* out_pairs /* [cap][2] or NULL */, int64_t cap, int flags);
int sgpu_prematch_images(sgpu_ctx* ctx, const int* image_pairs, int npairs, int top,
                         float distmax, float ratiomax, int mutual_best_match,
                         int* out_counts, int* out_pairs, int64_t cap);

/* Feature tracks from a pair list's matches, built on the device: the step between matching and
 * reconstruction (Wu, 3DV 2013).  A track is the set of features, at most one per set, that the
 * matches connect transitively.  No reference counterpart in SiftGPU.
 *
 * Rule (csrc/sift_tracks.h).  set_offsets, set_pairs, matches (set-local {i, j},
 * concatenated in pair order) and match_counts are the offsets, pair list, out_pairs and out_counts
 * of sgpu_match_batch, sgpu_match_batch_guided or sgpu_verify_batch.  A node is a buffer row
 * r = set_offsets[s] + i, rows = set_offsets[nsets]; match {i, j} of pair (a, b) is the edge
 * (set_offsets[a] + i, set_offsets[b] + j), a self-loop is none.  A connected component is
 * labelled by its smallest row.  With fewer than min_length rows it is short; otherwise, with more
 * rows than nsets or two rows in one set, inconsistent; otherwise a track.  Tracks are numbered
 * 0 .. T - 1 in ascending label order.
 *   out_track [rows]          the row's track id; SGPU_TRACK_NONE for an unmatched row or a row of
 *                             a short component, SGPU_TRACK_INCONSISTENT for a row of an
 *                             inconsistent one
 *   out_offsets [rows / 2 + 1], out_rows [rows]    both or neither: out_offsets[0 .. T] written,
 *                             out_rows[out_offsets[t] .. out_offsets[t + 1]) = track t's rows in
 *                             ascending order, which is set order
 *   out_stats [4] or NULL     {components of >= 2 rows, tracks, inconsistent components, short
 *                             components of >= 2 rows}
 * The result is a pure function of the inputs.  All arrays are host memory.  Returns T or a
 * negative error.
 * SGPU_EINVAL, all checked on the host before anything is queued, no output byte written: NULL
 * context, bad offsets or pair indices, a negative count, a match index outside its set,
 * min_length < 2, rows >= 2^31, NULL out_track, exactly one of out_offsets / out_rows NULL, a NULL
 * input that is needed.  SGPU_ENODEV: a device error, or the kernels' own termination check (a
 * union-find step that did not move to a smaller row; never with intact memory).
 * One upload (offsets, pair bases and matches in one block), at most two synchronisations; the
 * number of launches, copies and synchronisations depends neither on npairs, nsets nor T.
 * sgpu_last_timing's times[15] is the call's device time, from before its first kernel to after
 * its last; every other slot is left as it was.  A repeated call of the same shape allocates
 * nothing.
 * sgpu_tracks_images: the sets are the last extract's images (image_pairs and matches as
 * sgpu_match_images / sgpu_verify_images return them), with the error conditions of
 * sgpu_match_images. */
#define SGPU_TRACK_NONE (-1)
#define SGPU_TRACK_INCONSISTENT (-2)
int sgpu_tracks_batch(sgpu_ctx* ctx, const int64_t* set_offsets, int nsets,
                      const int* set_pairs /* [npairs][2] */, int npairs,
                      const int* matches /* [sum counts][2] */, const int* match_counts,
                      int min_length,
                      int* out_track /* [rows] */, int64_t* out_offsets /* [rows/2+1] or NULL */,
                      int* out_rows /* [rows] or NULL */, long long* out_stats /* [4] or NULL */);
int sgpu_tracks_images(sgpu_ctx* ctx, const int* image_pairs, int npairs,
                       const int* matches, const int* match_counts, int min_length,
                       int* out_track, int64_t* out_offsets, int* out_rows, long long* out_stats);

/* Relative pose and triangulation of verified pairs, on the device: the two-view step between a
 * pair's F (sgpu_estimate_* / sgpu_verify_*) and a reconstruction.  It says which of the four
 * decompositions of the pair's essential matrix is the physical one, how many matches lie in front
 * of both cameras and how many of those have a useful triangulation angle: what an initial pair is
 * chosen by, and what tells a pure rotation or a plane from a pair with a baseline.  No reference
 * counterpart in SiftGPU.
 *
 * loc, set_offsets, set_pairs, matches, match_counts, flags: exactly those of sgpu_estimate_batch
 * (loc host memory, or device memory with SGPU_INPUT_DEVICE; everything else host memory).
 * intrinsics[s] = {fx, fy, cx, cy} of set s: a pinhole camera without skew or distortion.  F + 9 p
 * = pair p's fundamental matrix as sgpu_estimate_* / sgpu_verify_* return it: set a is the first
 * view, x2' F x1 = 0.
 *
 * Rule (csrc/sift_pose.h defines the arithmetic, all of it in double):
 *  - a match participates when the guided matcher's own float test holds for it: Sampson error
 *    under F_p < f_threshold (squared pixels).  The matches of a guided pass under that F all
 *    participate; 1e20 takes every match;
 *  - E = K2' F K1 at unit Frobenius norm is decomposed through the eigenvectors of E'E (cyclic
 *    Jacobi, a fixed order and number of sweeps): E = U diag(s1, s2, .) V' with right-handed U and
 *    V.  No pose when F is zero or not finite, or when s2 is not above 1e-3 s1 (a rank-1 F);
 *  - the candidates, in this order: (U W V', +u3), (U W V', -u3), (U W' V', +u3), (U W' V', -u3),
 *    W = [0 -1 0; 1 0 0; 0 0 1]; every R has determinant +1;
 *  - a participant is triangulated under (R, t) by the midpoint method: rays a = inv(K1) (x1, y1,
 *    1), b = inv(K2) (x2, y2, 1), c = R a, depths l1, l2 from the normal equations of
 *    l1 c - l2 b = -t.  In front: |c x b|^2 > 1e-12, l1 > 0 and l2 > 0.  Its point is
 *    X = (l1 a + R' (l2 b - t)) / 2, in the first camera's frame at |t| = 1.  An in-front match is
 *    wide when the angle between c and b is at least min_angle (radians; cosines are compared);
 *  - the winner is the candidate with the most participants in front, the lowest index among
 *    equal counts.
 *   out_R [npairs][9], out_t [npairs][3]   the winner's R (row-major) and unit t, as float:
 *                                 x_cam2 = R x_cam1 + t
 *   out_counts [npairs][3]        {participants, in front under the winner, wide under the winner}
 *   out_mask [sum counts] or NULL     1 for a participant in front under the winner
 *   out_points [sum counts][3] or NULL   that match's X; zeros for every other match
 * A pair without a pose, without a participant or whose best count is 0 gets zeros for R, t, mask
 * and points, and counts {participants, 0, 0}.  The result is a pure function of the inputs.
 * SGPU_EINVAL, all checked on the host before anything is queued, no output byte written: every
 * argument error of sgpu_estimate_batch for the shared arguments; NULL F, intrinsics, out_R, out_t
 * or out_counts with pairs present; an intrinsic row of a set that some pair names with an entry
 * that is not finite or with fx, fy <= 0; a negative or non-finite f_threshold; min_angle outside
 * [0, pi/2].
 * One table upload (pair records, matches, F and intrinsics in one block), one download, one
 * synchronisation; the number of launches, copies and synchronisations does not depend on npairs.
 * sgpu_last_timing's times[16] is the call's device time; every other slot is left as it was.  A
 * repeated call of the same shape allocates nothing.
 * sgpu_pose_images: over the last extract.  The sets are the batch's images, the locations x, y of
 * its device keys (a multi-part batch: the gathered key buffer); error conditions of
 * sgpu_estimate_images. */
int sgpu_pose_batch(sgpu_ctx* ctx, const float* loc, const int64_t* set_offsets, int nsets,
                    const float* intrinsics /* [nsets][4]: fx, fy, cx, cy */,
                    const int* set_pairs /* [npairs][2] */, int npairs,
                    const int* matches /* [sum counts][2] */, const int* match_counts,
                    const float* F /* [npairs][9] */, float f_threshold, float min_angle /* rad */,
                    float* out_R /* [npairs][9] */, float* out_t /* [npairs][3] */,
                    int* out_counts /* [npairs][3]: participants, front, wide */,
                    uint8_t* out_mask /* [sum counts] or NULL */,
                    float* out_points /* [sum counts][3] or NULL */, int flags);
int sgpu_pose_images(sgpu_ctx* ctx, const float* intrinsics /* [batch][4] */,
                     const int* image_pairs, int npairs, const int* matches,
                     const int* match_counts, const float* F, float f_threshold, float min_angle,
                     float* out_R, float* out_t, int* out_counts, uint8_t* out_mask,
                     float* out_points);

#ifdef __cplusplus
}
#endif
#endif /* SGPU_H */
