/*
 * libfrt - MI355X-native (gfx950) detect -> crop -> embed -> match hot path; thin C ABI.
 *
 * This header is the drop-in boundary.  The reference has no C ABI: its boundary is three C++ classes
 * (RetinaFace / ArcFaceIR50 / MatMul) that sit directly on TensorRT + cuBLASLt + the CUDA runtime.  Every entry point
 * below names the reference member function (file:line under /root/reference) it replaces; the header-only C++ shells
 * in include/frt/{common,retinaface,arcface,matmul}.h rebuild the reference class surfaces on top of these calls.
 *
 * Conventions: plain pointers and sizes only; opaque handles; every function returns an frt_status (0 = ok) and
 * leaves a message retrievable with frt_last_error() (thread-local).  Host pointers unless the name ends in "_dev".
 * Threading (the reference objects are not thread-safe although the Crow server is multithreaded, src/app.cpp:367): every
 * object has a mutex around its entry points and object-level calls are synchronous; a pipeline borrows its three objects, takes
 * their mutexes while it enqueues, and leaves an event behind each stage that later object-level calls on the same object wait
 * for on the device - so object-level calls, frt_pipeline_run from several threads, and pipelined batches in flight may be
 * mixed freely.  Distinct objects may be used concurrently.
 *
 * Axis naming follows the reference: Bbox.x* are ROWS, Bbox.y* are COLUMNS (src/retinaface.cpp:165).
 */
#ifndef FRT_H
#define FRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum frt_status {
    FRT_OK = 0,
    FRT_ERR_INVALID = 1,     /* bad argument / shape                                   (reference: assert)            */
    FRT_ERR_NOT_FOUND = 2,   /* weight blob missing   (reference: throw std::logic_error("Cant find engine file"))   */
    FRT_ERR_FORMAT = 3,      /* weight blob malformed / wrong network kind                                           */
    FRT_ERR_DEVICE = 4,      /* HIP runtime failure   (reference: checkCudaStatus -> std::logic_error, common.cpp:43) */
    FRT_ERR_EMPTY = 5,       /* no faces / empty gallery (reference: throw const char*, src/arcface.cpp:198)          */
    FRT_ERR_EMPTY_ROI = 6,   /* zero-area crop rectangle (reference: cv::Exception from Mat::operator())             */
    FRT_ERR_CAPACITY = 7     /* more frames / faces than the object was created for                                  */
} frt_status;

/* Layout-identical to the reference's `struct Bbox` (src/common.h:13-16): 4 x int32 + float32 = 20 bytes. */
typedef struct frt_bbox {
    int32_t x1, y1, x2, y2; /* x = row, y = column */
    float score;
} frt_bbox;

typedef struct frt_detector frt_detector;
typedef struct frt_embedder frt_embedder;
typedef struct frt_matcher frt_matcher;
typedef struct frt_pipeline frt_pipeline;

const char *frt_last_error(void);
const char *frt_version(void);
/* Number of visible HIP devices (0 when none). */
int frt_device_count(void);
/* How long a blocking entry point (findFace, forward, frt_pipeline_wait ...) busy-polls for the device before it backs off: the wait spins
 * for `microseconds` (default 200, or FRT_WAIT_SPIN_US), then polls once per ~50 us sleep (the thread is off its core in between), then
 * parks in the interrupt wait.  Process-wide.  A server with many request threads keeps the default; a throughput driver that owns its
 * core may raise it (bench.py uses 50 000 and reports it).  Returns the previous value. */
long frt_set_wait_spin_us(long microseconds);
/* Measurement aid (no counterpart in the reference): what this device SUSTAINS on the recogniser's matrix-core instruction mix, in TFLOP/s.
 * Runs back-to-back v_mfma_f32_32x32x16_f16 on random fp16 operands on every SIMD for about `seconds` (0 < seconds <= 10) -
 * mix 0: MFMAs only; 1: + one ds_read_b128 per MFMA; 2: + the global loads of the dominant conv kernel's K loop as well - and returns
 * flop / elapsed.  The part is power-managed (1.4 kW), so this is well below the nominal 2.5 PFLOP/s; bench.py quotes the dominant
 * kernel against both (roofline.sustained_peak). */
int frt_probe_sustained_mfma(int device, int mix, double seconds, double *tflops_out);

/* ------------------------------------------------------------------------------------------------------------------
 * Detector  ==  class RetinaFace (src/retinaface.h:18-23)
 * ------------------------------------------------------------------------------------------------------------------ */

/* RetinaFace::RetinaFace (src/retinaface.cpp:3-29) + loadEngine (:31-55) + preInference (:81-104).
 * weights_path: FRTW blob instead of a TensorRT engine: kind 1 (RetinaFace mobilenet0.25), 4 (Slim) or 5 (RFB) - the three
 * networks of conversion/retina/torch2trt.py.  Each decodes with its own training anchors (cfg_mnet: 3 levels; cfg_slim / cfg_rfb: 4 levels,
 * steps 8/16/32/64, sizes {10,16,24} {32,48} {64,96} {128,192,256}).  in_c must be 3.  max_batch = frames per call. */
int frt_detector_create(const char *weights_path, int frame_w, int frame_h, int in_c, int in_h, int in_w, int max_batch,
                        int max_faces, float nms_threshold, float bbox_threshold, int device, frt_detector **out);
/* The network a detector blob holds, validated as frt_detector_create does, without a device: family = blob kind (1 mnet0.25, 4 Slim,
 * 5 RFB), levels = anchor pyramid levels (3 or 4), has_landmarks = 1 when the blob carries the landmark heads.  A missing, misshapen or
 * unexpected tensor of a Slim / RFB blob -> FRT_ERR_FORMAT naming it (frt_last_error).  Any out pointer may be NULL. */
int frt_detector_describe(const char *weights_path, int *family, int *levels, int *has_landmarks);
/* RetinaFace::~RetinaFace (src/retinaface.cpp:273-280) */
void frt_detector_destroy(frt_detector *d);
/* m_OUTPUT_SIZE_BASE (src/retinaface.cpp:13): anchors per frame */
int frt_detector_num_anchors(const frt_detector *d);
/* What the detector was created for (any out pointer may be NULL). */
int frt_detector_geometry(const frt_detector *d, int *frame_w, int *frame_h, int *max_batch, int *max_faces, int *device);

/* RetinaFace::findFace (src/retinaface.cpp:147-152).  bgr: u8 HWC frame of exactly frame_h x frame_w, row_stride bytes
 * per row.  out: capacity max_faces.  n_out: number of boxes written (score-descending, after NMS and cap). */
int frt_detector_find_faces(frt_detector *d, const uint8_t *bgr, int rows, int cols, size_t row_stride, frt_bbox *out, int *n_out);
/* New surface: n_frames <= max_batch contiguous frames; out[n_frames * max_faces], n_out[n_frames]. */
int frt_detector_find_faces_batch(frt_detector *d, const uint8_t *bgr, int n_frames, int rows, int cols, size_t row_stride,
                                  size_t frame_stride, frt_bbox *out, int *n_out);

/* RetinaFace::preprocess (src/retinaface.cpp:106-136): frame -> float32 planar [3][in_h][in_w] on the host. */
int frt_detector_preprocess(frt_detector *d, const uint8_t *bgr, int rows, int cols, size_t row_stride, float *chw_out);
/* RetinaFace::doInference (src/retinaface.cpp:138-145): bindings input_det -> output_det0 [batch][A][4],
 * output_det1 [batch][A][2] (softmaxed), conversion/retina/torch2trt.py:95-96. */
int frt_detector_infer(frt_detector *d, const float *chw, int batch, float *loc_out, float *conf_out);
/* RetinaFace::postprocessing (src/retinaface.cpp:154-208) for one frame of raw head outputs. */
int frt_detector_postprocess(frt_detector *d, const float *loc, const float *conf, frt_bbox *out, int *n_out);

/* ------------------------------------------------------------------------------------------------------------------
 * Crop  ==  free function getCroppedFaces (src/arcface.h:17, src/arcface.cpp:3-17)
 * ------------------------------------------------------------------------------------------------------------------ */
/* crops_out: u8 BGR [n][out_h][out_w][3].  device < 0 -> current device.  Returns FRT_ERR_EMPTY_ROI if any box has
 * a zero-area or out-of-frame rectangle (nothing is written for that face; the others are still produced). */
int frt_crop_faces(const uint8_t *bgr, int rows, int cols, size_t row_stride, const frt_bbox *boxes, int n, int out_w, int out_h,
                   uint8_t *crops_out, int device);

/* ------------------------------------------------------------------------------------------------------------------
 * Embedder  ==  class ArcFaceIR50 minus the gallery (src/arcface.h:19-39)
 * ------------------------------------------------------------------------------------------------------------------ */

/* ArcFaceIR50::ArcFaceIR50 (src/arcface.cpp:21-43) + loadEngine (:45-69) + preInference (:88-103).
 * weights_path: FRTW blob kind 2 (IR family: IR-50, the reference's network, IR-100, IR-152) or kind 3 (IR-SE family: IR-SE-50 /
 * 100 / 152); the depth is read from the blob's tensors (frt_embedder_describe).  in_c,in_h,in_w must be 3,112,112 and out_dim 512.
 * max_batch = faces per device launch (the reference default is 1, app/config.json:18). */
int frt_embedder_create(const char *weights_path, int in_c, int in_h, int in_w, int out_dim, int max_batch, int device,
                        frt_embedder **out);
/* The backbone a recogniser blob holds, with the validation frt_embedder_create runs and no HIP call (works without a device).
 * num_layers <- 50 / 100 / 152, se <- 1 for IR-SE, units_per_stage[4] <- {3,4,14,3} / {3,13,30,3} / {3,8,36,3} (model_irse.py
 * get_blocks); any output pointer may be NULL.  A blob with a missing or mis-sized tensor, a body.* tensor no unit owns, SE units mixed
 * with plain ones or another stage table gives FRT_ERR_FORMAT, and frt_last_error() names the tensor. */
int frt_embedder_describe(const char *weights_path, int *num_layers, int *se, int *units_per_stage);
void frt_embedder_destroy(frt_embedder *e);

/* IR-SE-50 only (no reference counterpart; the reference's engine is a black box): 1 (default, env FRT_SE_FUSED=0 turns it off) runs the
 * squeeze-and-excitation tail of a unit inside conv2's epilogue, where the workgroups of one face hand their partial channel sums
 * over through device-scope stores and a flag; 0 always uses the stand-alone pool + gate + apply launches (no cross-workgroup wait
 * anywhere).  Same arithmetic; the pooled sums are added in a different fixed order, so results agree to fp16 rounding of the gated activations (cosine >= 1 - 1e-5),
 * each mode bit-reproducible in itself.  A timed-out hand-over never kills the HIP context: the next synchronising call on the
 * embedder / pipeline returns FRT_ERR_DEVICE and this switch is the way back.  Takes effect for passes enqueued after the call; a
 * pipeline with hipGraph replay on must be told to re-capture (frt_pipeline_set_graph). */
int frt_embedder_set_se_fused(frt_embedder *e, int enable);
/* Arithmetic of the recogniser network for the passes enqueued after the call.  fp32 = 0 (default): fp16 activations and weights on the fp16
 * matrix cores with fp32 accumulation - what the reference's TensorRT engine is built with (conversion/arcface/torch2trt.py:42-43) and what
 * every throughput figure of this build is measured on (embeddings cosine-equal to the fp32 network within ~ 3e-6).  fp32 = 1: fp32
 * activations, fp32 weights, every product an exact fp32 fma (v_mfma_f32_32x32x2_f32 / v_fma_f32) - BASELINE configs[1]'s "fp32"; a simple,
 * separate path meant for a few faces per call (about 10x the time per face; 1 - cosine <= 1e-6 against the fp32 oracle).  The first call with
 * fp32 = 1 re-reads the weight blob the object was created from and uploads fp32 copies (175 MB).  Pipelines with hipGraph replay on must be
 * told to re-capture (frt_pipeline_set_graph). */
int frt_embedder_set_precision(frt_embedder *e, int fp32);
/* Flip-augmented embeddings (test-time flip augmentation, the way ArcFace models are evaluated; no reference counterpart).  enable = 0
 * (default): normalize(pre(x)), pre = the 512 values in front of the L2 normalisation.  enable = 1: normalize(pre(x) + pre(mirror x)), mirror
 * = the crop with its left and right sides swapped, on every path that goes through this embedder (frt_embedder_infer / _forward /
 * _forward_aligned / _embed_faces / _enrol_faces, the pipeline, the coalescer, the photo routes, either precision).  Gallery and probes must be
 * embedded in the same mode: a flip embedding is a different vector (cosine ~ 0.7 to the plain one on the synthetic weights), so switching
 * means re-enrolling.  About twice the recogniser time per face.  The call waits for the embedder's passes in flight, allocates the mode's
 * scratch once and holds for passes enqueued after it; a pipeline keys its captured graphs by the mode.  get: enabled_out <- 0 / 1. */
int frt_embedder_set_flip(frt_embedder *e, int enable);
int frt_embedder_get_flip(const frt_embedder *e, int *enabled_out);

/* ArcFaceIR50::preprocessFace (src/arcface.cpp:105-114): u8 BGR [in_h][in_w][3] -> float32 planar RGB. */
int frt_embedder_preprocess_face(frt_embedder *e, const uint8_t *bgr_crop, float *chw_out);
/* ArcFaceIR50::doInference, both overloads (src/arcface.cpp:131-148): float32 [batch][3][112][112] -> [batch][512]
 * L2-normalised.  batch may exceed max_batch (processed in chunks). */
int frt_embedder_infer(frt_embedder *e, const float *chw, int batch, float *embeds_out);
/* ArcFaceIR50::forward (src/arcface.cpp:166-187) with the evident intent of the batched branch:
 * getCroppedFaces + preprocessFaces + inference.  embeds_out [n][512]; crops_out (may be NULL) u8 BGR [n][112][112][3]
 * (= CroppedFace.face, src/app.cpp:329). */
int frt_embedder_forward(frt_embedder *e, const uint8_t *bgr, int rows, int cols, size_t row_stride, const frt_bbox *boxes, int n,
                         float *embeds_out, uint8_t *crops_out);

/* ------------------------------------------------------------------------------------------------------------------
 * Matcher  ==  class MatMul (src/matmul.h:6-21) + ArcFaceIR50::getOutputs argmax (src/arcface.cpp:203-217)
 * ------------------------------------------------------------------------------------------------------------------ */

/* MatMul::MatMul (src/matmul.cpp:3-7) */
int frt_matcher_create(int device, frt_matcher **out);
/* MatMul::~MatMul (src/matmul.cpp:79-91) */
void frt_matcher_destroy(frt_matcher *m);
/* MatMul::init (src/matmul.cpp:9-34): gallery A[num_row][num_col] row-major fp32, copied to the device.  Idempotent:
 * a second call frees the previous device copy (the reference leaks it on every /reload). */
int frt_matcher_init(frt_matcher *m, const float *gallery, int num_row, int num_col);
/* Storage precision of the gallery rows for the NEXT frt_matcher_init / frt_matcher_gallery_begin: 0 = fp32 rows (default; the
 * reference's MatMul), 1 = rows stored as fp16 on the device (BASELINE config 5, "fp16 embeddings": half the HBM bytes per scan
 * and per GPU).  With fp16 storage the similarities are DEFINED as the fp32 dot products with the fp16-rounded rows
 * (sum_k e[k] * float(half(g[k])), fp32 fmaf chain) - calculate / top1 / the pipeline all agree on them bit for bit. */
int frt_matcher_set_storage(frt_matcher *m, int fp16);
/* Screened top-1 on / off (default on).  Galleries of >= 32 768 rows answer top-1 calls with a coarse scan of a compact shadow copy
 * (int8 rows with a per-row scale for 512-column fp32 galleries, fp16 otherwise) followed by an EXACT fp32 re-rank of every row the
 * rigorous error bound cannot exclude - the result is bit-identical to the exact scan, its cost depends on the queries (a query that
 * matches keeps one candidate block, one that matches nothing a dozen).  on = 0 makes every call take the exact fp32 scan of the
 * whole gallery (MatMul::calculate's arithmetic, src/matmul.h:7-16, with the first-maximum epilogue of src/arcface.cpp:203-217 fused):
 * 4 * num_col * num_row bytes per call whatever the queries - the path's worst case, reported by bench.py as `match_worst_case`. */
int frt_matcher_set_screening(frt_matcher *m, int on);
/* A counter that changes whenever the gallery this matcher answers from changes (init / commit / row offset; also when its scratch buffers
 * move).  A caller that keeps (row index, similarity) pairs across calls compares it to know whether the indices still name the same rows
 * (include/frt/arcface.h: the coalesced fast path of featureMatching / getOutputs). */
unsigned frt_matcher_generation(frt_matcher *m);
/* Bytes of gallery data ONE top-1 call reads in the current mode (the coarse scan's shadow copy when screening is on and the gallery is
 * large enough for it, the stored rows otherwise; the exact re-rank's candidate rows come on top and depend on the queries). */
size_t frt_matcher_scan_bytes(frt_matcher *m);
/* Streaming gallery load == the loop of Database::getEmbeddings (src/db.cpp:316-346):
 *   initKnownEmbeds(n)            -> frt_matcher_gallery_begin(m, n, 512)
 *   addEmbedding(id, blob) x n    -> frt_matcher_gallery_append(m, blob, 1)     (blob = sqlite3_column_blob: raw little-endian
 *                                    float32[num_col]; any number of consecutive rows per call; copied before the call returns)
 *   initMatMul()                  -> frt_matcher_gallery_commit(m)
 * Rows are staged in pinned host chunks and uploaded asynchronously while the caller fetches the next ones; the previous gallery
 * stays searchable until commit swaps it (and frees it: the reference leaks both copies on every /reload).  commit with fewer
 * rows than reserved is fine (the count actually appended becomes num_row); appending more is FRT_ERR_CAPACITY. */
int frt_matcher_gallery_begin(frt_matcher *m, int row_capacity, int num_col);
int frt_matcher_gallery_append(frt_matcher *m, const void *rows, int n_rows);
int frt_matcher_gallery_commit(frt_matcher *m);
int frt_matcher_num_rows(const frt_matcher *m);
/* Live gallery edits: add rows to, and remove rows from, the gallery the matcher is answering from - the reference's /insert/face and
 * /delete/user (src/app.cpp:131-229) without the /reload (src/app.cpp:354-365) that re-reads every row.  The rows already there stay on the
 * device, the screening data is updated only where it changed.  After any sequence of edits the matcher answers EXACTLY as a fresh matcher
 * would that was frt_matcher_init'ed with the resulting row list in the same storage mode (indices, similarities, the first-maximum tie
 * rule; top1 / topk / calculate / the _dev forms / the pipeline's match stage; screening on or off).
 *   - An edit returns when its device work is complete; a call submitted after it returns is answered from the new gallery, a call in
 *     flight wholly from the old or wholly from the new one.  frt_matcher_generation changes on every edit that changes the gallery.
 *   - Limits: a matcher with a row offset (a shard, frt_matcher_set_row_offset != 0) is not edited - FRT_ERR_INVALID; reload the shard.  An
 *     edit while a streamed load is open (gallery_begin without commit) acts on the live gallery; the commit then replaces it, as always.
 *     Galleries screen from 32 768 rows on: the add that takes the gallery across builds the whole shadow (once), a remove that takes it
 *     below stops screening (the allocation is kept for the way back) - frt_matcher_scan_bytes describes either state.
 * gallery_reserve: room for edits up to row_capacity rows - the stored rows, the shadow, the per-row scales and the per-call scratch sized
 *   by tiles or blocks; an add inside it allocates nothing.  Never shrinks; contents and answers are unchanged.  On a matcher without rows it
 *   is the floor of the next allocation (init / gallery_begin / the first add).
 * gallery_add / gallery_add_dev: append n_rows rows [n_rows][num_col] fp32 from host memory / from device memory (the embedder's output:
 *   an enrolment never crosses PCIe twice; the rows must be complete when the call is made).  They get the indices N .. N + n_rows - 1,
 *   existing indices do not move.  Short of capacity the gallery is moved into an allocation 1.5 x as large (at least what is needed):
 *   allocate + device copy + free, which transiently needs BOTH copies.  num_col is that of the last init / gallery_begin (an empty
 *   gallery: gallery_begin(m, cap, num_col) + gallery_commit with zero rows).
 * gallery_remove: row indices in any order, duplicates count once; an index outside [0, N) is FRT_ERR_INVALID with nothing changed.
 *   Order-preserving, like the reference after a delete + /reload (SELECT order, src/db.cpp:316-346): the surviving rows keep their order
 *   and close up, a row behind r removed rows moves down by r.  Removing every row leaves an empty gallery (match calls: FRT_ERR_EMPTY).
 * edit_stats: cumulative { rows_uploaded (rows taken in by add), rows_moved (rows a remove moved down), shadow_rows_rebuilt (rows converted
 *   into the int8 / fp16 shadow by edits), reallocations (moves of a non-empty gallery into a larger allocation) }. */
int frt_matcher_gallery_reserve(frt_matcher *m, int row_capacity);
int frt_matcher_gallery_add(frt_matcher *m, const float *rows, int n_rows);
int frt_matcher_gallery_add_dev(frt_matcher *m, const void *rows_dev, int n_rows);
int frt_matcher_gallery_remove(frt_matcher *m, const int32_t *idx, int n_idx);
int frt_matcher_edit_stats(frt_matcher *m, long out[4]);
/* MatMul::calculate (src/matmul.cpp:36-77): outputs[i*num_row + j] = sum_k embeds[i][k] * gallery[j][k], fp32. */
int frt_matcher_calculate(frt_matcher *m, const float *embeds, int embed_count, float *outputs);
/* calculate and the first-maximum argmax of every row in ONE call: outputs (may be NULL: no matrix is materialised) as
 * frt_matcher_calculate, idx_out / sim_out as frt_matcher_top1 - the same accumulators, so idx_out[i] / sim_out[i] ARE std::max_element
 * over outputs row i, bit for bit.  The drop-in ArcFaceIR50 shell uses it so that featureMatching() + getOutputs() (src/arcface.cpp:189-217)
 * keep their signatures while the host-side O(F*N) scan disappears; with a pinned `outputs` (frt_pinned_alloc) the [F x N] copy is one DMA. */
int frt_matcher_calculate_top1(frt_matcher *m, const float *embeds, int embed_count, float *outputs, int32_t *idx_out, float *sim_out);
/* Page-locked host memory for buffers that cross PCIe on every call (the [F x N] matrix MatMul::calculate hands back is 4 MB per face at
 * N = 1M: pageable memory makes that copy a staged, synchronous one).  device: the device whose context registers it. */
int frt_pinned_alloc(size_t bytes, int device, void **out);
void frt_pinned_free(void *p);
/* Fused calculate + getOutputs argmax: idx_out[i] = FIRST j maximising the similarity (std::max_element semantics),
 * sim_out[i] = that similarity.  Never materialises the [n x num_row] matrix. */
int frt_matcher_top1(frt_matcher *m, const float *embeds, int embed_count, int32_t *idx_out, float *sim_out);
/* frt_matcher_top1 with everything resident in HBM, asynchronous on hip_stream (a hipStream_t as void*, NULL = default stream):
 * queries [n][num_col] fp32, idx_dev int32 [n], sim_dev fp32 [n].  The sharded-gallery path (dist.py) feeds it the RCCL
 * all-gathered embeddings without a host round trip. */
int frt_matcher_top1_dev(frt_matcher *m, const void *embeds_dev, int embed_count, void *idx_dev, void *sim_dev, void *hip_stream);
/* Sharded galleries: declare that local row 0 of this matcher is global row `row_offset`; top-1
 * indices (frt_matcher_top1, the pipeline's match_idx) are then global.  The full matrix of calculate() stays local. */
int frt_matcher_set_row_offset(frt_matcher *m, int row_offset);
/* Sharded-gallery variant: rows of this matcher are global rows [row_offset, row_offset+num_row).
 * Merges with an existing (idx, sim) pair per query, keeping the higher similarity and the LOWER global index on ties. */
int frt_merge_top1(int n, const int32_t *idx_a, const float *sim_a, const int32_t *idx_b, const float *sim_b, int32_t *idx_out,
                   float *sim_out);

/* Exact top-k (BASELINE configs[4]: "fp16 embeddings, RCCL top-k all-gather"; the reference itself only ever takes the first maximum,
 * src/arcface.cpp:203-217, which is k = 1).  idx_out / sim_out are [embed_count][k]: entry j of a query is the j-th row of its exact
 * ranking - higher similarity first, LOWER (global) index first among equal similarities, i.e. entry 0 is frt_matcher_top1's answer bit
 * for bit and entry j is "std::max_element over the rows not yet taken".  Fewer than k rows: idx -1, sim -inf in the unused slots.
 * 1 <= k <= 16. */
int frt_matcher_topk(frt_matcher *m, const float *embeds, int embed_count, int k, int32_t *idx_out, float *sim_out);
/* Device-resident form, asynchronous on hip_stream.  embeds_fp16 = 0: queries fp32 [n][num_col]; 1: queries IEEE fp16 [n][num_col] - what
 * the embedding exchange of configs[4] delivers (frt_embeds_to_half_dev + all-gather); they are widened exactly, so the similarities are
 * the fp32 dot products of the fp16-rounded embeddings with the stored rows. */
int frt_matcher_topk_dev(frt_matcher *m, const void *embeds_dev, int embeds_fp16, int embed_count, int k, void *idx_dev, void *sim_dev, void *hip_stream);
/* k-way merge of per-shard top-k lists with GLOBAL indices (frt_matcher_set_row_offset), idx_all / sim_all [shards][n][k] -> [n][k]:
 * same order rule as above (the lower global index wins a tie - the first-maximum rule carried across shards); idx < 0 = empty slot. */
int frt_merge_topk(int shards, int n, int k, const int32_t *idx_all, const float *sim_all, int32_t *idx_out, float *sim_out);
int frt_merge_topk_dev(int shards, int n, int k, const void *idx_all_dev, const void *sim_all_dev, void *idx_out_dev, void *sim_out_dev, void *hip_stream);
/* fp32 -> IEEE fp16 (round to nearest even) of n_values (a multiple of 8) device floats: the embeddings before they are exchanged. */
int frt_embeds_to_half_dev(const void *embeds_dev, size_t n_values, void *half_out_dev, void *hip_stream);

/* Top-k over IDENTITIES.  The reference's gallery holds several rows per person (USER 1-N FACE; addEmbedding(userId, blob) once per face), so
 * the k best ROWS can be one person k times.  A labelled gallery has one int32 label >= 0 per row, and the ranked search then ranks labels:
 *   similarities - those frt_matcher_calculate returns, the same accumulators bit for bit (fp16 storage: the fp16-row similarities above);
 *   row order    - higher similarity first, lower global index first among equals (the order of frt_matcher_topk);
 *   ranking      - walk the rows in that order, keep a row if no kept row has its label; the first k kept rows are the answer.  Entry j
 *                  reports (label, global row index, similarity) of the best row of the j-th best identity.
 * So entry 0 is frt_matcher_top1's answer bit for bit, all labels distinct gives frt_matcher_topk's lists, and with fewer than k identities
 * the unused slots hold label -1, idx -1, sim -inf.  1 <= k <= 16.  A matcher that never gets labels behaves exactly as before.
 * set_labels: labels[n], n == frt_matcher_num_rows; they are copied to the device and move with later edits.  labels == NULL, n == 0 clears
 *   them.  A negative label or a wrong n: FRT_ERR_INVALID, nothing changed.  frt_matcher_init and frt_matcher_gallery_commit REPLACE the
 *   gallery and therefore drop the labels: set them again after a reload.  frt_matcher_generation changes whenever the labels change.
 * labels_info: the number of distinct labels and an upper bound M of the rows any one label has (exact after set_labels and adds; a remove
 *   leaves it alone, so it may over-state but never under-states).  0, 0 for an unlabelled gallery.
 * gallery_add_labeled / _dev: frt_matcher_gallery_add / _add_dev with one label per new row (labels in HOST memory in both forms).  A
 *   gallery with rows takes only the form that matches it - the plain add on a labelled gallery and the labelled add on an unlabelled one
 *   are FRT_ERR_INVALID - an empty one takes either and becomes labelled or unlabelled by it.  frt_matcher_gallery_remove closes the labels
 *   up with the rows, frt_matcher_gallery_reserve makes room for them too.  After any edit sequence the identity answers equal those of a
 *   fresh matcher initialised with the resulting rows and labels.
 * topk_labels / _dev: label_out, idx_out, sim_out are [embed_count][k]; row offset, fp16 queries and stream semantics as frt_matcher_topk /
 *   _dev.  An unlabelled gallery: FRT_ERR_INVALID; an empty one: FRT_ERR_EMPTY.
 *   Cost: k exact scans of the stored rows per call (pass j is the top-1 search without the rows of the j labels already reported).  A
 *   screened gallery (>= 32 768 rows, screening on) with (k - 1) * M + 1 <= 16 instead runs ONE coarse scan and k short re-rank passes: with
 *   at most M rows per label the best (k - 1) * M + 1 rows hold k identities, which bounds the selection.  Same bits either way;
 *   frt_matcher_set_screening(m, 0) forces the exact passes. */
int frt_matcher_set_labels(frt_matcher *m, const int32_t *labels, int n);
int frt_matcher_labels_info(frt_matcher *m, int *n_identities, int *max_rows_per_label);
int frt_matcher_gallery_add_labeled(frt_matcher *m, const float *rows, const int32_t *labels, int n_rows);
int frt_matcher_gallery_add_labeled_dev(frt_matcher *m, const void *rows_dev, const int32_t *labels /* host */, int n_rows);
int frt_matcher_topk_labels(frt_matcher *m, const float *embeds, int embed_count, int k, int32_t *label_out, int32_t *idx_out, float *sim_out);
int frt_matcher_topk_labels_dev(frt_matcher *m, const void *embeds_dev, int embeds_fp16, int embed_count, int k, void *label_dev, void *idx_dev, void *sim_dev,
                                void *hip_stream);
/* frt_merge_topk for identity lists: label_all / idx_all / sim_all [shards][n][k] with global indices -> [n][k] by the ranking above.  An
 * identity that appears in several shards (one user's photos may sit on different shards) counts once, with its best row: higher
 * similarity, lower global index on a tie.  idx < 0 = empty slot.  Exact: an identity of the global top-k is in the top-k of distinct
 * identities of the shard that holds its best row, because every identity ahead of it there is ahead of it globally.  The host form needs
 * no device. */
int frt_merge_topk_labels(int shards, int n, int k, const int32_t *label_all, const int32_t *idx_all, const float *sim_all, int32_t *label_out,
                          int32_t *idx_out, float *sim_out);
int frt_merge_topk_labels_dev(int shards, int n, int k, const void *label_all_dev, const void *idx_all_dev, const void *sim_all_dev, void *label_out_dev,
                              void *idx_out_dev, void *sim_out_dev, void *hip_stream);

/* Template gallery: ONE row per identity.  From a labelled matcher `src` (N rows g_r as STORED - fp16 storage: the fp16 rows widened to
 * fp32 - labels l_r, width D) build, in one streaming pass of the device over the rows, for every identity i = 0 .. I - 1 (numbered in
 * first-appearance order, by the lowest row that carries the label; I = n_identities of frt_matcher_labels_info), rows r_1 < ... < r_M:
 *   s          = ((g_r1 + g_r2) + ...) + g_rM   per column, fp32, in ascending row order;
 *   template   t_i = s / ||s||_2                (fp32; all zeros when ||s||^2 == 0, e.g. g and -g under one label);
 *   n_rows[i]  = M,   labels[i] = the identity's label;
 *   min_sim[i] = min_j <g_rj, t_i>  (fp32 accumulation; 0 for a zero template) and min_row[i] = the GLOBAL row (row offset added) that
 *                attains it, the lowest among equals: the member that agrees least with its own identity - the mislabelled or poor photo.
 * Every output pointer may be NULL; labels_out / n_rows_out / min_sim_out / min_row_out are [I], templates_out is [I][D] (host memory).
 * dst (may be NULL: an audit only) afterwards holds exactly the I templates as a labelled gallery with labels[i], in its OWN storage mode
 * (frt_matcher_set_storage) and screening state: it is emptied and the templates enter it device to device by the route of
 * frt_matcher_gallery_add_labeled_dev, so its answers are those of a fresh matcher loaded with templates_out + labels_out.  dst is an
 * ordinary labelled matcher: frt_pipeline_create, the coalescer, top1, topk and topk_labels take it, and the row they answer with is a
 * person.  dst's mutex is held across the whole replacement (no caller sees it empty or half filled); the two mutexes are taken in address
 * order; match stages in flight on either matcher are waited for; src is only read and its generation does not change.
 * FRT_ERR_INVALID: src NULL, src without labels (and with rows), src == dst, matchers on different devices, dst with a row offset.  A src
 * with zero rows is no error: dst becomes an empty gallery of src's width.
 * Sharded galleries: a shard builds the templates of ITS rows only; an identity whose rows straddle shards gets one partial template per
 * shard, which is out of scope here - keep an identity's rows on one shard, or build from an unsharded matcher. */
int frt_matcher_build_templates(frt_matcher *src, frt_matcher *dst, int32_t *labels_out, int32_t *n_rows_out, float *min_sim_out, int32_t *min_row_out,
                                float *templates_out);

/* Group an UNLABELLED gallery into identities: single-linkage clustering at a similarity threshold, on the device.  Rows i < j are joined
 * iff S(i, j) >= threshold, S being the matcher's own exact fp32 similarity - the value frt_matcher_calculate returns for query = stored
 * row i against row j (fp16 storage: the stored fp16 rows widened to fp32).  The comparison is >= (the caller of knownPersonThreshold
 * treats sim < thr as unknown); a NaN similarity joins nothing; a row is never joined to itself.  The result is the connected components
 * of that graph:
 *   labels[i] = the smallest row index of i's component (>= 0, the same whatever order the device worked in; usable as they are by
 *               frt_matcher_set_labels);
 *   stats[0]  = number of components, stats[1] = number of joined pairs (i < j), stats[2] / stats[3] = 128-row query chunks that went
 *               through the screened path (shadow gallery, exact re-rank of the candidate blocks) / through the exact dense path
 *               (galleries without a screen, frt_matcher_set_screening(0), chunks whose candidate list overflowed).  Both paths decide on
 *               the same similarity bits, so the result does not depend on the path.
 * labels_out [N] (host) and stats_out may be NULL.  install_labels != 0: the result becomes the matcher's labels exactly as
 * frt_matcher_set_labels with the same array would make it (labels_info, topk_labels and build_templates work at once; the generation
 * moves as set_labels moves it).  Without it the gallery, its labels and its generation stay as they are.
 * frt_matcher_cluster_dev: labels_dev [N] int32 and stats_dev (4 x int64, may be NULL) are device memory, complete when hip_stream has
 * run; the call itself waits once for the device in the middle (the overflow flags of the chunks).
 * A gallery that holds a non-finite row (NaN, Inf) has no error bound for its shadow: every chunk's candidate list then overflows and the
 * whole call pays the screened front AND the dense pass for nearly every chunk (the result stays exact; the row itself joins nothing
 * unless a similarity of +Inf comes out).  Remove such rows first if the time matters.
 * The calls hold the matcher's mutex, wait for a match stage in flight and re-run from scratch after every edit (no incremental form).
 * An empty gallery: FRT_OK with zero clusters.  FRT_ERR_INVALID: a threshold that is not finite; a matcher with a row offset (a shard
 * cannot know its neighbours' rows: clustering across shards is out of scope). */
int frt_matcher_cluster(frt_matcher *m, float threshold, int32_t *labels_out /* [N] host, may be NULL */, int install_labels,
                        long long stats_out[4] /* clusters, edges, screened chunks, dense chunks; may be NULL */);
int frt_matcher_cluster_dev(frt_matcher *m, float threshold, void *labels_dev /* [N] int32 */, void *stats_dev /* 4 x int64, may be NULL */,
                            void *hip_stream);

/* Leave-one-out genuine / impostor scores of a LABELLED gallery: how well do the labels separate, and at which threshold.  m has N rows
 * with labels l and no row offset; S(i, j) is the exact fp32 similarity of frt_matcher_cluster above (query = stored row i against row j).
 * For every row i:
 *   genuine   candidates = the rows j != i with l[j] == l[i]   -> gen_sim[i], gen_row[i]
 *   impostor  candidates = the rows j with l[j] != l[i]        -> imp_sim[i], imp_row[i]
 * A j whose S(i, j) is NaN is no candidate; the winner is the candidate with the largest S, the lowest row among equal values (the order
 * of frt_matcher_top1); without a candidate - a person with one photo, a gallery with one identity, a NaN row - the outputs are -inf and
 * -1, the empty slot of frt_matcher_topk_labels.
 *   stats[0] = rows with a genuine candidate, stats[1] = rows with an impostor candidate,
 *   stats[2] = rows with both and imp_sim >= gen_sim: the photos that are closer to another person than to their own,
 *   stats[3] / stats[4] = 128-row query chunks whose impostor search went through the screen / through the exact scan (galleries without a
 *              screen, frt_matcher_set_screening(0), more than 15 rows under one label, chunks whose candidate list overflowed).  Both paths
 *              return the exact scan's bits: the result does not depend on the path.
 * The optional sweep over n_thresholds <= 64 finite thresholds (host memory in both forms, read before the call returns):
 *   counts[k][0] = rows with a genuine candidate and gen_sim < thresholds[k]   (the caller's `sim < knownPersonThreshold`: "unknown"),
 *   counts[k][1] = rows with an impostor candidate and imp_sim >= thresholds[k] (accepted as someone else if their own person were absent).
 * Every output pointer may be NULL.  frt_matcher_separation_dev: the arrays [N], counts [n_thresholds][2] int64 and stats 5 x int64 are
 * device memory, complete when hip_stream has run; the call waits once for that stream at its start (the upload of the identity -> rows
 * grouping).
 * This is the calibration of frt_matcher_cluster's threshold.  With t* = max_i imp_sim[i]:
 *   - frt_matcher_cluster at any t > t* puts no two labels into one component (no pair of rows with different labels has S >= t);
 *   - at t = t* it merges the two identities of the arg-max pair (i, imp_row[i]);
 *   - for t > t*, row i is a singleton component exactly when gen_sim[i] < t (it can only be joined to rows of its own label, and the best
 *     of them decides).
 * The calls hold the matcher's mutex, wait for a match stage in flight and only read the gallery: rows, labels and generation stay as they
 * are (the query scratch is allocated on first use, which moves the generation as the first search of a matcher does).  There is no
 * incremental form: after an edit the call runs from scratch.  Cost: N / 128 screened searches, or N / 128 exact scans.
 * An empty gallery: FRT_OK with zero stats and counts.  FRT_ERR_INVALID: m NULL; rows without labels; a matcher with a row offset (a shard
 * does not know its neighbours' rows: sharded galleries are out of scope); n_thresholds outside 0..64; a threshold that is not finite. */
int frt_matcher_separation(frt_matcher *m, float *gen_sim_out, int32_t *gen_row_out, float *imp_sim_out, int32_t *imp_row_out, const float *thresholds,
                           int n_thresholds, long long *counts_out /* [n_thresholds][2] */, long long stats_out[5]);
int frt_matcher_separation_dev(frt_matcher *m, void *gen_sim_dev, void *gen_row_dev, void *imp_sim_dev, void *imp_row_dev,
                               const float *thresholds /* host */, int n_thresholds, void *counts_dev, void *stats_dev, void *hip_stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Multi-GPU exchange.  The reference is one single-GPU C++ process (src/app.cpp:52-57, 367); north_star shards whole
 * frames over the GPUs of a node with an RCCL all-gather as the only exchange step.  These calls are that step for a C++ host: RCCL
 * (bound at run time from librccl.so.1) behind plain pointers.  One communicator per device - one process per GPU (get_unique_id on
 * rank 0, hand the 128 bytes to the other ranks by any means, frt_comm_create everywhere), or one process driving several devices
 * (frt_comm_create_all + one thread per device, or frt_comm_all_gather_multi from one thread).  Create communicators AFTER the
 * pipelines of the device (they own a stream; see frt_pipeline_check_overlap).
 * ------------------------------------------------------------------------------------------------------------------ */
#define FRT_COMM_ID_BYTES 128
typedef struct frt_comm frt_comm;
int frt_comm_get_unique_id(uint8_t *id_out /* [FRT_COMM_ID_BYTES] */);
/* RCCL's bootstrap calls (ncclGetUniqueId, ncclCommInitRank, ncclCommInitAll) block without a timeout of their own; frt_comm_get_unique_id,
 * frt_comm_create and frt_comm_create_all give up after this many seconds and return FRT_ERR_DEVICE with a message that says what to look at
 * (a rank that never called in, the interface RCCL chose).  Default 180 s (env FRT_COMM_BOOTSTRAP_TIMEOUT_S); <= 0: wait for ever.  Process-wide;
 * returns the previous value. */
double frt_comm_set_bootstrap_timeout(double seconds);
int frt_comm_create(const uint8_t *id, int rank, int world, int device, frt_comm **out);
int frt_comm_create_all(int n_devices, const int *devices, frt_comm **out /* [n_devices] */);
void frt_comm_destroy(frt_comm *c);
int frt_comm_rank(const frt_comm *c);
int frt_comm_world(const frt_comm *c);
/* the communicator's own exchange stream (a hipStream_t as void*) */
void *frt_comm_stream(frt_comm *c);
/* recv_dev [world][bytes_per_rank] <- every rank's send_dev [bytes_per_rank]; asynchronous on hip_stream (NULL: the communicator's
 * stream).  What travels: frt_face_result records (configs[3]), fp16 embeddings and (idx, sim) top-k lists (configs[4]). */
int frt_comm_all_gather(frt_comm *c, const void *send_dev, void *recv_dev, size_t bytes_per_rank, void *hip_stream);
/* the same collective for n communicators of ONE process issued from one thread (ncclGroupStart / End around the n calls) */
int frt_comm_all_gather_multi(int n, frt_comm *const *comms, const void *const *send_dev, void *const *recv_dev, size_t bytes_per_rank,
                              void *const *hip_streams);
int frt_comm_sync(frt_comm *c);

/* ------------------------------------------------------------------------------------------------------------------
 * Batched device-resident pipeline (new surface; the /inference call stack of src/app.cpp:304-310 for B frames at once,
 * without host round trips between the stages).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct frt_face_result {
    frt_bbox box;
    int32_t frame;     /* frame index inside the batch                          */
    int32_t match_idx; /* gallery row of the best match (-1: no gallery)        */
    float match_sim;   /* its cosine similarity                                 */
    int32_t valid;     /* 0: slot unused (fewer than max_faces boxes: box is all zeros, score 0) or empty ROI (box kept, score > 0) */
} frt_face_result;

/* Borrows the three objects (they must outlive the pipeline and live on the same device).  max_frames <= detector
 * max_batch.  Face slots are [frame][max_faces]. */
int frt_pipeline_create(frt_detector *d, frt_embedder *e, frt_matcher *m, int max_frames, frt_pipeline **out);
void frt_pipeline_destroy(frt_pipeline *p);
/* frames: host u8 BGR, n_frames contiguous frames.  results[n_frames*max_faces]; embeds_out (may be NULL)
 * [n_frames*max_faces][512]. */
int frt_pipeline_run(frt_pipeline *p, const uint8_t *frames, int n_frames, frt_face_result *results, float *embeds_out);
/* Asynchronous form of frt_pipeline_run for callers that keep several batches in flight (the reference's shell is synchronous,
 * app.cpp:293-352; this is the entry point a multi-threaded or double-buffered caller binds instead).  submit() queues the
 * H2D copy of `frames` on the pipeline's copy stream, the stages, and the D2H copies of `results` / `embeds_out`, and returns a
 * ticket; wait(ticket) blocks until that batch's outputs are in host memory.  All three host buffers must stay valid and
 * untouched until wait() returns, and should be pinned (hipHostMalloc / hipHostRegister): with pageable memory the copies
 * degrade to synchronous ones.  Up to 4 batches may be in flight; a 5th submit() first waits for the oldest.  Tickets complete
 * in order.  frt_pipeline_run (below the same path: submit + wait) may be called from several threads at once. */
int frt_pipeline_submit(frt_pipeline *p, const uint8_t *frames, int n_frames, frt_face_result *results, float *embeds_out, long *ticket_out);
int frt_pipeline_wait(frt_pipeline *p, long ticket);
/* frt_pipeline_submit that also returns the faces' u8 BGR 112x112 crops (what CroppedFace.face holds after ArcFaceIR50::forward,
 * src/arcface.cpp:3-17; the reply step JPEG-encodes one of them, src/app.cpp:328): crops_out [n_frames*max_faces][112][112][3], may be
 * NULL.  Crops of unused / empty-ROI slots are unspecified. */
int frt_pipeline_submit_crops(frt_pipeline *p, const uint8_t *frames, int n_frames, frt_face_result *results, float *embeds_out, uint8_t *crops_out,
                              long *ticket_out);
/* Same with everything resident in HBM: frames_dev u8 [n_frames][rows][cols][3]; results_dev / embeds_dev device
 * buffers (embeds_dev may be NULL).  Asynchronous on the pipeline stream; frt_pipeline_sync() waits. */
int frt_pipeline_run_dev(frt_pipeline *p, const void *frames_dev, int n_frames, void *results_dev, void *embeds_dev);
/* Same, ordered behind the caller's producer: ready_event is a hipEvent_t (as void*) the caller recorded after the work that
 * writes frames_dev (an upload, frt_jpeg_decode_batch_dev, frt_resize_frames_dev ... on ANY stream); the stages wait for it on the
 * device.  This is the form to use when the frames are produced asynchronously: with software pipelining on, plain
 * frt_pipeline_run_dev does not wait for earlier work on the pipeline stream (see frt_pipeline_set_overlap). */
int frt_pipeline_run_dev_after(frt_pipeline *p, const void *frames_dev, int n_frames, void *results_dev, void *embeds_dev, void *ready_event);
/* Safe mode for callers that produce the frames on the pipeline stream itself: every frt_pipeline_run_dev call first records an
 * event on that stream and the stages wait for it.  Correct by construction, but the pipeline stream also carries the joins of the
 * previous calls, so consecutive calls no longer overlap - prefer frt_pipeline_run_dev_after with a separate upload stream. */
int frt_pipeline_set_input_sync(frt_pipeline *p, int enable);
/* Stream-overlap self-check.  The three stages only overlap across calls when the pipeline's stage streams - and the caller's stream,
 * which carries the joins - sit on different hardware queues (ROCm maps streams round-robin onto 4 queues per priority level; a queue
 * runs in order).  This call MEASURES it: one 150 us single-wave probe kernel per stream, started together; *ratio_out = elapsed /
 * 150 us, about 1 when they run side by side, about n when n of them share a queue.  Above 1.5 the call still returns FRT_OK but
 * frt_last_error() holds a warning (also printed to stderr once unless FRT_QUIET is set) naming the remedy.  The same check runs over
 * the stage streams alone inside frt_pipeline_create (about 1 ms); call this one after
 * frt_pipeline_set_stream and after every other stream of the process (RCCL, copy streams) exists.  Waits for work in flight. */
int frt_pipeline_check_overlap(frt_pipeline *p, float *ratio_out);
int frt_pipeline_sync(frt_pipeline *p);
/* Run on a caller-owned HIP stream (a hipStream_t passed as void*, e.g. PyTorch's current stream, so that RCCL collectives
 * issued by the caller are ordered after the pipeline without a host synchronisation).  NULL restores the private stream. */
int frt_pipeline_set_stream(frt_pipeline *p, void *hip_stream);
/* Software pipelining across calls (default on): detector of call b+1, crop + recogniser of
 * call b and match + pack of call b-1 run on three internal streams; the pipeline stream joins at the end of every call, so
 * results stay ordered on it exactly as if the call had run there.  With overlap on, the frames passed to
 * frt_pipeline_run_dev must already be valid when the call is made (the internal streams do not wait for earlier work on
 * the pipeline stream) and must stay unchanged until that call's results are complete on the pipeline stream. */
int frt_pipeline_set_overlap(frt_pipeline *p, int enable);
/* hipGraph replay of a call's ~150 launches (opt-in through this call; measured neutral on one GPU).  A call whose buffers, batch size
 * and mode repeat is captured on its second occurrence and replayed afterwards; callers that never repeat their buffers stay
 * on eager launches.  Automatically off while frt_profile_enable() records events. */
int frt_pipeline_set_graph(frt_pipeline *p, int enable);
/* Pairing of consecutive calls (no reference counterpart - the reference answers one request at a time, src/app.cpp:243-287).
 * Below ~ 64 faces a recogniser pass is a chain of launch latencies, not work: 16 faces cost 0.59 ms, 32 faces 0.92 ms, and one match call
 * scans the gallery once whatever the number of queries.  The crop + recogniser + match stages of up to four CONSECUTIVE calls can run as
 * ONE pass: a call's detector stage is queued at the call as always; its later stages are queued together with a later call's.
 *
 * enable = -1 (DEFAULT since round 6): ADAPTIVE, frt_pipeline_submit calls only.  A call is held back only while the pipeline is backed up
 *   AND at least five earlier tickets are still running - the GPU then has work queued for longer than the held call waits (a caller that
 *   keeps two to four calls in flight is latency-coupled to each of them: any holding measured 3 - 20 % slower there, so it gets none).  Held
 *   submits are MERGED: the next submits' frames join the held ones in one staging set (up to four tickets / the pipeline's capacity) and run
 *   as ONE call - one detector pass, one recogniser pass, one match call, per-ticket result downloads (frt_pipeline_merge_stats); beyond that
 *   a call's recogniser pass may still wait for the next call's.  A call that finds the pipeline idle is queued at once: a lone caller sees
 *   exactly the unpaired pipeline and its latency.  Held calls are released by the submit that fills them or finds fewer than five tickets
 *   running, by frt_pipeline_wait on one of their tickets (or on any ticket once the backlog is gone), by frt_pipeline_run_dev,
 *   frt_pipeline_sync and any frt_pipeline_set_*; the submit / wait contract is unchanged.  frt_pipeline_run_dev calls are never held in
 *   this mode (their contract is the join on the pipeline stream AT the call).  -3: the same without the merging of submits.
 * enable = -2: adaptive for frt_pipeline_run_dev calls too.  What changes for such a caller: the pipeline stream joins a held call's results
 *   at a LATER call (or at frt_pipeline_sync), not at the call itself, and the frames must stay valid until then.
 * enable = 0: off.  enable = 1 or 2: ALWAYS pairs; 3, 4: always groups of three / four (both boundaries; results complete when the group
 *   is - up to three calls later - or at a flush; 64 faces per pass is where a pass stops being a latency chain).
 *
 * In every mode: boxes, validity and matched rows are the unpaired pipeline's; the embeddings come from the recogniser kernels chosen for
 * the faces of ALL the calls of a pass together (tile shapes follow the number of faces per pass) and agree with the unpaired ones to fp16
 * rounding (cosine >= 1 - 1e-5; the same relation as between any two batch sizes, tests/test_gpu_embedder.py, tests/test_gpu_pipeline.py).
 * A call is only held when it can be grouped: at least twice its face slots must fit max_frames * max_faces of the pipeline and the
 * recogniser's max_batch (a pipeline created for exactly the frames a call carries - the benchmark's 32-frame step - never groups).
 * frt_pipeline_pairing_stats counts the recogniser passes that served several calls and those that served one. */
int frt_pipeline_set_pairing(frt_pipeline *p, int enable);
int frt_pipeline_pairing_stats(frt_pipeline *p, long *paired_passes_out, long *single_passes_out);
/* Adaptive mode, host boundary: a frt_pipeline_submit that finds the DETECTOR still busy with earlier calls is not queued at once - its frames are
 * uploaded and held, the next submit's frames join them (up to 4 tickets / the pipeline's capacity), and the held frames run as ONE call: one
 * detector pass, one recogniser pass, one match call, per-ticket downloads (a 4-frame detector pass costs 258 us of kernels, a 32-frame one
 * 809).  Released like a held pass (above); a submit that finds the detector idle is never held.  Counts the calls that carried several
 * tickets and the tickets they carried. */
int frt_pipeline_merge_stats(frt_pipeline *p, long *merged_calls_out, long *merged_tickets_out);
/* hipGraph replay (frt_pipeline_set_graph): stage graphs captured / replayed so far (a key is captured on its second sighting). */
int frt_pipeline_graph_stats(frt_pipeline *p, long *captured_out, long *replayed_out);

/* ------------------------------------------------------------------------------------------------------------------
 * Request coalescing (opt-in).  The reference answers ONE frame per request (src/app.cpp:293-352) from a Crow server that runs
 * .multithreaded() (src/app.cpp:367); a one-frame call is 4 faces and leaves the device idle.  A coalescer gathers the frames of
 * requests that are being served at the same time into one pipeline batch: every request thread calls frt_coalescer_infer with its
 * frame and blocks; frames that arrive while earlier batches run (or within window_us of the first one when the device is idle)
 * travel together through frt_pipeline_submit; each caller gets its own frame's results.  Borrows the three objects like
 * frt_pipeline_create (m may be NULL or empty: no match).  max_frames <= the detector's max_batch.  Thread-safe.
 * The C++ shells use it behind RetinaFace::findFace / ArcFaceIR50::forward / featureMatching when asked to
 * (RetinaFace::coalesceWith, or FRT_COALESCE=<frames> in the environment).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct frt_coalescer frt_coalescer;
int frt_coalescer_create(frt_detector *d, frt_embedder *e, frt_matcher *m, int max_frames, int window_us, frt_coalescer **out);
void frt_coalescer_destroy(frt_coalescer *c);
/* One frame of the detector's frame size in, its max_faces result slots out (frt_face_result, frame = 0; slots [0, *n_boxes) hold the
 * boxes findFace returns, in its order); embeds_out (may be NULL) [max_faces][512].  Blocks until the frame's batch has completed. */
int frt_coalescer_infer(frt_coalescer *c, const uint8_t *bgr, int rows, int cols, size_t row_stride, frt_face_result *results, float *embeds_out,
                        int *n_boxes);
/* Same, and the faces' u8 BGR 112x112 crops (crops_out [max_faces][112][112][3], may be NULL) - everything ArcFaceIR50::forward leaves behind. */
int frt_coalescer_infer_crops(frt_coalescer *c, const uint8_t *bgr, int rows, int cols, size_t row_stride, frt_face_result *results, float *embeds_out,
                              uint8_t *crops_out, int *n_boxes);
/* Batches submitted and frames carried so far (frames / batches = the mean batch the load produced). */
int frt_coalescer_stats(frt_coalescer *c, long *batches_out, long *frames_out);

/* ------------------------------------------------------------------------------------------------------------------
 * Frame ingest: the caller's `cv::resize(img, img, Size(frameWidth, frameHeight))` (src/app.cpp:166,301;
 * default INTER_LINEAR, 8UC3) on the device, bit-identical to the CPU restatement of OpenCV's fixed-point path; and the JPEG decode
 * in front of it / the JPEG + base64 reply behind the hot path (below).
 * ------------------------------------------------------------------------------------------------------------------ */
/* host in, host out; out: out_rows x out_cols x 3, tight rows */
int frt_resize_frame(const uint8_t *bgr, int rows, int cols, size_t row_stride, uint8_t *out, int out_rows, int out_cols, int device);
/* device in, device out, asynchronous on hip_stream (null = default stream): n frames of rows x cols -> tight out_rows x out_cols,
 * e.g. straight into the buffer handed to frt_pipeline_run_dev */
int frt_resize_frames_dev(const void *src_dev, int n, int rows, int cols, size_t row_stride, size_t frame_stride, void *dst_dev,
                          int out_rows, int out_cols, void *hip_stream);

/* JPEG decode in front of the resize (src/app.cpp:296: cv::imdecode(byte_vector, IMREAD_UNCHANGED)) and the reply step behind the
 * hot path (src/app.cpp:328-340: cv::imencode(".jpg", best crop) + base64).  OpenCV hands both to libjpeg with its defaults (integer
 * "islow" DCT, triangle-filter chroma upsampling, quality 95, 4:2:0, Annex-K Huffman tables) - all-integer algorithms, reproduced
 * here bit for bit: Huffman coding on a pool of host threads (it is serial per scan), dequantisation + IDCT + upsampling + colour
 * conversion (+ the resize) and colour conversion + downsampling + FDCT + quantisation on the device.  Supported streams: baseline /
 * extended-sequential / progressive (spectral selection + successive approximation, any scan script) Huffman, 8 bit, grey or YCbCr
 * with 4:4:4 / 4:2:2 / 4:2:0 sampling, restart intervals; arithmetic-coded, lossless, RGB-coded and CMYK streams return
 * FRT_ERR_FORMAT.  Grey images come out with the value replicated to B, G and R. */
typedef struct frt_jpeg_decoder frt_jpeg_decoder;
/* header only; any of the out pointers may be NULL */
int frt_jpeg_info(const uint8_t *data, size_t size, int *width, int *height, int *components);
/* n_threads <= 0: one host thread per image up to the machine's core count (max 64).  max_images = JPEGs per decode_batch call. */
int frt_jpeg_decoder_create(int max_images, int max_width, int max_height, int n_threads, int device, frt_jpeg_decoder **out);
void frt_jpeg_decoder_destroy(frt_jpeg_decoder *d);
/* n JPEG byte strings -> frames_dev u8 BGR [n][out_h][out_w][3] (device; e.g. the buffer handed to frt_pipeline_run_dev_after).  Images
 * whose size differs from out_w x out_h are resized like frt_resize_frames_dev (cv::resize default INTER_LINEAR).  The call returns when
 * the entropy decoding is done and the device work is queued on hip_stream (NULL: the decoder's own stream); the JPEG bytes may be
 * released then, frames_dev is complete once hip_stream has run. */
int frt_jpeg_decode_batch_dev(frt_jpeg_decoder *d, const uint8_t *const *data, const size_t *sizes, int n, void *frames_dev, int out_h, int out_w,
                              void *hip_stream);
/* one image, host in / host out, at its own size: bgr_out [height][width][3] */
int frt_jpeg_decode(frt_jpeg_decoder *d, const uint8_t *data, size_t size, uint8_t *bgr_out, size_t capacity, int *width, int *height);
/* host half only (tests, tools): entropy-decoded, NOT dequantised coefficient blocks [total_blocks][64] in natural order (coef_out may
 * be NULL) and the geometry: int32[219] = width, height, ncomp, hmax, vmax, 3 x (h, v, blocks_w, blocks_h, samples_w, samples_h, first
 * block), total_blocks, 3 x 64 quantiser steps (natural order). */
int frt_jpeg_read_coefficients(const uint8_t *data, size_t size, int16_t *coef_out, size_t coef_capacity_blocks, int32_t *geometry_out);
/* Reply step: n equally sized u8 BGR images [n][rows][cols][3] (host pointer, or device pointer with device_input = 1, e.g. the crops
 * of frt_embedder_forward) -> n JFIF streams, slot i at out + i * out_stride, length out_sizes[i].  quality as cv::imencode's
 * IMWRITE_JPEG_QUALITY (the reference uses the default, 95). */
int frt_jpeg_encode_batch(frt_jpeg_decoder *d, const void *bgr, int device_input, int n, int rows, int cols, int quality, uint8_t *out, size_t out_stride,
                          size_t *out_sizes);
/* Same, ordered behind an asynchronous producer of a DEVICE input: ready_event is a hipEvent_t (as void*, NULL = none) the caller
 * recorded after the work that writes `bgr` (a pipeline stage, another stream's forward ...); the codec's stream waits for it on the
 * device.  frt_jpeg_encode_batch itself only orders against work the caller has already synchronised. */
int frt_jpeg_encode_batch_after(frt_jpeg_decoder *d, const void *bgr, int device_input, int n, int rows, int cols, int quality, uint8_t *out,
                                size_t out_stride, size_t *out_sizes, void *ready_event);
/* host half only: quantised blocks in zigzag order (all luma blocks [2*mcuy][2*mcux], then Cb, then Cr [mcuy][mcux]) -> JFIF stream */
int frt_jpeg_write_jfif(int quality, int width, int height, const int16_t *coef_zigzag, uint8_t *out, size_t capacity, size_t *size_out);
/* crow::utility::base64encode (src/app.cpp:331): standard alphabet with '=' padding, NUL-terminated.  Returns the string length, or
 * the capacity needed (length + 1) when out is NULL or too small. */
size_t frt_base64_encode(const uint8_t *data, size_t size, char *out, size_t capacity);

/* ------------------------------------------------------------------------------------------------------------------
 * Optional 5-point alignment mode (default OFF).  The reference has none: it trims the landmark head off the detector
 * (conversion/retina/torch2trt.py:7-9, src/retinaface.cpp:58-60) and feeds the embedder a bbox crop + bicubic resize
 * (src/arcface.cpp:3-17).  These entry points exist for accuracy work only and need a detector blob exported WITH
 * LandmarkHead.* (conversion/retina/models/retinaface.py:37-46,117); their oracle (oracle/align.py) is "parity
 * unpinned" - there is no reference behaviour to compare with.
 *   landmarks layout: 10 floats per face = (x0,y0,...,x4,y4), x = column, y = row in FRAME pixels, order
 *   left eye, right eye, nose, left mouth corner, right mouth corner (upstream RetinaFace order). */
int frt_detector_has_landmarks(const frt_detector *d);
/* findFace + landmarks of the kept boxes.  landmarks_out: capacity max_faces*10. */
int frt_detector_find_faces_landmarks(frt_detector *d, const uint8_t *bgr, int rows, int cols, size_t row_stride, frt_bbox *out,
                                      float *landmarks_out, int *n_out);
/* doInference with the third output: ldm_out [batch][A][10] raw head values. */
int frt_detector_infer_landmarks(frt_detector *d, const float *chw, int batch, float *loc_out, float *conf_out, float *ldm_out);
/* Counterpart of frt_crop_faces: least-squares similarity from the 5 landmarks to the ArcFace 112x112 template, bilinear
 * warp with zero border.  crops_out: n x 112 x 112 x 3 BGR u8.  FRT_ERR_EMPTY_ROI for degenerate (coincident) landmarks. */
int frt_align_faces(const uint8_t *bgr, int rows, int cols, size_t row_stride, const float *landmarks, int n, uint8_t *crops_out,
                    int device);
/* Counterpart of frt_embedder_forward with aligned crops instead of bbox crops. */
int frt_embedder_forward_aligned(frt_embedder *e, const uint8_t *bgr, int rows, int cols, size_t row_stride, const float *landmarks,
                                 int n, float *embeds_out, uint8_t *crops_out);
/* Switch a pipeline between the reference's crop (0, default) and the aligned crop (1). */
int frt_pipeline_set_align(frt_pipeline *p, int enable);

/* ------------------------------------------------------------------------------------------------------------------
 * Face images instead of frames.  The reference takes a pre-cropped face in three places - /recognize (src/app.cpp:243-287),
 * /insert/face with api_imgIsCropped (src/app.cpp:148-162) and the `gen` start-up mode that builds the database from a folder of face
 * images (src/app.cpp:69-99) - and does the same per image in all of them: cv::resize to 112x112 when the size differs (default
 * INTER_LINEAR), preprocessFace, one recogniser inference.  These entry points take a ragged batch of such images, of any sizes: the u8
 * bytes go up once (a quarter of the fp32 tensor's), resize + preprocessFace are one kernel, the recogniser runs full passes of
 * max_batch faces while the next images upload, and the embeddings go to the host or straight into the live gallery.
 *   All arguments are checked before any device work: a NULL image pointer, rows < 1, cols < 1, row_stride < cols * 3 or n < 0 is
 *   FRT_ERR_INVALID with the image's index in frt_last_error(), nothing written, nothing changed.  n == 0 succeeds and does nothing.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct frt_face_image { const uint8_t *bgr; int32_t rows, cols; size_t row_stride; } frt_face_image;
/* cv::resize(112x112) + preprocessFace for n images in one launch; crops_out u8 [n][112][112][3] and chw_out fp32 [n][3][112][112], either may be NULL */
int frt_preprocess_faces(const frt_face_image *faces, int n, uint8_t *crops_out, float *chw_out, int device);
/* the loop of gen / /insert/face / /recognize for n images: embeds_out [n][512] L2-normalised, crops_out may be NULL */
int frt_embedder_embed_faces(frt_embedder *e, const frt_face_image *faces, int n, float *embeds_out, uint8_t *crops_out);
/* embed n images and append their embeddings to the live gallery as ONE edit, device to device: labels NULL for an unlabelled gallery, else
 * [n] (host) as frt_matcher_gallery_add_labeled; embeds_out (may be NULL) also returns them; first_row_out <- index of the first new row.
 * At most 65536 images per call (FRT_ERR_CAPACITY, nothing done); the gallery gets all n rows or none; a labelled call on an unlabelled
 * gallery with rows (or the reverse) is FRT_ERR_INVALID.  Takes the embedder's lock, then the matcher's; both objects on one device. */
int frt_embedder_enrol_faces(frt_embedder *e, frt_matcher *m, const frt_face_image *faces, int n, const int32_t *labels, float *embeds_out, int *first_row_out);

/* ------------------------------------------------------------------------------------------------------------------
 * Whole photos of any sizes.  The other half of /insert/face - the default, api_imgIsCropped false (src/app.cpp:163-187) - and the head of
 * /inference (src/app.cpp:296-301) take a photo of any size: cv::resize it to frameWidth x frameHeight (default INTER_LINEAR, aspect not
 * kept), findFace, getCroppedFaces; /insert/face then requires exactly one face (ret = 2 for more than one, :172-174; ret = 3 for none,
 * :175-177), embeds it and stores it.  These entry points do that for a ragged batch: the photos' bytes go up once per chunk, ONE kernel
 * resizes a chunk into the pipeline's frame buffer (the arithmetic of frt_resize_frame, bit for bit), the chunks run through the
 * three-stage pipeline back to back while the next one uploads, and the "exactly one face" rule and the gallery edit stay on the device.
 *   Argument checks are frt_embedder_embed_faces's, made before any device work (and before the pipeline handle is looked at): a NULL image
 *   pointer, rows < 1, cols < 1, row_stride < cols * 3 or n < 0 is FRT_ERR_INVALID with the image's index in frt_last_error().  n == 0
 *   succeeds and does nothing.  Images are cut into chunks of at most the pipeline's max_frames photos and 64 MiB of pixels.
 *   Both pipeline calls may run beside frt_pipeline_submit / wait / run of other threads (lock order: the pipeline's image-stage mutex, then
 *   per chunk run_mu -> object mutexes; the matcher's for the edit last).  Every chunk is queued in full when it is handed over: in a pairing
 *   mode that holds frt_pipeline_run_dev calls (frt_pipeline_set_pairing 1 .. 4, -2) whatever is held or pending is flushed behind each chunk,
 *   so the answers are those of pairing off.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef enum frt_enrol_status {
    FRT_ENROL_OK = 1,        /* one box and valid != 0: the photo is (or would be) enrolled                                         */
    FRT_ENROL_MANY = 2,      /* more than one box (src/app.cpp:172-174).  With maxFacesPerScene == 1 the cap behind NMS leaves at most
                              * one box, so this status cannot occur - the reference behaves the same                               */
    FRT_ENROL_NONE = 3,      /* no box (src/app.cpp:175-177)                                                                        */
    FRT_ENROL_EMPTY_ROI = 4, /* one box whose ROI is empty (valid == 0, score > 0): OpenCV would throw there                       */
    FRT_ENROL_LOW_QUALITY = 5 /* one valid box whose quality record carries a flag ("Face quality" below); only the gated calls answer it */
} frt_enrol_status;
/* ragged counterpart of frt_resize_frame: n images of any sizes -> out u8 [n][out_rows][out_cols][3], one launch */
int frt_resize_images(const frt_face_image *images, int n, uint8_t *out, int out_rows, int out_cols, int device);
/* device building block for callers whose frames are already on the device (frt_jpeg_decode_batch_dev + frt_pipeline_run_dev_after):
 * results_dev frt_face_result [n_frames][max_faces] and embeds_dev float [n_frames][max_faces][512] as the pipeline leaves them (a frame's
 * boxes fill its slots from slot 0; an unused slot has score 0); status_dev int32[n_frames] <- frt_enrol_status, face_dev
 * frt_face_result[n_frames] (may be NULL) <- slot 0's record for OK / EMPTY_ROI, zeros otherwise, `frame` kept; rows_dev float
 * [>= *count + n_frames][512] <- the embeddings of the OK frames, dense, in frame order, from row *count on; count_dev int32 (read as base,
 * advanced by the number of OK frames).  One workgroup, asynchronous on hip_stream (the current device's; NULL = default stream): calls on
 * one stream append.  embeds_dev and rows_dev must be 16-byte aligned.  n_frames == 0 does nothing. */
int frt_enrol_select_dev(const void *results_dev, const void *embeds_dev, int n_frames, int max_faces, void *status_dev, void *face_dev,
                         void *rows_dev, void *count_dev, void *hip_stream);
/* /inference for n images of any sizes: results [n][max_faces] (frame = index of the image IN THE CALL; boxes in the resized
 * frame_w x frame_h frame, as the reference's), embeds_out [n][max_faces][512] and crops_out [n][max_faces][112][112][3] may be NULL */
int frt_pipeline_run_images(frt_pipeline *p, const frt_face_image *images, int n, frt_face_result *results, float *embeds_out, uint8_t *crops_out);
/* /insert/face without api_imgIsCropped for n photos, ONE gallery edit.  Needs a pipeline with a matcher whose gallery holds 512-column rows
 * (FRT_ERR_INVALID otherwise; an empty gallery: gallery_begin(m, cap, 512) + commit first).  At most 65536 images per call
 * (FRT_ERR_CAPACITY, nothing done).  labels: NULL for an unlabelled gallery, else [n] on the host, one per IMAGE (those of the accepted
 * images go to frt_matcher_gallery_add_labeled_dev); a negative label or the wrong form for a gallery with rows is FRT_ERR_INVALID before
 * any device work.  status_out [n] <- frt_enrol_status, always written on success.  faces_out [n] (may be NULL) <- the photo's face
 * (frame = index of the image in the call) with match_idx / match_sim against the gallery AS IT WAS BEFORE THE CALL: every chunk is matched
 * before the edit, photos of one call do not see each other; the match is reported, not acted on.  The rows of the FRT_ENROL_OK photos are
 * appended in image order as ONE edit - all of them or none; one step of frt_matcher_generation when the rows fit the reserved capacity
 * (an add that has to move the gallery also moves the scratch of a matcher bound to a pipeline, a step of its own); none accepted: no edit.  embeds_out (may be NULL, room
 * for [n][512]) <- [n_enrolled][512], exactly the rows added (what db.insertFace stores); first_row_out <- index of the first new row; n_enrolled_out <-
 * rows added.  On any error the gallery is unchanged. */
int frt_pipeline_enrol_images(frt_pipeline *p, const frt_face_image *images, int n, const int32_t *labels, int32_t *status_out,
                              frt_face_result *faces_out, float *embeds_out, int *first_row_out, int *n_enrolled_out);

/* ------------------------------------------------------------------------------------------------------------------
 * Large photos by tiles.  Every route above squeezes a photo into ONE frame_w x frame_h frame, so a small face of a large photo falls below
 * the smallest anchor.  Here the photo is cut into overlapping tiles of the detector's frame size (plus, optionally, the whole photo resized
 * into one more tile: the overview, for the faces too large for a tile), the detector runs on the tiles in chunks of max_batch, every
 * tile's boxes are mapped into photo coordinates and ONE greedy non-maximum suppression over all of them decides, on the device.  The
 * reference has nothing like it, so the semantics are fixed here, to the integer (tests/tiled_ref.py restates them in numpy).
 *   x is the row, y the column, corners inclusive (areas take + 1).  The tile is frame_h x frame_w = T_r x T_c.
 *   Plan, per axis of length L with tile T, overlap V, stride S = T - V: L <= T is one tile at origin 0 (padded when L < T); else
 *     n = ceil((L - T) / S) + 1 tiles at origin_i = min(i * S, L - T) - the last one is pulled inward, never padded.  Tiles are numbered
 *     row-major over the grid, the overview last.  At most 4096 tiles per photo (FRT_ERR_CAPACITY).
 *   Cut: grid tile t is the photo at [row0, row0 + T_r) x [col0, col0 + T_c); every byte outside the photo is 128 (the letterbox canvas
 *     value).  The overview is frt_resize_frame(photo -> T_r x T_c).
 *   Candidates: slot s < n_boxes[t] of tile t, source index t * slots + s; a NaN score is never one.
 *   Cut test (kind 0, tile coordinates): x1 == 0 && row0 > 0, y1 == 0 && col0 > 0, x2 == T_r - 1 && row0 + T_r < photo_rows,
 *     y2 == T_c - 1 && col0 + T_c < photo_cols: the box touches a tile edge that lies inside the photo.  drop_cut removes these first.
 *   Map: kind 0 adds row0 / col0, drops a box with x1 >= photo_rows or y1 >= photo_cols (wholly in padding), clips to [0, photo - 1];
 *     kind 1: x1' = (int64)x1 * photo_rows / T_r, x2' = (int64)(x2 + 1) * photo_rows / T_r - 1 raised to at least x1', columns alike, clip.
 *   Merge: order by score descending, then tile, then slot ascending; greedy: the first live candidate is kept, every live one whose
 *     overlap with it is >= the threshold dies; until none is live or max_out are kept.  Overlap is float32 in the detector's own operation
 *     order: metric 0 = inter / (area_a + area_b - inter) (one tile with metric 0 is the detector's NMS bit for bit), metric 1 =
 *     inter / min(area_a, area_b), which also catches a part-face box inside a whole-face box.
 *   out[i] = box in photo coordinates + score, src_out[i] = source index; unused slots are zeros / -1.
 *   Landmarks (blob with the LandmarkHead only) follow their box, unclipped: kind 0 x + col0, y + row0; kind 1 x * photo_cols / T_c,
 *     y * photo_rows / T_r in float32.
 *   Limits: n_tiles * slots <= 16384 and 1 <= max_out <= 16384, else FRT_ERR_CAPACITY.  The per-tile cap is the detector's max_faces: a
 *     crowd wants a detector created with 16 to 32.
 *   All arguments are checked before any device work: a NULL pointer, rows < 1, cols < 1, row_stride < cols * 3, an overlap outside
 *     0 <= overlap < T, a metric other than 0 / 1 is FRT_ERR_INVALID; a call that fails writes nothing.
 *   From boxes to names in one call, on the device: "Recognising a large photo by tiles" below (frt_pipeline_run_photo_tiled).  By hand:
 *   frt_embedder_forward / _forward_aligned take the photo of any size with the boxes (and landmarks) this returns.  The batched
 *   frt_pipeline_submit / run_images and the coalescer do not tile.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct frt_tile_options {
    int32_t overlap_rows, overlap_cols; /* pixels neighbouring tiles share; 0 <= overlap < T on its axis                          */
    int32_t overview;                   /* 1: one more tile, the whole photo resized to the tile                                   */
    int32_t metric;                     /* 0: IoU, 1: intersection over the smaller area                                           */
    int32_t drop_cut;                   /* 1: discard grid-tile boxes that touch a tile edge inside the photo                      */
    float merge_threshold;              /* suppress at overlap >= this; negative: the detector's nms_threshold                    */
} frt_tile_options;
typedef struct frt_tile { int32_t row0, col0, rows, cols, kind; } frt_tile; /* kind 0: grid tile, rows / cols = its part inside the photo;
                                                                             * kind 1: the overview, row0 = col0 = 0, rows / cols = the photo's */
/* the plan alone (pure host, no device; of options only the overlaps and overview are read).  tiles_out may be NULL with capacity 0 to ask
 * for the count; more tiles than capacity is FRT_ERR_CAPACITY with *n_tiles_out set and tiles_out untouched */
int frt_tile_plan(int rows, int cols, int tile_rows, int tile_cols, const frt_tile_options *options, frt_tile *tiles_out, int capacity,
                  int *n_tiles_out);
/* the cut alone: host in, host out u8 [n_tiles][tile_rows][tile_cols][3] */
int frt_cut_tiles(const uint8_t *bgr, int rows, int cols, size_t row_stride, const frt_tile *tiles, int n_tiles, int tile_rows, int tile_cols,
                  uint8_t *out, int device);
/* the device merge behind host pointers, also for callers who run a multi-scale scheme of their own: boxes [n_tiles][slots] in tile
 * coordinates, n_boxes [n_tiles]; out [max_out], src_out [max_out], n_out.  There is no detector here: merge_threshold must be >= 0 */
int frt_merge_boxes(const frt_bbox *boxes, const int32_t *n_boxes, const frt_tile *tiles, int n_tiles, int slots, int photo_rows,
                    int photo_cols, int tile_rows, int tile_cols, const frt_tile_options *options, int max_out, frt_bbox *out,
                    int32_t *src_out, int *n_out, int device);
/* photo of any size -> boxes in photo coordinates: one upload, cut + detector + post-processing per chunk of max_batch tiles, one merge,
 * one synchronisation.  options NULL: overlap = a quarter of the tile on each axis, overview 1, metric 1, drop_cut 1, threshold -1.
 * slots = the detector's max_faces.  landmarks_out [max_out][10] may be NULL (FRT_ERR_FORMAT for a blob without the LandmarkHead);
 * src_out [max_out] may be NULL */
int frt_detector_find_faces_tiled(frt_detector *d, const uint8_t *bgr, int rows, int cols, size_t row_stride, const frt_tile_options *options,
                                  int max_out, frt_bbox *out, float *landmarks_out, int32_t *src_out, int *n_out);

/* ------------------------------------------------------------------------------------------------------------------
 * Recognising a large photo by tiles.  frt_detector_find_faces_tiled stops at the boxes; this is the rest of the way - crop, embed, match -
 * without the photo going up a second time and without the box list, the embeddings or the matches visiting the host in between.
 *   Gate: a merged box is kept iff min(x2 - x1, y2 - y1) >= min_face - the extents of the crop's ROI, far corner excluded (a box of
 *     11 x 11 pixels has x2 - x1 = 10).  min_face <= 0 keeps every box, a zero-extent one included: its crop is empty, valid = 0.
 *   Work list: the kept boxes, dense and in merge order (score descending, then tile, then slot), with their source indices, their landmarks
 *     and keep_pos = their position in the merged list; zeros / -1 behind the count.  pass_count[j] = clamp(n_kept - j * max_batch, 0,
 *     max_batch), j < ceil(n / max_batch): the faces of recogniser pass j.  One launch for any list of 0 .. 16384 boxes, the same bits on
 *     every run (a stable compaction, no atomics).
 *   frt_pipeline_run_photo_tiled returns, to the bit, what this loop returns on the pipeline's three objects: frt_detector_find_faces_tiled
 *     (max_out caps the merged list BEFORE the gate); the gate; frt_embedder_forward on the photo with the kept boxes - after
 *     frt_pipeline_set_align(p, 1) frt_embedder_forward_aligned with the kept landmarks -; frt_matcher_top1 of those embeddings when the
 *     pipeline has a matcher with rows.  Recogniser passes are cut every max_batch kept faces, as frt_embedder_forward cuts them; its flip
 *     and fp32 modes apply.
 *   results[i], i < *n_out: the box in photo coordinates with its score, frame = 0, valid / match_idx / match_sim as everywhere in the
 *     pipeline: an empty ROI (or degenerate landmarks) is valid 0, match_idx -1, match_sim 0 and an all-zero embedding - reported here, not
 *     as FRT_ERR_EMPTY_ROI: one bad box must not fail a 300-face photo -; no gallery: match_idx -1.  Behind *n_out: results are unused
 *     slots (all zero but match_idx -1), src_out -1, landmarks_out 0; embeds_out and crops_out are written for the first *n_out faces only.
 *   Flow: one upload, tiled detection and merge as above, the select launch, ONE host read (the kept count: how many passes to queue), per
 *     pass crop or align out of the photo where the detector left it + the recogniser, one match, one pack, the downloads, one
 *     synchronisation.  Serial on the detector's stream; never graph-captured, never paired or merged with other calls.
 *   May run beside frt_pipeline_submit / wait / run of other threads.  Lock order: the pipeline's image-stage mutex, run_mu, then the
 *     detector's, the embedder's and the matcher's mutex, all held to the end of the call; whatever a pairing mode holds or has pending is
 *     flushed first, so the answers are those of pairing off.
 *   Checked before any device work, and before the pipeline handle is looked at: a NULL bgr / results / n_out, rows < 1, cols < 1,
 *     row_stride < cols * 3, a negative overlap, a metric other than 0 / 1: FRT_ERR_INVALID; max_out outside 1 .. 16384:
 *     FRT_ERR_CAPACITY.  Then a NULL pipeline: FRT_ERR_INVALID.  Then what needs the detector's tile: an overlap >= T (FRT_ERR_INVALID),
 *     landmarks_out with a blob without the LandmarkHead (FRT_ERR_FORMAT), more than 4096 tiles or n_tiles * max_faces > 16384
 *     (FRT_ERR_CAPACITY).  A call that fails writes nothing.
 * ------------------------------------------------------------------------------------------------------------------ */
/* the select launch behind host pointers: boxes [n], src [n] (may be NULL), landmarks [n][10] (may be NULL) -> boxes_out [n], src_out [n]
 * (with src), landmarks_out [n][10] (with landmarks), keep_pos_out [n], pass_count_out [ceil(n / max_batch)], *n_kept_out.  n outside
 * 0 .. 16384 is FRT_ERR_CAPACITY, max_batch < 1 or a NULL required pointer FRT_ERR_INVALID, before any device work; n == 0 writes
 * *n_kept_out = 0 alone */
int frt_select_faces(const frt_bbox *boxes, const int32_t *src /* may be NULL */, const float *landmarks /* may be NULL */, int n,
                     int min_face, int max_batch, frt_bbox *boxes_out, int32_t *src_out, float *landmarks_out, int32_t *keep_pos_out,
                     int32_t *pass_count_out, int *n_kept_out, int device);
/* options NULL: frt_detector_find_faces_tiled's defaults */
int frt_pipeline_run_photo_tiled(frt_pipeline *p, const uint8_t *bgr, int rows, int cols, size_t row_stride,
                                 const frt_tile_options *options, int min_face, int max_out,
                                 frt_face_result *results /* [max_out] */, float *landmarks_out /* [max_out][10], may be NULL */,
                                 float *embeds_out /* [max_out][512], may be NULL */, uint8_t *crops_out /* [max_out][112][112][3], may be NULL */,
                                 int32_t *src_out /* [max_out], may be NULL */, int *n_out);

/* ------------------------------------------------------------------------------------------------------------------
 * Face tracker: follow faces across the consecutive frames of a video stream, on the device.  The hot path this library replaces is
 * /inference, a WebSocket that receives the frames of ONE camera one after the other (src/app.cpp:293-352); every call above answers a frame
 * as if it were the only one.  A tracker carries, in HBM and for up to 1024 independent streams, what joins the frames: which face of this
 * frame is which face of the last one (a stable track id), the running template of the track (the re-normalised sum of its embeddings, the
 * template of frt_matcher_build_templates) and the identity of THAT TEMPLATE rather than of the single frame.  It follows the results_dev /
 * embeds_dev frt_pipeline_run_dev leaves on the pipeline stream; nothing visits the host.  The reference has no tracker, so the semantics
 * are fixed here, to the integer (tests/track_ref.py restates them in numpy).
 *   Object: n_streams (1 .. 1024) streams; each has max_tracks (1 .. 64) slots, next_id (starts at 0, never reused, survives reset), tick
 *     (the updates the stream took part in) and dropped.  max_faces (1 .. 64) and dim (a multiple of 4, 4 .. 2048) are fixed at creation.
 *   One update takes n_frames (1 .. 256, else FRT_ERR_CAPACITY) frames and stream_ids[n_frames] on the host (NULL: frame i is stream i); the
 *     ids lie in 0 .. n_streams - 1 and are pairwise distinct.  A stream absent from the call is not touched at all.  Per frame f of stream
 *     s, with results[f][0 .. max_faces) as the pipeline writes them:
 *     1. detection slot d is PRESENT iff box.score > 0 (an unused slot has score 0; an empty-ROI slot - valid 0, score > 0 - is present).
 *     2. Association: present detections in slot order (the detector emits them score-descending); candidates are the tracks of s that were
 *        live at entry and are not yet taken; ovr = the float32 IoU of the detector's NMS (metric 0 of "Large photos by tiles") of the
 *        detection's box with the track's; the winner is the largest ovr, the lowest slot among equals, and it is matched iff
 *        ovr >= iou_threshold (a NaN never matches).  A match: track.box = det.box (score included), hits += 1, missed = 0.
 *     3. Expiry: every track live at entry and not matched gets missed += 1; missed > max_missed frees the slot and zeroes its state.
 *     4. Births: every present, unmatched detection, in slot order, takes the lowest free slot (those freed in step 3 included):
 *        id = next_id++, born = tick, hits = 1, missed = 0, n_embeds = 0, sum = 0, match_idx = -1, match_sim = 0.  Without a free slot the
 *        detection is UNTRACKED (track_id = slot = -1) and dropped += 1.
 *     5. Embedding, every tracked detection with valid != 0: sum[k] = fl(fl(decay * sum[k]) + e[k]) (two roundings, never an fma: the bits
 *        of numpy float32), n_embeds += 1.
 *     6. Template of a tracked detection: sum / ||sum||_2 when n_embeds > 0 and the norm is non-zero, else zeros (the norm reduced as
 *        frt_matcher_build_templates reduces it) -> templates[f][d][dim]; rows of absent or untracked detections are zeros.
 *     7. Identity, only with a matcher that has rows: ONE frt_matcher_top1_dev over all n_frames * max_faces template rows on the caller's
 *        stream; for tracked detections with n_embeds > 0 the answer goes to the track (match_idx, match_sim) and to the output, every
 *        other detection reports -1 / 0.  A coasting track (not seen in this frame) keeps its last identity.
 *     8. tick += 1.
 *   Output per face slot: frt_track_result.  age = tick - born + 1 (tick before step 8), confirmed = hits >= min_hits; an absent detection
 *     is all zero with track_id = slot = match_idx = -1.
 *   Every argument check runs before any device work - NULL pointers and ranges, then duplicate or out-of-range stream ids, then a matcher
 *     whose num_col != dim (FRT_ERR_INVALID) -; a refused call writes nothing and changes no state.  embeds_dev / templates_dev must be
 *     16-byte aligned.  The tracker has one mutex; updates queued on different HIP streams are the caller's to order.
 *
 *   Appearance (frt_tracker_set_appearance; off by default, and with it off an update is launch for launch and byte for byte the one
 *   described above).  Overlap alone loses a face that stays away longer than max_missed or jumps further than iou_threshold allows, and
 *   swaps two faces that cross.  With appearance on, the detection's embedding is compared with the track's running sum, in the same call
 *   (tests/track_reid_ref.py restates this block in numpy, to the bit).
 *     The reduction dot2r(x, y), with G = ceil(dim / 256): lane l (0 .. 63) starts at acc = 0; for g = 0 .. G-1 and j = 0 .. 3, with
 *       k = 256 g + 4 l + j < dim: acc = fl(acc + fl(x[k] * y[k])) - two roundings, never an fma -; then six butterfly steps, off = 32, 16,
 *       8, 4, 2, 1: v_l = fl(v_l + v_(l xor off)).  The result is lane 0's value (all lanes hold the same bits).  It is NOT step 6's fmaf
 *       chain: numpy float32 reproduces it bit for bit (pad to [G][64][4] with zeros, chain, then the six v + v[perm] steps).
 *     The similarity of detection d of a frame and slot t of its stream, sum_t being the track's sum AT ENTRY (before this update's step 5):
 *       n2 = dot2r(sum_t, sum_t), S[d][t] = fl(dot2r(e_d, sum_t) / fl(sqrt(n2))), division and square root correctly rounded.
 *       S[d][t] is DEFINED iff d is present with valid != 0, t was live at entry with n_embeds > 0, and n2 > 0.  The embedding is taken as
 *       the recogniser leaves it (unit norm) and is not re-normalised.  A NaN S never vetoes and never matches: every comparison below
 *       fails for it.
 *     Two settings per tracker: reid_threshold in (0, 1] or the off value 2.0; iou_min_sim in [-1, 1] or the off value -2.0.  Any other
 *       value, a NaN included, is FRT_ERR_INVALID.  Both default to off.
 *     Step 2 becomes 2a and 2b.
 *       2a is step 2 with one more exclusion: when iou_min_sim is on, track t is no candidate for detection d if S[d][t] is DEFINED and
 *          S[d][t] < iou_min_sim.
 *       2b runs only when reid_threshold is on.  It walks every present detection with valid != 0 that 2a left unmatched, in slot order;
 *          candidates are the tracks live at entry, not yet taken (by 2a or by an earlier detection of 2b), with S[d][t] DEFINED and
 *          S[d][t] >= reid_threshold; the winner is the largest S, the lowest slot among equals.  A match does what a 2a match does:
 *          track.box = det.box, hits += 1, missed = 0.
 *       Steps 3 to 8 are unchanged; expiry sees the tracks 2b took as taken.
 *     How each detection was associated: frt_track_assoc per face slot, an optional output of the frt_tracker_update_assoc* entry points
 *       (with both settings off they report how / gap / ovr / sim of the update above).
 *     Nobody has measured S on real faces with this library: no threshold is recommended here, and the synthetic weights of the tests say
 *       nothing about where genuine and impostor similarities lie.  frt_matcher_separation over an enrolled gallery is the place to start.
 *
 *   Motion (frt_tracker_set_motion; off by default, and a tracker that never switches it on allocates nothing more and produces the bytes
 *   described above).  The overlap of step 2 is taken with the track's last measured box: a face that moves more than about half its width
 *   between two updates is born again under a new id, a coasting track is compared where it was last seen, and the gate's skip_iou sends a
 *   walking person through the recogniser on every frame.  With motion on every track carries a constant-velocity term and every place
 *   that compares a detection with a track's box uses the PREDICTED box (tests/track_motion_ref.py restates this block in Python ints).
 *     State: vel int32 [n_streams][max_tracks][2] beside the sums, (vx, vy) of the box centre in 1/256 pixel per update; allocated and
 *       zeroed by the first call that needs it with motion on.  A free slot's velocity is (0, 0).  frt_track_state, frt_track_result and
 *       frt_tracker_tracks do not change: a slot's box stays the last MEASURED box.
 *     Setting: gain 0 is off (the default), 1 .. 256 on; anything else is FRT_ERR_INVALID and changes nothing.  Off -> on zeroes every
 *       velocity (no device work while the array does not exist; otherwise synchronous behind the last queued update, like
 *       frt_tracker_reset); on -> another on value keeps them; on -> off leaves the array alone - it is never read while off.
 *       frt_tracker_reset zeroes the velocity rows of the streams it resets when the array exists.
 *     All arithmetic is in integers; tdiv(a, b) = sign(a) * (|a| / b) for b > 0 is truncation toward zero (C's division, not a floor).
 *     M1. Prediction, for a track live at entry: k = missed + 1; sx = clamp(tdiv((int64) vx * k, 256), -2^30, 2^30), sy likewise; the
 *         predicted box is (x1 + sx, y1 + sy, x2 + sx, y2 + sy, score), each coordinate computed in int64 and clamped to the int32 range
 *         (the clamp is monotone: x1 <= x2 survives).  It replaces the track's box in step 2 / 2a's overlap, in the ovr 2b reports, in
 *         the gate's peek (G2) and skip_iou comparison (G3), and so in frt_track_assoc.ovr and frt_track_gate.ovr.  Nothing else reads it.
 *     M2. Velocity update, on every match (2a or 2b), of the track that won: g = missed at entry + 1;
 *         dcx = clamp((int64) (det.x1 + det.x2) - (trk.x1 + trk.x2), -2^22, 2^22), the doubled centre displacement from the last MEASURED
 *         box; raw_x = tdiv(dcx * 128, g).  If the track's hits at entry is 1 (the first match after the birth) vx = raw_x; otherwise
 *         vx = vx + tdiv((int64) (raw_x - vx) * gain, 256).  The same for y.  |v| <= 2^29 follows.  Then the match does what it always
 *         does: box = det.box, hits += 1, missed = 0.
 *     M3. Expiry zeroes the slot's velocity; a birth sets it to (0, 0).
 *     M4. The gate reads the velocities and writes none; with appearance off its peek is still the update's step 2, exactly.
 *     M5. Steps 3 to 8, the sums, the templates, the identity search and the sightings are unchanged.
 *     A track that was already live when motion is switched on starts from (0, 0) with hits > 1, so its first match takes the EMA branch
 *       and reaches only gain / 256 of the measured velocity.  That is intended: the switch does not pretend to a first measurement.
 *     Nobody has measured a gain on real video with this library: none is recommended here.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct frt_tracker frt_tracker;
typedef struct frt_track_options {
    float iou_threshold; /* default 0.3; (0, 1]                                                                        */
    int32_t max_missed;  /* default 5;   >= 0: updates a track may coast unseen                                        */
    int32_t min_hits;    /* default 3;   >= 1: matched detections (the birth included) that make a track `confirmed` */
    float decay;         /* default 1.0; (0, 1]: weight of the running sum against the new embedding                   */
} frt_track_options;
typedef struct frt_track_result {
    int32_t track_id, slot, age, hits, n_embeds, confirmed, match_idx;
    float match_sim;
} frt_track_result; /* 32 bytes */
typedef struct frt_track_state {
    int32_t live, id;
    frt_bbox box;
    int32_t born, hits, missed, n_embeds, match_idx;
    float match_sim;
} frt_track_state; /* 52 bytes: one slot as frt_tracker_tracks returns it; a free slot is all zero */
#define FRT_TRACK_ASSOC_ABSENT 0     /* the detection slot is not present */
#define FRT_TRACK_ASSOC_IOU 1        /* matched by overlap (step 2a) */
#define FRT_TRACK_ASSOC_APPEARANCE 2 /* matched by appearance (step 2b) */
#define FRT_TRACK_ASSOC_BIRTH 3      /* a new track (step 4) */
#define FRT_TRACK_ASSOC_UNTRACKED 4  /* no free slot (step 4) */
typedef struct frt_track_assoc {
    int32_t how; /* FRT_TRACK_ASSOC_* */
    int32_t gap; /* how 1, 2: the matched track's `missed` at entry; else 0 */
    float ovr;   /* how 1, 2: the IoU of the detection with the matched track's box at entry; else 0 */
    float sim;   /* how 1, 2: S[d][t] of the matched pair where DEFINED; else 0 */
} frt_track_assoc; /* 16 bytes */
#define FRT_TRACK_REID_OFF 2.0f     /* reid_threshold: step 2b does not run */
#define FRT_TRACK_MIN_SIM_OFF -2.0f /* iou_min_sim: step 2a excludes nothing */

/* options NULL: the defaults; a value outside its range is FRT_ERR_INVALID.  Creation itself does no device work: the state is allocated
 * and zeroed by the first call that passes its checks (a device that does not exist is FRT_ERR_DEVICE there). */
int frt_tracker_create(int n_streams, int max_tracks, int max_faces, int dim, const frt_track_options *options, int device, frt_tracker **out);
void frt_tracker_destroy(frt_tracker *t);
/* results_dev frt_face_result [n_frames][max_faces], embeds_dev float [n_frames][max_faces][dim], tracks_dev frt_track_result
 * [n_frames][max_faces], templates_dev float [n_frames][max_faces][dim] (may be NULL); m may be NULL (or hold no rows): no identity.
 * Asynchronous on hip_stream (a hipStream_t as void*, NULL = default stream), no host synchronisation. */
int frt_tracker_update_dev(frt_tracker *t, frt_matcher *m, const void *results_dev, const void *embeds_dev, int n_frames,
                           const int32_t *stream_ids /* host, may be NULL */, void *tracks_dev, void *templates_dev, void *hip_stream);
/* the same behind host pointers: upload, update, download, one synchronisation */
int frt_tracker_update(frt_tracker *t, frt_matcher *m, const frt_face_result *results, const float *embeds, int n_frames,
                       const int32_t *stream_ids, frt_track_result *tracks_out, float *templates_out /* may be NULL */);
/* "Appearance" above.  Takes effect with the next update (the settings travel with its launches); under the tracker's mutex, no device
 * work.  reid_threshold in (0, 1] or FRT_TRACK_REID_OFF, iou_min_sim in [-1, 1] or FRT_TRACK_MIN_SIM_OFF: anything else, a NaN included, is
 * FRT_ERR_INVALID and changes nothing.  frt_tracker_update_dev, frt_tracker_update and frt_pipeline_run_tracked honour the settings. */
int frt_tracker_set_appearance(frt_tracker *t, float reid_threshold, float iou_min_sim);
int frt_tracker_get_appearance(frt_tracker *t, float *reid_threshold_out, float *iou_min_sim_out);
/* "Motion" above.  gain 0 switches it off, 1 .. 256 on; anything else is FRT_ERR_INVALID and changes nothing.  Takes effect with the next
 * update or gate; under the tracker's mutex.  Off -> on zeroes the velocities: no device work while they do not exist yet, otherwise
 * synchronous behind the last queued update.  frt_tracker_update*, frt_tracker_gate*, frt_pipeline_run_tracked, _run_tracked_gated and
 * _run_sighted honour the setting. */
int frt_tracker_set_motion(frt_tracker *t, int gain);
int frt_tracker_get_motion(frt_tracker *t, int *gain_out);
/* one stream's velocities, after everything queued (like frt_tracker_tracks): vel_out int32 [max_tracks][2]; pred_out [max_tracks] (may be
 * NULL) M1's box of every slot for the NEXT update, all zero for a free slot.  FRT_ERR_INVALID while motion is off. */
int frt_tracker_motion(frt_tracker *t, int stream, int32_t *vel_out, frt_bbox *pred_out /* may be NULL */);
/* frt_tracker_update_dev / frt_tracker_update with how each detection was associated: assoc_dev / assoc_out frt_track_assoc
 * [n_frames][max_faces] (may be NULL: the call is then the plain one).  The same checks, all before any device work. */
int frt_tracker_update_assoc_dev(frt_tracker *t, frt_matcher *m, const void *results_dev, const void *embeds_dev, int n_frames,
                                 const int32_t *stream_ids /* host, may be NULL */, void *tracks_dev, void *templates_dev, void *assoc_dev,
                                 void *hip_stream);
int frt_tracker_update_assoc(frt_tracker *t, frt_matcher *m, const frt_face_result *results, const float *embeds, int n_frames,
                             const int32_t *stream_ids, frt_track_result *tracks_out, float *templates_out /* may be NULL */,
                             frt_track_assoc *assoc_out /* may be NULL */);
/* one stream's state, after everything queued on the streams the tracker has been updated on: slots_out [max_tracks] (every slot, live or
 * not), sums_out [max_tracks][dim] (may be NULL), counters_out [3] = next_id, tick, dropped (may be NULL) */
int frt_tracker_tracks(frt_tracker *t, int stream, frt_track_state *slots_out, float *sums_out, int32_t *counters_out);
/* frees the slots and zeroes tick / dropped of one stream (-1: of all); next_id is kept */
int frt_tracker_reset(frt_tracker *t, int stream);
/* frt_pipeline_run with the tracker behind it: the upload, frt_pipeline_run_dev on the pipeline stream, frt_tracker_update_dev on that same
 * stream with the pipeline's matcher, the downloads, one synchronisation.  results / embeds_out are frt_pipeline_run's, bit for bit;
 * tracks_out [n_frames][max_faces], templates_out [n_frames][max_faces][512] (may be NULL).  Serial under the pipeline's run mutex, like
 * frt_pipeline_run_photo_tiled.  The tracker's max_faces and dim must equal the pipeline's, n_frames <= max_frames, both on one device:
 * FRT_ERR_INVALID before any device work otherwise. */
int frt_pipeline_run_tracked(frt_pipeline *p, frt_tracker *t, const uint8_t *frames, int n_frames, const int32_t *stream_ids,
                             frt_face_result *results, frt_track_result *tracks_out, float *embeds_out /* may be NULL */,
                             float *templates_out /* may be NULL */);

/* Gate: skip the recogniser for the faces a confirmed track follows.  frt_pipeline_run_tracked embeds every face of every frame; on a video
 * stream a face that sat on a confirmed track one frame ago and overlaps its old box is the same person, and the track already carries a
 * template and an identity.  The gate runs between the detector and the recogniser and sorts the detections into those the recogniser must
 * see (EMBED) and those the tracker can follow by their boxes alone (FOLLOW).  The reference has no tracker, so the rules are fixed here, to
 * the integer (tests/track_gate_ref.py restates them in numpy).
 *   Options, frt_track_gate_options: refresh >= 1, min_embeds >= 1, skip_iou in (0, 1]; anything else, a NaN included, is FRT_ERR_INVALID
 *     before any device work.  There are NO defaults and no recommended values - nobody has measured these on real video with this library
 *     -: a NULL options pointer is FRT_ERR_INVALID.
 *   Per frame f of stream s; the gate reads the tracker's state AT ENTRY and writes no state.
 *     G1. detection d is PRESENT iff d < n_boxes[f] (when n_boxes is given) and box.score > 0 - step 1 of the update.
 *     G2. Peek - step 2 of the update, exactly, by overlap only (the appearance settings are ignored): present detections in slot order;
 *         candidates are the tracks live at entry and not yet taken by an earlier detection of this peek; ovr is the same float32 IoU; the
 *         largest ovr wins, the lowest slot among equals; a match needs ovr >= iou_threshold.  -> peek[d] (a slot, or -1) and ovr[d].
 *     G3. d is FOLLOWED iff peek[d] = t >= 0 and track t at entry has hits >= min_hits, n_embeds >= min_embeds, ovr[d] >= skip_iou and
 *         (hits + 1) % refresh != 0.  Every other present detection is EMBED; refresh == 1 therefore embeds everything.
 *     G4. One frt_track_gate per face slot: decision (0 absent, 1 EMBED, 2 FOLLOW); slot / ovr, the peek's, or -1 / 0 without a match; why,
 *         set only for EMBED, the OR of FRT_TRACK_GATE_NO_TRACK (no match), _UNCONFIRMED (hits < min_hits), _FEW_EMBEDS (n_embeds <
 *         min_embeds), _LOW_OVERLAP (ovr < skip_iou) and _REFRESH ((hits + 1) % refresh == 0: at refresh == 1 every matched detection
 *         carries it).  An absent slot is all zero with slot = -1.
 *   The work list: the face indices f * max_faces + d of the EMBED detections, ascending; n_embed of them; every entry behind them is -1.
 *     pass_count[j] = min(max_batch, max(0, n_embed - j * max_batch)) for j < ceil(n_frames * max_faces / max_batch): the faces of
 *     recogniser pass j, as frt_select_faces writes it.
 *   The peek is a PREDICTION, not a promise.  With appearance off it IS the update's step 2: the update that follows associates every
 *     present detection exactly as the peek said.  With appearance on, a FOLLOWED detection reaches the update with valid == 0: its S is
 *     never DEFINED, so it is never vetoed and never re-attached by appearance, and the update does with it what it always does with such a
 *     detection; the embedded ones take part in 2a / 2b as always, and the update - not the gate - decides.
 *   Staleness: a FOLLOWED face gets no frame-level match - its record has valid = 0, match_idx = -1, match_sim = 0 and keeps its box -; its
 *     identity is the track's, from the unchanged step 7, which searches the template rows on every call: a gallery edit still reaches a
 *     followed track in the next call.
 *   How much time a gated call saves depends on the stream; DESIGN 3.40 has what was measured. */
typedef struct frt_track_gate_options {
    int32_t refresh;    /* >= 1: a followed track is embedded again whenever (hits + 1) % refresh == 0; 1 embeds everything */
    int32_t min_embeds; /* >= 1: embeddings a track must hold before its faces may be followed                              */
    float skip_iou;     /* (0, 1]: overlap with the track's box below which the face is embedded                            */
} frt_track_gate_options;
#define FRT_TRACK_GATE_ABSENT 0
#define FRT_TRACK_GATE_EMBED 1
#define FRT_TRACK_GATE_FOLLOW 2
#define FRT_TRACK_GATE_NO_TRACK 1
#define FRT_TRACK_GATE_UNCONFIRMED 2
#define FRT_TRACK_GATE_FEW_EMBEDS 4
#define FRT_TRACK_GATE_LOW_OVERLAP 8
#define FRT_TRACK_GATE_REFRESH 16
typedef struct frt_track_gate {
    int32_t decision; /* FRT_TRACK_GATE_ABSENT / _EMBED / _FOLLOW */
    int32_t slot;     /* the peek's slot, or -1 */
    float ovr;        /* the peek's overlap, or 0 */
    int32_t why;      /* EMBED only: the OR of the reasons above; else 0 */
} frt_track_gate; /* 16 bytes */
/* The gate alone, asynchronous on hip_stream behind the tracker's last queued update: boxes_dev frt_bbox [n_frames][max_faces], n_boxes_dev
 * int32 [n_frames] (may be NULL), stream_ids on the host (may be NULL) -> gate_dev frt_track_gate [n_frames][max_faces], list_dev int32
 * [n_frames * max_faces], n_embed_dev int32 [1], pass_count_dev int32 [ceil(n_frames * max_faces / max_batch)].  max_batch >= 1.  The
 * checks are the update's, all before any device work; a refused call writes nothing. */
int frt_tracker_gate_dev(frt_tracker *t, const frt_track_gate_options *options, const void *boxes_dev, const void *n_boxes_dev, int n_frames,
                         const int32_t *stream_ids /* host, may be NULL */, void *gate_dev, void *list_dev, void *n_embed_dev,
                         void *pass_count_dev, int max_batch, void *hip_stream);
/* the same behind host pointers: upload, gate, download, one synchronisation */
int frt_tracker_gate(frt_tracker *t, const frt_track_gate_options *options, const frt_bbox *boxes, const int32_t *n_boxes /* may be NULL */,
                     int n_frames, const int32_t *stream_ids, frt_track_gate *gate_out, int32_t *list_out, int32_t *n_embed_out,
                     int32_t *pass_count_out, int max_batch);
/* frt_pipeline_run_tracked with the gate in front of the recogniser: upload, detector, gate, ONE host read of n_embed, gather crop (or
 * alignment, frt_pipeline_set_align) + recogniser over the n_embed listed faces in passes of the recogniser's max_batch, one top-1 search
 * of the compact rows (none when n_embed == 0 or there is no gallery), scatter into face slots, the records, the tracker's update with the
 * pipeline's matcher, the downloads, one synchronisation.  results / tracks_out / gate_out (may be NULL) [n_frames][max_faces], embeds_out
 * / templates_out [n_frames][max_faces][512] (may be NULL; a slot that was not embedded has a zero embedding row), crops_out
 * [*n_embed_out][112][112][3] (may be NULL; room for n_frames * max_faces crops) in LIST order.  The embeddings are those of passes cut from
 * the compact list: the same faces as frt_pipeline_run_tracked's, not bit for bit its embeddings.  Serial under the pipeline's run mutex
 * with whatever a pairing mode holds flushed first, like frt_pipeline_run_photo_tiled.  The checks are frt_pipeline_run_tracked's and the
 * options', all before any device work; a refused call writes nothing. */
int frt_pipeline_run_tracked_gated(frt_pipeline *p, frt_tracker *t, const frt_track_gate_options *options, const uint8_t *frames, int n_frames,
                                   const int32_t *stream_ids, frt_face_result *results, frt_track_result *tracks_out,
                                   frt_track_gate *gate_out /* may be NULL */, float *embeds_out /* may be NULL */,
                                   float *templates_out /* may be NULL */, uint8_t *crops_out /* may be NULL */, int32_t *n_embed_out);

/* ------------------------------------------------------------------------------------------------------------------
 * Face quality: is a face good enough to use?  Every route above takes pixels to identities and none asks.  /insert/face applies the
 * "exactly one face" rule and nothing else, so a 20-pixel, blurred or blown-out face is embedded and appended to the live gallery, where it
 * costs false matches for as long as it stays; the reply step of /inference sends one crop back (src/app.cpp:328) with no measure by which
 * a caller could pick or drop one.  These entry points score the u8 BGR 112x112 crops the pipeline already keeps in HBM
 * (frt_pipeline_submit_crops) and gate enrolment by the score.  The reference has no quality measure, so the semantics are fixed here, to
 * the integer (tests/quality_ref.py restates them in numpy): every answer is compared for equality, not within a tolerance.
 *   Per crop u8 [112][112][3], B G R:
 *     Y = (29 * B + 150 * G + 77 * R + 128) >> 8                                   luma, 0 .. 255 (the weights sum to 256)
 *     sum_y = sum Y, sum_y2 = sum Y * Y                                            over all N = 12544 pixels (both fit uint32)
 *     L = 4 * Y[r][c] - Y[r-1][c] - Y[r+1][c] - Y[r][c-1] - Y[r][c+1]              on the M = 12100 interior pixels (rows, columns 1 .. 110)
 *     sum_lap = sum L (int32), sum_lap2 = sum L * L (uint64: a 0 / 255 checkerboard gives 12 588 840 000)
 *     n_dark = #{Y < 32}, n_bright = #{Y > 223}
 *     mean      = float32(sum_y / 12544.0)
 *     luma_var  = float32((N * sum_y2 - sum_y^2) / float64(N^2))
 *     sharpness = float32((M * sum_lap2 - sum_lap^2) / float64(M^2))               the variance of the Laplacian
 *     The numerators are exact integers below 2^53 and the denominators are exact: one correctly rounded float64 division, one rounding to
 *     float32.
 *   With a record (frt_face_result) beside the crop: size = min(x2 - x1, y2 - y1) - the extents of the crop's ROI, as the gate of
 *     frt_pipeline_run_photo_tiled takes them - and score = box.score.  Without records size = 0 and score = 0.
 *   Presence: a slot is PRESENT iff there is no record array or its record has valid != 0 (the crops of unused and empty-ROI slots are
 *     unspecified).  An absent slot's record is all zero and its crop is not read.
 *   flags (frt_quality_flag): each comparison is strict as written - a value EQUAL to its threshold passes; SMALL and LOW_SCORE are
 *     evaluated only with records.  A face PASSES iff it is present and flags == 0.
 *   options NULL: {0, 0, 0, 0, 255, 12544, 0}, under which nothing can be flagged.  A negative min_size or max_clipped, a NaN, or
 *     min_mean > max_mean is FRT_ERR_INVALID before any device work.
 *   THERE ARE NO RECOMMENDED THRESHOLDS.  Nobody has measured these values on real faces with this library (the tests run on synthetic
 *     weights and synthetic faces): measure sharpness / luma_var / mean on your own cameras' accepted and rejected faces before gating.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct frt_quality_options {
    int32_t min_size;    /* default 0;     >= 0                                                                          */
    float min_sharpness; /* default 0                                                                                    */
    float min_luma_var;  /* default 0                                                                                    */
    float min_mean;      /* default 0;     <= max_mean                                                                   */
    float max_mean;      /* default 255                                                                                  */
    int32_t max_clipped; /* default 12544; >= 0: pixels that may be darker than 32 or brighter than 223, together        */
    float min_score;     /* default 0                                                                                    */
} frt_quality_options;
typedef enum frt_quality_flag {
    FRT_QUALITY_SMALL = 1,      /* size < min_size              (records only) */
    FRT_QUALITY_BLURRED = 2,    /* sharpness < min_sharpness                   */
    FRT_QUALITY_FLAT = 4,       /* luma_var < min_luma_var                     */
    FRT_QUALITY_DARK = 8,       /* mean < min_mean                             */
    FRT_QUALITY_BRIGHT = 16,    /* mean > max_mean                             */
    FRT_QUALITY_CLIPPED = 32,   /* n_dark + n_bright > max_clipped             */
    FRT_QUALITY_LOW_SCORE = 64  /* score < min_score            (records only) */
} frt_quality_flag;
struct frt_face_quality {
    uint32_t sum_y, sum_y2;               /* offsets  0,  4     */
    int32_t sum_lap;                      /*          8         */
    uint32_t n_dark, n_bright;            /*         12, 16     */
    int32_t size;                         /*         20         */
    uint64_t sum_lap2;                    /*         24         */
    float mean, luma_var, sharpness, score; /*       32, 36, 40, 44 */
    uint32_t flags;                       /*         48: frt_quality_flag bits */
    int32_t present;                      /*         52: 1 or 0 */
}; /* 56 bytes; an absent slot is all zero.  The record shares its name with the host entry point below, so there is no typedef:
    * the type is always written `struct frt_face_quality`, in C and in C++ */

/* crops_dev u8 [n][112][112][3] (16-byte aligned; read for the present slots only), results_dev frt_face_result [n] (may be NULL: every
 * slot is present, size = score = 0), options on the HOST (may be NULL, read before the call returns) -> quality_dev frt_face_quality [n]
 * (8-byte aligned), every record written.  One launch of one workgroup per slot, asynchronous on hip_stream (the current device's; a
 * hipStream_t as void*, NULL = default stream), no host synchronisation.  Checked before any device work: n < 0 or n > 1 048 576 is
 * FRT_ERR_CAPACITY; then the option ranges; n == 0 does nothing; a NULL or misaligned crops_dev / quality_dev is FRT_ERR_INVALID.  A
 * refused call writes nothing. */
int frt_face_quality_dev(const void *crops_dev, const void *results_dev /* may be NULL */, int n, const frt_quality_options *options /* host, may be NULL */,
                         void *quality_dev, void *hip_stream);
/* the same behind host pointers: upload (the crops, and the records when given), one launch, download, one synchronisation.  device < 0:
 * the current device.  The same checks, before any device work; a refused call leaves quality_out untouched. */
int frt_face_quality(const uint8_t *crops, const frt_face_result *results /* may be NULL */, int n, const frt_quality_options *options,
                     struct frt_face_quality *quality_out, int device);
/* frt_enrol_select_dev with the gate: quality_dev frt_face_quality [n_frames][max_faces] (may be NULL) as frt_face_quality_dev leaves it
 * for the call's results / crops.  A frame that would be FRT_ENROL_OK and whose SLOT 0 record has flags != 0 is FRT_ENROL_LOW_QUALITY
 * instead: face_dev gets its record as for OK, no row is appended.  The other slots' records are not looked at.  quality_dev NULL: exactly
 * frt_enrol_select_dev, which is unchanged.  Reads, writes and checks are frt_enrol_select_dev's. */
int frt_enrol_select_gated_dev(const void *results_dev, const void *embeds_dev, int n_frames, int max_faces, void *status_dev, void *face_dev,
                               void *rows_dev, void *count_dev, void *hip_stream, const void *quality_dev /* may be NULL */);
/* frt_pipeline_run that also scores every face slot: the upload, frt_pipeline_run_dev with the crop buffer on the pipeline stream, the
 * quality launch over [n_frames][max_faces] on that same stream, the downloads, one synchronisation.  results / embeds_out are
 * frt_pipeline_run's, bit for bit; crops_out [n_frames * max_faces][112][112][3] (may be NULL) is frt_pipeline_submit_crops's;
 * quality_out [n_frames * max_faces], an unused or empty-ROI slot all zero.  Serial under the pipeline's run mutex, like
 * frt_pipeline_run_tracked; whatever a pairing mode holds or has pending is flushed behind the call's stages, so the answers are those of
 * pairing off.  Checked before any device work: a NULL p / frames / results / quality_out and the option ranges are FRT_ERR_INVALID,
 * n_frames < 1 or > max_frames FRT_ERR_CAPACITY; a refused call writes nothing. */
int frt_pipeline_run_quality(frt_pipeline *p, const uint8_t *frames, int n_frames, const frt_quality_options *options, frt_face_result *results,
                             struct frt_face_quality *quality_out, float *embeds_out /* may be NULL */, uint8_t *crops_out /* may be NULL */);
/* frt_pipeline_enrol_images with the gate at the door: every chunk also leaves its crops on the device, the quality launch follows the
 * chunk's stages on the pipeline stream, and the gated selection follows that: a photo with exactly one valid face whose record carries a
 * flag is FRT_ENROL_LOW_QUALITY - faces_out[i] filled as for OK, no row added.  quality_out [n] (may be NULL) <- slot 0's record of photo i,
 * all zero when slot 0 is absent (no face, or an empty ROI).  Everything else - arguments, checks, the ONE edit, the error behaviour - is
 * frt_pipeline_enrol_images's; the option ranges are checked with the other arguments, before any device work.  options NULL flags
 * nothing: status, faces, rows and the gallery are then those of frt_pipeline_enrol_images (which is unchanged and computes no quality). */
int frt_pipeline_enrol_images_gated(frt_pipeline *p, const frt_face_image *images, int n, const int32_t *labels, const frt_quality_options *options,
                                    int32_t *status_out, frt_face_result *faces_out, struct frt_face_quality *quality_out /* [n], may be NULL */,
                                    float *embeds_out, int *first_row_out, int *n_enrolled_out);

/* ------------------------------------------------------------------------------------------------------------------
 * Sightings: one event per finished track, with its best shot.  (The section follows the gate in subject; it stands behind "Face quality"
 * because it uses that section's types.)  The tracker frees an expired slot by zeroing it (step 3) - id, hits, template and identity are
 * gone in that launch -, and the crop the quality record measured is overwritten by the next call.  A sighting book is attached to ONE
 * tracker and shadows every live track: it keeps each track's best shot - the crop, its embedding, the quality numbers - and, when the
 * track ends, appends one frt_sighting to a FIFO on the device that the host drains when it likes.  The reference has no tracker, so the
 * semantics are fixed here, to the integer (tests/sightings_ref.py restates them in numpy); every answer is compared for equality.
 *   Memory: n_streams * max_tracks + capacity rows of 96 + 8 * dim (+ 37 632 with keep_crops) bytes, allocated by the first call that
 *     passes its checks.  keep_crops = 0 is the setting for trackers with many streams: 1024 x 64 tracks with crops would be 2.5 GB.
 *   Beside every record, open or queued, sit two or three payload rows: best_embed float [dim], template float [dim] and - keep_crops -
 *     best_crop u8 [112][112][3].  The best_embed and best_crop rows of an entry with best_tick < 0 are zeros wherever they become visible.
 *   One book update follows ONE tracker update of the same frames and the same stream_ids: it reads the tracker's slots and ticks as that
 *     update left them.  This is a contract on the caller, not checked on the device (a slot index outside 0 .. max_tracks - 1 in tracks
 *     is skipped).  tick of a frame of stream s is counters[s].tick - 1, the tick the tracker update just used.  Frames of one call belong
 *     to pairwise distinct streams; they are independent except for the order of the queue.  Per frame f of stream s:
 *     S1. Close, slots t ascending: an open entry E[s][t] ends iff the tracker's slot is not (live != 0 and id == E.track_id); reason is
 *         FRT_SIGHTING_EXPIRED when live == 0, else _REPLACED (a birth of this same update took the slot step 3 had just freed);
 *         close_tick = tick.  E.hits < min_hits: discarded += 1, nothing is queued.  Otherwise, with fewer than capacity rows queued, the
 *         record and its payload rows are appended; else overflowed += 1 and the sighting is lost.  The entry is free in every case (all
 *         zero, its payload rows zero).  Queue order: frames in call order, then slots ascending.
 *     S2. Observe, detection slots d ascending with tracks[f][d].track_id >= 0, t = tracks[f][d].slot: a free entry opens - stream,
 *         track_id, first_tick = tick - age + 1, close_tick = -1, reason = 0, n_shots = 0, best_tick = -1, the best fields zero -; then
 *         last_tick = tick, and hits, n_embeds, confirmed, match_idx, match_sim are copied from tracks[f][d].  The template row becomes
 *         templates[f][d] when the call has templates, else it is left as it is (zeros if it was never written).
 *     S3. Best shot: a tracked detection is a CANDIDATE iff results[f][d].valid != 0 and quality[f][d].present != 0; n_shots += 1.  Its key
 *         is (quality.flags == 0, metric), metric = quality.sharpness (rank FRT_SHOT_RANK_SHARPNESS), quality.size (_SIZE) or quality.score
 *         (_SCORE).  It replaces the best shot iff best_tick < 0, or its pass bit is greater, or the pass bits are equal and its metric is
 *         strictly greater than the metric the best shot was taken with (a float or int32 comparison: a tie keeps the earlier shot, a NaN
 *         never replaces a shot that exists).  On replace: best_tick = tick, best_box = results.box, best_sharpness / _luma_var / _mean /
 *         _flags / _size = the record's, best_embed = embeds[f][d], best_crop = crops[f][d].
 *   The thresholds inside the quality options that produced `flags` are the caller's: THERE ARE NO RECOMMENDED THRESHOLDS ("Face quality").
 *   Every argument check runs before any device work; a refused call writes nothing and changes no state.  Every call takes the tracker's
 *     mutex; the book borrows the tracker and must be destroyed before it.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct frt_sightings frt_sightings;
#define FRT_SHOT_RANK_SHARPNESS 0
#define FRT_SHOT_RANK_SIZE 1
#define FRT_SHOT_RANK_SCORE 2
#define FRT_SIGHTING_EXPIRED 1
#define FRT_SIGHTING_REPLACED 2
#define FRT_SIGHTING_CLOSED 3
typedef struct frt_sighting_options {
    int32_t rank;        /* FRT_SHOT_RANK_SHARPNESS 0 | _SIZE 1 | _SCORE 2: what "best" means                  */
    int32_t min_hits;    /* >= 1: a track that ends with fewer hits is discarded (counted), not queued         */
    int32_t keep_crops;  /* 0 | 1: keep the u8 112x112x3 crop of the best shot (37 632 B per track and per queue row) */
} frt_sighting_options;   /* NULL: {0, 1, 1}; anything outside its range is FRT_ERR_INVALID */
typedef struct frt_sighting {       /* 96 bytes, every field 4 bytes, reserved words zero */
    int32_t stream, track_id;
    int32_t first_tick, last_tick;  /* the track's birth; the last update in which it had a detection */
    int32_t close_tick;             /* the update that saw it end; -1 while open */
    int32_t reason;                 /* 0 open, FRT_SIGHTING_EXPIRED 1, _REPLACED 2, _CLOSED 3 */
    int32_t hits, n_embeds, confirmed, match_idx;  float match_sim;   /* as the tracker last reported them */
    int32_t n_shots, best_tick;     /* candidates seen; tick of the best one, -1 without one */
    frt_bbox best_box;
    float best_sharpness, best_luma_var, best_mean;  uint32_t best_flags;  int32_t best_size;
    int32_t reserved;
} frt_sighting;

/* capacity 1 .. 65 536 (else FRT_ERR_CAPACITY): the rows of the queue.  n_streams, max_tracks, max_faces, dim and the device are the
 * tracker's.  Creation does no device work. */
int frt_sightings_create(frt_tracker *t, int capacity, const frt_sighting_options *options /* may be NULL */, frt_sightings **out);
void frt_sightings_destroy(frt_sightings *b);
/* One book update (S1 - S3) behind the tracker update of the same frames: results_dev frt_face_result, tracks_dev frt_track_result,
 * quality_dev struct frt_face_quality (8-byte aligned) [n_frames][max_faces]; embeds_dev, templates_dev (may be NULL) float
 * [n_frames][max_faces][dim], 16-byte aligned; crops_dev u8 [n_frames][max_faces][112][112][3], 16-byte aligned as frt_face_quality_dev
 * asks, required iff keep_crops (NULL without: FRT_ERR_INVALID either way round).  stream_ids on the host (may be NULL), checked as the
 * tracker checks them.  Two launches, asynchronous on hip_stream behind the tracker's last queued update, no host synchronisation; the
 * tracker's host forms then wait for it. */
int frt_sightings_update_dev(frt_sightings *b, const void *results_dev, const void *tracks_dev, const void *embeds_dev, const void *templates_dev,
                             const void *quality_dev, const void *crops_dev, int n_frames, const int32_t *stream_ids /* host, may be NULL */,
                             void *hip_stream);
/* the same behind host pointers: upload, update, one synchronisation */
int frt_sightings_update(frt_sightings *b, const frt_face_result *results, const frt_track_result *tracks, const float *embeds,
                         const float *templates /* may be NULL */, const struct frt_face_quality *quality, const uint8_t *crops, int n_frames,
                         const int32_t *stream_ids);
/* Ends every open entry of `stream` (-1: of every stream, ascending), slots ascending, with reason FRT_SIGHTING_CLOSED and close_tick =
 * last_tick; S1's rules for min_hits and capacity apply.  Synchronous, like frt_tracker_reset.  Meant for the end of a stream, or to be
 * called before frt_tracker_reset: without it the next update closes the entries as EXPIRED (REPLACED where a birth took the slot), with
 * first_tick / last_tick from before the reset.  A track
 * that goes on after a close opens a second sighting with the same track_id (first_tick is still the track's birth). */
int frt_sightings_close(frt_sightings *b, int stream);
/* The oldest min(queued, max_out) sightings in queue order, removed: records_out [max_out]; crops_out [max_out][112][112][3] (keep_crops
 * only, else it must be NULL), embeds_out, templates_out float [max_out][dim] - all three may be NULL -; *n_out of them are returned, the
 * rows of the output arrays at and behind *n_out are unspecified.  counters_out [4] (may be NULL): queued before the call, and the running
 * totals overflowed, discarded, closed (every entry that ended: queued, overflowed or discarded).  max_out >= 1.  Runs after everything
 * queued on the book; the rest keep their order and the room is free at once.  One synchronisation. */
int frt_sightings_drain(frt_sightings *b, int max_out, frt_sighting *records_out, uint8_t *crops_out, float *embeds_out, float *templates_out,
                        int *n_out, int32_t *counters_out);
/* The open entries of one stream, every slot, a free one all zero: records_out [max_tracks]; best_embeds_out, templates_out
 * [max_tracks][dim], crops_out [max_tracks][112][112][3] (keep_crops only) may be NULL.  One synchronisation. */
int frt_sightings_open(frt_sightings *b, int stream, frt_sighting *records_out, float *best_embeds_out, float *templates_out, uint8_t *crops_out);
/* frt_pipeline_run_tracked and frt_pipeline_run_quality in one call, with the book behind them, on the pipeline stream: the upload,
 * frt_pipeline_run_dev with the crop buffer, the quality launch, the tracker update with templates, the book update; the downloads, one
 * synchronisation.  results / tracks_out are frt_pipeline_run_tracked's and quality_out (may be NULL) frt_pipeline_run_quality's, bit for
 * bit; embeds_out may be NULL.  The checks are those two calls' plus one: b must belong to t.  Serial under the run mutex with pairing
 * flushed, like its parents.  frt_pipeline_run_tracked_gated has no sighted variant: a followed face has no crop to rank. */
int frt_pipeline_run_sighted(frt_pipeline *p, frt_tracker *t, frt_sightings *b, const frt_quality_options *quality, const uint8_t *frames,
                             int n_frames, const int32_t *stream_ids, frt_face_result *results, frt_track_result *tracks_out,
                             struct frt_face_quality *quality_out /* may be NULL */, float *embeds_out /* may be NULL */);

/* ------------------------------------------------------------------------------------------------------------------
 * Profiling hooks (HIP events on the library's own stream; used by bench.py for the roofline object).
 * ------------------------------------------------------------------------------------------------------------------ */
/* kinds: 0 = off (drops the records), 1 = time every launch of the dominant kernel family (conv3x3 MFMA), 2 = time every stage,
 * 3 = time the stages of every chunk of frt_matcher_cluster / frt_matcher_separation (two events per stage and chunk: size frt_profile_collect's arrays for them; the
 *     call creates the events it needs before its first chunk, and the records between the launches still slow it by about a sixth),
 * -1 = pause: stop recording but keep the records (bench.py samples ONE step of its timed region: the events around every conv
 * launch cost 11 % of a step when left on for all of them).  Every call with kind >= 0 also makes sure a pool of events exists, so that
 * no event is created between the two records of a bracket (call it with 0 once before a timed region). */
int frt_profile_enable(int kind);
/* Drains recorded events.  names_out: '\n'-separated labels; returns the number of records written (<= cap). */
int frt_profile_collect(char *names_out, size_t names_cap, double *ms_out, double *work_out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* FRT_H */
