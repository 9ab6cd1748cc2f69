// Internal declarations shared by the HIP translation units of libfrt.so (gfx950 only; no other targets, no shims).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/frt.h"
#include "frt_faces.hpp"

typedef _Float16 half_t;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

// One-time per-DEVICE setup of a kernel (hipFuncSetAttribute for > 64 KB of dynamic LDS is per device, not per process).
constexpr int FRT_MAX_DEVICES = 32;
inline bool frt_first_use_on_device(bool (&done)[FRT_MAX_DEVICES]) {
    int d = 0;
    (void)hipGetDevice(&d);
    d &= FRT_MAX_DEVICES - 1;
    if (done[d]) return false;
    done[d] = true;
    return true;
}

// ---------------------------------------------------------------- utilities (kernels_util.hip)
void launch_spin(double microseconds, hipStream_t s);  // one wave busy-waiting on the constant device clock
// sustained matrix-core rate probe (kernels_util.hip); returns the flop of the launch
double launch_mfma_probe(int mix, int n_wg, int iters, const void *src, float *out, hipStream_t s);

// ---------------------------------------------------------------- match (kernels_match.hip)
struct MatchPartial {  // one per (workgroup, query)
    float sim;
    int32_t idx;
};
// Every launcher that reads gallery rows is a template on their storage type GT, instantiated for float (the reference's row-major fp32
// layout) and half_t (the fp16-STORED gallery of BASELINE config 5, MFMA-fragment order; rows widened exactly to fp32 while they are staged).
// top-1 by the exact scan: rows [N][D], queries [F][D] fp32 -> idx[F], sim[F].  partial: scratch [grid][F].
template <typename GT>
void launch_match_top1(const GT *rows, int N, int D, const float *queries, int F, MatchPartial *partial, int partial_blocks, int32_t *idx_out,
                       float *sim_out, int row_offset, hipStream_t s);
int match_top1_blocks(int N, int F);
// full matrix: out[F][N]
template <typename GT>
void launch_match_full(const GT *rows, int N, int D, const float *queries, int F, float *out, hipStream_t s);
// screened search: shadow gallery (int8 or fp16) + coarse MFMA pass + exact re-rank of the few 32-row blocks that can hold the answer.
// What the host sizes the scratch by:
constexpr int FRT_MATCH_COARSE_WG = 256;  // persistent workgroups of the coarse scan (one per CU), each with at least one 128-row tile
constexpr int FRT_MATCH_SEL_SUB = 64;     // sub-lists of the candidate pair list (16 tile segments x 4 query classes), one counter each
constexpr int FRT_MATCH_CTL_WORDS = 32 + FRT_MATCH_SEL_SUB * 32;
struct MatchPair {                        // one entry of the candidate pair list
    int q, tile;  // tile: bits 0 - 27 the 128-row tile, bits 28 - 31 which of its four 32-row blocks are inside the band
};
constexpr int FRT_MATCH_PAIR_TILE_MASK = (1 << 28) - 1;
// ctl words: [FRT_MATCH_CTL_OVERFLOW] the pair list overflowed, [FRT_MATCH_CTL_SEG0 + s * FRT_MATCH_CTL_STRIDE] number of pairs in sub-list s
constexpr int FRT_MATCH_CTL_OVERFLOW = 1, FRT_MATCH_CTL_SEG0 = 32, FRT_MATCH_CTL_STRIDE = 32;
struct ScreenScratch {
    float *tilemax;               // [F][tiles][4] coarse maxima: one per 32-row block of a 128-row tile
    float *wgmax;                 // [FRT_MATCH_COARSE_WG][F] maxima of a workgroup's coarse entries
    void *pairs;                  // (query, tile) candidate pairs
    int pair_cap;                 // a multiple of FRT_MATCH_SEL_SUB
    int *ctl;                     // [FRT_MATCH_CTL_WORDS] control words: overflow flag, per-sub-list pair counts, one 128-byte line each (kernels_match.hip)
    unsigned long long *qkey;     // [F] packed (similarity, ~row) winners of the scalar re-rank
    // int8 shadow gallery (D = 512, fp32-stored galleries): null -> the fp16 shadow is scanned
    // Row g, column k (D = 512, ks = k >> 4) of the int8 shadow lives at byte
    //   ((((g >> 7) * 4 + ((g >> 5) & 3)) * (D / 32) + (ks >> 1)) * 64 + ((k >> 3) & 1) * 32 + (g & 31)) * 16 + (ks & 1) * 8 + (k & 7)
    // i.e. [128-row tile][32-row wave block][32-wide k pair][lane = (k half, row)][16 bytes = k-step 2p, k-step 2p + 1]; pad rows are 0x80, scale 0.
    const uint8_t *g8;            // fragment-ordered biased bytes (value + 128), gallery8_bytes(N, D)
    const float *g8_scale;        // [tiles * 128] per-row scale (row = scale * int8 row + error)
    float gerr;                   // max over rows of || row - scale * int8 row ||
};
size_t gallery8_bytes(int N, int D);
// fp32 rows -> int8 shadow (+ per-row scales, largest quantisation error norm^2 and largest row norm^2 as float bit patterns, atomicMax)
void launch_gallery_shadow8(const float *gallery, int N, int D, uint8_t *g8, float *scale, int *max_err2_bits, int *max_norm2_bits, hipStream_t s);
void launch_gallery_shadow(const float *gallery, int N, int D, half_t *g16, int *max_norm2_bits, hipStream_t s);
// exact top-k [F][k] through the screen, k = 1 being the top-1 search: one coarse scan, then k passes of the exact re-rank over the rows
// behind the previous winner.  The exact passes read `gallery`, or the stored fp16 rows g16 when gallery == nullptr.  Needs
// ceil(N / 128) >= FRT_MATCH_COARSE_WG; kth_scratch [F] floats (k > 1 only).
void launch_match_screened(const float *gallery, const half_t *g16, int N, int D, const float *queries, int F, int k, float gmax_norm,
                           const ScreenScratch &w, float *kth_scratch, MatchPartial *partial, int partial_blocks, int32_t *idx_out, float *sim_out,
                           int row_offset, hipStream_t s);
// exact top-k [F][k]: screen -> launch_match_screened, else k passes of the exact scan over the rows behind the previous winner
void launch_match_topk(const float *gallery, const half_t *g16, int N, int D, const float *queries, int F, int k, bool screen, float gmax_norm,
                       const ScreenScratch &w, float *kth_scratch, MatchPartial *partial, int partial_blocks, int32_t *idx_out, float *sim_out,
                       int row_offset, hipStream_t s);
int match_topk_max();
// The two front stages of the screened search on their own, for the clustering chunks: the coarse scan (true: it read the int8 shadow), and
// behind it the pairs whose 32-row block can hold a row with S >= threshold (absolute: not relative to the query's best entry), tiles from
// tile_min on.  Same scratch and same need of FRT_MATCH_COARSE_WG tiles as the screened search.
bool launch_match_coarse(const half_t *g16, int N, int D, const float *queries, int F, const ScreenScratch &w, hipStream_t s);
void launch_match_select_threshold(int N, int D, const float *queries, int F, float threshold, int tile_min, float gmax_norm, const ScreenScratch &w, bool i8,
                                   hipStream_t s);
// exact top-k over identities [F][k] (labels [N]: one int32 >= 0 per local row): kth_count > 0 -> one screened search whose selection hangs on
// the kth_count-th largest coarse entry (<= match_topk_max()), then k label-excluded re-rank passes; 0 -> k label-excluded exact scans
void launch_match_topk_labels(const float *gallery, const half_t *g16, int N, int D, const float *queries, int F, int k, int kth_count, float gmax_norm,
                              const ScreenScratch &w, float *kth_scratch, MatchPartial *partial, int partial_blocks, const int32_t *labels,
                              int32_t *label_out, int32_t *idx_out, float *sim_out, int row_offset, hipStream_t s);
void launch_half_to_float(const half_t *in, long n, float *out, hipStream_t s);
void launch_float_to_half(const float *in, long n, half_t *out, hipStream_t s);
void launch_merge_topk(const int32_t *idx_all, const float *sim_all, int shards, int n, int k, int32_t *idx_out, float *sim_out, hipStream_t s);
void launch_merge_topk_labels(const int32_t *label_all, const int32_t *idx_all, const float *sim_all, int shards, int n, int k, int32_t *label_out,
                              int32_t *idx_out, float *sim_out, hipStream_t s);
// The fp16 gallery (shadow or stored) is kept in MFMA-fragment order and padded to whole 128-row tiles (see kernels_match.hip):
size_t gallery16_elems(int N, int D);
// Row g, column k of it lives at
//   ((((g >> 7) * 4 + ((g >> 5) & 3)) * (D / 16) + (k >> 4)) * 64 + ((k >> 3) & 1) * 32 + (g & 31)) * 8 + (k & 7)
// i.e. [128-row tile][32-row wave block][16-wide k step][lane = (k half, row)][8 halfs].  (Row-major rows made a lane of the coarse scan fetch
// 16 bytes of its own 1 KB row per instruction: 32 different lines per load, each line requested four times - both earlier coarse kernels
// stalled at 4.0 TB/s on it.)  Pad rows are zero.
__device__ __forceinline__ long g16_index(long g, int k, int D) {
    return ((((g >> 7) * 4 + ((g >> 5) & 3)) * (long)(D >> 4) + (k >> 4)) * 64 + ((k >> 3) & 1) * 32 + (g & 31)) * 8 + (k & 7);
}
// four columns k .. k + 3 (k % 4 == 0) of stored row g as fp32, whichever the storage type (fp16 values widen exactly)
__device__ __forceinline__ floatx4 load_g4(const float *G, long g, int D, int k) { return *reinterpret_cast<const floatx4 *>(G + g * D + k); }
__device__ __forceinline__ floatx4 load_g4(const half_t *G, long g, int D, int k) {  // (four columns never straddle an 8-group)
    const half4 h = *reinterpret_cast<const half4 *>(G + g16_index(g, k, D));
    return floatx4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}
// S(query, stored row g) with the bits of the exact scan: the k order of match_kernel's MFMA chain - per 8 columns, k = 8 ks + s (lanes 0-31
// of the MFMA) then k = 8 ks + 4 + s (lanes 32-63) - and one fused multiply-add per term.  q: the query's D floats (LDS or global).  The
// pair re-rank (kernels_match.hip) and the genuine pass (kernels_separation.hip) both call this; the chain itself stays sequential, the
// unroll keeps 16 row loads in flight per thread.
template <typename GT>
__device__ __forceinline__ float exact_row_dot(const GT *__restrict__ G, long g, int D, const float *q) {
    float acc = 0.f;
#pragma unroll 8
    for (int k0 = 0; k0 < D; k0 += 8) {
        const floatx4 a = load_g4(G, g, D, k0), b = load_g4(G, g, D, k0 + 4);
        const floatx4 x = *reinterpret_cast<const floatx4 *>(q + k0), y = *reinterpret_cast<const floatx4 *>(q + k0 + 4);
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) {
            acc = __builtin_fmaf(a[s2], x[s2], acc);
            acc = __builtin_fmaf(b[s2], y[s2], acc);
        }
    }
    return acc;
}
bool match_screen_supported(int D);  // D the coarse kernel is instantiated for
// fp32 rows [n_rows][D] (first row = global row row0) -> their place in the fp16 gallery (whose rows never written must be zero)
void launch_rows_to_half(const float *in, long row0, long n_rows, int D, half_t *g16, hipStream_t s);
// largest squared row norm of rows [row0, row0 + n_rows) as a float bit pattern (all an fp16-stored gallery needs: it is its own shadow)
template <typename GT>
void launch_rows_norm(const GT *G, int row0, int n_rows, int D, int *max_norm2_bits, hipStream_t s);
// live gallery edits (frt_matcher_gallery_add / _remove): row-range forms of the shadow build, and the gather half of the chunked in-place
// compaction (keys / klo / khi: frt_holes.h; the bounce buffer receives the chunk in its final layout, a copy on the same stream places it)
void launch_gallery_shadow8_rows(const float *rows, int row0, int n_rows, uint8_t *g8, float *scale, int *max_err2_bits, int *max_norm2_bits, hipStream_t s);
void launch_gather_rows(const float *G, int D, int a, int n_rows, const int *keys, int klo, int khi, float *bounce, hipStream_t s);
void launch_gather_rows16(const half_t *G, int D, long tile0, long n_tiles, int n_new, const int *keys, int klo, int khi, half_t *bounce, hipStream_t s);

// ---------------------------------------------------------------- clustering (kernels_cluster.hip; frt_matcher_cluster)
// Single linkage at a similarity threshold t on a union-find forest parent[N] (parent[x] <= x: a component's root is its smallest row).
// stats: 4 x int64 on the device = clusters, joined pairs, screened chunks, dense chunks.
void launch_cluster_init(int32_t *parent, int N, long long *stats, hipStream_t s);
// n stored rows from row0 on -> fp32 row-major queries [n][D] (fp16 storage: the fragment-ordered rows widened exactly)
void launch_cluster_queries(const half_t *rows, int row0, int n, int D, float *out, hipStream_t s);
// screened chunk: the pairs launch_match_select_threshold listed for queries = rows q_row0 .. of the gallery; every live row j > i with
// S(i, j) >= t is united with i.  rows / N: the whole gallery; the list's tile numbers count from tile_origin (where the coarse scan and the
// selection of this chunk began).  Does nothing when the pair list overflowed; chunk_overflow receives that flag.
template <typename GT>
void launch_cluster_rerank_union(const GT *rows, int N, int D, const float *queries, int q_row0, int tile_origin, const ScreenScratch &w, float t,
                                 int32_t *parent, long long *stats, int *chunk_overflow, hipStream_t s);
// dense chunk: full [F][N] = the similarities of queries = rows q_row0 .. q_row0 + F - 1 (match_kernel's out_full); same joins
void launch_cluster_dense_union(const float *full, int F, int N, int q_row0, float t, int32_t *parent, long long *stats, hipStream_t s);
// label[i] = root(i); stats[0] = number of roots, stats[2] / stats[3] = the host's chunk counts
void launch_cluster_flatten(const int32_t *parent, int N, int32_t *labels, long long *stats, long long screened_chunks, long long dense_chunks,
                            hipStream_t s);

// ---------------------------------------------------------------- separation (kernels_separation.hip; frt_matcher_separation)
constexpr int FRT_SEPARATION_MAX_THRESHOLDS = 64;
// Impostor side (kernels_match.hip).  launch_match_select_kth: the selection stage behind launch_match_coarse, pairs under every query's
// kth_count-th largest coarse entry (kth_scratch [F] floats).  launch_match_top1_excluding: one label-excluded top-1 search, query q leaving
// out the rows labelled excluded[q].  screened: the re-rank stage behind those two, *overflow_out (device) = the pair list overflowed and the
// gated exact scan answered; otherwise one label-excluded exact scan, overflow_out untouched.  idx_out / sim_out [F] (local rows).
void launch_match_select_kth(int N, int D, const float *queries, int F, int kth_count, float gmax_norm, const ScreenScratch &w, float *kth_scratch, bool i8,
                             hipStream_t s);
void launch_match_top1_excluding(const float *gallery, const half_t *g16, int N, int D, const float *queries, int F, bool screened, const ScreenScratch &w,
                                 MatchPartial *partial, int partial_blocks, const int32_t *labels, const int32_t *excluded, int32_t *idx_out, float *sim_out,
                                 int *overflow_out, hipStream_t s);
// Genuine side: for every row the best OTHER row of its identity by the exact similarity (first maximum; NaN is no candidate; -inf / -1
// without one).  group_off [I + 1] / group_rows [N]: frt_templates.hpp; pos_ident [N]: the identity of position p of group_rows.
template <typename GT>
void launch_separation_genuine(const GT *rows, int N, int D, const int *group_off, const int *group_rows, const int *pos_ident, float *gen_sim,
                               int32_t *gen_row, hipStream_t s);
// stats [5] and counts [n_thresholds][2] (device, int64; zeroed here) from the four arrays; thresholds: host memory, read before this returns.
// chunk_overflow [chunks]: the impostor searches' flags (read when screened; otherwise every chunk counts as an exact scan).
void launch_separation_reduce(const float *gen_sim, const int32_t *gen_row, const float *imp_sim, const int32_t *imp_row, int N, const float *thresholds,
                              int n_thresholds, const int *chunk_overflow, int chunks, bool screened, long long *counts, long long *stats, hipStream_t s);

// ---------------------------------------------------------------- template gallery (kernels_templates.hip)
// One template per identity (include/frt.h, frt_matcher_build_templates).  rows: the stored gallery (fp32 row-major or fragment-ordered fp16);
// identity i owns the LOCAL rows group_rows[group_off[i] .. group_off[i + 1]), ascending (frt_templates.hpp).  -> templates [I][D] fp32,
// min_sim [I], min_row [I] (row_offset added).
template <typename GT>
void launch_template_build(const GT *rows, int D, const int *group_off, const int *group_rows, int I, int row_offset, float *templates, float *min_sim,
                           int32_t *min_row, hipStream_t s);

// ---------------------------------------------------------------- post-processing (kernels_post.hip)
constexpr int DET_MAX_LEVELS = 4, DET_MAX_SIZES = 3;
struct DetGeom {  // anchor table of one detector (mnet: 3 levels x 2 sizes; Slim / RFB: 4 levels x 3/2/2/3 sizes)
    int in_w, in_h, frame_w, frame_h;
    int levels;
    int fw[DET_MAX_LEVELS], fh[DET_MAX_LEVELS];  // feature-map sizes per level (ceil(dim/step))
    int base[DET_MAX_LEVELS];                    // first anchor index per level
    int nsz[DET_MAX_LEVELS];                     // anchor sizes per cell
    int min_size[DET_MAX_LEVELS][DET_MAX_SIZES];
    float step[DET_MAX_LEVELS];
    int A;                 // anchors per frame
    float scale_w, scale_h;
    float nms_thr, bbox_thr;
    int max_faces;
};
// The DetGeom of one detector (host, frt_detector.cpp): family 1 = the mnet table over `levels` = 3 levels, any other family = the Slim / RFB
// table over 4; steps 8 << level, feature maps ceil(dim / step).  frt_detector_create calls it, and so does tests/cpp/det_tail_check.cpp.
DetGeom det_geometry(int family, int levels, int in_w, int in_h, int frame_w, int frame_h, float nms_threshold, float bbox_threshold, int max_faces);
struct Candidate {
    frt_bbox box;
    int32_t anchor;
};
void launch_decode(const float *loc, const float *conf, int n_frames, const DetGeom &g, Candidate *cand, int *cand_count, hipStream_t s);
void launch_nms(Candidate *cand, const float *loc, int *cand_count, int n_frames, const DetGeom &g, uint8_t *dead, frt_bbox *out, int *n_out,
                int *kept_anchor, hipStream_t s);
// landmarks of the kept boxes: raw head output ldm [B][A][10] + kept anchors [B][K] -> frame coordinates (x0,y0,...,x4,y4) [B][K][10]
void launch_landmark_decode(const float *ldm, const int *kept_anchor, const int *n_out, int n_frames, const DetGeom &g, float *out, hipStream_t s);
// 5-point similarity alignment (ArcFace 112x112 template) + bilinear warp, fused with the recogniser's normalisation
void launch_align_faces(const uint8_t *frames, int frame_h, int frame_w, size_t row_stride, size_t frame_stride, const float *landmarks,
                        const int *n_boxes, int max_faces, int F, int frames_shared, uint8_t *crops, float *chw, int *valid, hipStream_t s);

// ---------------------------------------------------------------- image ops (kernels_image.hip)
// u8 BGR frames [n][frame_h][frame_w][3] (row_stride / frame_stride in bytes) -> fp32 planar [n][3][in_h][in_w]
void launch_det_preprocess(const uint8_t *frames, int n, int frame_h, int frame_w, size_t row_stride, size_t frame_stride, int in_h,
                           int in_w, float *out, hipStream_t s);
// per face slot f: box = boxes[f]; valid iff f%max_faces < n_boxes[f/max_faces] (n_boxes == nullptr: all valid) and ROI non-empty.
// writes u8 BGR crops [F][oh][ow][3] (may be null), fp32 planar RGB normalised [F][3][oh][ow], valid flags [F].
void launch_crop_faces(const uint8_t *frames, int frame_h, int frame_w, size_t row_stride, size_t frame_stride, const frt_bbox *boxes,
                       const int *n_boxes, int max_faces, int F, int frames_shared, int oh, int ow, uint8_t *crops, float *chw, int *valid,
                       hipStream_t s);
// The gather forms of launch_crop_faces (112 x 112) and launch_align_faces, the same arithmetic: face j < *count (device) of the launch is
// face i = list[j] of a call of n_slots = n_frames * max_faces slots - frame i / max_faces, boxes[i] / landmarks[i] - and is written at the
// compact position j of crops (may be null) / chw / valid.  cap: the faces the grid covers; positions *count .. cap - 1 are left alone.
void launch_crop_faces_gather(const uint8_t *frames, int frame_h, int frame_w, size_t row_stride, size_t frame_stride, const frt_bbox *boxes,
                              const int32_t *list, const int32_t *count, int max_faces, int n_slots, int cap, uint8_t *crops, float *chw, int *valid,
                              hipStream_t s);
void launch_align_faces_gather(const uint8_t *frames, int frame_h, int frame_w, size_t row_stride, size_t frame_stride, const float *landmarks,
                               const int32_t *list, const int32_t *count, int max_faces, int n_slots, int cap, uint8_t *crops, float *chw, int *valid,
                               hipStream_t s);
// n frames u8 HWC [sh][sw][3] -> [dh][dw][3], cv::resize INTER_LINEAR semantics (frame ingest, app.cpp:301)
void launch_resize_linear(const uint8_t *src, int n, int sh, int sw, size_t sstride, size_t sframe, uint8_t *dst, int dh, int dw, size_t dstride,
                          size_t dframe, hipStream_t s);
void launch_face_normalize(const uint8_t *crops, int F, int oh, int ow, float *chw, hipStream_t s);
// F face images of any size, tightly packed in `arena` at desc[f] (frt_faces.hpp) -> cv::resize INTER_LINEAR to 112x112 + preprocessFace:
// u8 BGR crops [F][112][112][3] and fp32 planar RGB [F][3][112][112], either may be null
void launch_faces_prepare(const uint8_t *arena, const frt_face_desc *desc, int F, uint8_t *crops, float *chw, hipStream_t s);
// the same kernel for whole photos: n images of any size at desc[i] of `arena` -> cv::resize INTER_LINEAR to dh x dw, u8 BGR [n][dh][dw][3]
void launch_images_resize(const uint8_t *arena, const frt_face_desc *desc, int n, int dh, int dw, uint8_t *out, hipStream_t s);

// ---------------------------------------------------------------- large photos by tiles (kernels_tiles.hip; semantics: include/frt.h)
// grid tiles (kind 0) of tiles[0 .. n_tiles) cut from the photo into out [n_tiles][tile_rows][tile_cols][3], 128 outside the photo; the slot of
// a kind 1 tile is left alone (launch_images_resize writes it).  out must be 16-byte aligned.
void launch_cut_tiles(const uint8_t *photo, int rows, int cols, size_t row_stride, const frt_tile *tiles, int n_tiles, int tile_rows, int tile_cols,
                      uint8_t *out, hipStream_t s);
// boxes [n_tiles][slots] in tile coordinates -> out / src_out [max_out], n_out: map + cut test, sort, suppression bit matrix, one wave's scan.
// 1 <= n_tiles * slots <= 16384.  Scratch per candidate: keys, mbox, order; mask: tile_merge_mask_words(n_tiles * slots) words.
struct TileMergeArgs {
    const frt_bbox *boxes;
    const int32_t *n_boxes;
    const frt_tile *tiles;
    int n_tiles, slots, photo_rows, photo_cols, tile_rows, tile_cols, metric, drop_cut;
    float thr;
    int max_out;
    unsigned long long *keys;
    frt_bbox *mbox;
    int *order;
    unsigned long long *mask;
    frt_bbox *out;
    int32_t *src_out;
    int *n_out;
};
size_t tile_merge_mask_words(int candidates);
void launch_tile_merge(const TileMergeArgs &a, hipStream_t s);
// landmarks of the kept boxes: ldm [n_tiles][slots][10] in tile coordinates -> out [max_out][10] in photo coordinates
void launch_tile_landmarks(const float *ldm, const frt_tile *tiles, const int32_t *src, const int *n_out, int slots, int max_out, int photo_rows,
                           int photo_cols, int tile_rows, int tile_cols, float *out, hipStream_t s);
// the recogniser's work list out of a merged list: boxes / src (may be null) / ldm (may be null) [cap] with *n_in entries (device,
// clamped to 0 .. cap) -> the boxes with min(x2 - x1, y2 - y1) >= min_face (min_face <= 0: all), dense and in order, in boxes_kept / src_kept
// (with src) / ldm_kept (with ldm) / keep_pos [cap], zeros / -1 behind *n_kept; pass_count [ceil(cap / max_batch)] <- faces per pass of
// max_batch.  One workgroup, cap <= 16384 is what the callers allow (any cap >= 0 works), max_batch >= 1.  Inputs and outputs must not overlap.
void launch_tile_faces_select(const frt_bbox *boxes, const int32_t *src, const float *ldm, const int *n_in, int cap, int min_face, int max_batch,
                              frt_bbox *boxes_kept, int32_t *src_kept, float *ldm_kept, int32_t *keep_pos, int *n_kept, int32_t *pass_count,
                              hipStream_t s);

// ---------------------------------------------------------------- the "exactly one face" rule of /insert/face (kernels_enrol.hip)
// results [n_frames][max_faces], embeds [n_frames][max_faces][512] -> status [n_frames] (frt_enrol_status), face_out [n_frames] (may be
// null), the OK frames' embeddings to rows[*count ...], *count advanced; one workgroup.  quality [n_frames][max_faces] (may be null): an OK
// frame whose slot 0 record carries a flag is FRT_ENROL_LOW_QUALITY instead and adds no row
void launch_enrol_select(const frt_face_result *results, const float *embeds, int n_frames, int max_faces, int32_t *status, frt_face_result *face_out,
                         float *rows, int32_t *count, hipStream_t s, const struct frt_face_quality *quality = nullptr);

// ---------------------------------------------------------------- face quality (kernels_quality.hip; frt_quality.cpp, include/frt.h "Face quality")
// crops u8 [n][112][112][3] (16-byte aligned), results [n] (may be null: every slot present) -> out [n], every record written; one
// workgroup per slot; n < 1 launches nothing
void launch_face_quality(const uint8_t *crops, const frt_face_result *results, int n, const frt_quality_options &opt, struct frt_face_quality *out,
                         hipStream_t s);

// ---------------------------------------------------------------- detector network (kernels_det.hip), fp32 NCHW
struct DwPwArgs {
    const float *in; float *out;
    const float *wd, *bd;   // depthwise [Cin][9], bias [Cin] (BN folded); null wd -> plain 1x1 conv
    const float *wp, *bp;   // pointwise, TRANSPOSED [Cin][Cout], bias [Cout]
    const float *add;       // optional tensor to add after ReLU, nearest-upsampled from [B][Cout][add_h][add_w]
    int add_h, add_w;
    int B, Cin, H, W, Cout, Ho, Wo, stride, relu;
    float *tmp;             // scratch [B][Cin][Ho][Wo] for the split depthwise -> pointwise path (null: always fused)
    const float *wd12;      // depthwise weights packed [Cin][12] = 9 taps, bias, 2 pad (matrix-core kernel); null: scalar kernels only
    const half_t *wph;      // pointwise weights as fp16 hi/lo split [Cout][Cin/16][hi16 | lo16] (Cin % 16 == 0); null: fp32 MFMA path
    const float *wdp;       // depthwise weights of channel pairs [Cin/2][10][2] (kernels_det_wave.hip); null: that kernel does not apply
    const half_t *wpf;      // the split pointwise weights in fragment order [Cin/16][Cout/32][hi|lo][64][8] (kernels_det_wave.hip)
    const float *wdt;       // the same depthwise weights tap-major [10][Cin/2][2] (tap 9 = bias; kernels_det_stem.hip); Cin <= 16 only
    const float *stem;      // 8 -> 16 block only: the gathered weights of the fused stem kernel (det_stem_pack, kernels_det_stem.hip); null: not fused
    const float *zeros;     // dwpw_wave_zero_bytes() of zeros (kernels_det_wave.hip: the source of input rows outside the image)
};
size_t dwpw_wave_zero_bytes();
bool launch_dwpw_wave(const DwPwArgs &a, hipStream_t s);  // one wave = 64 pixels x all channels (round 4); false: shape not covered
void launch_dwpw(const DwPwArgs &a, hipStream_t s);
bool launch_dwpw_mfma(const DwPwArgs &a, hipStream_t s);  // false: shape not covered, use the scalar kernels
struct Conv3Args {
    const float *in; float *out;
    const float *w, *b;     // [Cin][9][Cout] (transposed), bias [Cout]
    int B, Cin, H, W, Cout, Ho, Wo, stride, relu;
    int out_ctotal, out_coff;  // write into channels [coff, coff+Cout) of a [B][ctotal][Ho][Wo] tensor
    const half_t *wh;          // matrix-core path, optional: fp16 hi/lo split weights [Cin/16][9][64][hi16|lo16] (kernels_det_conv3h.hip); null: scalar kernels only
    float *out2;               // channels >= split go to out2 (channel co - split of a [B][out2_ctotal][Ho][Wo] tensor, + out2_coff)
    int split, out2_ctotal, out2_coff;
};
void launch_conv3x3(const Conv3Args &a, hipStream_t s);
// the detector's first three layers in one kernel (kernels_det_stem.hip); false: not applicable, run them one by one
size_t det_stem_weight_floats();
void det_stem_pack(const Conv3Args &c, const DwPwArgs &d1, const DwPwArgs &d2, float *dst, hipStream_t s);
bool launch_det_stem(const uint8_t *frames, size_t row_stride, size_t frame_stride, const Conv3Args &c, const DwPwArgs &d1, const DwPwArgs &d2, hipStream_t s);
// first detector conv fed by the u8 frames directly (only valid when the letterbox is the identity); false: not applicable
bool launch_det_conv1_u8(const uint8_t *frames, size_t row_stride, size_t frame_stride, const Conv3Args &a, hipStream_t s);
bool launch_conv3x3_split(const Conv3Args *a, int n, hipStream_t s);  // fp16 hi/lo split MFMA version (stride 1, Cin 64 or 16); false: n/a, use the scalar kernels
void launch_conv3x3_multi(const Conv3Args *a, int n, hipStream_t s);  // up to 3 same-Cout problems in one launch
struct HeadArgs {
    const float *in;        // [B][64][H][W]
    const float *wb, *bb;   // bbox head [64][8], [8]
    const float *wc, *bc;   // class head [64][4], [4]
    float *loc, *conf;      // [B][A][4], [B][A][2]
    int B, C, H, W, A, base;
    const float *wl, *bl;   // optional landmark head [64][20], [20] (null: trimmed network, the reference's default)
    float *ldm;             // [B][A][10]
};
void launch_heads(const HeadArgs &a, hipStream_t s);
void launch_heads_multi(const HeadArgs *a, int n, hipStream_t s);

// ---------------------------------------------------------------- Slim / RFB detector parts (kernels_det_slim.hip), fp32 NCHW
struct SlimHeadArgs {       // one of pyramid levels 0-2: the loc / conf / landm depth_conv2d heads (dw3x3 + bias -> ReLU -> 1x1 + bias)
    const float *in;        // [B][C][H][W]
    const float *wd;        // [C][3 heads][9 taps + bias]
    const float *wp, *bp;   // [C][48], [48]: loc 4*3 | conf 2*3 | ldm 10*3 (zero beyond the level's na anchors)
    int C, H, W, na, base;  // na anchors per cell, first anchor index of the level
};
struct SlimHeadsArgs {
    SlimHeadArgs lv[3];
    float *loc, *conf, *ldm;  // [B][A][4], [B][A][2] (softmax), [B][A][10]; ldm null: no landmark heads
    int B, A;
};
void launch_slim_heads(const SlimHeadsArgs &a, int n, hipStream_t s);
struct DenseHeadArgs {      // last level: dense 3x3 (pad 1) C -> cout = na*(4 + 2 [+ 10]) + bias, channels loc | conf | ldm
    const float *in;        // [B][C][H][W]
    const float *w, *b;     // [C][9][cpad] (cpad = cout rounded up to 16, zero-padded), [cpad]
    float *loc, *conf, *ldm;
    int B, C, H, W, na, cout, cpad, A, base;
};
void launch_dense_head(const DenseHeadArgs &a, hipStream_t s);
struct RfbProjArgs {        // BasicRFB's 1x1 convs of x (64 channels): branch reductions 3 x 8 -> red [B][24], shortcut 64 -> sc [B][64]
    const float *in;
    const float *w, *b;     // [64][88] (24 reductions | 64 shortcut), [88]; BN folded
    float *red, *sc;
    int B, H, W;
};
void launch_rfb_proj(const RfbProjArgs &a, hipStream_t s);
struct RfbConvArgs {        // 3x3, stride 1, dilation = padding = dil; reads channels [in_coff, +Cin) of a [B][in_ctotal] tensor
    const float *in; float *out;
    const float *w, *b;     // [Cin][9][16], [16] (Cout <= 16, zero-padded); BN folded
    int Cin, Cout, dil, relu, in_ctotal, in_coff, out_ctotal, out_coff;
};
struct RfbConvMulti {       // up to 3 problems on the same H x W (blockIdx.z)
    RfbConvArgs p[3];
    int B, H, W;
};
void launch_rfb_conv(const RfbConvMulti &a, int n, hipStream_t s);
struct RfbTailArgs {        // relu((ConvLinear 48 -> 64 + BN) * scale + shortcut)
    const float *cat;       // [B][48][H][W]
    const float *w, *b;     // [48][64], [64]
    const float *sc;        // [B][64][H][W]
    float *out;
    float scale;
    int B, H, W;
};
void launch_rfb_tail(const RfbTailArgs &a, hipStream_t s);

// ---------------------------------------------------------------- recogniser network (kernels_arc.hip), fp16 NHWC + MFMA
// Precondition of every launch below: the activation tensors (x, sc, scx, out0, out1) live in buffers of the embedder's sizes - F * 112 * 112 * 64
// halves for a pass of at most F faces (F * 28 * 28 * 128 for a shortcut conv's output; frt_embedder::alloc_act_set).  Strip kernels compute
// whole pixel tiles, so a compact strip READS pixel slots of images behind the batch; what it reads there is never stored, and nothing is
// written outside the logical outputs (tests/test_gpu_arc_launches.py runs every planned launch alone on such buffers).  A launch with the SE
// scratch (se_pool, se_counter) gets the embedder's too: F * 512 * 4 floats of partial sums, then F arrival counters and, se_flag_off = F ints behind
// them, F gate-ready flags; counters at zero, flags at no epoch still to come.  The fused tail (EPI_BN_SE) writes se_pool[part][face][channel] for
// the strips of a face, leaves every counter at zero and every flag at se_epoch, and touches no other word of it (the same test, fused cases).
enum { EPI_PRELU = 0, EPI_BN = 1, EPI_BN_ADD_BN = 2, EPI_PARTIAL = 3, EPI_BN_SE = 4 };  // EPI_BN_SE: BN -> SE gate -> + shortcut -> BN_next (IR-SE unit tail)
struct ConvMfmaArgs {
    const half_t *x;   // [B][H][W][Cin]
    const half_t *w;   // [Cout][ks*ks*Cin]
    const half_t *wf;  // optional fragment-ordered copy for the strip kernel: [Cout/32][Cin/64][9][4][64 lanes][8] (3x3, Cin % 64 == 0); null: none
    const half_t *wf2; // same for the stride-2 strip kernel (kernels_arc_s2.hip): taps in ITS step order 0,2,6,8,4,1,7,3,5; null: none
    int B, H, W, Cin, Ho, Wo, Cout, ks, stride, pad;
    int mode;
    const float *p0, *p1, *p2, *p3;
    const half_t *sc;  // shortcut tensor [B][sc_h][sc_w][Cout], sampled at (oh*sc_stride, ow*sc_stride)
    int sc_h, sc_w, sc_stride;
    // fused 1x1 stride-2 shortcut CONVOLUTION (stride-2 strip kernel, mode EPI_BN_ADD_BN, instead of `sc`): out = BN(conv3x3(x)) + BNsc(conv1x1_s2(scx))
    const half_t *scx;   // the unit's raw input [B][H][W][Csc]; null: shortcut tensor `sc`
    const half_t *wscf;  // 1x1 weights in fragment order [Cout/32][Csc/64][4 kk][64 lanes][8]
    const float *psc0, *psc1;  // the shortcut's folded BatchNorm
    int Csc;
    half_t *out0, *out1;
    float *outf;       // EPI_PARTIAL: [splits][M][Cout]
    int splits;
    const half_t *zeros;  // >= 16 bytes of zeros (source of padded taps for the LDS-DMA path)
    // IR-SE unit tail inside conv2's epilogue (mode EPI_BN_SE; only when the launch's ConvPlan says se_fused() - the strip kernels' main variants): y (out0) =
    // BN(conv) * gate + sc, z (out1) = y * p2 + p3, gate from the image-wide channel means through fc1 [C/16][C] / fc2 [C][C/16].
    float *se_pool;      // scratch [4][B][Cout] partial channel sums
    const float *se_w1, *se_w2;
    int *se_counter;     // [>= B] arrival counters, zero between launches; the gate-ready flags sit se_flag_off ints behind
    int se_flag_off;
    int se_epoch;        // launch number (> 0, different from every earlier launch's on this scratch): what the flags are set to
    int *se_error;       // error word in mapped host memory: set (to the launch number) when a hand-over wait timed out
    // strip family only, attached by its launchers (never by a caller; null when value-initialised): the device copy of the launch
    // geometry's strip tables (strip_tables below), its period in strips and the pixels one period covers
    const int *strip_tab;
    int strip_period, strip_ppx;
};
// Strip tables: everything conv_patch_body (kernels_arc.hip) needs per thread that depends only on the strip geometry and on the strip's
// position in its period - never on the tensors, the weights, the cout tile, Cin or the batch.  One block of `stride` ints per position:
//   [0, nslot * threads)   poff[q][t]: the input pixel, relative to the period's first pixel, that DMA slot q of thread t copies one
//                          16-byte piece of; -1 where the slot is structurally dead (halo, separator row, padding piece, past the patch)
//   [.., + nt * 64)        pbase[j][lane]: LDS byte offset of the B fragment of pixel tile j for tap (0, 0)
//   compact strips:        [nt][2] 64-bit lane masks: the lanes of tile j whose pixel sits in the first / last image column
//   padded strips:         eoff[nt * 32]: pixel slot -> output pixel relative to the period's first pixel, -1 for dead slots
// Periods: a compact strip is nt * 32 consecutive pixels, so the (image, row) phase repeats every lcm(H * W, nt * 32) pixels (14x14 in 7 tiles:
// 7 strips = 8 images; 7x7 in 4 tiles: 49 strips = 128 images); a padded strip repeats with the strips of one image group.
struct StripGeometry {
    int H, W;
    int compact;  // conv_patchc_kernel: consecutive pixels of the stacked images; else rows of n_img images with halo columns
    int linear;   // padded strips: slots enumerated over the padded row width
    int nt;       // pixel tiles per strip
    int R;        // image rows per strip (compact: rows of the patch window)
    int n_img;    // images per strip (padded strips)
    int nslot;    // DMA slots per thread
    int threads;  // threads that stage one patch: 256, or 128 in pair mode
};
struct StripTables {
    int period = 0;  // strips
    int ppx = 0;     // pixels per period
    int stride = 0;  // ints per strip position
    std::vector<int> data;  // [period][stride]
};
constexpr int strip_table_stride(const StripGeometry &g) { return g.nslot * g.threads + g.nt * 64 + (g.compact ? g.nt * 4 : g.nt * 32); }
// pure host function (no HIP call), exact integer division throughout
StripTables strip_tables(const StripGeometry &g);
// One conv launch, decided once: the instantiation that runs, the geometry its launcher needs, its label.  conv_plan() is a pure host
// function of the arguments (no HIP call: it runs on a machine without a device) and the ONE place a recogniser kernel is registered:
// an ordered list of families, each of which owns a table of (label, launcher) rows - one row per instantiation.
enum ConvFamily { CONV_SMALL, CONV_KS, CONV_C64, CONV_S2, CONV_STRIP };
struct ConvPlan {
    int family = CONV_STRIP;   // ConvFamily
    int row = 0;               // the instantiation: index into the family's table
    const char *label = "";    // its kernel symbol (as rocprofv3 prints it; also the profiling label bench.py and the tests key on)
    int R = 0, n_img = 1;      // strip families: image rows (compact strips: patch rows) and images per strip
    int M = 0;                 // CONV_SMALL: output pixels of the launch
    bool uses_scx = false;     // the kernel computes the fused 1x1 stride-2 shortcut conv (a.scx) itself
    // IR-SE (a = the unit's conv2 described as EPI_BN_ADD_BN + the se_* scratch): se_row >= 0 when the launch can carry the whole SE tail in its
    // epilogue - se_row / se_label name the twin instantiation that does (same family, same geometry).  The per-device occupancy gate
    // (conv_se_fits_device) is not part of the plan.
    int se_row = -1;
    const char *se_label = nullptr;
    bool se_fused() const { return se_row >= 0; }
    void take_se_tail() { row = se_row; label = se_label; }  // for the launch whose mode has become EPI_BN_SE
};
// a family's table row: every instantiation appears once, with its label next to its launcher
struct ConvRow {
    const char *label;
    void (*launch)(const ConvMfmaArgs &a, const ConvPlan &p, hipStream_t s);
    int se_row;  // the row of the twin instantiation with the SE tail in its epilogue; -1: none
};
inline void conv_plan_row(ConvPlan &p, int family, const ConvRow *table, int row) {
    p.family = family;
    p.row = row;
    p.label = table[row].label;
}
// IR-SE, for a planner whose strip geometry suits the tail: the plan gets the row's SE twin when `a` is a unit's conv2 described with the SE scratch
inline void conv_plan_se_twin(ConvPlan &p, const ConvRow *table, const ConvMfmaArgs &a) {
    if (table[p.row].se_row < 0 || a.mode != EPI_BN_ADD_BN || !a.se_pool || !a.sc || !a.out1) return;
    p.se_row = table[p.row].se_row;
    p.se_label = table[p.se_row].label;
}
ConvPlan conv_plan(const ConvMfmaArgs &a);
// the strip geometry of a planned launch; false: the plan's kernel reads no table (another family, the im2col kernel)
bool conv_strip_geometry(const ConvMfmaArgs &a, const ConvPlan &p, StripGeometry &g);
// first use of the launch's geometry on the current device: checks every entry, allocates and copies (so synchronises); frt_embedder::build()
// calls it for every plan it can reach, so that no launch allocates in steady state or inside a captured graph
void conv_strip_tables_warm(const ConvMfmaArgs &a, const ConvPlan &p);
void launch_conv_mfma(const ConvMfmaArgs &a, const ConvPlan &p, hipStream_t s);
bool conv_se_fits_device();  // HIP query, once per device: enough workgroups of the SE-tail instantiations are resident together (kernels_arc.hip)
// the families, in conv_plan's order; plan_X: false = not this family's launch (p untouched)
bool plan_small(const ConvMfmaArgs &a, ConvPlan &p);   // kernels_arc_small.hip: 3x3 convs of a small batch (few pixel tiles)
void launch_small(const ConvMfmaArgs &a, const ConvPlan &p, hipStream_t s);
bool plan_ks(const ConvMfmaArgs &a, ConvPlan &p);      // kernels_arc_ks.hip: 3x3 stride 1 at 14x14x256 / 7x7x512, medium batches (K split over the waves)
void launch_ks(const ConvMfmaArgs &a, const ConvPlan &p, hipStream_t s);
bool plan_c64(const ConvMfmaArgs &a, ConvPlan &p);     // kernels_arc_c64.hip: Cin = Cout = 64, 3x3, stride 1
void launch_c64(const ConvMfmaArgs &a, const ConvPlan &p, hipStream_t s);
bool plan_s2(const ConvMfmaArgs &a, ConvPlan &p);      // kernels_arc_s2.hip: 3x3 stride 2, Cout % 128 == 0 or 64 -> 64 at 112 -> 56
void launch_s2(const ConvMfmaArgs &a, const ConvPlan &p, hipStream_t s);
struct ArcInputArgs {
    const float *x;       // [F][3][112][112] planar RGB
    const float *w;       // [27][64]  (k = ci*9 + kh*3 + kw)
    const float *s0, *b0; // folded BN after the conv
    const float *slope;   // PReLU
    const float *s1, *b1; // next unit's leading BN
    half_t *y, *z;        // z [F][112][112][64]; y (shortcut of unit 0) only at even positions: [F][56][56][64]
    int F, H, W;
    const half_t *wh;     // matrix-core path: [64][32] fp16, k < 27: w * s0, k == 27: b0 (multiplies a constant 1), else 0
};
void launch_arc_input(const ArcInputArgs &a, hipStream_t s);
bool launch_arc_input_mfma(const ArcInputArgs &a, hipStream_t s);  // kernels_arc_input.hip; false: shape not covered
// output Linear 25088 -> 512 as 49 K-slices (kernels_arc_fc.hip): z [F][25088] fp16, wfrag = weights in MFMA-fragment order
// [512/32 output blocks][25088/16 k steps][64 lanes][8 halfs] (lane = (output row r, k half hi)), partial [49][F][512] fp32
void launch_fc_slices(const half_t *z, const half_t *wfrag, int F, float *partial, hipStream_t s);
// partial [splits][F][512] -> +bias -> BN1d -> L2 normalise -> out [F][512] fp32; rows with valid[f]==0 become zeros.
// fp32 end-to-end recogniser path (kernels_arc_f32.hip; frt_embedder_set_precision)
struct Conv32Args {
    const float *x, *w, *ps, *pb;  // w: fragment-ordered (pack_conv32_weights)
    float *out;
    int F, H, W, Cin, Ho, Wo, Cout, ks, stride, pad, mode;  // mode 0: PReLU(p0)  1: BN(p0, p1)  2: BN(p0, p1) + shortcut
    const float *p0, *p1, *sc;
    int sc_h, sc_w, sc_stride;
};
void launch_arc32_input(const float *x, const float *w, const float *s0, const float *b0, const float *slope, float *y, int F, hipStream_t s);
void launch_conv32(const Conv32Args &c, hipStream_t s);
void pack_conv32_weights(const float *w, int cout, int taps, int cin, float *out);  // host: [Cout][taps][Cin] -> the kernel's fragment order
void launch_fc32(const float *y, const float *sn, const float *bn, const float *w, float *out, int F, hipStream_t s);
void launch_se32(const float *res, const float *w1, const float *w2, float *gate, const float *sc, float *out, int F, int Ho, int Wo, int C, int sc_h, int sc_w, int sc_stride,
                 hipStream_t s);
void launch_fc_finalize(const float *partial, int splits, int F, const float *bias, const float *s, const float *b, const int *valid,
                        float *out, hipStream_t s_);
// flip-augmented embeddings (kernels_arc_flip.hip; frt_embedder_set_flip).  All pointers 16-byte aligned.
// chw [n][3][112][112] -> pair [2n][3][112][112]: faces 0 .. n-1 the originals, n .. 2n-1 the same images with the W axis reversed; bit-exact
void launch_arc_flip_pair(const float *chw, float *pair, int n, hipStream_t s);
// ... the mirror images alone -> mirror [n][3][112][112]
void launch_arc_flip_mirror(const float *chw, float *mirror, int n, hipStream_t s);
// partial_a, partial_b [splits][rows][512], each addressed at row f < n: pre = (slice sums in slice order + bias) * s + b of both, then
// out[f] = (pre_a + pre_b) / max(|pre_a + pre_b|, 1e-12), zeros where valid[f] == 0 (valid may be null).  One 2n-face pass: partial_b =
// partial_a + n * 512, rows = 2n.
void launch_fc_finalize_pair(const float *partial_a, const float *partial_b, int splits, int rows, int n, const float *bias, const float *s, const float *b,
                             const int *valid, float *out, hipStream_t s_);
// SE tail (IR-SE): pool -> fc1 -> relu -> fc2 -> sigmoid -> scale, + shortcut, + next BN
struct SeArgs {
    const half_t *res;   // [F][H][W][C] = BN2(conv2)
    const float *w1;     // [C/16][C]
    const float *w2;     // [C][C/16]
    const half_t *sc; int sc_h, sc_w, sc_stride;
    const float *s1, *b1;
    half_t *y, *z;
    float *pool;         // scratch [4][F][C] (partial sums over pixel ranges)
    float *gate;         // scratch [F][C]
    int F, H, W, C;
    int *counter;        // [F] arrival counters of the pooling pass, zero between launches
};
void launch_se(const SeArgs &a, hipStream_t s);

// ---------------------------------------------------------------- face tracker (kernels_track.hip; frt_tracker.cpp, include/frt.h "Face tracker")
constexpr int FRT_TRACK_MAX_FRAMES = 256, FRT_TRACK_MAX_STREAMS = 1024, FRT_TRACK_MAX_SLOTS = 64, FRT_TRACK_MAX_DIM = 2048;
struct TrackStreamIds {  // by value with the launch: the ids reach the kernel without a staging copy or a host synchronisation
    uint16_t id[FRT_TRACK_MAX_FRAMES];
};
struct TrackArgs {
    frt_track_state *slots;  // [n_streams][max_tracks]
    float *sums;             // [n_streams][max_tracks][dim]; the rows of free slots are zero
    int32_t *counters;       // [n_streams][4]: next_id, tick, dropped, -
    int max_tracks, max_faces, dim;
    float iou_threshold, decay;
    int max_missed, min_hits;
    const frt_face_result *results;  // [n_frames][max_faces]
    const float *embeds;             // [n_frames][max_faces][dim], 16-byte aligned
    frt_track_result *tracks;        // [n_frames][max_faces]
    float *templates;                // [n_frames][max_faces][dim], 16-byte aligned, or null
    // ---- appearance (include/frt.h "Appearance"): read by the similarity kernel and by the update kernel's APPEARANCE instantiation only
    float reid_threshold, iou_min_sim;  // 2.0 / -2.0: off
    float *sim;                         // scratch S [n_frames][max_faces][max_tracks]; an entry is written iff its bit below is set
    unsigned long long *sim_defined;    // scratch [n_frames][max_faces]: bit t set iff S[f][d][t] is DEFINED
    frt_track_assoc *assoc;             // [n_frames][max_faces], or null
    // ---- motion (include/frt.h "Motion"): read by the update kernel's MOTION instantiations only (and, for null, by the reset kernel)
    int2 *vel;        // [n_streams][max_tracks]: (vx, vy) of the box centre in 1/256 pixel per update; null until a call with motion on needs it
    int motion_gain;  // 0: off; 1 .. 256
};
// S and its defined bits of every detection x slot pair of the call, from the sums as they are BEFORE the update: one workgroup per detection
void launch_track_similarity(const TrackArgs &a, const TrackStreamIds &ids, int n_frames, hipStream_t s);
// steps 1 - 6 and 8 of an update, one workgroup per frame; the records leave with match_idx -1 / match_sim 0.  appearance: the instantiation
// that reads a.sim / a.sim_defined (steps 2a, 2b; launch_track_similarity ran before it on s) and writes a.assoc; without it the launch is
// the one of a tracker that has no appearance settings.  a.motion_gain > 0: the instantiation that reads and writes a.vel (M1 - M3)
void launch_track_update(const TrackArgs &a, const TrackStreamIds &ids, int n_frames, bool appearance, hipStream_t s);
// step 7 behind the top-1 search of the template rows: idx / sim [n_frames * max_faces] -> the tracked records with n_embeds > 0 and their slots
void launch_track_identity(const TrackArgs &a, const TrackStreamIds &ids, int n_frames, const int32_t *idx, const float *sim, hipStream_t s);
// frees the slots of `stream` (-1: of every one of n_streams) and zeroes tick / dropped; next_id stays
void launch_track_reset(const TrackArgs &a, int n_streams, int stream, hipStream_t s);
// ---- the gate in front of the recogniser (include/frt.h "Gate")
struct TrackGateArgs {
    const frt_track_state *slots;  // [n_streams][max_tracks], read only
    int max_tracks, max_faces;
    float iou_threshold;
    int min_hits;
    int refresh, min_embeds;  // frt_track_gate_options, checked on the host: refresh >= 1
    float skip_iou;
    const frt_bbox *boxes;    // [n_frames][max_faces]
    const int32_t *n_boxes;   // [n_frames], or null: every slot with score > 0 is present
    int n_frames;             // 1 .. FRT_TRACK_MAX_FRAMES
    frt_track_gate *gate;     // [n_frames][max_faces]
    int32_t *list;            // [n_frames * max_faces]: the EMBED face indices ascending, -1 behind them
    int32_t *n_embed;         // [1]
    int32_t *pass_count;      // [ceil(n_frames * max_faces / max_batch)]
    int max_batch;            // >= 1
    // ---- motion: read by the MOTION instantiation only, which the launch takes iff motion_gain > 0
    const int2 *vel;  // [n_streams][max_tracks], read only
    int motion_gain;
};
// G1 - G4 and the work list of one call in one launch of one workgroup; writes no tracker state
void launch_track_gate(const TrackGateArgs &a, const TrackStreamIds &ids, hipStream_t s);
// the compact rows of the recogniser back into face slots: embeds [F][dim] (zero rows for the slots not in the list), valid / idx / sim [F]
// (0 / -1 / 0 there).  idx_c / sim_c may be null (no gallery: -1 / 0 everywhere), idx / sim may be null (not written).  embeds and embeds_c
// 16-byte aligned, dim a multiple of 4; *n_embed is clamped to 0 .. F
struct TrackScatterArgs {
    const int32_t *list, *n_embed;
    const float *embeds_c;
    const int *valid_c;
    const int32_t *idx_c;
    const float *sim_c;
    int F, dim;
    float *embeds;
    int *valid;
    int32_t *idx;
    float *sim;
};
void launch_track_gate_scatter(const TrackScatterArgs &a, hipStream_t s);

// ---------------------------------------------------------------- sighting book (kernels_sightings.hip; frt_sightings.cpp, include/frt.h "Sightings")
constexpr int FRT_SIGHTING_CROP_BYTES = 112 * 112 * 3;
// What one entry (an open one of a tracker slot, or a queue row) has to have moved, written by the plan kernels and read by the copy kernel
struct SightingJob {
    int32_t entry;  // the row of the open entry, stream * max_tracks + slot
    int32_t qrow;   // -1: the entry did not end; -2: it ended and nothing is queued; >= 0: its payload goes to this queue row first
    int32_t face;   // -1, or the face slot f * max_faces + d that was observed: its template row is taken, and with `replace` its embedding and crop
    int32_t replace;
};
struct SightingArgs {
    // ---- the book: rows 0 .. n_open - 1 are the open entries [n_streams][max_tracks], rows n_open .. n_open + capacity - 1 the queue
    frt_sighting *records;
    float *best_embeds, *templates;  // [rows][dim]
    uint8_t *crops;                  // [rows][112][112][3], or null (keep_crops 0)
    uint32_t *best_key;              // [n_open]: the bits of the best shot's metric
    int32_t *state;                  // [4]: rows queued (those the host has taken and not yet reported included), overflowed, discarded, closed
    SightingJob *jobs;               // [n_open]
    int n_open, capacity, head, taken;  // head: the queue row of the oldest sighting; taken: rows drained since the last launch
    int max_tracks, max_faces, dim, rank, min_hits;
    // ---- the tracker's state, read only, as its update left it
    const frt_track_state *slots;
    const int32_t *counters;
    // ---- the call
    const frt_face_result *results;
    const frt_track_result *tracks;
    const float *embeds, *call_templates;  // call_templates may be null
    const struct frt_face_quality *quality;
    const uint8_t *call_crops;             // null iff crops is null
};
// S1 - S3 of one update: the records, the queue rows and the job list, in one launch of one workgroup; then the payloads, one workgroup per
// entry of the call's streams.  Both on s, in this order.
void launch_sightings_plan(const SightingArgs &a, const TrackStreamIds &ids, int n_frames, hipStream_t s);
void launch_sightings_copy(const SightingArgs &a, int n_jobs, hipStream_t s);
// frt_sightings_close: ends every open entry of `stream` (-1: of each of n_streams) with reason CLOSED; jobs [n_streams * max_tracks] or
// [max_tracks], to be followed by launch_sightings_copy over as many
void launch_sightings_close(const SightingArgs &a, int n_streams, int stream, hipStream_t s);
