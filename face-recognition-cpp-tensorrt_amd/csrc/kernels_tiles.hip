// Large photos by tiles (include/frt.h, "Large photos by tiles"): the cut of a once-uploaded photo into the detector's frame buffer, and
// the merge of every tile's boxes into one list in photo coordinates.  The reference has no counterpart; the semantics are the header's,
// restated in numpy by tests/tiled_ref.py.
//
// The merge is a greedy NMS over up to 16384 candidates.  nms_kernel's scheme (kernels_post.hip: one workgroup-wide arg-max per kept box)
// would be thousands of dependent rounds here, so it is split into launches that are each wide or short:
//   tile_map_kernel   one thread per (tile, slot): candidate test, cut test, map to the photo, 64-bit sort key
//   tile_rank_kernel  the sort, as a rank count: keys are unique, so rank = number of smaller keys; order[rank] = source index
//   tile_mask_kernel  suppression bit matrix over the SORTED order: bit j of word (p, j / 64) = "p suppresses j" for j > p
//   tile_scan_kernel  ONE wave walks the sorted order 64 candidates at a time and ORs the rows of the kept ones into the dead set
// Launch order on one stream is the only synchronisation between them: no counters, no atomics, nothing to reset between calls.
// Overlap arithmetic is float32 in nms_kernel's operation order (this translation unit is compiled with -ffp-contract=off).
// Behind the merge, for the route that goes on to the recogniser: tile_faces_select_kernel, the merged list -> the kept faces, dense.
#include "frt_kernels.h"

namespace {

constexpr unsigned long long KEY_NONE_HI = 0xFFFFFFFFull;  // no candidate: sorts behind every score (a score's inverted key is <= 0xFF800000)

// ---------------------------------------------------------------------------------------------------------------- cut
// One thread writes CH consecutive bytes of one tile row: CH = 16 / 4 (one wide store; the launcher picks the widest that divides
// tile_cols * 3, rows and tiles then start on that alignment in the hipMalloc'ed frame buffer) or 1.  Source rows are read bytewise: a
// tile's column origin puts them at any alignment.
template <int CH>
__global__ __launch_bounds__(256) void cut_tiles_kernel(const uint8_t *__restrict__ photo, int rows, int cols, size_t row_stride,
                                                        const frt_tile *__restrict__ tiles, int tile_rows, int tile_cols, uint8_t *__restrict__ out) {
    const int row_bytes = tile_cols * 3, per_row = row_bytes / CH;
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= per_row) return;
    const int r = blockIdx.y, t = blockIdx.z;
    const frt_tile tl = tiles[t];
    if (tl.kind != 0) return;  // (uniform) the overview's slot is written by the resize
    const int pr = tl.row0 + r;
    const long b0 = (long)tl.col0 * 3 + (long)c * CH;  // byte of the photo row
    const long photo_bytes = (long)cols * 3;
    uint8_t v[CH];
    const uint8_t *src = photo + (size_t)(pr < rows ? pr : 0) * row_stride;
    const bool row_in = pr >= 0 && pr < rows && tl.row0 >= 0 && tl.col0 >= 0;
    if (row_in && b0 + CH <= photo_bytes) {
        __builtin_memcpy(v, src + b0, CH);
    } else {
#pragma unroll
        for (int k = 0; k < CH; ++k) v[k] = (row_in && b0 + k < photo_bytes) ? src[b0 + k] : (uint8_t)128;
    }
    uint8_t *dst = out + ((size_t)t * tile_rows + r) * row_bytes + (size_t)c * CH;
    if (CH == 16) {
        uint4 w;
        __builtin_memcpy(&w, v, 16);
        *reinterpret_cast<uint4 *>(dst) = w;
    } else if (CH == 4) {
        uint32_t w;
        __builtin_memcpy(&w, v, 4);
        *reinterpret_cast<uint32_t *>(dst) = w;
    } else {
        dst[0] = v[0];
    }
}

// ---------------------------------------------------------------------------------------------------------------- merge
// score -> 32 bits whose unsigned order is the floats' order; -0 counts as +0 ("by score" compares them equal, tile and slot decide)
__device__ __forceinline__ uint32_t score_bits(float s) {
    uint32_t b = __float_as_uint(s == 0.f ? 0.f : s);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(256) void tile_map_kernel(TileMergeArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int M = a.n_tiles * a.slots;
    if (i >= M) return;
    const int t = i / a.slots, s = i - t * a.slots;
    const frt_tile tl = a.tiles[t];
    frt_bbox b = a.boxes[i];
    bool ok = s < a.n_boxes[t] && !(b.score != b.score);
    if (tl.kind == 0) {
        const bool cut = (b.x1 == 0 && tl.row0 > 0) || (b.y1 == 0 && tl.col0 > 0) || (b.x2 == a.tile_rows - 1 && (long)tl.row0 + a.tile_rows < a.photo_rows) ||
                         (b.y2 == a.tile_cols - 1 && (long)tl.col0 + a.tile_cols < a.photo_cols);
        if (a.drop_cut && cut) ok = false;
        const long x1 = (long)b.x1 + tl.row0, y1 = (long)b.y1 + tl.col0, x2 = (long)b.x2 + tl.row0, y2 = (long)b.y2 + tl.col0;
        if (x1 >= a.photo_rows || y1 >= a.photo_cols) ok = false;
        const long hr = a.photo_rows - 1, hc = a.photo_cols - 1;
        b.x1 = (int)(x1 < 0 ? 0 : (x1 > hr ? hr : x1));
        b.x2 = (int)(x2 < 0 ? 0 : (x2 > hr ? hr : x2));
        b.y1 = (int)(y1 < 0 ? 0 : (y1 > hc ? hc : y1));
        b.y2 = (int)(y2 < 0 ? 0 : (y2 > hc ? hc : y2));
    } else {
        const long long x1 = (long long)b.x1 * a.photo_rows / a.tile_rows, y1 = (long long)b.y1 * a.photo_cols / a.tile_cols;
        long long x2 = ((long long)b.x2 + 1) * a.photo_rows / a.tile_rows - 1, y2 = ((long long)b.y2 + 1) * a.photo_cols / a.tile_cols - 1;
        if (x2 < x1) x2 = x1;
        if (y2 < y1) y2 = y1;
        const long long hr = a.photo_rows - 1, hc = a.photo_cols - 1;
        b.x1 = (int)(x1 < 0 ? 0 : (x1 > hr ? hr : x1));
        b.x2 = (int)(x2 < 0 ? 0 : (x2 > hr ? hr : x2));
        b.y1 = (int)(y1 < 0 ? 0 : (y1 > hc ? hc : y1));
        b.y2 = (int)(y2 < 0 ? 0 : (y2 > hc ? hc : y2));
    }
    a.mbox[i] = b;
    const unsigned long long hi = ok ? (unsigned long long)(~score_bits(b.score)) : KEY_NONE_HI;
    a.keys[i] = (hi << 32) | (unsigned)i;
}

// 64 candidates per workgroup, one per lane; the four waves each count a quarter of the keys (a wave-uniform read per key)
__global__ __launch_bounds__(256) void tile_rank_kernel(const unsigned long long *__restrict__ keys, int M, int *__restrict__ order) {
    __shared__ int s_part[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + lane;
    const unsigned long long mine = i < M ? keys[i] : ~0ull;
    const int q = (M + 3) / 4, j0 = w * q, j1 = j0 + q < M ? j0 + q : M;
    int r = 0;
    for (int j = j0; j < j1; ++j) r += keys[j] < mine ? 1 : 0;
    s_part[w][lane] = r;
    __syncthreads();
    if (w == 0 && i < M) {
        r = s_part[0][lane] + s_part[1][lane] + s_part[2][lane] + s_part[3][lane];
        order[r] = (mine >> 32) == KEY_NONE_HI ? -1 : i;  // keys are unique: r is a permutation of 0 .. M-1, the non-candidates last
    }
}

__device__ __forceinline__ float box_area(const frt_bbox &b) {
    // (float) of the exact product: nms_kernel's (float)((x2 - x1 + 1) * (y2 - y1 + 1)) wherever that int product does not overflow
    return (float)((long long)(b.x2 - b.x1 + 1) * (long long)(b.y2 - b.y1 + 1));
}

// overlap of the earlier (winning) box wb with b: nms_kernel's statements, then the metric's quotient
__device__ __forceinline__ float overlap(const frt_bbox &wb, float warea, const frt_bbox &b, float area, int metric) {
    const float xx1 = (float)(wb.x1 > b.x1 ? wb.x1 : b.x1);
    const float yy1 = (float)(wb.y1 > b.y1 ? wb.y1 : b.y1);
    const float xx2 = (float)(wb.x2 < b.x2 ? wb.x2 : b.x2);
    const float yy2 = (float)(wb.y2 < b.y2 ? wb.y2 : b.y2);
    float w = xx2 - xx1 + 1;
    float h = yy2 - yy1 + 1;
    if (w < 0.f) w = 0.f;
    if (h < 0.f) h = 0.f;
    const float inter = w * h;
    if (metric == 0) return inter / (warea + area - inter);
    return inter / (warea < area ? warea : area);
}

// workgroup (cb, rb) = one wave: lane = sorted position p = rb * 64 + lane against the 64 positions of column block cb >= rb
__global__ __launch_bounds__(64) void tile_mask_kernel(const int *__restrict__ order, const frt_bbox *__restrict__ mbox, int M, int W, int metric,
                                                       float thr, unsigned long long *__restrict__ mask) {
    const int cb = blockIdx.x, rb = blockIdx.y, lane = threadIdx.x;
    if (cb < rb) return;
    if (order[rb * 64] < 0) return;  // the order ends before this row block: its rows are never read
    __shared__ frt_bbox s_box[64];
    __shared__ float s_area[64];
    __shared__ int s_ok[64];
    const int j = cb * 64 + lane;
    const int oj = j < M ? order[j] : -1;
    if (oj >= 0) {
        const frt_bbox b = mbox[oj];
        s_box[lane] = b;
        s_area[lane] = box_area(b);
    }
    s_ok[lane] = oj >= 0;
    __syncthreads();
    const int p = rb * 64 + lane;
    if (p >= M) return;
    const int op = order[p];
    unsigned long long bits = 0;
    if (op >= 0) {
        const frt_bbox wb = mbox[op];
        const float warea = box_area(wb);
        for (int k = 0; k < 64; ++k) {
            if (!s_ok[k] || cb * 64 + k <= p) continue;
            if (overlap(wb, warea, s_box[k], s_area[k], metric) >= thr) bits |= 1ull << k;
        }
    }
    mask[(size_t)p * W + cb] = bits;
}

__global__ __launch_bounds__(64) void tile_scan_kernel(const int *__restrict__ order, const frt_bbox *__restrict__ mbox,
                                                       const unsigned long long *__restrict__ mask, int M, int W, int max_out,
                                                       frt_bbox *__restrict__ out, int32_t *__restrict__ src_out, int *__restrict__ n_out) {
    __shared__ unsigned long long s_dead[256];  // W <= 256 words; word ww is only ever written by lane ww % 64
    const int lane = threadIdx.x;
    for (int ww = lane; ww < W; ww += 64) s_dead[ww] = 0;
    __syncthreads();
    int kept = 0;
    for (int w = 0; w < W && kept < max_out; ++w) {
        const int p = w * 64 + lane;
        const int op = p < M ? order[p] : -1;
        const unsigned long long present = __ballot(op >= 0);
        if (present == 0ull) break;  // (uniform) the order ends here
        const unsigned long long diag = op >= 0 ? mask[(size_t)p * W + w] : 0ull;
        const uint32_t dlo = (uint32_t)diag, dhi = (uint32_t)(diag >> 32);
        // the serial part, on wave-uniform values only: lane b's diagonal word comes by v_readlane (b is a constant of the unrolled loop)
        const unsigned long long dead_w = s_dead[w];
        unsigned long long cur = (((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(dead_w >> 32)) << 32) |
                                  (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)dead_w)) | ~present;
        unsigned long long keep = 0;
#pragma unroll
        for (int b = 0; b < 64; ++b) {
            const unsigned long long row = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane(dhi, b) << 32) | (uint32_t)__builtin_amdgcn_readlane(dlo, b);  // (the builtin returns int: no sign extension)
            if (!((cur >> b) & 1ull)) {
                keep |= 1ull << b;
                cur |= row;
            }
        }
        const int pos = kept + __popcll(keep & ((1ull << lane) - 1ull));
        if (((keep >> lane) & 1ull) && pos < max_out) {
            out[pos] = mbox[op];
            src_out[pos] = op;
        }
        // rows of the kept ones into the dead set of the later blocks (those past max_out change nothing that is still read)
        // A lane gathers its (at most four) words in registers, so the loads of all kept rows are in flight together.
        unsigned long long acc[4] = {0ull, 0ull, 0ull, 0ull};
        for (unsigned long long k = keep; k; k &= k - 1) {
            const size_t row = (size_t)(w * 64 + __builtin_ctzll(k)) * W;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ww = lane + 64 * q;
                if (ww > w && ww < W) acc[q] |= mask[row + ww];
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (lane + 64 * q < W) s_dead[lane + 64 * q] |= acc[q];
        kept += __popcll(keep);
        __syncthreads();  // (s_dead[w + 1] is read by every lane next)
    }
    if (kept > max_out) kept = max_out;
    if (lane == 0) *n_out = kept;
    for (int i = kept + lane; i < max_out; i += 64) {
        frt_bbox z;
        z.x1 = z.y1 = z.x2 = z.y2 = 0;
        z.score = 0.f;
        out[i] = z;
        src_out[i] = -1;
    }
}

// landmarks of the kept boxes: ldm [n_tiles][slots][10] in tile coordinates -> out [max_out][10] in photo coordinates (zeros behind n_out)
__global__ void tile_landmarks_kernel(const float *__restrict__ ldm, const frt_tile *__restrict__ tiles, const int32_t *__restrict__ src,
                                      const int *__restrict__ n_out, int slots, int max_out, int photo_rows, int photo_cols, int tile_rows,
                                      int tile_cols, float *__restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= max_out * 5) return;
    const int i = t / 5;
    float x = 0.f, y = 0.f;
    if (i < *n_out) {
        const int sidx = src[i];
        const frt_tile tl = tiles[sidx / slots];
        const float *p = ldm + (size_t)sidx * 10 + 2 * (t - i * 5);
        if (tl.kind == 0) {
            x = p[0] + (float)tl.col0;
            y = p[1] + (float)tl.row0;
        } else {
            x = p[0] * (float)photo_cols / (float)tile_cols;
            y = p[1] * (float)photo_rows / (float)tile_rows;
        }
    }
    out[(size_t)t * 2] = x;
    out[(size_t)t * 2 + 1] = y;
}

// ---------------------------------------------------------------------------------------------------------------- faces of a tiled photo
// The recogniser's work list out of the merged list (include/frt.h, "Recognising a large photo by tiles"): a box is kept iff
// min(x2 - x1, y2 - y1) >= min_face - crop_faces_kernel's rh / rw, far corner excluded; min_face <= 0 keeps every box - and the kept ones
// are packed in merge order.  ONE workgroup of 16 waves walks the list 1024 boxes at a time: a wave's ballot gives every lane its place
// inside the wave, the 16 wave counts (LDS) the place of the wave inside the step, a running base the place of the step.  No atomics: the
// order, and with it every output bit, is the same on every run.  Behind the count the outputs are zeros / -1; pass_count[j] is the number
// of faces of recogniser pass j (faces [j * max_batch, (j + 1) * max_batch)), the crop / align kernels' n_boxes for that pass.
__global__ __launch_bounds__(1024) void tile_faces_select_kernel(const frt_bbox *__restrict__ boxes, const int32_t *__restrict__ src,
                                                                 const float *__restrict__ ldm, const int *__restrict__ n_in, int cap, int min_face,
                                                                 int max_batch, frt_bbox *__restrict__ boxes_kept, int32_t *__restrict__ src_kept,
                                                                 float *__restrict__ ldm_kept, int32_t *__restrict__ keep_pos,
                                                                 int *__restrict__ n_kept, int32_t *__restrict__ pass_count) {
    __shared__ int s_wave[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int n = *n_in;
    n = n < 0 ? 0 : (n > cap ? cap : n);
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 1024) {  // (uniform: every thread takes every step)
        const int i = i0 + tid;
        frt_bbox b;
        b.x1 = b.y1 = b.x2 = b.y2 = 0;
        b.score = 0.f;
        bool keep = false;
        if (i < n) {
            b = boxes[i];
            const int rh = b.x2 - b.x1, rw = b.y2 - b.y1;
            keep = min_face <= 0 || (rh < rw ? rh : rw) >= min_face;
        }
        const unsigned long long vote = __ballot(keep);
        if (lane == 0) s_wave[w] = __popcll(vote);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int c = s_wave[k];
            before += k < w ? c : 0;
            total += c;
        }
        if (keep) {
            const int pos = base + before + __popcll(vote & ((1ull << lane) - 1ull));  // pos <= i < n <= cap
            boxes_kept[pos] = b;
            keep_pos[pos] = i;
            if (src_kept) src_kept[pos] = src[i];
            if (ldm_kept)
                for (int k = 0; k < 10; ++k) ldm_kept[(size_t)pos * 10 + k] = ldm[(size_t)i * 10 + k];
        }
        base += total;
        __syncthreads();  // (s_wave is rewritten by the next step)
    }
    for (int i = base + tid; i < cap; i += 1024) {
        frt_bbox z;
        z.x1 = z.y1 = z.x2 = z.y2 = 0;
        z.score = 0.f;
        boxes_kept[i] = z;
        keep_pos[i] = -1;
        if (src_kept) src_kept[i] = -1;
        if (ldm_kept)
            for (int k = 0; k < 10; ++k) ldm_kept[(size_t)i * 10 + k] = 0.f;
    }
    if (tid == 0) *n_kept = base;
    const int passes = (int)(((long long)cap + max_batch - 1) / max_batch);
    for (int j = tid; j < passes; j += 1024) {
        const long long left = (long long)base - (long long)j * max_batch;
        pass_count[j] = (int32_t)(left < 0 ? 0 : (left > max_batch ? max_batch : left));
    }
}

}  // namespace

void launch_cut_tiles(const uint8_t *photo, int rows, int cols, size_t row_stride, const frt_tile *tiles, int n_tiles, int tile_rows, int tile_cols,
                      uint8_t *out, hipStream_t s) {
    if (n_tiles < 1) return;
    const int row_bytes = tile_cols * 3;
    const int ch = row_bytes % 16 == 0 ? 16 : (row_bytes % 4 == 0 ? 4 : 1);
    dim3 grid((row_bytes / ch + 255) / 256, tile_rows, n_tiles);
    if (ch == 16) hipLaunchKernelGGL(cut_tiles_kernel<16>, grid, dim3(256), 0, s, photo, rows, cols, row_stride, tiles, tile_rows, tile_cols, out);
    else if (ch == 4) hipLaunchKernelGGL(cut_tiles_kernel<4>, grid, dim3(256), 0, s, photo, rows, cols, row_stride, tiles, tile_rows, tile_cols, out);
    else hipLaunchKernelGGL(cut_tiles_kernel<1>, grid, dim3(256), 0, s, photo, rows, cols, row_stride, tiles, tile_rows, tile_cols, out);
}

size_t tile_merge_mask_words(int candidates) { return (size_t)candidates * (size_t)((candidates + 63) / 64); }

void launch_tile_merge(const TileMergeArgs &a, hipStream_t s) {
    const int M = a.n_tiles * a.slots, W = (M + 63) / 64;  // (the callers keep 1 <= M <= 16384: W <= 256)
    hipLaunchKernelGGL(tile_map_kernel, dim3((M + 255) / 256), dim3(256), 0, s, a);
    hipLaunchKernelGGL(tile_rank_kernel, dim3(W), dim3(256), 0, s, a.keys, M, a.order);
    hipLaunchKernelGGL(tile_mask_kernel, dim3(W, W), dim3(64), 0, s, a.order, a.mbox, M, W, a.metric, a.thr, a.mask);
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(64), 0, s, a.order, a.mbox, a.mask, M, W, a.max_out, a.out, a.src_out, a.n_out);
}

void launch_tile_landmarks(const float *ldm, const frt_tile *tiles, const int32_t *src, const int *n_out, int slots, int max_out, int photo_rows,
                           int photo_cols, int tile_rows, int tile_cols, float *out, hipStream_t s) {
    hipLaunchKernelGGL(tile_landmarks_kernel, dim3((max_out * 5 + 255) / 256), dim3(256), 0, s, ldm, tiles, src, n_out, slots, max_out, photo_rows,
                       photo_cols, tile_rows, tile_cols, out);
}

void launch_tile_faces_select(const frt_bbox *boxes, const int32_t *src, const float *ldm, const int *n_in, int cap, int min_face, int max_batch,
                              frt_bbox *boxes_kept, int32_t *src_kept, float *ldm_kept, int32_t *keep_pos, int *n_kept, int32_t *pass_count,
                              hipStream_t s) {
    hipLaunchKernelGGL(tile_faces_select_kernel, dim3(1), dim3(1024), 0, s, boxes, src, ldm, n_in, cap, min_face, max_batch, boxes_kept,
                       src ? src_kept : nullptr, ldm ? ldm_kept : nullptr, keep_pos, n_kept, pass_count);
}
