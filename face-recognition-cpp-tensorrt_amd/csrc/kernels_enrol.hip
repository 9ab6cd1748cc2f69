// The "exactly one face" rule of /insert/face (/root/reference/src/app.cpp:163-187) on the device, for the frames of one pipeline call.
//
// The reference resizes the photo, runs findFace + getCroppedFaces and then answers ret = 2 for more than one face (:172-174), ret = 3 for
// none (:175-177) and embeds + stores the face otherwise.  enrol_select_kernel reads what the pipeline left on the device - records
// frt_face_result[n_frames][max_faces] (boxes fill a frame's slots from slot 0, an unused slot has score 0) and embeddings
// [n_frames][max_faces][512] - and per frame
//   - counts the slots with box.score > 0 and writes status[frame] (FRT_ENROL_*: one box with valid != 0 is OK, one box whose ROI is empty
//     - valid == 0, score > 0 - is EMPTY_ROI: OpenCV would throw there); with quality records [n_frames][max_faces] (may be null: the
//     gate is off and nothing below changes) an OK frame whose SLOT 0 record has flags != 0 is LOW_QUALITY instead: its face is written
//     as for OK, its row is not copied;
//   - writes face_out[frame] (may be null): slot 0's record for OK and EMPTY_ROI, zeros otherwise, `frame` kept either way;
//   - copies slot 0's embedding of every OK frame to rows[base + rank], in frame order: base = *count at entry, rank = exclusive prefix sum
//     of the OK flags; 16-byte loads and stores;
//   - stores *count = base + n_ok: one plain vector store from one thread behind a barrier, no atomics - calls on one stream are ordered,
//     so consecutive chunks append to one dense buffer without a host round trip between them.
// One workgroup per call: it walks the frames 256 at a time (any n_frames >= 0, any max_faces >= 1).  No scratch.
#include "frt_kernels.h"

namespace {

constexpr int SEL_THREADS = 256, SEL_WAVES = SEL_THREADS / 64, ROW_VEC = 512 / 4;  // a 512-float row is 128 float4

__global__ __launch_bounds__(SEL_THREADS) void enrol_select_kernel(const frt_face_result *__restrict__ results, const float *__restrict__ embeds,
                                                                   int n_frames, int max_faces, int32_t *__restrict__ status,
                                                                   frt_face_result *__restrict__ face_out, float *__restrict__ rows,
                                                                   int32_t *__restrict__ count, const struct frt_face_quality *__restrict__ quality) {
    __shared__ int s_wave[SEL_WAVES];
    __shared__ int s_dst[SEL_THREADS];  // rank of the tile's frame among the call's OK frames, -1: not OK
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int base = *count;  // (every thread reads it before the first barrier; the one store comes behind the last)
    const float4 *__restrict__ emb4 = reinterpret_cast<const float4 *>(embeds);
    float4 *__restrict__ rows4 = reinterpret_cast<float4 *>(rows);
    int n_ok = 0;  // OK frames of the tiles done so far (the same in every thread)
    for (int t0 = 0; t0 < n_frames; t0 += SEL_THREADS) {
        const int frame = t0 + tid;
        bool ok = false;
        if (frame < n_frames) {
            const frt_face_result *r = results + (size_t)frame * max_faces;
            int boxes = 0;
            for (int k = 0; k < max_faces; ++k) boxes += r[k].box.score > 0.f ? 1 : 0;
            const frt_face_result r0 = r[0];
            int st = boxes == 0 ? FRT_ENROL_NONE : boxes > 1 ? FRT_ENROL_MANY : r0.valid != 0 ? FRT_ENROL_OK : FRT_ENROL_EMPTY_ROI;
            if (quality && st == FRT_ENROL_OK && quality[(size_t)frame * max_faces].flags != 0u) st = FRT_ENROL_LOW_QUALITY;
            ok = st == FRT_ENROL_OK;
            status[frame] = st;
            if (face_out) {
                frt_face_result o = r0;
                if (st != FRT_ENROL_OK && st != FRT_ENROL_EMPTY_ROI && st != FRT_ENROL_LOW_QUALITY) {
                    o.box = frt_bbox{0, 0, 0, 0, 0.f};
                    o.match_idx = 0;
                    o.match_sim = 0.f;
                    o.valid = 0;
                }
                face_out[frame] = o;
            }
        }
        const unsigned long long m = __ballot(ok);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < SEL_WAVES; ++w) {
            const int c = s_wave[w];
            before += w < wave ? c : 0;
            total += c;
        }
        s_dst[tid] = ok ? n_ok + before + __popcll(m & ((1ull << lane) - 1ull)) : -1;
        __syncthreads();
        const int nt = n_frames - t0 < SEL_THREADS ? n_frames - t0 : SEL_THREADS;
        for (int i = tid; i < nt * ROW_VEC; i += SEL_THREADS) {
            const int fi = i / ROW_VEC, q = i - fi * ROW_VEC;
            const int d = s_dst[fi];
            if (d >= 0) rows4[((size_t)base + (size_t)d) * ROW_VEC + q] = emb4[(size_t)(t0 + fi) * max_faces * ROW_VEC + q];
        }
        n_ok += total;
        __syncthreads();  // s_wave / s_dst are rewritten by the next tile
    }
    __syncthreads();
    if (tid == 0) *count = base + n_ok;
}

}  // namespace

void launch_enrol_select(const frt_face_result *results, const float *embeds, int n_frames, int max_faces, int32_t *status, frt_face_result *face_out,
                         float *rows, int32_t *count, hipStream_t s, const struct frt_face_quality *quality) {
    hipLaunchKernelGGL(enrol_select_kernel, dim3(1), dim3(SEL_THREADS), 0, s, results, embeds, n_frames, max_faces, status, face_out, rows, count,
                       quality);
}
