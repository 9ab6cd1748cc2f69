// Sighting book (include/frt.h "Sightings"): the device side.  Two launches per update.
//
// sightings_plan_kernel - ONE workgroup of 16 waves for the whole call, in the style of track_gate_kernel: the queue is a single FIFO whose
//   order is "frames in call order, then slots ascending" and whose room ends at `capacity`, so which closer gets which row is a prefix sum
//   over the call, and one workgroup that owns the queue count needs no atomics on it.  A wave takes a frame in turn, lane t is slot t of
//   that frame's stream and the ONLY writer of entry E[s][t]:
//     pass 0  lane d of a frame's wave writes its detection index into s_det[f][tracks[f][d].slot] (the slots of one frame's tracked
//             detections are pairwise distinct: a track takes one detection);
//     pass A  S1's decision per slot: a ballot gives the frame's closers and those of them that are to be queued; the discards and the
//             closes are counted per wave and added up in LDS;
//     prefix  wave 0 turns the 256 per-frame counts into exclusive offsets (four frames per lane, a shuffle scan);
//     pass B  lane t works on its entry's row in place: S1 (the record goes to queue row (head + queued + rank) % capacity while rank < room,
//             as six 16-byte vectors, and the row is zeroed), then S2 and S3 for the detection pass 0 found, field by field - a free entry
//             is all zero, so opening one sets five fields -, then one job for the copy kernel.
//   Thread 0 stores the queue count and the three running totals: plain loads and stores.
// sightings_copy_kernel - one workgroup per job, early exit on an empty one.  In this order, every thread on the same vectors in each step,
//   so that a slot that closed and is reopened in the same update hands its OLD payload to the queue: entry rows -> queue row; zero the entry
//   rows; the observed face's template / embedding / crop -> entry rows.  Crops move as 2 352 16-byte vectors, dim floats as floatx4.
// sightings_close_kernel - frt_sightings_close: S1 with "ends" = "is open", over streams instead of frames (up to 1024: 16 per lane in the prefix).
#include "frt_kernels.h"

namespace {

constexpr int PLAN_WAVES = 16, COPY_THREADS = 256;
constexpr int CROP_VECS = FRT_SIGHTING_CROP_BYTES / 16;  // 2 352
typedef unsigned int uintx4 __attribute__((ext_vector_type(4)));

// exclusive offsets of N = 64 * PER_LANE counts popc(s_mask[i]), by wave 0; s_total <- their sum
template <int PER_LANE>
__device__ __forceinline__ void prefix_counts(const unsigned long long *s_mask, int *s_off, int *s_total, int lane) {
    int c[PER_LANE], sum = 0;
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) {
        c[k] = __popcll(s_mask[lane * PER_LANE + k]);
        sum += c[k];
    }
    int incl = sum;
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    int run = incl - sum;
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) {
        s_off[lane * PER_LANE + k] = run;
        run += c[k];
    }
    if (lane == 63) *s_total = incl;
}

// S1 for the entry `g` a lane owns, once it is known to end: the record leaves for queue row (head + queued + rank) % capacity - its six
// 16-byte vectors, with close_tick and reason (words 4 and 5) set on the way - or is counted lost; the entry is zeroed.  -> the job's qrow
static_assert(sizeof(frt_sighting) == 96 && offsetof(frt_sighting, close_tick) == 16 && offsetof(frt_sighting, reason) == 20, "frt_sighting");
__device__ __forceinline__ int close_entry(const SightingArgs &a, frt_sighting &g, int reason, int close_tick, bool queue, int rank, int queued,
                                           int room) {
    uintx4 *src = reinterpret_cast<uintx4 *>(&g);
    int qrow = -2;
    if (queue && rank < room) {
        qrow = (a.head + queued + rank) % a.capacity;
        uintx4 *dst = reinterpret_cast<uintx4 *>(a.records + a.n_open + qrow);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            uintx4 v = src[k];
            if (k == 1) {
                v.x = (unsigned)close_tick;
                v.y = (unsigned)reason;
            }
            dst[k] = v;
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) src[k] = uintx4{0u, 0u, 0u, 0u};
    return qrow;
}

__device__ __forceinline__ void store_totals(const SightingArgs &a, int queued, int room, int total, int discarded, int closed) {
    const int appended = total < room ? total : room;
    a.state[0] = queued + appended;
    a.state[1] += total - appended;
    a.state[2] += discarded;
    a.state[3] += closed;
}

__global__ __launch_bounds__(64 * PLAN_WAVES) void sightings_plan_kernel(SightingArgs a, TrackStreamIds ids, int n_frames) {
    __shared__ unsigned long long s_queue[FRT_TRACK_MAX_FRAMES];  // the closers of a frame that are to be queued
    __shared__ unsigned long long s_close[FRT_TRACK_MAX_FRAMES];  // all its closers
    __shared__ int s_off[FRT_TRACK_MAX_FRAMES];
    __shared__ signed char s_det[FRT_TRACK_MAX_FRAMES * FRT_TRACK_MAX_SLOTS];  // [f][t]: the detection slot 0 .. 63 tracked into slot t, or -1
    __shared__ int s_total, s_discarded, s_closed;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int T = a.max_tracks, MF = a.max_faces, NF = n_frames;
    if (tid < FRT_TRACK_MAX_FRAMES && tid >= NF) s_queue[tid] = 0;
    if (tid == 0) s_discarded = s_closed = 0;
    for (int i = tid; i < NF * FRT_TRACK_MAX_SLOTS; i += 64 * PLAN_WAVES) s_det[i] = -1;
    __syncthreads();

    // ---- pass 0
    for (int f = wave; f < NF; f += PLAN_WAVES) {
        if (lane < MF) {
            const frt_track_result tr = a.tracks[(long)f * MF + lane];
            if (tr.track_id >= 0 && tr.slot >= 0 && tr.slot < T) s_det[f * FRT_TRACK_MAX_SLOTS + tr.slot] = (signed char)lane;
        }
    }
    // ---- pass A
    int n_disc = 0, n_close = 0;
    for (int f = wave; f < NF; f += PLAN_WAVES) {
        const long row = (long)ids.id[f] * T + lane;
        bool ends = false, queue = false;
        if (lane < T) {
            const frt_sighting &e = a.records[row];
            const frt_track_state &st = a.slots[row];
            ends = e.close_tick == -1 && !(st.live != 0 && st.id == e.track_id);
            queue = ends && e.hits >= a.min_hits;
        }
        const unsigned long long mc = __ballot(ends), mq = __ballot(queue);
        if (lane == 0) {
            s_close[f] = mc;
            s_queue[f] = mq;
        }
        n_close += __popcll(mc);
        n_disc += __popcll(mc & ~mq);
    }
    if (lane == 0 && n_close) {
        atomicAdd(&s_closed, n_close);
        atomicAdd(&s_discarded, n_disc);
    }
    __syncthreads();
    if (wave == 0) prefix_counts<FRT_TRACK_MAX_FRAMES / 64>(s_queue, s_off, &s_total, lane);
    __syncthreads();

    // ---- pass B
    const int queued = a.state[0] - a.taken, room = a.capacity - queued;
    for (int f = wave; f < NF; f += PLAN_WAVES) {
        const int stream = ids.id[f];
        const int tick = a.counters[stream * 4 + 1] - 1;
        const long row = (long)stream * T + lane;
        const unsigned long long mc = s_close[f], mq = s_queue[f];
        const int d = lane < T ? (int)s_det[f * FRT_TRACK_MAX_SLOTS + lane] : -1;
        const bool ends = (mc >> lane) & 1;
        SightingJob job = {(int32_t)row, -1, -1, 0};
        if (lane < T && (ends || d >= 0)) {
            frt_sighting &g = a.records[row];  // this lane's alone; what it reads below it has not written in this launch
            bool open = !ends && g.close_tick == -1;
            if (ends)  // ---- S1
                job.qrow = close_entry(a, g, a.slots[row].live == 0 ? FRT_SIGHTING_EXPIRED : FRT_SIGHTING_REPLACED, tick, (mq >> lane) & 1,
                                       s_off[f] + __popcll(mq & ((1ull << lane) - 1ull)), queued, room);
            if (d >= 0) {
                const long face = (long)f * MF + d;
                const frt_track_result tr = a.tracks[face];
                int n_shots = 0, best_tick = -1;
                unsigned best_flags = 0, best_key = 0;
                if (open) {
                    n_shots = g.n_shots;
                    best_tick = g.best_tick;
                    best_flags = g.best_flags;
                    best_key = a.best_key[row];
                } else {  // ---- S2: a free entry is all zero
                    g.stream = stream;
                    g.track_id = tr.track_id;
                    g.first_tick = tick - tr.age + 1;
                    g.close_tick = -1;
                    g.best_tick = -1;
                }
                g.last_tick = tick;
                g.hits = tr.hits;
                g.n_embeds = tr.n_embeds;
                g.confirmed = tr.confirmed;
                g.match_idx = tr.match_idx;
                g.match_sim = tr.match_sim;
                job.face = (int32_t)face;
                const frt_face_result &r = a.results[face];
                const struct frt_face_quality &q = a.quality[face];
                if (r.valid != 0 && q.present != 0) {  // ---- S3
                    g.n_shots = n_shots + 1;
                    const unsigned flags = q.flags;
                    const int size = q.size;
                    const unsigned key = a.rank == FRT_SHOT_RANK_SIZE ? (unsigned)size
                                                                      : __float_as_uint(a.rank == FRT_SHOT_RANK_SCORE ? q.score : q.sharpness);
                    const bool greater = a.rank == FRT_SHOT_RANK_SIZE ? (int)key > (int)best_key : __uint_as_float(key) > __uint_as_float(best_key);
                    const int pass = flags == 0, old_pass = best_flags == 0;
                    if (best_tick < 0 || pass > old_pass || (pass == old_pass && greater)) {
                        g.best_tick = tick;
                        g.best_box = r.box;
                        g.best_sharpness = q.sharpness;
                        g.best_luma_var = q.luma_var;
                        g.best_mean = q.mean;
                        g.best_flags = flags;
                        g.best_size = size;
                        a.best_key[row] = key;
                        job.replace = 1;
                    }
                }
            }
        }
        if (lane < T) a.jobs[f * T + lane] = job;
    }
    if (tid == 0) store_totals(a, queued, room, s_total, s_discarded, s_closed);
}

// grid: the streams in groups of 64 * CLOSE_PER_LANE at most - one group, n_streams <= 1024
constexpr int CLOSE_PER_LANE = FRT_TRACK_MAX_STREAMS / 64;
__global__ __launch_bounds__(64 * PLAN_WAVES) void sightings_close_kernel(SightingArgs a, int first_stream, int n) {
    __shared__ unsigned long long s_queue[FRT_TRACK_MAX_STREAMS];
    __shared__ int s_off[FRT_TRACK_MAX_STREAMS];
    __shared__ int s_total, s_discarded, s_closed;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int T = a.max_tracks;
    if (tid >= n) s_queue[tid] = 0;  // (the workgroup has FRT_TRACK_MAX_STREAMS threads)
    if (tid == 0) s_discarded = s_closed = 0;
    __syncthreads();
    int n_disc = 0, n_close = 0;
    for (int i = wave; i < n; i += PLAN_WAVES) {
        bool ends = false, queue = false;
        if (lane < T) {
            const frt_sighting &e = a.records[(long)(first_stream + i) * T + lane];
            ends = e.close_tick == -1;
            queue = ends && e.hits >= a.min_hits;
        }
        const unsigned long long mc = __ballot(ends), mq = __ballot(queue);
        if (lane == 0) s_queue[i] = mq;
        n_close += __popcll(mc);
        n_disc += __popcll(mc & ~mq);
    }
    if (lane == 0 && n_close) {
        atomicAdd(&s_closed, n_close);
        atomicAdd(&s_discarded, n_disc);
    }
    __syncthreads();
    if (wave == 0) prefix_counts<CLOSE_PER_LANE>(s_queue, s_off, &s_total, lane);
    __syncthreads();
    const int queued = a.state[0] - a.taken, room = a.capacity - queued;
    for (int i = wave; i < n; i += PLAN_WAVES) {
        const long row = (long)(first_stream + i) * T + lane;
        const unsigned long long mq = s_queue[i];
        if (lane < T) {
            SightingJob job = {(int32_t)row, -1, -1, 0};
            frt_sighting &g = a.records[row];
            if (g.close_tick == -1)
                job.qrow = close_entry(a, g, FRT_SIGHTING_CLOSED, g.last_tick, (mq >> lane) & 1, s_off[i] + __popcll(mq & ((1ull << lane) - 1ull)),
                                       queued, room);
            a.jobs[i * T + lane] = job;
        }
    }
    if (tid == 0) store_totals(a, queued, room, s_total, s_discarded, s_closed);
}

// dst row <- src row (null: zeros), dim floats and - with crops - one crop
__device__ __forceinline__ void move_rows(const SightingArgs &a, int tid, float *dst_e, const float *src_e, float *dst_t, const float *src_t,
                                          uint8_t *dst_c, const uint8_t *src_c, bool zero) {
    for (int k = tid * 4; k < a.dim; k += COPY_THREADS * 4) {
        if (dst_e) *reinterpret_cast<floatx4 *>(dst_e + k) = zero ? floatx4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const floatx4 *>(src_e + k);
        if (dst_t) *reinterpret_cast<floatx4 *>(dst_t + k) = zero ? floatx4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const floatx4 *>(src_t + k);
    }
    if (dst_c)
        for (int v = tid; v < CROP_VECS; v += COPY_THREADS)
            reinterpret_cast<uintx4 *>(dst_c)[v] = zero ? uintx4{0u, 0u, 0u, 0u} : reinterpret_cast<const uintx4 *>(src_c)[v];
}

__global__ __launch_bounds__(COPY_THREADS) void sightings_copy_kernel(SightingArgs a) {
    const SightingJob job = a.jobs[blockIdx.x];
    if (job.qrow == -1 && job.face < 0) return;  // (workgroup-uniform)
    const int tid = threadIdx.x;
    const long D = a.dim, e = job.entry;
    float *ee = a.best_embeds + e * D, *et = a.templates + e * D;
    uint8_t *ec = a.crops ? a.crops + e * FRT_SIGHTING_CROP_BYTES : nullptr;
    if (job.qrow >= 0) {
        const long q = (long)a.n_open + job.qrow;
        move_rows(a, tid, a.best_embeds + q * D, ee, a.templates + q * D, et, ec ? a.crops + q * FRT_SIGHTING_CROP_BYTES : nullptr, ec, false);
    }
    if (job.qrow != -1) move_rows(a, tid, ee, nullptr, et, nullptr, ec, nullptr, true);
    if (job.face >= 0) {
        const long f = job.face;
        move_rows(a, tid, job.replace ? ee : nullptr, a.embeds + f * D, a.call_templates ? et : nullptr, a.call_templates + f * D,
                  job.replace ? ec : nullptr, a.call_crops + f * FRT_SIGHTING_CROP_BYTES, false);
    }
}

}  // namespace

void launch_sightings_plan(const SightingArgs &a, const TrackStreamIds &ids, int n_frames, hipStream_t s) {
    if (n_frames <= 0) return;
    hipLaunchKernelGGL(sightings_plan_kernel, dim3(1), dim3(64 * PLAN_WAVES), 0, s, a, ids, n_frames);
}

void launch_sightings_copy(const SightingArgs &a, int n_jobs, hipStream_t s) {
    if (n_jobs <= 0) return;
    hipLaunchKernelGGL(sightings_copy_kernel, dim3((unsigned)n_jobs), dim3(COPY_THREADS), 0, s, a);
}

void launch_sightings_close(const SightingArgs &a, int n_streams, int stream, hipStream_t s) {
    const int first = stream < 0 ? 0 : stream, count = stream < 0 ? n_streams : 1;
    hipLaunchKernelGGL(sightings_close_kernel, dim3(1), dim3(64 * PLAN_WAVES), 0, s, a, first, count);
}
