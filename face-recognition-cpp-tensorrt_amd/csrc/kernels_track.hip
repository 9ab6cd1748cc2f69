// Face tracker for gfx950: the per-stream track state in HBM and one update of it (include/frt.h "Face tracker"; DESIGN §3.37;
// tests/track_ref.py is the contract, to the integer and - for the sums - to the bit).
//
// track_update_kernel, one workgroup of four waves per frame:
//   - wave 0 holds the stream's slots one per lane and walks the frame's detections in slot order: the overlap of the detection with every
//     candidate track is one value per lane, the winner one 64-lane max-reduction over (overlap bits, 63 - lane) - the largest overlap, the
//     lowest slot among equals -, the free-slot mask of a birth one ballot and the slot its first set bit.  It writes the slots, the
//     counters and the records, and leaves the detection -> slot table and the mask of the slots that expired in LDS;
//   - behind one barrier every wave zeroes the sums of the expired slots, and behind a second one the waves take the detections in turn:
//     a row of `dim` floats is 16 bytes per lane and 256-column group, as template_build_kernel holds a row, the squared norm is its fmaf
//     chain per lane and its xor butterfly over the wave, the template is scaled in registers.
// The sum is fl(fl(decay * sum) + e): two roundings.  This file is compiled without fp contraction (Makefile: EXACT) and the update is
// written with the rounding intrinsics as well, so neither the sums nor the overlaps can turn into an fma.
// Bounds: a frame index is blockIdx.x < n_frames, a stream id was checked on the host against n_streams, a slot index is < max_tracks <= 64,
// a column is tested against dim before every access.
//
// Appearance (include/frt.h "Appearance"; tests/track_reid_ref.py), only for a tracker that has it on:
//   - track_similarity_kernel, one workgroup of four waves per detection, runs BEFORE the update and so reads the sums at entry.  Every wave
//     holds the detection's row in registers, 16 bytes per lane and 256-column group, and takes the slots wave, wave + 4, ...: a pair is
//     one wave.  dot2r is a chain of __fadd_rn(acc, __fmul_rn(x, y)) per lane - two roundings, the order of the header - and the xor
//     butterfly; S = dot2r(e, sum) / sqrtf(dot2r(sum, sum)), both correctly rounded in this build (the toolchain's __fsqrt_rn is the native
//     square root, which is not).  A pair that cannot be DEFINED is skipped before its sum is read; lane 0 writes S[f][d][t], and the
//     workgroup one 64-bit mask of the defined slots per detection (four words of LDS carry the waves' parts to thread 0).
//   - track_update_kernel<true>: lane t of wave 0 reads S[d][t] and its bit per detection; 2a drops the vetoed candidates, 2b is a second
//     walk over the detections under the same reduction, keyed by (S bits, 63 - lane) - S >= reid_threshold > 0 keeps the bits monotone.
//     Lane d collects how its detection was associated.  track_update_kernel<false> is the kernel of a tracker without appearance.
//   Bounds: the grid of the similarity kernel is (max_faces, n_frames); its slot index is tested against max_tracks, its columns against dim;
//   the update kernel reads S[d][lane] only where the defined bit of lane is set, and bits are set for slots < max_tracks only.
//
// Gate (include/frt.h "Gate"; tests/track_gate_ref.py), in front of the recogniser of frt_pipeline_run_tracked_gated:
//   - track_gate_kernel, ONE workgroup of sixteen waves for the whole call; wave w takes the frames w, w + 16, ...  A wave holds its frame's
//     stream one slot per lane as wave 0 of the update does and walks the detections with the update's own reduction (step 2 without the
//     appearance terms, and without writing the state: a winner is only marked taken).  Lane d keeps the record of detection d; the frame's
//     EMBED set is one ballot, kept in LDS.  Behind one barrier wave 0 turns the 256 popcounts into exclusive offsets (four frames per lane,
//     a shuffle scan over the lanes); behind a second one every wave writes its frames' part of the list - a detection's place is the frame's
//     offset plus the set bits below its own -, so the list is ascending without a sort and the same on every run.  The entries past the count
//     are -1, pass_count[j] is tile_faces_select_kernel's.
//   - track_gate_scatter_kernel, one wave per face slot: the list is ascending, so whether slot i is in it, and where, is a binary search of
//     at most 14 wave-uniform steps; the row is 16 bytes per lane and 256-column group, zeros for a slot that is not in the list.
//   Bounds: a frame index is < n_frames <= 256 (the LDS tables' length), a stream id was checked on the host, a slot index is the lane and
//   tested against max_tracks, a detection index is < max_faces <= 64; a list position is offset + bits below < the count <= n_frames *
//   max_faces, the list's length; n_boxes[f] is only compared.  The scatter clamps the count it reads to 0 .. n_frames * max_faces, reads
//   list[j] for j below it only and the compact rows at such j only; its own row index is tested against n_frames * max_faces.
//
// Motion (include/frt.h "Motion"; tests/track_motion_ref.py), only for a tracker that has it on: track_update_kernel<.., true>
// and track_gate_kernel<true>.  Lane t of the wave that holds the slots loads its slot's (vx, vy) as one 8-byte load and computes its
// predicted box once, in front of the detection walk (M1: the state at entry decides it); every iou() with a track's box takes that box
// instead.  The lane that wins a detection applies M2 before it overwrites its box, expiry and birth zero the pair (M3), and the update
// stores it beside the slot; the gate stores nothing.  Integers throughout: the one real division is an unsigned 32-bit one, the two / 256
// are a 64-bit multiply and a sign-corrected shift.  The MOTION = false instantiations do not touch the vel / motion_gain arguments.
//   Bounds: the velocity index is stream * max_tracks + lane with lane < max_tracks, the index of the slot it sits beside; the array holds
//   n_streams * max_tracks pairs and exists whenever motion_gain > 0 (frt_tracker.cpp: ensure_state, checked again before the launch).
#include "frt_kernels.h"

namespace {

constexpr int WAVES = 4, GROUPS = FRT_TRACK_MAX_DIM / 256;

__device__ __forceinline__ float wave_sum(float v) {  // xor butterfly: every lane ends with the same bits
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ float dot4(floatx4 a, floatx4 b, float acc) { return fmaf(a[3], b[3], fmaf(a[2], b[2], fmaf(a[1], b[1], fmaf(a[0], b[0], acc)))); }

__device__ __forceinline__ float box_area(const frt_bbox &b) {  // (float) of the exact product
    return (float)(((long long)b.x2 - b.x1 + 1) * ((long long)b.y2 - b.y1 + 1));
}
// nms_kernel's statements (kernels_post.hip), metric 0
__device__ __forceinline__ float iou(const frt_bbox &a, const frt_bbox &b) {
    const float xx1 = (float)(a.x1 > b.x1 ? a.x1 : b.x1);
    const float yy1 = (float)(a.y1 > b.y1 ? a.y1 : b.y1);
    const float xx2 = (float)(a.x2 < b.x2 ? a.x2 : b.x2);
    const float yy2 = (float)(a.y2 < b.y2 ? a.y2 : b.y2);
    float w = xx2 - xx1 + 1;
    float h = yy2 - yy1 + 1;
    if (w < 0.f) w = 0.f;
    if (h < 0.f) h = 0.f;
    const float inter = w * h;
    return inter / (box_area(a) + box_area(b) - inter);
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, off), hi = __shfl_xor((unsigned)(v >> 32), off);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

// ---- motion (include/frt.h "Motion"): integers throughout; tests/track_motion_ref.py restates them
// tdiv(a, 256) for an int64: the arithmetic shift floors, so a negative a gets 255 first - truncation toward zero without a 64-bit divide
__device__ __forceinline__ long long tdiv256(long long a) { return (a + ((a >> 63) & 255)) >> 8; }
__device__ __forceinline__ int clamp_i32(long long v) { return (int)(v < -2147483648ll ? -2147483648ll : (v > 2147483647ll ? 2147483647ll : v)); }
// M1: the box of a track live at entry, moved by its velocity times (missed + 1)
__device__ __forceinline__ frt_bbox predicted_box(const frt_track_state &st, int vx, int vy) {
    const long long k = (long long)st.missed + 1, lim = 1ll << 30;
    long long sx = tdiv256((long long)vx * k), sy = tdiv256((long long)vy * k);
    sx = sx < -lim ? -lim : (sx > lim ? lim : sx);
    sy = sy < -lim ? -lim : (sy > lim ? lim : sy);
    return frt_bbox{clamp_i32(st.box.x1 + sx), clamp_i32(st.box.y1 + sy), clamp_i32(st.box.x2 + sx), clamp_i32(st.box.y2 + sy), st.box.score};
}
// M2, one axis: dc2 the doubled centre displacement from the last measured box, g = missed at entry + 1 (as unsigned: 1 .. 2^31).  |dc * 128|
// <= 2^29, so the one real division is an unsigned 32-bit one and its sign is put back
__device__ __forceinline__ int matched_velocity(int v, long long dc2, unsigned g, bool first, int gain) {
    const long long lim = 1ll << 22;
    const int num = (int)(dc2 < -lim ? -lim : (dc2 > lim ? lim : dc2)) * 128;
    const int q = (int)((unsigned)(num < 0 ? -num : num) / g), raw = num < 0 ? -q : q;
    return first ? raw : v + (int)tdiv256((long long)(raw - v) * gain);
}

// M2 of the lane that won: st is its state at entry (the last measured box, hits, missed), det the detection it takes
__device__ __forceinline__ int2 matched(int2 v, const frt_bbox &det, const frt_track_state &st, int gain) {
    const unsigned g = (unsigned)st.missed + 1u;
    const bool first = st.hits == 1;
    return int2{matched_velocity(v.x, ((long long)det.x1 + det.x2) - ((long long)st.box.x1 + st.box.x2), g, first, gain),
                matched_velocity(v.y, ((long long)det.y1 + det.y2) - ((long long)st.box.y1 + st.box.y2), g, first, gain)};
}

// columns k .. k + 3 of a row of dim floats, zeros past dim: the load is of column 0 there and a select drops it, so no lane branches
__device__ __forceinline__ floatx4 row_at(const float *row, int k, int dim) {
    const floatx4 v = *reinterpret_cast<const floatx4 *>(row + (k < dim ? k : 0));
    return k < dim ? v : floatx4{0.f, 0.f, 0.f, 0.f};
}

// grid (max_faces, n_frames)
__global__ __launch_bounds__(64 * WAVES) void track_similarity_kernel(TrackArgs a, TrackStreamIds ids) {
    __shared__ unsigned long long s_defined[WAVES];
    const int d = blockIdx.x, f = blockIdx.y, stream = ids.id[f];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int T = a.max_tracks, MF = a.max_faces, D = a.dim;
    const frt_face_result *r = a.results + (long)f * MF + d;
    unsigned long long defined = 0;  // (wave-uniform) the slots this wave found DEFINED
    if (r->box.score > 0.f && r->valid != 0) {
        const float *e = a.embeds + ((long)f * MF + d) * D;
        const frt_track_state *slots = a.slots + (long)stream * T;
        const float *sums = a.sums + (long)stream * T * D;
        float *S = a.sim + ((long)f * MF + d) * T;
        floatx4 x[GROUPS];
#pragma unroll
        for (int g = 0; g < GROUPS; ++g) {
            const int k = g * 256 + lane * 4;
            x[g] = row_at(e, k, D);
        }
        for (int t = wave; t < T; t += WAVES) {
            if (slots[t].live == 0 || slots[t].n_embeds <= 0) continue;  // (wave-uniform) not DEFINED: the sum is not read
            const float *sum = sums + (long)t * D;
            float n2 = 0.f, dp = 0.f;
#pragma unroll
            for (int g = 0; g < GROUPS; ++g) {
                if (g * 256 >= D) break;  // (wave-uniform)
                const int k = g * 256 + lane * 4;
                const floatx4 y = row_at(sum, k, D);
                // a column past dim adds fl(0 * 0) = +0, which leaves acc as it is: acc is never -0 (it starts at +0, and a sum that
                // cancels rounds to +0), so the lanes of a partial group need no branch of their own
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    n2 = __fadd_rn(n2, __fmul_rn(y[j], y[j]));
                    dp = __fadd_rn(dp, __fmul_rn(x[g][j], y[j]));
                }
            }
            n2 = wave_sum(n2);
            dp = wave_sum(dp);
            if (!(n2 > 0.f)) continue;
            if (lane == 0) S[t] = dp / sqrtf(n2);
            defined |= 1ull << t;
        }
    }
    if (lane == 0) s_defined[wave] = defined;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0;
        for (int w = 0; w < WAVES; ++w) all |= s_defined[w];
        a.sim_defined[(long)f * MF + d] = all;
    }
}

template <bool APPEARANCE, bool MOTION>
__global__ __launch_bounds__(64 * WAVES) void track_update_kernel(TrackArgs a, TrackStreamIds ids) {
    __shared__ int s_slot[FRT_TRACK_MAX_SLOTS];  // detection -> slot; -1: untracked or absent
    __shared__ unsigned long long s_expired;     // slots freed by this update (their sums are zeroed before a birth's embedding lands)
    const int f = blockIdx.x, stream = ids.id[f];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int T = a.max_tracks, MF = a.max_faces, D = a.dim;
    const frt_face_result *res = a.results + (long)f * MF;
    frt_track_state *slots = a.slots + (long)stream * T;
    float *sums = a.sums + (long)stream * T * D;

    if (wave == 0) {
        int32_t *cnt = a.counters + stream * 4;
        int next_id = cnt[0], dropped = cnt[2];
        const int tick = cnt[1];
        const bool mine = lane < T;
        frt_track_state st = {};
        if (mine) st = slots[lane];
        const bool live_entry = mine && st.live != 0;
        // MOTION: lane t holds its slot's velocity and, from the state at entry, the box every overlap below is taken with (M1)
        int2 v = {0, 0};
        frt_bbox pred = st.box;
        if constexpr (MOTION) {
            if (mine) v = a.vel[(long)stream * T + lane];
            if (live_entry) pred = predicted_box(st, v.x, v.y);
        }
        bool taken = false;
        int my_slot = -1;        // lane d: the slot of detection d
        bool my_present = false;
        // APPEARANCE: lane d keeps how detection d was associated; S and its defined bits of this frame, [max_faces][max_tracks] / [max_faces]
        frt_track_assoc my_assoc = {};
        const bool veto_on = APPEARANCE && a.iou_min_sim >= -1.f, reid_on = APPEARANCE && a.reid_threshold <= 1.f;
        const float *S = APPEARANCE ? a.sim + (long)f * MF * T : nullptr;
        const unsigned long long *S_defined = APPEARANCE ? a.sim_defined + (long)f * MF : nullptr;

        // ---- steps 1, 2 (2a): association by overlap, detections in slot order
        for (int d = 0; d < MF; ++d) {
            const frt_face_result r = res[d];
            if (!(r.box.score > 0.f)) continue;  // (wave-uniform)
            if (lane == d) my_present = true;
            bool defined = false;  // lane t: S[d][t] is DEFINED, and s is its value
            float s = 0.f;
            if constexpr (APPEARANCE) {
                defined = (S_defined[d] >> lane) & 1;
                if (defined) s = S[(long)d * T + lane];
            }
            unsigned long long key = 0;  // (overlap bits, 63 - lane); an overlap that reaches the threshold is > 0, so 0 is "no candidate"
            if (live_entry && !taken && !(veto_on && defined && s < a.iou_min_sim)) {
                const float ovr = iou(r.box, MOTION ? pred : st.box);
                if (ovr >= a.iou_threshold) key = ((unsigned long long)__float_as_uint(ovr) << 32) | (unsigned)(63 - lane);
            }
            key = wave_max_u64(key);
            if (key == 0) continue;
            const int win = 63 - (int)(key & 63);
            if constexpr (APPEARANCE) {
                const int gap = __shfl(st.missed, win);
                const float sim = __shfl(s, win);
                if (lane == d) my_assoc = frt_track_assoc{1, gap, __uint_as_float((unsigned)(key >> 32)), sim};
            }
            if (lane == win) {
                if constexpr (MOTION) v = matched(v, r.box, st, a.motion_gain);
                st.box = r.box;
                st.hits += 1;
                st.missed = 0;
                taken = true;
            }
            if (lane == d) my_slot = win;
        }
        // ---- step 2b: what 2a left unmatched, by appearance, detections in slot order
        if constexpr (APPEARANCE) {
            for (int d = 0; reid_on && d < MF; ++d) {
                const int present = __shfl((int)my_present, d), slot_d = __shfl(my_slot, d);
                if (!present || slot_d >= 0) continue;  // (wave-uniform)
                const unsigned long long defined_d = S_defined[d];  // (0 for a detection with valid == 0)
                if (defined_d == 0) continue;
                const frt_face_result r = res[d];
                const bool defined = (defined_d >> lane) & 1;
                const float s = defined ? S[(long)d * T + lane] : 0.f;
                unsigned long long key = 0;  // (S bits, 63 - lane): S >= reid_threshold > 0, so the bits order as the values do
                if (live_entry && !taken && defined && s >= a.reid_threshold) key = ((unsigned long long)__float_as_uint(s) << 32) | (unsigned)(63 - lane);
                key = wave_max_u64(key);
                if (key == 0) continue;
                const int win = 63 - (int)(key & 63);
                const int gap = __shfl(st.missed, win);
                const float ovr = __shfl(iou(r.box, MOTION ? pred : st.box), win);
                if (lane == d) {
                    my_assoc = frt_track_assoc{2, gap, ovr, __uint_as_float((unsigned)(key >> 32))};
                    my_slot = win;
                }
                if (lane == win) {
                    if constexpr (MOTION) v = matched(v, r.box, st, a.motion_gain);
                    st.box = r.box;
                    st.hits += 1;
                    st.missed = 0;
                    taken = true;
                }
            }
        }
        // ---- step 3: expiry
        bool expired = false;
        if (live_entry && !taken) {
            st.missed += 1;
            if (st.missed > a.max_missed) {
                st = frt_track_state{};
                if constexpr (MOTION) v = int2{0, 0};  // M3
                expired = true;
            }
        }
        const unsigned long long expired_mask = __ballot(expired);
        // ---- step 4: births, the lowest free slot each
        for (int d = 0; d < MF; ++d) {
            const int present = __shfl((int)my_present, d), slot_d = __shfl(my_slot, d);
            if (!present || slot_d >= 0) continue;  // (wave-uniform)
            const unsigned long long free_mask = __ballot(mine && st.live == 0);
            if (free_mask == 0) {
                ++dropped;
                if (lane == d) my_assoc.how = 4;
                continue;
            }
            const int b = __ffsll((long long)free_mask) - 1;
            if (lane == b) {
                st.live = 1;
                st.id = next_id;
                st.box = res[d].box;
                st.born = tick;
                st.hits = 1;
                st.missed = 0;
                st.n_embeds = 0;
                st.match_idx = -1;
                st.match_sim = 0.f;
                if constexpr (MOTION) v = int2{0, 0};  // M3
            }
            ++next_id;
            if (lane == d) {
                my_slot = b;
                my_assoc.how = 3;
            }
        }
        // ---- step 5, the count: a track is matched by at most one detection
        for (int d = 0; d < MF; ++d) {
            const int slot_d = __shfl(my_slot, d);
            if (slot_d >= 0 && res[d].valid != 0 && lane == slot_d) st.n_embeds += 1;
        }
        // ---- the records: lane d fetches the state of its slot
        {
            const int src = my_slot >= 0 ? my_slot : 0;
            const int id = __shfl(st.id, src), born = __shfl(st.born, src), hits = __shfl(st.hits, src), ne = __shfl(st.n_embeds, src);
            if (lane < MF) {
                frt_track_result o = {};
                o.track_id = o.slot = o.match_idx = -1;
                if (my_slot >= 0) {
                    o.track_id = id;
                    o.slot = my_slot;
                    o.age = tick - born + 1;
                    o.hits = hits;
                    o.n_embeds = ne;
                    o.confirmed = hits >= a.min_hits ? 1 : 0;
                }
                a.tracks[(long)f * MF + lane] = o;
                s_slot[lane] = my_slot;
                if constexpr (APPEARANCE)
                    if (a.assoc) a.assoc[(long)f * MF + lane] = my_assoc;
            }
        }
        if (mine) {
            slots[lane] = st;
            if constexpr (MOTION) a.vel[(long)stream * T + lane] = v;
        }
        if (lane == 0) {
            cnt[0] = next_id;
            cnt[1] = tick + 1;  // step 8
            cnt[2] = dropped;
            s_expired = expired_mask;
        }
    }
    __syncthreads();

    // ---- the sums of the slots that expired: zero, whether or not a birth has taken the slot again
    const unsigned long long expired_mask = s_expired;
    for (int t = wave; t < T; t += WAVES) {
        if (!((expired_mask >> t) & 1)) continue;
        for (int k = lane * 4; k < D; k += 256) *reinterpret_cast<floatx4 *>(sums + (long)t * D + k) = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();

    // ---- steps 5, 6: one wave per detection
    for (int d = wave; d < MF; d += WAVES) {
        const int slot = s_slot[d];
        float *tout = a.templates ? a.templates + ((long)f * MF + d) * D : nullptr;
        if (slot < 0) {
            if (tout)
                for (int k = lane * 4; k < D; k += 256) *reinterpret_cast<floatx4 *>(tout + k) = floatx4{0.f, 0.f, 0.f, 0.f};
            continue;
        }
        const bool valid = res[d].valid != 0;
        float *sum = sums + (long)slot * D;
        const float *e = a.embeds + ((long)f * MF + d) * D;
        floatx4 v[GROUPS];
        float n2 = 0.f;
#pragma unroll
        for (int g = 0; g < GROUPS; ++g) {
            const int k = g * 256 + lane * 4;
            v[g] = floatx4{0.f, 0.f, 0.f, 0.f};
            if (k < D) {
                v[g] = *reinterpret_cast<const floatx4 *>(sum + k);
                if (valid) {
                    const floatx4 x = *reinterpret_cast<const floatx4 *>(e + k);
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[g][j] = __fadd_rn(__fmul_rn(a.decay, v[g][j]), x[j]);
                    *reinterpret_cast<floatx4 *>(sum + k) = v[g];
                }
            }
            n2 = dot4(v[g], v[g], n2);
        }
        if (!tout) continue;
        n2 = wave_sum(n2);
        const bool zero = n2 == 0.f;
        const float nrm = sqrtf(n2);
#pragma unroll
        for (int g = 0; g < GROUPS; ++g) {
            const int k = g * 256 + lane * 4;
            if (k < D) *reinterpret_cast<floatx4 *>(tout + k) = zero ? floatx4{0.f, 0.f, 0.f, 0.f} : v[g] / nrm;
        }
    }
}

// one thread per face slot of the call
__global__ __launch_bounds__(256) void track_identity_kernel(TrackArgs a, TrackStreamIds ids, int n_frames, const int32_t *__restrict__ idx,
                                                             const float *__restrict__ sim) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_frames * a.max_faces) return;
    frt_track_result &o = a.tracks[i];
    if (o.slot < 0 || o.n_embeds <= 0) return;  // (the update kernel left -1 / 0 there)
    frt_track_state &st = a.slots[(long)ids.id[i / a.max_faces] * a.max_tracks + o.slot];
    st.match_idx = o.match_idx = idx[i];
    st.match_sim = o.match_sim = sim[i];
}

// grid (slots, streams to reset): a wave zeroes one slot and its sums; slot 0's wave the stream's tick and dropped
__global__ __launch_bounds__(64) void track_reset_kernel(TrackArgs a, int first_stream) {
    const int stream = first_stream + blockIdx.y, t = blockIdx.x, lane = threadIdx.x;
    float *sum = a.sums + ((long)stream * a.max_tracks + t) * a.dim;
    for (int k = lane * 4; k < a.dim; k += 256) *reinterpret_cast<floatx4 *>(sum + k) = floatx4{0.f, 0.f, 0.f, 0.f};
    if (lane == 0) {
        a.slots[(long)stream * a.max_tracks + t] = frt_track_state{};
        if (a.vel) a.vel[(long)stream * a.max_tracks + t] = int2{0, 0};
        if (t == 0) a.counters[stream * 4 + 1] = a.counters[stream * 4 + 2] = 0;
    }
}

constexpr int GATE_WAVES = 16;

// one workgroup for the call (see the header comment)
template <bool MOTION>
__global__ __launch_bounds__(64 * GATE_WAVES) void track_gate_kernel(TrackGateArgs a, TrackStreamIds ids) {
    __shared__ unsigned long long s_mask[FRT_TRACK_MAX_FRAMES];  // the EMBED detections of a frame
    __shared__ int s_off[FRT_TRACK_MAX_FRAMES];                  // list entries in front of a frame's
    __shared__ int s_total;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int T = a.max_tracks, MF = a.max_faces, NF = a.n_frames;
    if (tid < FRT_TRACK_MAX_FRAMES && tid >= NF) s_mask[tid] = 0;

    for (int f = wave; f < NF; f += GATE_WAVES) {
        const int stream = ids.id[f];
        const frt_bbox *boxes = a.boxes + (long)f * MF;
        const int n_present = a.n_boxes ? a.n_boxes[f] : MF;
        frt_track_state st = {};
        int2 v = {0, 0};
        if (lane < T) {
            st = a.slots[(long)stream * T + lane];
            // loaded beside the slot, not behind its `live`: a free slot's velocity is (0, 0) and is not used
            if constexpr (MOTION) v = a.vel[(long)stream * T + lane];
        }
        const bool live_entry = lane < T && st.live != 0;
        frt_bbox pred = st.box;  // MOTION: M1's box, from the state at entry; the gate reads the velocities and writes none
        if constexpr (MOTION) {
            if (live_entry) pred = predicted_box(st, v.x, v.y);
        }
        bool taken = false;
        frt_track_gate mine = {0, -1, 0.f, 0};  // lane d: the record of detection d
        // ---- G1, G2: the update's steps 1 and 2, overlap only
        for (int d = 0; d < MF; ++d) {
            if (d >= n_present) break;  // (wave-uniform)
            const frt_bbox b = boxes[d];
            if (!(b.score > 0.f)) continue;  // (wave-uniform)
            unsigned long long key = 0;
            if (live_entry && !taken) {
                const float ovr = iou(b, MOTION ? pred : st.box);
                if (ovr >= a.iou_threshold) key = ((unsigned long long)__float_as_uint(ovr) << 32) | (unsigned)(63 - lane);
            }
            key = wave_max_u64(key);
            frt_track_gate g = {FRT_TRACK_GATE_EMBED, -1, 0.f, FRT_TRACK_GATE_NO_TRACK};
            if (key != 0) {
                const int win = 63 - (int)(key & 63);
                const int hits = __shfl(st.hits, win), ne = __shfl(st.n_embeds, win);
                const float ovr = __uint_as_float((unsigned)(key >> 32));
                if (lane == win) taken = true;
                // ---- G3
                int why = 0;
                if (hits < a.min_hits) why |= FRT_TRACK_GATE_UNCONFIRMED;
                if (ne < a.min_embeds) why |= FRT_TRACK_GATE_FEW_EMBEDS;
                if (!(ovr >= a.skip_iou)) why |= FRT_TRACK_GATE_LOW_OVERLAP;
                if ((hits + 1) % a.refresh == 0) why |= FRT_TRACK_GATE_REFRESH;
                g = frt_track_gate{why ? FRT_TRACK_GATE_EMBED : FRT_TRACK_GATE_FOLLOW, win, ovr, why};
            }
            if (lane == d) mine = g;
        }
        // ---- G4
        if (lane < MF) a.gate[(long)f * MF + lane] = mine;
        const unsigned long long embed = __ballot(lane < MF && mine.decision == FRT_TRACK_GATE_EMBED);
        if (lane == 0) s_mask[f] = embed;
    }
    __syncthreads();

    // ---- the work list: exclusive offsets of the frames, four frames per lane of wave 0
    if (wave == 0) {
        int c[4], sum = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            c[k] = __popcll(s_mask[lane * 4 + k]);
            sum += c[k];
        }
        int incl = sum;
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off);
            if (lane >= off) incl += o;
        }
        int run = incl - sum;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s_off[lane * 4 + k] = run;
            run += c[k];
        }
        if (lane == 63) s_total = incl;
    }
    __syncthreads();
    const int n_embed = s_total, cap = NF * MF;
    for (int f = wave; f < NF; f += GATE_WAVES) {
        const unsigned long long m = s_mask[f];
        if ((m >> lane) & 1) a.list[s_off[f] + __popcll(m & ((1ull << lane) - 1ull))] = f * MF + lane;
    }
    for (int i = n_embed + tid; i < cap; i += 64 * GATE_WAVES) a.list[i] = -1;
    if (tid == 0) *a.n_embed = n_embed;
    const int passes = (cap + a.max_batch - 1) / a.max_batch;
    for (int j = tid; j < passes; j += 64 * GATE_WAVES) {
        const long long left = (long long)n_embed - (long long)j * a.max_batch;
        a.pass_count[j] = (int32_t)(left < 0 ? 0 : (left > a.max_batch ? a.max_batch : left));
    }
}

// one wave per face slot of the call, four to a workgroup (see the header comment)
__global__ __launch_bounds__(64 * WAVES) void track_gate_scatter_kernel(TrackScatterArgs a) {
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * WAVES + (threadIdx.x >> 6)));
    if (i >= a.F) return;
    int n = *a.n_embed;
    n = n < 0 ? 0 : (n > a.F ? a.F : n);
    int lo = 0, hi = n;  // the first position whose entry is >= i
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.list[mid] < i) lo = mid + 1;
        else hi = mid;
    }
    const bool found = lo < n && a.list[lo] == i;
    float *out = a.embeds + (long)i * a.dim;
    if (found) {  // (wave-uniform)
        const float *row = a.embeds_c + (long)lo * a.dim;
        for (int k = lane * 4; k < a.dim; k += 256) *reinterpret_cast<floatx4 *>(out + k) = *reinterpret_cast<const floatx4 *>(row + k);
    } else {
        for (int k = lane * 4; k < a.dim; k += 256) *reinterpret_cast<floatx4 *>(out + k) = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    if (lane == 0) {
        a.valid[i] = found ? a.valid_c[lo] : 0;
        if (a.idx) a.idx[i] = (found && a.idx_c) ? a.idx_c[lo] : -1;
        if (a.sim) a.sim[i] = (found && a.sim_c) ? a.sim_c[lo] : 0.f;
    }
}

}  // namespace

void launch_track_similarity(const TrackArgs &a, const TrackStreamIds &ids, int n_frames, hipStream_t s) {
    if (n_frames <= 0) return;
    hipLaunchKernelGGL(track_similarity_kernel, dim3((unsigned)a.max_faces, (unsigned)n_frames), dim3(64 * WAVES), 0, s, a, ids);
}

void launch_track_update(const TrackArgs &a, const TrackStreamIds &ids, int n_frames, bool appearance, hipStream_t s) {
    if (n_frames <= 0) return;
    const dim3 grid((unsigned)n_frames), block(64 * WAVES);
    const bool motion = a.motion_gain > 0;
    if (appearance && motion)
        hipLaunchKernelGGL((track_update_kernel<true, true>), grid, block, 0, s, a, ids);
    else if (appearance)
        hipLaunchKernelGGL((track_update_kernel<true, false>), grid, block, 0, s, a, ids);
    else if (motion)
        hipLaunchKernelGGL((track_update_kernel<false, true>), grid, block, 0, s, a, ids);
    else
        hipLaunchKernelGGL((track_update_kernel<false, false>), grid, block, 0, s, a, ids);
}

void launch_track_identity(const TrackArgs &a, const TrackStreamIds &ids, int n_frames, const int32_t *idx, const float *sim, hipStream_t s) {
    if (n_frames <= 0) return;
    hipLaunchKernelGGL(track_identity_kernel, dim3((unsigned)((n_frames * a.max_faces + 255) / 256)), dim3(256), 0, s, a, ids, n_frames, idx, sim);
}

void launch_track_gate(const TrackGateArgs &a, const TrackStreamIds &ids, hipStream_t s) {
    if (a.n_frames <= 0) return;
    if (a.motion_gain > 0)
        hipLaunchKernelGGL(track_gate_kernel<true>, dim3(1), dim3(64 * GATE_WAVES), 0, s, a, ids);
    else
        hipLaunchKernelGGL(track_gate_kernel<false>, dim3(1), dim3(64 * GATE_WAVES), 0, s, a, ids);
}

void launch_track_gate_scatter(const TrackScatterArgs &a, hipStream_t s) {
    if (a.F <= 0) return;
    hipLaunchKernelGGL(track_gate_scatter_kernel, dim3((unsigned)((a.F + WAVES - 1) / WAVES)), dim3(64 * WAVES), 0, s, a);
}

void launch_track_reset(const TrackArgs &a, int n_streams, int stream, hipStream_t s) {
    const int first = stream < 0 ? 0 : stream, count = stream < 0 ? n_streams : 1;
    hipLaunchKernelGGL(track_reset_kernel, dim3((unsigned)a.max_tracks, (unsigned)count), dim3(64), 0, s, a, first);
}
