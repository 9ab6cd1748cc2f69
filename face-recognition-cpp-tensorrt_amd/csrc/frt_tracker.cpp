// Face tracker, host side (include/frt.h "Face tracker"): the object, the argument checks that run before any device work, the three
// launches of an update (four with appearance on: the similarity kernel goes first), the appearance and motion settings, the host forms and
// frt_pipeline_run_tracked; the gate in front of the recogniser ("Gate": frt_tracker_gate / _gate_dev) and frt_pipeline_run_tracked_gated,
// which strings detector, gate, gather crop, recogniser, search, scatter and the unchanged update together.  The kernels are in
// kernels_track.hip (the gather crop and alignment in kernels_image.hip).
#include "frt_pipeline.hpp"
#include "frt_tracker.hpp"

TrackStreamIds tracker_check_ids(const frt_tracker *t, int n_frames, const int32_t *stream_ids) {
    if (n_frames < 1) raise(FRT_ERR_INVALID, "tracker: n_frames < 1");
    if (n_frames > FRT_TRACK_MAX_FRAMES) raise(FRT_ERR_CAPACITY, "tracker: more than 256 frames in one update");
    TrackStreamIds ids{};
    bool seen[FRT_TRACK_MAX_STREAMS] = {};
    for (int i = 0; i < n_frames; ++i) {
        const int s = stream_ids ? stream_ids[i] : i;
        if (s < 0 || s >= t->n_streams) raise(FRT_ERR_INVALID, "tracker: stream id " + std::to_string(s) + " of frame " + std::to_string(i) + " is outside 0 .. n_streams - 1");
        if (seen[s]) raise(FRT_ERR_INVALID, "tracker: stream id " + std::to_string(s) + " appears twice in one update");
        seen[s] = true;
        ids.id[i] = (uint16_t)s;
    }
    return ids;
}

void tracker_check_matcher(const frt_tracker *t, frt_matcher *m) {
    if (!m) return;
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->device != t->device) raise(FRT_ERR_INVALID, "tracker: the matcher lives on another device");
    if (m->N > 0 && m->D != t->dim) raise(FRT_ERR_INVALID, "tracker: the matcher's num_col is not the tracker's dim");
}

void tracker_update_locked(frt_tracker *t, frt_matcher *m, const frt_face_result *results_dev, const float *embeds_dev, int n_frames,
                           const TrackStreamIds &ids, frt_track_result *tracks_dev, float *templates_dev, frt_track_assoc *assoc_dev, hipStream_t s) {
    const int F = n_frames * t->max_faces;
    std::unique_lock<std::mutex> lm;
    if (m) {
        lm = std::unique_lock<std::mutex>(m->mu);
        if (m->N > 0 && (m->D != t->dim || m->device != t->device)) raise(FRT_ERR_INVALID, "tracker: the matcher's num_col is not the tracker's dim");
    }
    const bool identity = m && m->N > 0;
    if (identity) {
        if (!templates_dev) {
            t->q_templates.reserve((size_t)F * t->dim);
            templates_dev = t->q_templates.get();
        }
        t->q_idx.reserve(F);
        t->q_sim.reserve(F);
    }
    // the association records name S of the matched pair, so a call that asks for them takes the appearance launches whatever the settings
    const bool appearance = t->appearance_on() || assoc_dev;
    if (appearance) {
        t->sim.reserve((size_t)F * t->max_tracks);
        t->sim_defined.reserve(F);
    }
    TrackArgs a = t->args();
    if (a.motion_gain > 0 && !a.vel) raise(FRT_ERR_DEVICE, "tracker: motion is on and the velocities are not allocated");  // (ensure_state ran: cannot happen)
    a.results = results_dev;
    a.embeds = embeds_dev;
    a.tracks = tracks_dev;
    a.templates = templates_dev;
    a.sim = t->sim.get();
    a.sim_defined = t->sim_defined.get();
    a.assoc = assoc_dev;
    if (appearance) {
        ProfScope ps(2, "track_similarity", (double)F * t->max_tracks, s);
        launch_track_similarity(a, ids, n_frames, s);
        HIPCHK(hipGetLastError());
    }
    {
        ProfScope ps(2, "track_update", (double)F, s);
        launch_track_update(a, ids, n_frames, appearance, s);
        HIPCHK(hipGetLastError());
    }
    if (identity) {
        // what frt_matcher_top1_dev does, with the matcher's mutex already held
        m->wait_idle(s);
        m->ensure_queries(F);
        m->top1_dev(templates_dev, F, t->q_idx.get(), t->q_sim.get(), s);
        HIPCHK(hipEventRecord(m->ev_busy, s));
        m->busy = true;
        ProfScope ps(2, "track_identity", (double)F, s);
        launch_track_identity(a, ids, n_frames, t->q_idx.get(), t->q_sim.get(), s);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(t->ev_last, s));
    t->pending = true;
}

namespace {

void check_options(const frt_track_options &o) {
    if (!(o.iou_threshold > 0.f && o.iou_threshold <= 1.f)) raise(FRT_ERR_INVALID, "tracker: iou_threshold outside (0, 1]");
    if (o.max_missed < 0) raise(FRT_ERR_INVALID, "tracker: max_missed < 0");
    if (o.min_hits < 1) raise(FRT_ERR_INVALID, "tracker: min_hits < 1");
    if (!(o.decay > 0.f && o.decay <= 1.f)) raise(FRT_ERR_INVALID, "tracker: decay outside (0, 1]");
}

// (written so that a NaN fails both)
void check_appearance(float reid_threshold, float iou_min_sim) {
    if (!((reid_threshold > 0.f && reid_threshold <= 1.f) || reid_threshold == FRT_TRACK_REID_OFF))
        raise(FRT_ERR_INVALID, "tracker: reid_threshold outside (0, 1] and not the off value 2.0");
    if (!((iou_min_sim >= -1.f && iou_min_sim <= 1.f) || iou_min_sim == FRT_TRACK_MIN_SIM_OFF))
        raise(FRT_ERR_INVALID, "tracker: iou_min_sim outside [-1, 1] and not the off value -2.0");
}

// "Gate": no defaults, so a null pointer is refused like a value out of range (written so that a NaN fails)
frt_track_gate_options checked_gate_options(const frt_track_gate_options *o) {
    if (!o) raise(FRT_ERR_INVALID, "tracker gate: null options (the gate has no defaults)");
    if (o->refresh < 1) raise(FRT_ERR_INVALID, "tracker gate: refresh < 1");
    if (o->min_embeds < 1) raise(FRT_ERR_INVALID, "tracker gate: min_embeds < 1");
    if (!(o->skip_iou > 0.f && o->skip_iou <= 1.f)) raise(FRT_ERR_INVALID, "tracker gate: skip_iou outside (0, 1]");
    return *o;
}

// One gate launch queued on s, with t->mu held, the state allocated and every argument checked
void gate_locked(frt_tracker *t, const frt_track_gate_options &o, const frt_bbox *boxes_dev, const int32_t *n_boxes_dev, int n_frames,
                 const TrackStreamIds &ids, frt_track_gate *gate_dev, int32_t *list_dev, int32_t *n_embed_dev, int32_t *pass_count_dev, int max_batch,
                 hipStream_t s) {
    TrackGateArgs a{};
    a.slots = t->slots.get();
    a.max_tracks = t->max_tracks;
    a.max_faces = t->max_faces;
    a.iou_threshold = t->opt.iou_threshold;
    a.min_hits = t->opt.min_hits;
    a.refresh = o.refresh;
    a.min_embeds = o.min_embeds;
    a.skip_iou = o.skip_iou;
    a.boxes = boxes_dev;
    a.n_boxes = n_boxes_dev;
    a.n_frames = n_frames;
    a.gate = gate_dev;
    a.list = list_dev;
    a.n_embed = n_embed_dev;
    a.pass_count = pass_count_dev;
    a.max_batch = max_batch;
    a.vel = t->vel.get();
    a.motion_gain = t->motion_gain;
    if (a.motion_gain > 0 && !a.vel) raise(FRT_ERR_DEVICE, "tracker gate: motion is on and the velocities are not allocated");
    if (t->pending) HIPCHK(hipStreamWaitEvent(s, t->ev_last, 0));  // the state the gate reads is the last queued update's
    ProfScope ps(2, "track_gate", (double)n_frames * t->max_faces, s);
    launch_track_gate(a, ids, s);
    HIPCHK(hipGetLastError());
}

// "Motion": the velocities, zeroed, on the first call that needs the state with motion on
void ensure_vel(frt_tracker *t) {
    if (t->motion_gain <= 0 || t->vel) return;
    const size_t S = (size_t)t->n_streams * t->max_tracks;
    try {
        t->vel.reserve(S);
        HIPCHK(hipMemsetAsync(t->vel.get(), 0, S * sizeof(int2), t->stream));
        HIPCHK(hipStreamSynchronize(t->stream));
    } catch (...) {
        t->vel.reset();
        throw;
    }
}

// The stream, the events and the zeroed state (with motion on, the velocities among it), on the first call that passed its checks.  All
// of it or nothing: a failure leaves the object without state, as it was created.  Where the state exists and only the velocities are
// missing (motion was switched on later), a failure leaves the state as it was and the velocities missing; the next call tries again
void ensure_state(frt_tracker *t) {
    use_device(t->device);
    if (t->slots) return ensure_vel(t);
    try {
        if (!t->stream) HIPCHK(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
        if (!t->ev_last) HIPCHK(hipEventCreateWithFlags(&t->ev_last, hipEventDisableTiming));
        if (!t->ev_up) HIPCHK(hipEventCreateWithFlags(&t->ev_up, hipEventDisableTiming));
        const size_t S = (size_t)t->n_streams * t->max_tracks;
        t->sums.reserve(S * t->dim);
        t->counters.reserve((size_t)t->n_streams * 4);
        t->slots.reserve(S);
        HIPCHK(hipMemsetAsync(t->slots.get(), 0, S * sizeof(frt_track_state), t->stream));
        HIPCHK(hipMemsetAsync(t->sums.get(), 0, S * t->dim * sizeof(float), t->stream));
        HIPCHK(hipMemsetAsync(t->counters.get(), 0, (size_t)t->n_streams * 4 * sizeof(int32_t), t->stream));
        HIPCHK(hipStreamSynchronize(t->stream));
        ensure_vel(t);  // (drops the velocities itself where it fails)
    } catch (...) {
        t->slots.reset();
        t->sums.reset();
        t->counters.reset();
        throw;
    }
}

// M1 on the host, for frt_tracker_motion: kernels_track.hip's predicted_box
int32_t clamp_i32(long long v) { return (int32_t)std::min<long long>(std::max<long long>(v, INT32_MIN), INT32_MAX); }
long long motion_shift(int32_t v, int32_t missed) {
    const long long lim = 1ll << 30;
    return std::min(std::max((long long)v * ((long long)missed + 1) / 256, -lim), lim);  // C's division truncates toward zero
}

// `stream` behind the last update queued on any stream
void join_updates(frt_tracker *t) {
    if (t->pending) HIPCHK(hipStreamWaitEvent(t->stream, t->ev_last, 0));
}

void destroy(frt_tracker *t) {
    if (t->stream || t->slots) (void)hipSetDevice(t->device);
    if (t->stream) {
        (void)hipStreamSynchronize(t->stream);
        (void)hipStreamDestroy(t->stream);
    }
    if (t->ev_last) {
        if (t->pending) (void)hipEventSynchronize(t->ev_last);
        (void)hipEventDestroy(t->ev_last);
    }
    if (t->ev_up) (void)hipEventDestroy(t->ev_up);
    delete t;
}

}  // namespace

void tracker_ensure_state(frt_tracker *t) { ensure_state(t); }
void tracker_join_updates(frt_tracker *t) { join_updates(t); }

extern "C" {

int frt_tracker_create(int n_streams, int max_tracks, int max_faces, int dim, const frt_track_options *options, int device, frt_tracker **out) {
    return guarded([&] {
        if (!out) raise(FRT_ERR_INVALID, "tracker: null out");
        if (n_streams < 1 || n_streams > FRT_TRACK_MAX_STREAMS) raise(FRT_ERR_INVALID, "tracker: n_streams outside 1 .. 1024");
        if (max_tracks < 1 || max_tracks > FRT_TRACK_MAX_SLOTS) raise(FRT_ERR_INVALID, "tracker: max_tracks outside 1 .. 64");
        if (max_faces < 1 || max_faces > FRT_TRACK_MAX_SLOTS) raise(FRT_ERR_INVALID, "tracker: max_faces outside 1 .. 64");
        if (dim < 4 || dim > FRT_TRACK_MAX_DIM || (dim & 3)) raise(FRT_ERR_INVALID, "tracker: dim must be a multiple of 4 in 4 .. 2048");
        frt_track_options o{0.3f, 5, 3, 1.0f};
        if (options) o = *options;
        check_options(o);
        if (device < 0) raise(FRT_ERR_INVALID, "tracker: bad device");
        frt_tracker *t = new frt_tracker;  // (no device work here: the state is allocated by the first call that needs it, ensure_state)
        t->device = device;
        t->n_streams = n_streams;
        t->max_tracks = max_tracks;
        t->max_faces = max_faces;
        t->dim = dim;
        t->opt = o;
        *out = t;
    });
}

void frt_tracker_destroy(frt_tracker *t) {
    if (t) destroy(t);
}

int frt_tracker_set_appearance(frt_tracker *t, float reid_threshold, float iou_min_sim) {
    return guarded([&] {
        if (!t) raise(FRT_ERR_INVALID, "tracker appearance: null argument");
        check_appearance(reid_threshold, iou_min_sim);
        std::lock_guard<std::mutex> lk(t->mu);
        t->reid_threshold = reid_threshold;
        t->iou_min_sim = iou_min_sim;
    });
}

int frt_tracker_get_appearance(frt_tracker *t, float *reid_threshold_out, float *iou_min_sim_out) {
    return guarded([&] {
        if (!t || !reid_threshold_out || !iou_min_sim_out) raise(FRT_ERR_INVALID, "tracker appearance: null argument");
        std::lock_guard<std::mutex> lk(t->mu);
        *reid_threshold_out = t->reid_threshold;
        *iou_min_sim_out = t->iou_min_sim;
    });
}

int frt_tracker_set_motion(frt_tracker *t, int gain) {
    return guarded([&] {
        if (!t) raise(FRT_ERR_INVALID, "tracker motion: null argument");
        if (gain < 0 || gain > 256) raise(FRT_ERR_INVALID, "tracker motion: gain outside 0 .. 256");
        std::lock_guard<std::mutex> lk(t->mu);
        if (t->motion_gain == 0 && gain > 0 && t->vel) {  // off -> on: every velocity starts from zero, behind the last queued update
            use_device(t->device);
            join_updates(t);
            HIPCHK(hipMemsetAsync(t->vel.get(), 0, (size_t)t->n_streams * t->max_tracks * sizeof(int2), t->stream));
            sync_stream_spinning(t->stream);
        }
        t->motion_gain = gain;
    });
}

int frt_tracker_get_motion(frt_tracker *t, int *gain_out) {
    return guarded([&] {
        if (!t || !gain_out) raise(FRT_ERR_INVALID, "tracker motion: null argument");
        std::lock_guard<std::mutex> lk(t->mu);
        *gain_out = t->motion_gain;
    });
}

int frt_tracker_motion(frt_tracker *t, int stream, int32_t *vel_out, frt_bbox *pred_out) {
    return guarded([&] {
        if (!t || !vel_out) raise(FRT_ERR_INVALID, "tracker motion: null argument");
        if (stream < 0 || stream >= t->n_streams) raise(FRT_ERR_INVALID, "tracker motion: stream outside 0 .. n_streams - 1");
        std::lock_guard<std::mutex> lk(t->mu);
        if (t->motion_gain == 0) raise(FRT_ERR_INVALID, "tracker motion: motion is off (frt_tracker_set_motion)");
        ensure_state(t);
        hipStream_t s = t->stream;
        join_updates(t);
        const size_t T = (size_t)t->max_tracks;
        std::vector<frt_track_state> slots(pred_out ? T : 0);
        HIPCHK(hipMemcpyAsync(vel_out, t->vel.get() + stream * T, T * sizeof(int2), hipMemcpyDeviceToHost, s));
        if (pred_out) HIPCHK(hipMemcpyAsync(slots.data(), t->slots.get() + stream * T, T * sizeof(frt_track_state), hipMemcpyDeviceToHost, s));
        sync_stream_spinning(s);
        for (size_t i = 0; pred_out && i < T; ++i) {
            const frt_track_state &st = slots[i];
            frt_bbox b{};
            if (st.live != 0) {
                const long long sx = motion_shift(vel_out[2 * i], st.missed), sy = motion_shift(vel_out[2 * i + 1], st.missed);
                b = frt_bbox{clamp_i32(st.box.x1 + sx), clamp_i32(st.box.y1 + sy), clamp_i32(st.box.x2 + sx), clamp_i32(st.box.y2 + sy), st.box.score};
            }
            pred_out[i] = b;
        }
    });
}

int frt_tracker_update_dev(frt_tracker *t, frt_matcher *m, const void *results_dev, const void *embeds_dev, int n_frames, const int32_t *stream_ids,
                           void *tracks_dev, void *templates_dev, void *hip_stream) {
    return frt_tracker_update_assoc_dev(t, m, results_dev, embeds_dev, n_frames, stream_ids, tracks_dev, templates_dev, nullptr, hip_stream);
}

int frt_tracker_update_assoc_dev(frt_tracker *t, frt_matcher *m, const void *results_dev, const void *embeds_dev, int n_frames,
                                 const int32_t *stream_ids, void *tracks_dev, void *templates_dev, void *assoc_dev, void *hip_stream) {
    return guarded([&] {
        if (!t || !results_dev || !embeds_dev || !tracks_dev) raise(FRT_ERR_INVALID, "tracker update: null argument");
        if (((uintptr_t)embeds_dev | (uintptr_t)templates_dev) & 15) raise(FRT_ERR_INVALID, "tracker update: embeds_dev and templates_dev must be 16-byte aligned");
        std::lock_guard<std::mutex> lk(t->mu);
        const TrackStreamIds ids = tracker_check_ids(t, n_frames, stream_ids);
        tracker_check_matcher(t, m);
        ensure_state(t);
        tracker_update_locked(t, m, reinterpret_cast<const frt_face_result *>(results_dev), reinterpret_cast<const float *>(embeds_dev), n_frames, ids,
                              reinterpret_cast<frt_track_result *>(tracks_dev), reinterpret_cast<float *>(templates_dev),
                              reinterpret_cast<frt_track_assoc *>(assoc_dev), reinterpret_cast<hipStream_t>(hip_stream));
    });
}

int frt_tracker_update(frt_tracker *t, frt_matcher *m, const frt_face_result *results, const float *embeds, int n_frames, const int32_t *stream_ids,
                       frt_track_result *tracks_out, float *templates_out) {
    return frt_tracker_update_assoc(t, m, results, embeds, n_frames, stream_ids, tracks_out, templates_out, nullptr);
}

int frt_tracker_update_assoc(frt_tracker *t, frt_matcher *m, const frt_face_result *results, const float *embeds, int n_frames,
                             const int32_t *stream_ids, frt_track_result *tracks_out, float *templates_out, frt_track_assoc *assoc_out) {
    return guarded([&] {
        if (!t || !results || !embeds || !tracks_out) raise(FRT_ERR_INVALID, "tracker update: null argument");
        std::lock_guard<std::mutex> lk(t->mu);
        const TrackStreamIds ids = tracker_check_ids(t, n_frames, stream_ids);
        tracker_check_matcher(t, m);
        ensure_state(t);
        const size_t F = (size_t)n_frames * t->max_faces;
        hipStream_t s = t->stream;
        join_updates(t);
        HIPCHK(hipStreamSynchronize(s));  // the staging is rewritten below
        t->reserve_staging(n_frames, 0);
        if (assoc_out) t->d_assoc.reserve(F);
        HIPCHK(hipMemcpyAsync(t->d_results.get(), results, F * sizeof(frt_face_result), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(t->d_embeds.get(), embeds, F * t->dim * sizeof(float), hipMemcpyHostToDevice, s));
        tracker_update_locked(t, m, t->d_results.get(), t->d_embeds.get(), n_frames, ids, t->d_tracks.get(), templates_out ? t->d_templates.get() : nullptr,
                              assoc_out ? t->d_assoc.get() : nullptr, s);
        HIPCHK(hipMemcpyAsync(tracks_out, t->d_tracks.get(), F * sizeof(frt_track_result), hipMemcpyDeviceToHost, s));
        if (assoc_out) HIPCHK(hipMemcpyAsync(assoc_out, t->d_assoc.get(), F * sizeof(frt_track_assoc), hipMemcpyDeviceToHost, s));
        if (templates_out) HIPCHK(hipMemcpyAsync(templates_out, t->d_templates.get(), F * t->dim * sizeof(float), hipMemcpyDeviceToHost, s));
        sync_stream_spinning(s);
    });
}

int frt_tracker_tracks(frt_tracker *t, int stream, frt_track_state *slots_out, float *sums_out, int32_t *counters_out) {
    return guarded([&] {
        if (!t || !slots_out) raise(FRT_ERR_INVALID, "tracker tracks: null argument");
        if (stream < 0 || stream >= t->n_streams) raise(FRT_ERR_INVALID, "tracker tracks: stream outside 0 .. n_streams - 1");
        std::lock_guard<std::mutex> lk(t->mu);
        ensure_state(t);
        hipStream_t s = t->stream;
        join_updates(t);
        const size_t T = (size_t)t->max_tracks;
        int32_t cnt[4] = {};
        HIPCHK(hipMemcpyAsync(slots_out, t->slots.get() + stream * T, T * sizeof(frt_track_state), hipMemcpyDeviceToHost, s));
        if (sums_out) HIPCHK(hipMemcpyAsync(sums_out, t->sums.get() + stream * T * t->dim, T * t->dim * sizeof(float), hipMemcpyDeviceToHost, s));
        if (counters_out) HIPCHK(hipMemcpyAsync(cnt, t->counters.get() + (size_t)stream * 4, sizeof(cnt), hipMemcpyDeviceToHost, s));
        sync_stream_spinning(s);
        if (counters_out) std::memcpy(counters_out, cnt, 3 * sizeof(int32_t));
    });
}

int frt_tracker_reset(frt_tracker *t, int stream) {
    return guarded([&] {
        if (!t) raise(FRT_ERR_INVALID, "tracker reset: null argument");
        if (stream < -1 || stream >= t->n_streams) raise(FRT_ERR_INVALID, "tracker reset: stream outside -1 .. n_streams - 1");
        std::lock_guard<std::mutex> lk(t->mu);
        ensure_state(t);
        join_updates(t);
        launch_track_reset(t->args(), t->n_streams, stream, t->stream);
        HIPCHK(hipGetLastError());
        sync_stream_spinning(t->stream);
    });
}

int frt_pipeline_run_tracked(frt_pipeline *p, frt_tracker *t, const uint8_t *frames, int n_frames, const int32_t *stream_ids, frt_face_result *results,
                             frt_track_result *tracks_out, float *embeds_out, float *templates_out) {
    return guarded([&] {
        if (!p || !t || !frames || !results || !tracks_out) raise(FRT_ERR_INVALID, "runTracked: null argument");
        std::lock_guard<std::mutex> lk(t->mu);
        if (t->max_faces != p->max_faces || t->dim != 512) raise(FRT_ERR_INVALID, "runTracked: the tracker's max_faces and dim must be the pipeline's");
        if (t->device != p->det->device) raise(FRT_ERR_INVALID, "runTracked: tracker and pipeline live on different devices");
        const TrackStreamIds ids = tracker_check_ids(t, n_frames, stream_ids);
        if (n_frames > p->max_frames) raise(FRT_ERR_INVALID, "runTracked: more frames than the pipeline's max_frames");
        tracker_check_matcher(t, p->mat);
        ensure_state(t);
        const size_t frame_bytes = (size_t)p->det->g.frame_h * p->det->g.frame_w * 3, F = (size_t)n_frames * t->max_faces;
        join_updates(t);
        HIPCHK(hipStreamSynchronize(t->stream));  // a host form may still be reading the staging
        t->reserve_staging(n_frames, frame_bytes);
        std::lock_guard<std::mutex> lr(p->run_mu);
        p->ensure_stream();
        hipStream_t s = p->stream;
        try {
            HIPCHK(hipMemcpyAsync(t->d_frames.get(), frames, n_frames * frame_bytes, hipMemcpyHostToDevice, s));
            HIPCHK(hipEventRecord(t->ev_up, s));
            frt_pipeline::Request r;
            r.frames = t->d_frames.get();
            r.n = n_frames;
            r.results = t->d_results.get();
            r.embeds = t->d_embeds.get();
            r.after = t->ev_up;
            p->run_dev(r);
            p->flush();  // (a pairing mode that holds run_dev calls: the join must be on the stream before the tracker reads the results)
            tracker_update_locked(t, p->mat, t->d_results.get(), t->d_embeds.get(), n_frames, ids, t->d_tracks.get(),
                                  templates_out ? t->d_templates.get() : nullptr, nullptr, s);
            HIPCHK(hipMemcpyAsync(results, t->d_results.get(), F * sizeof(frt_face_result), hipMemcpyDeviceToHost, s));
            if (embeds_out) HIPCHK(hipMemcpyAsync(embeds_out, t->d_embeds.get(), F * 512 * sizeof(float), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(tracks_out, t->d_tracks.get(), F * sizeof(frt_track_result), hipMemcpyDeviceToHost, s));
            if (templates_out) HIPCHK(hipMemcpyAsync(templates_out, t->d_templates.get(), F * 512 * sizeof(float), hipMemcpyDeviceToHost, s));
            sync_stream_spinning(s);
        } catch (...) {  // leave nothing in flight that reads or writes the staging of a call that has returned
            p->drain(false);
            throw;
        }
        p->emb->check_se_error();
    });
}

int frt_tracker_gate_dev(frt_tracker *t, const frt_track_gate_options *options, const void *boxes_dev, const void *n_boxes_dev, int n_frames,
                         const int32_t *stream_ids, void *gate_dev, void *list_dev, void *n_embed_dev, void *pass_count_dev, int max_batch,
                         void *hip_stream) {
    return guarded([&] {
        if (!t || !boxes_dev || !gate_dev || !list_dev || !n_embed_dev || !pass_count_dev) raise(FRT_ERR_INVALID, "tracker gate: null argument");
        const frt_track_gate_options o = checked_gate_options(options);
        if (max_batch < 1) raise(FRT_ERR_INVALID, "tracker gate: max_batch < 1");
        std::lock_guard<std::mutex> lk(t->mu);
        const TrackStreamIds ids = tracker_check_ids(t, n_frames, stream_ids);
        ensure_state(t);
        gate_locked(t, o, reinterpret_cast<const frt_bbox *>(boxes_dev), reinterpret_cast<const int32_t *>(n_boxes_dev), n_frames, ids,
                    reinterpret_cast<frt_track_gate *>(gate_dev), reinterpret_cast<int32_t *>(list_dev), reinterpret_cast<int32_t *>(n_embed_dev),
                    reinterpret_cast<int32_t *>(pass_count_dev), max_batch, reinterpret_cast<hipStream_t>(hip_stream));
    });
}

int frt_tracker_gate(frt_tracker *t, const frt_track_gate_options *options, const frt_bbox *boxes, const int32_t *n_boxes, int n_frames,
                     const int32_t *stream_ids, frt_track_gate *gate_out, int32_t *list_out, int32_t *n_embed_out, int32_t *pass_count_out,
                     int max_batch) {
    return guarded([&] {
        if (!t || !boxes || !gate_out || !list_out || !n_embed_out || !pass_count_out) raise(FRT_ERR_INVALID, "tracker gate: null argument");
        const frt_track_gate_options o = checked_gate_options(options);
        if (max_batch < 1) raise(FRT_ERR_INVALID, "tracker gate: max_batch < 1");
        std::lock_guard<std::mutex> lk(t->mu);
        const TrackStreamIds ids = tracker_check_ids(t, n_frames, stream_ids);
        ensure_state(t);
        const size_t F = (size_t)n_frames * t->max_faces, passes = (F + (size_t)max_batch - 1) / (size_t)max_batch;
        hipStream_t s = t->stream;
        join_updates(t);
        HIPCHK(hipStreamSynchronize(s));  // the staging is rewritten below
        frt_tracker::Gated &g = t->gated;
        g.boxes.reserve(F);
        g.n_boxes.reserve((size_t)n_frames);
        g.gate.reserve(F);
        g.list.reserve(F);
        g.n_embed.reserve(1);
        g.pass_count.reserve(passes);
        HIPCHK(hipMemcpyAsync(g.boxes.get(), boxes, F * sizeof(frt_bbox), hipMemcpyHostToDevice, s));
        if (n_boxes) HIPCHK(hipMemcpyAsync(g.n_boxes.get(), n_boxes, (size_t)n_frames * sizeof(int32_t), hipMemcpyHostToDevice, s));
        gate_locked(t, o, g.boxes.get(), n_boxes ? g.n_boxes.get() : nullptr, n_frames, ids, g.gate.get(), g.list.get(), g.n_embed.get(),
                    g.pass_count.get(), max_batch, s);
        HIPCHK(hipMemcpyAsync(gate_out, g.gate.get(), F * sizeof(frt_track_gate), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(list_out, g.list.get(), F * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(n_embed_out, g.n_embed.get(), sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(pass_count_out, g.pass_count.get(), passes * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        sync_stream_spinning(s);
    });
}

int frt_pipeline_run_tracked_gated(frt_pipeline *p, frt_tracker *t, const frt_track_gate_options *options, const uint8_t *frames, int n_frames,
                                   const int32_t *stream_ids, frt_face_result *results, frt_track_result *tracks_out, frt_track_gate *gate_out,
                                   float *embeds_out, float *templates_out, uint8_t *crops_out, int32_t *n_embed_out) {
    return guarded([&] {
        if (!p || !t || !frames || !results || !tracks_out || !n_embed_out) raise(FRT_ERR_INVALID, "runTrackedGated: null argument");
        const frt_track_gate_options o = checked_gate_options(options);
        // ---- tracker -> run_mu -> detector, embedder -> matcher
        std::lock_guard<std::mutex> lk(t->mu);
        if (t->max_faces != p->max_faces || t->dim != 512) raise(FRT_ERR_INVALID, "runTrackedGated: the tracker's max_faces and dim must be the pipeline's");
        if (t->device != p->det->device) raise(FRT_ERR_INVALID, "runTrackedGated: tracker and pipeline live on different devices");
        const TrackStreamIds ids = tracker_check_ids(t, n_frames, stream_ids);
        if (n_frames > p->max_frames) raise(FRT_ERR_INVALID, "runTrackedGated: more frames than the pipeline's max_frames");
        tracker_check_matcher(t, p->mat);
        ensure_state(t);
        frt_detector *d = p->det;
        frt_embedder *e = p->emb;
        frt_matcher *m = p->mat;
        const DetGeom &dg = d->g;
        const int MF = t->max_faces, Fi = n_frames * MF, B = e->max_batch;
        const size_t row = (size_t)dg.frame_w * 3, frame_bytes = (size_t)dg.frame_h * row, F = (size_t)Fi;
        constexpr size_t CROP = (size_t)112 * 112 * 3;
        join_updates(t);
        HIPCHK(hipStreamSynchronize(t->stream));  // a host form may still be reading the staging
        t->reserve_staging(n_frames, frame_bytes);
        frt_tracker::Gated &g = t->gated;
        g.boxes.reserve(F);
        g.n_boxes.reserve((size_t)n_frames);
        if (d->has_landmarks) g.ldm.reserve(F * 10);
        g.gate.reserve(F);
        g.list.reserve(F);
        g.n_embed.reserve(1);
        g.h_n_embed.reserve(1);
        g.pass_count.reserve((F + (size_t)B - 1) / (size_t)B);
        g.embeds_c.reserve(F * 512);
        g.sim_c.reserve(F);
        g.sim.reserve(F);
        g.idx_c.reserve(F);
        g.idx.reserve(F);
        g.valid_c.reserve(F);
        g.valid.reserve(F);
        if (crops_out) g.crops.reserve(F * CROP);

        std::lock_guard<std::mutex> lr(p->run_mu);
        p->flush();  // whatever a pairing mode holds or has pending goes first (takes the object mutexes itself)
        p->ensure_stream();
        hipStream_t s = p->stream;
        std::lock_guard<std::mutex> ld(d->mu), le(e->mu);
        std::unique_lock<std::mutex> lm;
        if (m) lm = std::unique_lock<std::mutex>(m->mu);
        const bool align = p->align;  // (frt_pipeline_set_align refuses a detector without the LandmarkHead)
        try {
            d->wait_idle(s);
            e->wait_idle(s);
            HIPCHK(hipMemcpyAsync(t->d_frames.get(), frames, n_frames * frame_bytes, hipMemcpyHostToDevice, s));
            d->forward_frames(t->d_frames.get(), n_frames, row, frame_bytes, s);
            d->postprocess(n_frames, s, g.boxes.get(), g.n_boxes.get(), d->has_landmarks ? g.ldm.get() : nullptr);
            HIPCHK(hipEventRecord(d->ev_busy, s));
            d->busy = true;
            gate_locked(t, o, g.boxes.get(), g.n_boxes.get(), n_frames, ids, g.gate.get(), g.list.get(), g.n_embed.get(), g.pass_count.get(), B, s);
            // the one host read in front of the recogniser: how many passes to queue
            HIPCHK(hipMemcpyAsync(g.h_n_embed.get(), g.n_embed.get(), sizeof(int32_t), hipMemcpyDeviceToHost, s));
            sync_stream_spinning(s);
            const int ne = *g.h_n_embed.get();
            if (ne < 0 || ne > Fi) raise(FRT_ERR_DEVICE, "runTrackedGated: the gate returned an impossible count");
            for (int f0 = 0, j = 0; f0 < ne; f0 += B, ++j) {  // passes cut as frt_embedder_forward cuts them
                const int nf = std::min(B, ne - f0);
                uint8_t *crops = crops_out ? g.crops.get() + (size_t)f0 * CROP : nullptr;
                if (align) {
                    ProfScope ps(2, "align_faces_gather", (double)nf * CROP, s);
                    launch_align_faces_gather(t->d_frames.get(), dg.frame_h, dg.frame_w, row, frame_bytes, g.ldm.get(), g.list.get() + f0,
                                              g.pass_count.get() + j, MF, Fi, nf, crops, e->d_in, g.valid_c.get() + f0, s);
                } else {
                    ProfScope ps(2, "crop_faces_gather", (double)nf * CROP, s);
                    launch_crop_faces_gather(t->d_frames.get(), dg.frame_h, dg.frame_w, row, frame_bytes, g.boxes.get(), g.list.get() + f0,
                                             g.pass_count.get() + j, MF, Fi, nf, crops, e->d_in, g.valid_c.get() + f0, s);
                }
                HIPCHK(hipGetLastError());
                e->forward(0, e->d_in, nf, g.valid_c.get() + f0, g.embeds_c.get() + (size_t)f0 * 512, s);
            }
            if (ne > 0) {
                HIPCHK(hipEventRecord(e->ev_busy[0], s));
                e->busy[0] = true;
            }
            const bool gallery = m && m->N > 0, searched = gallery && ne > 0;
            if (searched) {
                m->wait_idle(s);
                m->ensure_queries(ne);
                m->top1_dev(g.embeds_c.get(), ne, g.idx_c.get(), g.sim_c.get(), s);
                HIPCHK(hipEventRecord(m->ev_busy, s));
                m->busy = true;
            }
            {
                ProfScope ps(2, "track_gate_scatter", (double)F * 512, s);
                TrackScatterArgs sa{g.list.get(), g.n_embed.get(), g.embeds_c.get(), g.valid_c.get(), searched ? g.idx_c.get() : nullptr,
                                    searched ? g.sim_c.get() : nullptr, Fi, 512, t->d_embeds.get(), g.valid.get(), g.idx.get(), g.sim.get()};
                launch_track_gate_scatter(sa, s);
                HIPCHK(hipGetLastError());
            }
            {
                ProfScope ps(2, "pack_results", (double)F, s);
                launch_pack_results(g.boxes.get(), g.n_boxes.get(), g.valid.get(), gallery ? g.idx.get() : nullptr, gallery ? g.sim.get() : nullptr, MF,
                                    Fi, t->d_results.get(), s);
                HIPCHK(hipGetLastError());
            }
            if (m) lm.unlock();  // (the update takes the matcher's mutex itself)
            tracker_update_locked(t, m, t->d_results.get(), t->d_embeds.get(), n_frames, ids, t->d_tracks.get(),
                                  templates_out ? t->d_templates.get() : nullptr, nullptr, s);
            HIPCHK(hipMemcpyAsync(results, t->d_results.get(), F * sizeof(frt_face_result), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(tracks_out, t->d_tracks.get(), F * sizeof(frt_track_result), hipMemcpyDeviceToHost, s));
            if (gate_out) HIPCHK(hipMemcpyAsync(gate_out, g.gate.get(), F * sizeof(frt_track_gate), hipMemcpyDeviceToHost, s));
            if (embeds_out) HIPCHK(hipMemcpyAsync(embeds_out, t->d_embeds.get(), F * 512 * sizeof(float), hipMemcpyDeviceToHost, s));
            if (templates_out) HIPCHK(hipMemcpyAsync(templates_out, t->d_templates.get(), F * 512 * sizeof(float), hipMemcpyDeviceToHost, s));
            if (crops_out && ne > 0) HIPCHK(hipMemcpyAsync(crops_out, g.crops.get(), (size_t)ne * CROP, hipMemcpyDeviceToHost, s));
            sync_stream_spinning(s);
            *n_embed_out = ne;
        } catch (...) {  // leave nothing in flight that reads the caller's frames or writes the caller's arrays
            (void)hipStreamSynchronize(s);
            throw;
        }
        e->check_se_error();
    });
}

}  // extern "C"
