// Sighting book, host side (include/frt.h "Sightings"): the object, the argument checks that run before any device work, the two launches of
// an update, close / drain / open on the tracker's own stream, and frt_pipeline_run_sighted, which strings frt_pipeline_run_tracked's and
// frt_pipeline_run_quality's stages and the book update together on the pipeline stream.  The kernels are in kernels_sightings.hip.
#include "frt_pipeline.hpp"
#include "frt_sightings.hpp"

namespace {

constexpr size_t CROP = FRT_SIGHTING_CROP_BYTES;
constexpr int MAX_CAPACITY = 65536;

// The rows, zeroed, on the first call that passed its checks (t->mu held, the tracker's state there).  All of it or nothing
void ensure_state(frt_sightings *b) {
    if (b->records) return;
    frt_tracker *t = b->t;
    const size_t rows = (size_t)b->n_open + b->capacity, D = (size_t)t->dim;
    try {
        b->records.reserve(rows);
        b->best_embeds.reserve(rows * D);
        b->templates.reserve(rows * D);
        if (b->opt.keep_crops) b->crops.reserve(rows * CROP);
        b->best_key.reserve(b->n_open);
        b->state.reserve(4);
        b->jobs.reserve(b->n_open);
        b->h_state.reserve(4);
        hipStream_t s = t->stream;
        HIPCHK(hipMemsetAsync(b->records.get(), 0, rows * sizeof(frt_sighting), s));
        HIPCHK(hipMemsetAsync(b->best_embeds.get(), 0, rows * D * sizeof(float), s));
        HIPCHK(hipMemsetAsync(b->templates.get(), 0, rows * D * sizeof(float), s));
        if (b->opt.keep_crops) HIPCHK(hipMemsetAsync(b->crops.get(), 0, rows * CROP, s));
        HIPCHK(hipMemsetAsync(b->best_key.get(), 0, (size_t)b->n_open * sizeof(uint32_t), s));
        HIPCHK(hipMemsetAsync(b->state.get(), 0, 4 * sizeof(int32_t), s));
        HIPCHK(hipStreamSynchronize(s));
    } catch (...) {
        b->records.reset();
        b->best_embeds.reset();
        b->templates.reset();
        b->crops.reset();
        throw;
    }
}

// crops are required iff the book keeps them: both forms of the update
void check_crops(const frt_sightings *b, const void *crops, const char *who) {
    if (b->opt.keep_crops && !crops) raise(FRT_ERR_INVALID, std::string(who) + ": the book keeps crops, crops is null");
    if (!b->opt.keep_crops && crops) raise(FRT_ERR_INVALID, std::string(who) + ": the book keeps no crops (keep_crops 0), crops must be null");
}

// One book update queued on s, with t->mu held, both states allocated and every argument checked
void update_locked(frt_sightings *b, const frt_face_result *results, const frt_track_result *tracks, const float *embeds, const float *templates,
                   const struct frt_face_quality *quality, const uint8_t *crops, int n_frames, const TrackStreamIds &ids, bool join, hipStream_t s) {
    frt_tracker *t = b->t;
    if (join && t->pending) HIPCHK(hipStreamWaitEvent(s, t->ev_last, 0));  // the state the book reads is the last queued update's
    SightingArgs a = b->args();
    a.results = results;
    a.tracks = tracks;
    a.embeds = embeds;
    a.call_templates = templates;
    a.quality = quality;
    a.call_crops = crops;
    const int n_jobs = n_frames * t->max_tracks;
    {
        ProfScope ps(2, "sightings_plan", (double)n_jobs, s);
        launch_sightings_plan(a, ids, n_frames, s);
        HIPCHK(hipGetLastError());
    }
    b->taken = 0;
    b->bound = std::min<long>(b->capacity, (long)b->bound + n_jobs);
    {
        ProfScope ps(2, "sightings_copy", (double)n_jobs, s);
        launch_sightings_copy(a, n_jobs, s);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(t->ev_last, s));
    t->pending = true;
}

}  // namespace

extern "C" {

int frt_sightings_create(frt_tracker *t, int capacity, const frt_sighting_options *options, frt_sightings **out) {
    return guarded([&] {
        if (!t || !out) raise(FRT_ERR_INVALID, "sightings: null argument");
        if (capacity < 1 || capacity > MAX_CAPACITY) raise(FRT_ERR_CAPACITY, "sightings: capacity outside 1 .. 65536");
        frt_sighting_options o{FRT_SHOT_RANK_SHARPNESS, 1, 1};
        if (options) o = *options;
        if (o.rank < FRT_SHOT_RANK_SHARPNESS || o.rank > FRT_SHOT_RANK_SCORE) raise(FRT_ERR_INVALID, "sightings: rank outside 0 .. 2");
        if (o.min_hits < 1) raise(FRT_ERR_INVALID, "sightings: min_hits < 1");
        if (o.keep_crops != 0 && o.keep_crops != 1) raise(FRT_ERR_INVALID, "sightings: keep_crops is neither 0 nor 1");
        frt_sightings *b = new frt_sightings;  // (no device work here: the rows are allocated by the first call that needs them)
        b->t = t;
        b->capacity = capacity;
        b->opt = o;
        b->n_open = t->n_streams * t->max_tracks;
        *out = b;
    });
}

void frt_sightings_destroy(frt_sightings *b) {
    if (!b) return;
    {
        std::lock_guard<std::mutex> lk(b->t->mu);
        if (b->records) {  // nothing queued on any stream may still touch the rows
            (void)hipSetDevice(b->t->device);
            if (b->t->pending) (void)hipEventSynchronize(b->t->ev_last);
        }
    }
    delete b;
}

int frt_sightings_update_dev(frt_sightings *b, const void *results_dev, const void *tracks_dev, const void *embeds_dev, const void *templates_dev,
                             const void *quality_dev, const void *crops_dev, int n_frames, const int32_t *stream_ids, void *hip_stream) {
    return guarded([&] {
        if (!b || !results_dev || !tracks_dev || !embeds_dev || !quality_dev) raise(FRT_ERR_INVALID, "sightings update: null argument");
        check_crops(b, crops_dev, "sightings update");
        if (((uintptr_t)embeds_dev | (uintptr_t)templates_dev | (uintptr_t)crops_dev) & 15)
            raise(FRT_ERR_INVALID, "sightings update: embeds_dev, templates_dev and crops_dev must be 16-byte aligned");
        if (((uintptr_t)quality_dev & 7) || (((uintptr_t)results_dev | (uintptr_t)tracks_dev) & 3))
            raise(FRT_ERR_INVALID, "sightings update: quality_dev must be 8-byte, results_dev and tracks_dev 4-byte aligned");
        frt_tracker *t = b->t;
        std::lock_guard<std::mutex> lk(t->mu);
        const TrackStreamIds ids = tracker_check_ids(t, n_frames, stream_ids);
        tracker_ensure_state(t);
        ensure_state(b);
        update_locked(b, reinterpret_cast<const frt_face_result *>(results_dev), reinterpret_cast<const frt_track_result *>(tracks_dev),
                      reinterpret_cast<const float *>(embeds_dev), reinterpret_cast<const float *>(templates_dev),
                      reinterpret_cast<const struct frt_face_quality *>(quality_dev), reinterpret_cast<const uint8_t *>(crops_dev), n_frames, ids, true,
                      reinterpret_cast<hipStream_t>(hip_stream));
    });
}

int frt_sightings_update(frt_sightings *b, const frt_face_result *results, const frt_track_result *tracks, const float *embeds, const float *templates,
                         const struct frt_face_quality *quality, const uint8_t *crops, int n_frames, const int32_t *stream_ids) {
    return guarded([&] {
        if (!b || !results || !tracks || !embeds || !quality) raise(FRT_ERR_INVALID, "sightings update: null argument");
        check_crops(b, crops, "sightings update");
        frt_tracker *t = b->t;
        std::lock_guard<std::mutex> lk(t->mu);
        const TrackStreamIds ids = tracker_check_ids(t, n_frames, stream_ids);
        tracker_ensure_state(t);
        ensure_state(b);
        const size_t F = (size_t)n_frames * t->max_faces, D = (size_t)t->dim;
        hipStream_t s = t->stream;
        tracker_join_updates(t);
        HIPCHK(hipStreamSynchronize(s));  // the staging is rewritten below
        b->d_results.reserve(F);
        b->d_tracks.reserve(F);
        b->d_embeds.reserve(F * D);
        if (templates) b->d_templates.reserve(F * D);
        b->d_quality.reserve(F);
        if (crops) b->d_crops.reserve(F * CROP);
        HIPCHK(hipMemcpyAsync(b->d_results.get(), results, F * sizeof(frt_face_result), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(b->d_tracks.get(), tracks, F * sizeof(frt_track_result), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(b->d_embeds.get(), embeds, F * D * sizeof(float), hipMemcpyHostToDevice, s));
        if (templates) HIPCHK(hipMemcpyAsync(b->d_templates.get(), templates, F * D * sizeof(float), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(b->d_quality.get(), quality, F * sizeof(struct frt_face_quality), hipMemcpyHostToDevice, s));
        if (crops) HIPCHK(hipMemcpyAsync(b->d_crops.get(), crops, F * CROP, hipMemcpyHostToDevice, s));
        update_locked(b, b->d_results.get(), b->d_tracks.get(), b->d_embeds.get(), templates ? b->d_templates.get() : nullptr, b->d_quality.get(),
                      crops ? b->d_crops.get() : nullptr, n_frames, ids, false, s);
        sync_stream_spinning(s);
    });
}

int frt_sightings_close(frt_sightings *b, int stream) {
    return guarded([&] {
        if (!b) raise(FRT_ERR_INVALID, "sightings close: null argument");
        frt_tracker *t = b->t;
        if (stream < -1 || stream >= t->n_streams) raise(FRT_ERR_INVALID, "sightings close: stream outside -1 .. n_streams - 1");
        std::lock_guard<std::mutex> lk(t->mu);
        tracker_ensure_state(t);
        ensure_state(b);
        tracker_join_updates(t);
        const SightingArgs a = b->args();
        const int n_jobs = (stream < 0 ? t->n_streams : 1) * t->max_tracks;
        launch_sightings_close(a, t->n_streams, stream, t->stream);
        HIPCHK(hipGetLastError());
        b->taken = 0;
        b->bound = std::min<long>(b->capacity, (long)b->bound + n_jobs);
        launch_sightings_copy(a, n_jobs, t->stream);
        HIPCHK(hipGetLastError());
        sync_stream_spinning(t->stream);
    });
}

int frt_sightings_drain(frt_sightings *b, int max_out, frt_sighting *records_out, uint8_t *crops_out, float *embeds_out, float *templates_out, int *n_out,
                        int32_t *counters_out) {
    return guarded([&] {
        if (!b || !records_out || !n_out) raise(FRT_ERR_INVALID, "sightings drain: null argument");
        if (max_out < 1) raise(FRT_ERR_INVALID, "sightings drain: max_out < 1");
        if (crops_out && !b->opt.keep_crops) raise(FRT_ERR_INVALID, "sightings drain: the book keeps no crops (keep_crops 0), crops_out must be null");
        frt_tracker *t = b->t;
        std::lock_guard<std::mutex> lk(t->mu);
        tracker_ensure_state(t);
        ensure_state(b);
        tracker_join_updates(t);
        hipStream_t s = t->stream;
        const size_t D = (size_t)t->dim;
        // how many rows are queued is known on the device alone; `bound` is what the launches since the last drain can have made of it, and
        // that many rows leave with the count, so that one synchronisation serves both
        const int m = std::min(max_out, b->bound);
        HIPCHK(hipMemcpyAsync(b->h_state.get(), b->state.get(), 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        for (int done = 0; done < m;) {  // at most two pieces: the ring wraps once
            const size_t q = (size_t)(b->head + done) % b->capacity, n = std::min<size_t>(m - done, b->capacity - q), row = b->n_open + q;
            HIPCHK(hipMemcpyAsync(records_out + done, b->records.get() + row, n * sizeof(frt_sighting), hipMemcpyDeviceToHost, s));
            if (embeds_out) HIPCHK(hipMemcpyAsync(embeds_out + done * D, b->best_embeds.get() + row * D, n * D * sizeof(float), hipMemcpyDeviceToHost, s));
            if (templates_out) HIPCHK(hipMemcpyAsync(templates_out + done * D, b->templates.get() + row * D, n * D * sizeof(float), hipMemcpyDeviceToHost, s));
            if (crops_out) HIPCHK(hipMemcpyAsync(crops_out + done * CROP, b->crops.get() + row * CROP, n * CROP, hipMemcpyDeviceToHost, s));
            done += (int)n;
        }
        sync_stream_spinning(s);
        const int32_t *h = b->h_state.get();
        const int queued = h[0] - b->taken, n = std::min(queued, m);
        if (queued < 0 || queued > b->capacity || queued > b->bound) raise(FRT_ERR_DEVICE, "sightings drain: the queue holds an impossible count");
        b->head = (b->head + n) % b->capacity;
        b->taken += n;
        b->bound = queued - n;
        *n_out = n;
        if (counters_out) {
            counters_out[0] = queued;
            counters_out[1] = h[1];
            counters_out[2] = h[2];
            counters_out[3] = h[3];
        }
    });
}

int frt_sightings_open(frt_sightings *b, int stream, frt_sighting *records_out, float *best_embeds_out, float *templates_out, uint8_t *crops_out) {
    return guarded([&] {
        if (!b || !records_out) raise(FRT_ERR_INVALID, "sightings open: null argument");
        frt_tracker *t = b->t;
        if (stream < 0 || stream >= t->n_streams) raise(FRT_ERR_INVALID, "sightings open: stream outside 0 .. n_streams - 1");
        if (crops_out && !b->opt.keep_crops) raise(FRT_ERR_INVALID, "sightings open: the book keeps no crops (keep_crops 0), crops_out must be null");
        std::lock_guard<std::mutex> lk(t->mu);
        tracker_ensure_state(t);
        ensure_state(b);
        tracker_join_updates(t);
        hipStream_t s = t->stream;
        const size_t T = (size_t)t->max_tracks, D = (size_t)t->dim, row = (size_t)stream * T;
        HIPCHK(hipMemcpyAsync(records_out, b->records.get() + row, T * sizeof(frt_sighting), hipMemcpyDeviceToHost, s));
        if (best_embeds_out) HIPCHK(hipMemcpyAsync(best_embeds_out, b->best_embeds.get() + row * D, T * D * sizeof(float), hipMemcpyDeviceToHost, s));
        if (templates_out) HIPCHK(hipMemcpyAsync(templates_out, b->templates.get() + row * D, T * D * sizeof(float), hipMemcpyDeviceToHost, s));
        if (crops_out) HIPCHK(hipMemcpyAsync(crops_out, b->crops.get() + row * CROP, T * CROP, hipMemcpyDeviceToHost, s));
        sync_stream_spinning(s);
    });
}

int frt_pipeline_run_sighted(frt_pipeline *p, frt_tracker *t, frt_sightings *b, const frt_quality_options *quality, const uint8_t *frames, int n_frames,
                             const int32_t *stream_ids, frt_face_result *results, frt_track_result *tracks_out, struct frt_face_quality *quality_out,
                             float *embeds_out) {
    return guarded([&] {
        if (!t || !b) raise(FRT_ERR_INVALID, "runSighted: null argument");
        if (b->t != t) raise(FRT_ERR_INVALID, "runSighted: the book belongs to another tracker");
        if (!p || !frames || !results || !tracks_out) raise(FRT_ERR_INVALID, "runSighted: null argument");
        const frt_quality_options opt = quality_checked_options(quality, "runSighted");
        std::lock_guard<std::mutex> lk(t->mu);
        if (t->max_faces != p->max_faces || t->dim != 512) raise(FRT_ERR_INVALID, "runSighted: the tracker's max_faces and dim must be the pipeline's");
        if (t->device != p->det->device) raise(FRT_ERR_INVALID, "runSighted: tracker and pipeline live on different devices");
        const TrackStreamIds ids = tracker_check_ids(t, n_frames, stream_ids);
        if (n_frames > p->max_frames) raise(FRT_ERR_INVALID, "runSighted: more frames than the pipeline's max_frames");
        tracker_check_matcher(t, p->mat);
        tracker_ensure_state(t);
        ensure_state(b);
        const size_t frame_bytes = (size_t)p->det->g.frame_h * p->det->g.frame_w * 3, F = (size_t)n_frames * t->max_faces;
        tracker_join_updates(t);
        HIPCHK(hipStreamSynchronize(t->stream));  // a host form may still be reading the staging
        t->reserve_staging(n_frames, frame_bytes);
        b->d_quality.reserve(F);
        b->d_crops.reserve(F * CROP);  // (the quality launch reads the crops whether the book keeps them or not)
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
            r.crops = b->d_crops.get();
            r.after = t->ev_up;
            p->run_dev(r);
            p->flush();  // (a pairing mode that holds run_dev calls: the join must be on the stream before anything reads the results)
            {
                ProfScope ps(2, "face_quality", (double)F, s);
                launch_face_quality(b->d_crops.get(), t->d_results.get(), (int)F, opt, b->d_quality.get(), s);
                HIPCHK(hipGetLastError());
            }
            tracker_update_locked(t, p->mat, t->d_results.get(), t->d_embeds.get(), n_frames, ids, t->d_tracks.get(), t->d_templates.get(), nullptr, s);
            update_locked(b, t->d_results.get(), t->d_tracks.get(), t->d_embeds.get(), t->d_templates.get(), b->d_quality.get(),
                          b->opt.keep_crops ? b->d_crops.get() : nullptr, n_frames, ids, false, s);
            HIPCHK(hipMemcpyAsync(results, t->d_results.get(), F * sizeof(frt_face_result), hipMemcpyDeviceToHost, s));
            if (embeds_out) HIPCHK(hipMemcpyAsync(embeds_out, t->d_embeds.get(), F * 512 * sizeof(float), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(tracks_out, t->d_tracks.get(), F * sizeof(frt_track_result), hipMemcpyDeviceToHost, s));
            if (quality_out) HIPCHK(hipMemcpyAsync(quality_out, b->d_quality.get(), F * sizeof(struct frt_face_quality), hipMemcpyDeviceToHost, s));
            sync_stream_spinning(s);
        } catch (...) {  // leave nothing in flight that reads or writes the staging of a call that has returned
            p->drain(false);
            throw;
        }
        p->emb->check_se_error();
    });
}

}  // extern "C"
