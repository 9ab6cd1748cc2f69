// struct frt_tracker: the object behind frt_tracker_* (include/frt.h "Face tracker").  Internal header of libfrt.so.  The track state
// lives in HBM for the object's lifetime; the scratch of an update and the staging of the host forms grow to fit.  Every buffer is a
// DevBuf member: frt_tracker_destroy sets the device, retires the stream and the events, and `delete` frees the rest.
#pragma once
#include "frt_internal.hpp"

struct frt_tracker {
    int device = 0;
    int n_streams = 0, max_tracks = 0, max_faces = 0, dim = 0;
    frt_track_options opt{};
    float reid_threshold = FRT_TRACK_REID_OFF, iou_min_sim = FRT_TRACK_MIN_SIM_OFF;  // frt_tracker_set_appearance
    int motion_gain = 0;  // frt_tracker_set_motion: 0 off, 1 .. 256
    std::mutex mu;
    hipStream_t stream = nullptr;   // the host forms, frt_tracker_tracks and frt_tracker_reset
    hipEvent_t ev_last = nullptr;   // end of the last update queued (on whichever stream): what `stream` waits for before it reads the state
    bool pending = false;
    hipEvent_t ev_up = nullptr;     // frt_pipeline_run_tracked: the frames are on the device

    // ---- the state
    DevBuf<frt_track_state> slots;  // [n_streams][max_tracks]; a free slot is all zero
    DevBuf<float> sums;             // [n_streams][max_tracks][dim]; the rows of free slots are zero
    DevBuf<int32_t> counters;       // [n_streams][4]: next_id, tick, dropped, -
    DevBuf<int2> vel;               // [n_streams][max_tracks]: "Motion"; allocated and zeroed by the first call that needs it with motion on
    // ---- scratch of an update with a matcher: the template rows when the caller takes none, and the search's answers
    DevBuf<float> q_templates, q_sim;
    DevBuf<int32_t> q_idx;
    // ---- scratch of an update with appearance on (or one that reports the association): S and its defined bits, for the most frames seen
    DevBuf<float> sim;                       // [n_frames][max_faces][max_tracks]
    DevBuf<unsigned long long> sim_defined;  // [n_frames][max_faces]
    // ---- staging of the host forms
    DevBuf<uint8_t> d_frames;
    DevBuf<frt_face_result> d_results;
    DevBuf<float> d_embeds, d_templates;
    DevBuf<frt_track_result> d_tracks;
    DevBuf<frt_track_assoc> d_assoc;  // (only once a host form has asked for it)
    // ---- the gate (frt_tracker_gate, frt_pipeline_run_tracked_gated), grown to the call: the detector's boxes / counts / landmarks, the
    //      gate's records and work list, the compact rows the recogniser and the search leave, and their scatter into face slots
    struct Gated {
        DevBuf<frt_bbox> boxes;                             // [n_frames][max_faces]
        DevBuf<float> ldm;                                  // [n_frames][max_faces][10] (a detector with the LandmarkHead)
        DevBuf<frt_track_gate> gate;                        // [n_frames][max_faces]
        DevBuf<int32_t> n_boxes, list, n_embed, pass_count; // [n_frames], [F], [1], [ceil(F / max_batch)]
        PinnedBuf<int32_t> h_n_embed;                       // the one host read in front of the recogniser
        DevBuf<float> embeds_c, sim_c, sim;                 // [F][512], [F], [F]
        DevBuf<int32_t> idx_c, idx;                         // [F]
        DevBuf<int> valid_c, valid;                         // [F]
        DevBuf<uint8_t> crops;                              // [F][112][112][3], calls that ask for crops
    } gated;

    TrackArgs args() const {
        TrackArgs a{};
        a.slots = slots.get();
        a.sums = sums.get();
        a.counters = counters.get();
        a.max_tracks = max_tracks;
        a.max_faces = max_faces;
        a.dim = dim;
        a.iou_threshold = opt.iou_threshold;
        a.decay = opt.decay;
        a.max_missed = opt.max_missed;
        a.min_hits = opt.min_hits;
        a.reid_threshold = reid_threshold;
        a.iou_min_sim = iou_min_sim;
        a.vel = vel.get();
        a.motion_gain = motion_gain;
        return a;
    }
    bool appearance_on() const { return reid_threshold != FRT_TRACK_REID_OFF || iou_min_sim != FRT_TRACK_MIN_SIM_OFF; }
    // room for the host forms' n_frames frames (frame_bytes: 0 without frames)
    void reserve_staging(int n_frames, size_t frame_bytes) {
        const size_t F = (size_t)n_frames * max_faces;
        if (frame_bytes) d_frames.reserve((size_t)n_frames * frame_bytes);
        d_results.reserve(F);
        d_embeds.reserve(F * dim);
        d_tracks.reserve(F);
        d_templates.reserve(F * dim);
    }
};

// What an update checks before any device work (frt_tracker.cpp); both need t->mu.
//   the call's own arguments -> the stream ids by value
TrackStreamIds tracker_check_ids(const frt_tracker *t, int n_frames, const int32_t *stream_ids);
//   the matcher: on the tracker's device, and dim columns when it has rows.  Takes m->mu for the look; m may be null
void tracker_check_matcher(const frt_tracker *t, frt_matcher *m);
// For the objects attached to a tracker (frt_sightings.cpp), with t->mu held: the stream, the events and the zeroed state exist after the
// first; the second puts t->stream behind the last update queued on any stream
void tracker_ensure_state(frt_tracker *t);
void tracker_join_updates(frt_tracker *t);
// One update, queued on s, with t->mu held and every argument checked: - appearance on, or assoc_dev given - the similarity kernel, the
// update kernel, then - m with rows - the top-1 search of the template rows and the identity kernel.  Takes m->mu for the search.
void tracker_update_locked(frt_tracker *t, frt_matcher *m, const frt_face_result *results_dev, const float *embeds_dev, int n_frames,
                           const TrackStreamIds &ids, frt_track_result *tracks_dev, float *templates_dev, frt_track_assoc *assoc_dev, hipStream_t s);
