// Extension (no counterpart in the reference, which answers every frame of the /inference WebSocket as if it were the only one): the face
// tracker of include/frt.h ("Face tracker") behind a C++11 class.  One FaceTracker serves up to 1024 video streams - one stream per
// WebSocket connection -; its state lives on the device.  ArcFaceIR50::trackFaces (arcface.h) puts it behind the pipeline.
#ifndef FRT_TRACKER_H
#define FRT_TRACKER_H

#include <vector>

#include "common.h"

class FaceTracker {
  public:
    // options null: iou_threshold 0.3, max_missed 5, min_hits 3, decay 1.0
    FaceTracker(int nStreams, int maxTracks, int maxFaces, int dim = 512, const frt_track_options *options = nullptr, int device = 0)
        : h_(nullptr), nStreams_(nStreams), maxTracks_(maxTracks), maxFaces_(maxFaces), dim_(dim) {
        checkFrtStatus(frt_tracker_create(nStreams, maxTracks, maxFaces, dim, options, device, &h_));
    }
    ~FaceTracker() { frt_tracker_destroy(h_); }
    FaceTracker(const FaceTracker &) = delete;
    FaceTracker &operator=(const FaceTracker &) = delete;

    // One update from host memory: results [nFrames x maxFaces] and embeds [nFrames x maxFaces x dim] as the pipeline returns them, frame i
    // belonging to stream streamIds[i] (empty: to stream i).  matcher (may be null): the gallery the tracks' templates are identified in.
    // Returns the track records [nFrames x maxFaces]; templates (may be null) receives [nFrames x maxFaces x dim].
    std::vector<frt_track_result> update(const std::vector<frt_face_result> &results, const std::vector<float> &embeds,
                                         const std::vector<int> &streamIds = std::vector<int>(), frt_matcher *matcher = nullptr,
                                         std::vector<float> *templates = nullptr) {
        const int nFrames = (int)(results.size() / (size_t)maxFaces_);
        std::vector<frt_track_result> out(results.size());
        if (templates) templates->assign(results.size() * (size_t)dim_, 0.f);
        const std::vector<int32_t> ids(streamIds.begin(), streamIds.end());
        checkFrtStatus(frt_tracker_update(h_, matcher, results.data(), embeds.data(), nFrames, ids.empty() ? nullptr : ids.data(), out.data(),
                                          templates ? templates->data() : nullptr));
        return out;
    }
    // The same, and how each detection was associated: assoc receives [nFrames x maxFaces] records (frt_track_assoc: by overlap, by
    // appearance, a birth, untracked or absent; the matched track's gap, overlap and similarity).
    std::vector<frt_track_result> update(const std::vector<frt_face_result> &results, const std::vector<float> &embeds,
                                         std::vector<frt_track_assoc> &assoc, const std::vector<int> &streamIds = std::vector<int>(),
                                         frt_matcher *matcher = nullptr, std::vector<float> *templates = nullptr) {
        const int nFrames = (int)(results.size() / (size_t)maxFaces_);
        std::vector<frt_track_result> out(results.size());
        assoc.assign(results.size(), frt_track_assoc());
        if (templates) templates->assign(results.size() * (size_t)dim_, 0.f);
        const std::vector<int32_t> ids(streamIds.begin(), streamIds.end());
        checkFrtStatus(frt_tracker_update_assoc(h_, matcher, results.data(), embeds.data(), nFrames, ids.empty() ? nullptr : ids.data(), out.data(),
                                                templates ? templates->data() : nullptr, assoc.data()));
        return out;
    }
    // Appearance (include/frt.h "Appearance"): re-attach a lost face to its track when its embedding is at least reidThreshold (0 .. 1] like
    // the track's running sum, and refuse an overlap match whose similarity is below iouMinSim [-1 .. 1].  FRT_TRACK_REID_OFF /
    // FRT_TRACK_MIN_SIM_OFF switch either off; both are off until set.  No threshold is recommended: measure on your own faces.
    void setAppearance(float reidThreshold, float iouMinSim) { checkFrtStatus(frt_tracker_set_appearance(h_, reidThreshold, iouMinSim)); }
    void getAppearance(float &reidThreshold, float &iouMinSim) { checkFrtStatus(frt_tracker_get_appearance(h_, &reidThreshold, &iouMinSim)); }
    // Motion (include/frt.h "Motion"): a constant-velocity term per track; with it on every overlap - the association's, the gate's - is
    // taken with the track's PREDICTED box.  gain 0 switches it off (the default), 1 .. 256 is the weight of a new measurement in the
    // velocity's running mean, in 1/256.  No gain is recommended: nobody has measured one on real video with this library.
    void setMotion(int gain) { checkFrtStatus(frt_tracker_set_motion(h_, gain)); }
    int getMotion() {
        int gain = 0;
        checkFrtStatus(frt_tracker_get_motion(h_, &gain));
        return gain;
    }
    // One stream's velocities [maxTracks x 2] (vx, vy in 1/256 pixel per update); predicted (may be null) receives the box each slot is
    // compared with in the NEXT update, zeros for a free slot.  Throws while motion is off.
    std::vector<int32_t> motion(int stream, std::vector<frt_bbox> *predicted = nullptr) {
        std::vector<int32_t> vel((size_t)maxTracks_ * 2, 0);
        if (predicted) predicted->assign((size_t)maxTracks_, frt_bbox());
        checkFrtStatus(frt_tracker_motion(h_, stream, vel.data(), predicted ? predicted->data() : nullptr));
        return vel;
    }
    // The gate alone (include/frt.h "Gate"): which of these boxes [nFrames x maxFaces] - nBoxes (may be empty) the detector's counts per
    // frame - must go through the recogniser and which a confirmed track follows.  Returns one record per face slot; list receives the face
    // indices to embed, ascending (list.size() is n_embed), passCount (may be null) the faces of each recogniser pass of maxBatch.  Reads the
    // state and writes none.  The options have no defaults: nobody has measured them on real video with this library.
    std::vector<frt_track_gate> gate(const std::vector<frt_bbox> &boxes, const frt_track_gate_options &options, std::vector<int> &list,
                                     const std::vector<int> &streamIds = std::vector<int>(), const std::vector<int> &nBoxes = std::vector<int>(),
                                     int maxBatch = 128, std::vector<int> *passCount = nullptr) {
        const int nFrames = (int)(boxes.size() / (size_t)maxFaces_);
        std::vector<frt_track_gate> out(boxes.size());
        std::vector<int32_t> l(boxes.size() ? boxes.size() : 1), pc(maxBatch > 0 ? (boxes.size() + (size_t)maxBatch - 1) / (size_t)maxBatch + 1 : 1);
        const std::vector<int32_t> ids(streamIds.begin(), streamIds.end()), nb(nBoxes.begin(), nBoxes.end());
        int32_t nEmbed = 0;
        checkFrtStatus(frt_tracker_gate(h_, &options, boxes.data(), nb.empty() ? nullptr : nb.data(), nFrames, ids.empty() ? nullptr : ids.data(),
                                        out.data(), l.data(), &nEmbed, pc.data(), maxBatch));
        list.assign(l.begin(), l.begin() + nEmbed);
        if (passCount) passCount->assign(pc.begin(), pc.begin() + (long)((boxes.size() + (size_t)maxBatch - 1) / (size_t)maxBatch));
        return out;
    }
    // every slot of one stream, live or not; counters (may be null) <- next_id, tick, dropped
    std::vector<frt_track_state> tracks(int stream, int counters[3] = nullptr, std::vector<float> *sums = nullptr) {
        std::vector<frt_track_state> out((size_t)maxTracks_);
        if (sums) sums->assign((size_t)maxTracks_ * (size_t)dim_, 0.f);
        int32_t cnt[3] = {0, 0, 0};
        checkFrtStatus(frt_tracker_tracks(h_, stream, out.data(), sums ? sums->data() : nullptr, cnt));
        for (int i = 0; counters && i < 3; ++i) counters[i] = cnt[i];
        return out;
    }
    // a connection closed (stream), or all of them (-1): its tracks go, track ids are never reused
    void reset(int stream = -1) { checkFrtStatus(frt_tracker_reset(h_, stream)); }

    int numStreams() const { return nStreams_; }
    int maxTracks() const { return maxTracks_; }
    int maxFaces() const { return maxFaces_; }
    int dim() const { return dim_; }
    frt_tracker *handle() { return h_; }

  private:
    frt_tracker *h_;
    int nStreams_, maxTracks_, maxFaces_, dim_;
};

#endif  // FRT_TRACKER_H
