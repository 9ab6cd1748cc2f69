// Extension (no counterpart in the reference): the sighting book of include/frt.h ("Sightings") behind a C++11 class.  A FaceSightings is
// attached to one FaceTracker, which it borrows - destroy the book first -, keeps every live track's best shot and hands out ONE record per
// finished track: what a video product stores and alerts on.
#ifndef FRT_SIGHTINGS_H
#define FRT_SIGHTINGS_H

#include <cstdint>
#include <vector>

#include "tracker.h"

struct Sighting {
    frt_sighting record;
    std::vector<float> bestEmbed, trackTemplate;  // [dim]
    std::vector<uint8_t> bestCrop;                // [112 x 112 x 3] B G R, empty without keep_crops
};

class FaceSightings {
  public:
    // options null: rank by sharpness, min_hits 1, crops kept.  capacity: the sightings that may wait for a drain (1 .. 65536)
    FaceSightings(FaceTracker &tracker, int capacity, const frt_sighting_options *options = nullptr)
        : h_(nullptr), dim_(tracker.dim()), maxFaces_(tracker.maxFaces()), maxTracks_(tracker.maxTracks()),
          keepCrops_(options ? options->keep_crops != 0 : true) {
        checkFrtStatus(frt_sightings_create(tracker.handle(), capacity, options, &h_));
    }
    ~FaceSightings() { frt_sightings_destroy(h_); }
    FaceSightings(const FaceSightings &) = delete;
    FaceSightings &operator=(const FaceSightings &) = delete;

    // One update from host memory, after FaceTracker::update of the same frames and stream ids: its inputs, its track records and
    // templates (may be empty), the quality records of the faces (faceQuality, arcface.h) and - a book that keeps crops - their crops
    void update(const std::vector<frt_face_result> &results, const std::vector<frt_track_result> &tracks, const std::vector<float> &embeds,
                const std::vector<float> &templates, const std::vector<struct frt_face_quality> &quality, const std::vector<uint8_t> &crops,
                const std::vector<int> &streamIds = std::vector<int>()) {
        const int nFrames = (int)(results.size() / (size_t)maxFaces_);
        const std::vector<int32_t> ids(streamIds.begin(), streamIds.end());
        checkFrtStatus(frt_sightings_update(h_, results.data(), tracks.data(), embeds.data(), templates.empty() ? nullptr : templates.data(),
                                            quality.data(), crops.empty() ? nullptr : crops.data(), nFrames, ids.empty() ? nullptr : ids.data()));
    }
    // a connection closed (stream), or all of them (-1): its open sightings end with reason FRT_SIGHTING_CLOSED.  Before FaceTracker::reset
    void close(int stream = -1) { checkFrtStatus(frt_sightings_close(h_, stream)); }
    // the oldest sightings, at most maxOut of them, removed from the queue; counters (may be null) <- queued before the call, overflowed,
    // discarded, closed
    std::vector<Sighting> drain(int maxOut, int counters[4] = nullptr) {
        const size_t cap = (size_t)(maxOut > 0 ? maxOut : 1), crop = (size_t)112 * 112 * 3;
        std::vector<frt_sighting> rec(cap);
        std::vector<float> emb(cap * (size_t)dim_), tpl(cap * (size_t)dim_);
        std::vector<uint8_t> crops(keepCrops_ ? cap * crop : 0);
        int n = 0;
        int32_t cnt[4] = {0, 0, 0, 0};
        checkFrtStatus(frt_sightings_drain(h_, maxOut, rec.data(), keepCrops_ ? crops.data() : nullptr, emb.data(), tpl.data(), &n, cnt));
        for (int i = 0; counters && i < 4; ++i) counters[i] = cnt[i];
        std::vector<Sighting> out((size_t)n);
        for (size_t i = 0; i < (size_t)n; ++i) {
            out[i].record = rec[i];
            out[i].bestEmbed.assign(emb.begin() + (long)(i * (size_t)dim_), emb.begin() + (long)((i + 1) * (size_t)dim_));
            out[i].trackTemplate.assign(tpl.begin() + (long)(i * (size_t)dim_), tpl.begin() + (long)((i + 1) * (size_t)dim_));
            if (keepCrops_) out[i].bestCrop.assign(crops.begin() + (long)(i * crop), crops.begin() + (long)((i + 1) * crop));
        }
        return out;
    }
    // the open entries of one stream, every slot (a free one all zero): a live display
    std::vector<frt_sighting> open(int stream, std::vector<float> *bestEmbeds = nullptr, std::vector<uint8_t> *bestCrops = nullptr) {
        std::vector<frt_sighting> out((size_t)maxTracks_);
        if (bestEmbeds) bestEmbeds->assign((size_t)maxTracks_ * (size_t)dim_, 0.f);
        if (bestCrops) bestCrops->assign(keepCrops_ ? (size_t)maxTracks_ * 112 * 112 * 3 : 0, 0);
        checkFrtStatus(frt_sightings_open(h_, stream, out.data(), bestEmbeds ? bestEmbeds->data() : nullptr, nullptr,
                                          bestCrops && keepCrops_ ? bestCrops->data() : nullptr));
        return out;
    }

    bool keepsCrops() const { return keepCrops_; }
    frt_sightings *handle() { return h_; }

  private:
    frt_sightings *h_;
    int dim_, maxFaces_, maxTracks_;
    bool keepCrops_;
};

#endif  // FRT_SIGHTINGS_H
