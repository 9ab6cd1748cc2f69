// struct frt_sightings: the object behind frt_sightings_* (include/frt.h "Sightings").  Internal header of libfrt.so.  A book borrows one
// tracker and is guarded by THAT tracker's mutex; its synchronous calls run on the tracker's own stream.  The open entries and the queue
// share their arrays: rows 0 .. n_open - 1 shadow the tracker's slots, rows n_open .. n_open + capacity - 1 are the ring.  The ring's head
// is known to the host alone (only frt_sightings_drain moves it) and travels by value with every launch, together with the rows drained
// since the last launch; the count lives on the device, where the appends are decided.  Every buffer is a DevBuf member.
#pragma once
#include "frt_tracker.hpp"

struct frt_sightings {
    frt_tracker *t = nullptr;
    int capacity = 0;
    frt_sighting_options opt{};
    int n_open = 0;  // n_streams * max_tracks
    int head = 0;    // the queue row of the oldest sighting
    int taken = 0;   // rows drained that the device count still includes: the next launch subtracts them
    int bound = 0;   // no more rows than this are queued: exact after a drain, plus the entries every launch since could have ended

    // ---- the state
    DevBuf<frt_sighting> records;      // [n_open + capacity]; a free entry is all zero
    DevBuf<float> best_embeds, templates;  // [n_open + capacity][dim]
    DevBuf<uint8_t> crops;             // [n_open + capacity][112][112][3], keep_crops only
    DevBuf<uint32_t> best_key;         // [n_open]
    DevBuf<int32_t> state;             // [4]
    DevBuf<SightingJob> jobs;          // [n_open]
    PinnedBuf<int32_t> h_state;        // [4]: what frt_sightings_drain reads
    // ---- staging of the host form, and of frt_pipeline_run_sighted what the tracker's staging lacks
    DevBuf<frt_face_result> d_results;
    DevBuf<frt_track_result> d_tracks;
    DevBuf<float> d_embeds, d_templates;
    DevBuf<struct frt_face_quality> d_quality;
    DevBuf<uint8_t> d_crops;

    SightingArgs args() const {
        SightingArgs a{};
        a.records = records.get();
        a.best_embeds = best_embeds.get();
        a.templates = templates.get();
        a.crops = crops.get();
        a.best_key = best_key.get();
        a.state = state.get();
        a.jobs = jobs.get();
        a.n_open = n_open;
        a.capacity = capacity;
        a.head = head;
        a.taken = taken;
        a.max_tracks = t->max_tracks;
        a.max_faces = t->max_faces;
        a.dim = t->dim;
        a.rank = opt.rank;
        a.min_hits = opt.min_hits;
        a.slots = t->slots.get();
        a.counters = t->counters.get();
        return a;
    }
};
