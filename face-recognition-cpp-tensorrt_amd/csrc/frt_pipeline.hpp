// struct frt_pipeline: the batched, three-stage pipeline behind frt_pipeline_* (include/frt.h).  Internal header of libfrt.so.
#pragma once
#include "frt_detector.hpp"
#include "frt_embedder.hpp"
#include "frt_matcher.hpp"

struct frt_pipeline {
    frt_detector *det;
    frt_embedder *emb;
    frt_matcher *mat;
    int max_frames, max_faces, F_cap;
    hipStream_t stream = nullptr, own_stream = nullptr;
    // Three-stage software pipeline over consecutive calls: detector of call b+1 (det_stream), crop + recogniser of call b
    // (emb_stream / emb_stream2 alternately), match + pack of call b-1 (behind its recogniser pass on the same stream, i.e. beside
    // the other set's pass) - three stages with different bottlenecks (latency / MFMA+LDS / HBM) that overlap on the same CUs.  `stream` (the caller's) only joins.  Fork/join with events; boxes, embeddings and validity
    // flags of a call live in one of two slots so that a later stage of the previous call can still read them.
    hipStream_t det_stream = nullptr, emb_stream = nullptr, emb_stream2 = nullptr;
    float *d_chw2 = nullptr;
    hipEvent_t ev_serial = nullptr;  // end of the last serial (profiled) call while overlap is on
    bool serial_pending = false;
    // calls in flight between the start of D and the end of M (2: 32.5k, 3: 33.6k, 4: 33.6k faces/s).  Six since pairing exists: paired calls finish
    // two at a time and one call late, so two pairs in the later stages + the detector a call or two ahead need six slots (with three the detector
    // of call b + 5 waited for the pair (b + 2, b + 3) and the recogniser passes ran one after the other: 0.84 instead of 0.74 ms per 4-frame call)
    static constexpr int NSLOT = 10;  // (groups of four: 2 * 4 + 2)
    hipEvent_t ev_det[NSLOT] = {}, ev_emb[NSLOT] = {}, ev_done[NSLOT] = {};
    float *slot_embeds[NSLOT] = {};
    int *slot_valid[NSLOT] = {};
    frt_bbox *slot_boxes[NSLOT] = {};
    int *slot_nout[NSLOT] = {};
    float *slot_landmarks[NSLOT] = {};
    bool align = false;  // optional: 5-point similarity warp instead of the reference's bbox crop + bicubic resize
    unsigned seq = 0;
    bool overlap = true;
    Arena arena;
    float *d_chw, *d_sim;
    int32_t *d_idx;
    std::mutex run_mu;               // serialises run(): stream selection, slot counters and the stage enqueue order are per-call state
    bool input_sync = false;         // frt_pipeline_set_input_sync: order every run_dev call behind the work queued on `stream` so far
    hipEvent_t ev_input = nullptr;   // ... recorded on `stream` at the call

    // ---- asynchronous host boundary (frt_pipeline_submit / frt_pipeline_wait): NBUF staging sets so that the H2D copy of batch
    //      b+1 (copy_stream, the SDMA engine) and the D2H of batch b-1 run under the stages of batch b
    static constexpr int NBUF = 12;  // (4 until pairing: up to eleven batches between submit and wait)
    struct AsyncBuf {
        uint8_t *d_frames = nullptr;
        frt_face_result *d_results = nullptr;
        float *d_embeds = nullptr;
        uint8_t *d_crops = nullptr;  // u8 BGR 112x112 crops of the batch's faces (frt_pipeline_submit_crops)
        hipEvent_t ev_h2d = nullptr, ev_out = nullptr;
        long ticket = -1;  // ticket whose results ev_out guards; -1: never used
        std::atomic<bool> failed{false};  // the held stages of this ticket could not be queued (flush_pending / start_held): frt_pipeline_wait reports it
    };
    AsyncBuf abuf[NBUF];
    hipStream_t copy_stream = nullptr;
    int copy_prio = 0;
    long next_ticket = 0;
    std::mutex async_mu;

    // ---- pairing (frt_pipeline_set_pairing; off by default).  A recogniser pass over 16 faces costs 0.59 ms, one over 32 faces 0.92 ms
    //      (profiles/r05z_small_batch_layers.txt: below ~ 64 faces a pass is a chain of launch latencies, not work), and one match call scans
    //      the gallery once whatever the number of queries.  With pairing on, the crop + recogniser + match stages of TWO consecutive calls
    //      run as one pass: a call's detector stage is queued at the call as always, its later stages wait for the next call (or for a
    //      flush: frt_pipeline_wait on its ticket, frt_pipeline_sync, any mode switch).  Nothing about a result changes except when it is
    //      ready - one call later - and which batch-size class of recogniser kernels produced it (the class of the two calls' faces together).
    //      A call is only ever deferred when it could be paired: both calls' face slots together must fit this pipeline's max_frames *
    //      max_faces and the recogniser's max_batch, i.e. create the pipeline for twice the frames a call carries.
    struct Sub {  // one frt_pipeline_submit ticket inside a call: `n` frames, where its results go, the staging set that carries its events
        AsyncBuf *ab = nullptr;
        frt_face_result *h_results = nullptr;
        float *h_embeds = nullptr;
        uint8_t *h_crops = nullptr;
        int n = 0;
        long ticket = -1;
    };
    static constexpr int MAXSUB = 4;
    // Everything that describes ONE call, handed through run() by reference: nothing about a call is parked in the object between an entry point and
    // run().  frt_pipeline_run_dev / _run_dev_after fill the device pointers (and `after`), submit() fills all of it, a held call is one being filled.
    struct Request {
        const uint8_t *frames = nullptr;  // device
        int n = 0;
        frt_face_result *results = nullptr;  // device
        float *embeds = nullptr;             // device, or null
        uint8_t *crops = nullptr;            // device, or null: the crop kernel also writes the u8 crops there
        // the one event the detector stream waits for first, or null: the upload of the frames on the copy stream (submit), or the caller's
        // "frames are ready" event of frt_pipeline_run_dev_after (borrowed)
        hipEvent_t after = nullptr;
        bool serial = false;  // every stage on the caller's stream (a synchronous call with nothing else in flight, see submit())
        // host side of frt_pipeline_submit: the downloads of this call's results follow its match stage, wherever that is queued.  One entry per
        // ticket: a call is the frames of up to MAXSUB consecutive submits when they were merged at the host boundary (Held, below)
        int nsub = 0;
        Sub sub[MAXSUB];
    };
    struct CallRec : Request {  // a call that run() has numbered
        unsigned call = 0;
        int slot = 0;
    };
    static constexpr int MAXG = 4;  // calls per recogniser pass at most
    CallRec pend[MAXG];  // the calls whose later stages are still to be queued (fewer than `group` of them)
    int npend = 0;
    // group: 0 off; 2 .. MAXG: ALWAYS wait for that many calls per recogniser pass (results up to group - 1 calls late);
    //        -1 (default, round 6) ADAPTIVE: a call's later stages are held back only while the recogniser is still busy with earlier calls -
    //        the pass could not start now anyway, so waiting for the next call costs a lone caller nothing - and go out together with the
    //        next call's (up to MAXG calls per pass while the backlog lasts).  A call that finds the recogniser idle is queued at once,
    //        exactly like group == 0.  frt_pipeline_wait on ANY ticket releases held calls once the recogniser has gone idle.
    //        Only calls that came through frt_pipeline_submit are held (their contract is the ticket); frt_pipeline_run_dev promises that
    //        the pipeline stream joins the results AT the call, so device-resident calls are held only on request (adaptive_dev).
    int group = -1;
    bool adaptive_dev = false;
    bool merge_submits = true;   // adaptive mode: merge held submits at the host boundary (Held, below)
    // ---- merging of consecutive submits at the host boundary (adaptive mode only, round 6).  A small call's DETECTOR stage is as much a chain of
    //      launch latencies as its recogniser pass (4 frames: 258 us of kernels, 32 frames: 809 - profiles/r06g_det_tables.txt).  A submit that
    //      finds the pipeline backed up (detector or recogniser still busy with earlier calls) is not queued at all: its frames are uploaded into its staging set and the call is
    //      HELD; the next submit's frames go into the same staging set behind them, and the held frames then run as ONE call (one detector pass,
    //      one recogniser pass, one match call; per-ticket result downloads).  Released by: the submit that fills it (MAXSUB tickets / the
    //      pipeline's capacity) or finds the detector idle, any submit that cannot join, frt_pipeline_wait on one of its tickets - or on any
    //      ticket once the detector has gone idle -, run_dev, sync, set_*, destroy.  A call that finds the detector idle is never held.
    struct Held : Request {  // the call being filled (`after`: base->ev_h2d, recorded behind the last ticket's upload)
        AsyncBuf *base = nullptr;  // the staging set that holds the frames / results / embeddings / crops of every ticket of the call; null: nothing held
    } held;
    long merged_calls = 0, merged_tickets = 0;
    std::string held_error;  // why the last held call could not be queued
    bool detector_busy() const { return det->busy && hipEventQuery(det->ev_busy) == hipErrorNotReady; }
    // "backed up": a stage of an earlier call is still running or queued.  (The detector alone is the wrong signal: under load the recogniser is
    // the bottleneck and the detector is often idle at the moment of a submit - single 4-frame calls then slip in between the merged ones:
    // measured 0.559 ms per 4-frame step against 0.524 without any merging.)
    bool backed_up() const { return detector_busy() || recogniser_busy(); }
    bool holds(long ticket) const {  // is this ticket one of the held call's?
        for (int j = 0; j < held.nsub; ++j)
            if (held.sub[j].ticket == ticket) return true;
        return false;
    }
    // tickets whose stages are queued and whose results have not left yet (held / pending ones are not counted: nothing of theirs is queued)
    int tickets_running() const {
        int n = 0;
        for (const AsyncBuf &b : abuf)
            if (b.ticket >= 0 && !is_pending(b.ticket) && !holds(b.ticket) && hipEventQuery(b.ev_out) == hipErrorNotReady) ++n;
        return n;
    }
    // Holding is only free while the GPU has enough queued work to stay busy until the held frames are released: a submit is held only when at
    // least HOLD_MIN tickets are running, and the held ones go out as soon as fewer are.  Measured with 4-frame calls (tools/proxy_only.py, ms
    // per call; pairing off 0.71 - 0.72 at every depth): without the threshold 2 / 3 / 4 calls in flight cost 0.98 / 0.86 / 0.74 - a caller that
    // keeps few calls in flight is latency-coupled to each of them; with HOLD_MIN = 5 and the release rule: <= 5 in flight as without pairing,
    // 6: 0.58, 7: 0.55, 8: 0.52, 11: 0.49 (profiles/r06_adaptive_hold_sweep.txt).
    static constexpr int HOLD_MIN = 5;
    bool held_must_go() const { return !backed_up() || tickets_running() < HOLD_MIN; }
    bool mergeable() const { return group < 0 && merge_submits && overlap && g_prof_kind == 0; }
    bool can_join(int n) const {  // a submit of n frames behind the held ones
        const int nt = held.n + n;
        return mergeable() && held.nsub < MAXSUB && nt <= max_frames && nt * max_faces <= emb->max_batch;
    }
    bool may_hold(int n) const {  // a submit of n frames becomes a held call (room for a second one like it, and the GPU has work meanwhile)
        return mergeable() && 2 * n <= max_frames && 2 * n * max_faces <= emb->max_batch && !held_must_go();
    }
    unsigned epass = 0;  // recogniser passes queued so far (activation set / stream of the next one)
    long paired_passes = 0, single_passes = 0;
    // is a recogniser pass queued earlier still running (or waiting to run)?  Two event queries, ~ 1 us each
    bool recogniser_busy() const {
        for (int k = 0; k < 2; ++k)
            if (emb->busy[k] && hipEventQuery(emb->ev_busy[k]) == hipErrorNotReady) return true;
        return false;
    }
    bool is_pending(long ticket) const {
        for (int i = 0; i < npend; ++i)
            for (int j = 0; j < pend[i].nsub; ++j)
                if (pend[i].sub[j].ticket == ticket) return true;
        return false;
    }
    void ensure_async() {
        if (copy_stream) return;
        // The upload stream sits in the stage streams' priority class (its own hardware-queue pool): as a normal-priority stream it is
        // dealt round-robin onto the four queues the CALLER's streams live on, and whenever it lands on the queue of the caller's joining
        // stream the next batch's upload sits behind the pending joins of the batches in flight (measured with RCCL's streams in the
        // process: 4-frame step 0.96 -> 1.69 ms, 32-frame step 3.28 -> 3.45 ms).  copy_prio: see frt_pipeline_create.
        HIPCHK(hipStreamCreateWithPriority(&copy_stream, hipStreamNonBlocking, copy_prio));
        const size_t F = (size_t)F_cap;
        for (AsyncBuf &b : abuf) {
            b.d_frames = arena.alloc<uint8_t>((size_t)max_frames * det->g.frame_h * det->g.frame_w * 3);
            b.d_results = arena.alloc<frt_face_result>(F);
            b.d_embeds = arena.alloc<float>(F * 512);
            b.d_crops = arena.alloc<uint8_t>(F * 112 * 112 * 3);
            HIPCHK(hipEventCreateWithFlags(&b.ev_h2d, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&b.ev_out, hipEventDisableTiming));
        }
    }

    // ---- whole photos of any sizes (frt_pipeline_run_images / _enrol_images, frt_images.cpp), allocated on first use.  A call's chunks go
    //      through run_dev one after the other; two staging sets, so that chunk i + 1 is packed, uploaded and resized on `ingest` while
    //      chunk i runs and chunk i - 1's results are copied out of pinned memory.  images_mu serialises these calls among themselves and
    //      is taken BEFORE run_mu (which they take per chunk, never async_mu): images_mu -> run_mu -> object mutexes.
    struct ImageStage {
        static constexpr int NSET = 2;
        bool built = false;                                  // the fixed-size part below exists, all of it
        hipStream_t ingest = nullptr;                        // upload + resize kernel of a chunk
        PackPair pack[NSET];                                 // pinned / device: [max_frames] descriptors, then the chunk's photos, row strides removed
        hipEvent_t uploaded[NSET] = {};                      // pack[b].h may be rewritten
        hipEvent_t ready[NSET] = {};                         // d_frames[b] holds the chunk's resized frames (Request::after)
        hipEvent_t done[NSET] = {};                          // the chunk's stages and downloads are complete on the pipeline stream
        DevBuf<uint8_t> d_frames[NSET];                      // [max_frames][frame_h][frame_w][3]
        DevBuf<frt_face_result> d_results[NSET];             // [F_cap]; h_*: the same, pinned
        PinnedBuf<frt_face_result> h_results[NSET];
        DevBuf<float> d_embeds[NSET];                        // [F_cap][512]
        PinnedBuf<float> h_embeds[NSET];
        DevBuf<uint8_t> d_crops[NSET];                       // [F_cap][112][112][3] (first call that asks for crops)
        PinnedBuf<uint8_t> h_crops[NSET];
        // one enrolment call (grown to its photo count): the dense rows of the accepted photos, status word and face per photo, the row count
        DevBuf<float> d_rows;
        DevBuf<int32_t> d_status, d_count;
        PinnedBuf<int32_t> h_status, h_count;
        DevBuf<frt_face_result> d_face;
        PinnedBuf<frt_face_result> h_face;
        hipEvent_t finished = nullptr;
        // face quality (frt_quality.cpp, include/frt.h "Face quality"): a chunk's records of the gated enrolment, and the staging of one
        // frt_pipeline_run_quality call (grown to its frame count) with its "frames are on the device" event
        DevBuf<struct frt_face_quality> d_quality[NSET];            // [F_cap]
        PinnedBuf<struct frt_face_quality> h_quality[NSET];
        DevBuf<uint8_t> q_frames, q_crops;
        DevBuf<frt_face_result> q_results;
        DevBuf<float> q_embeds;
        DevBuf<struct frt_face_quality> q_quality;
        hipEvent_t q_up = nullptr;
    } images;
    std::mutex images_mu;
    void release_images();  // (frt_pipeline_destroy)

    // ---- a large photo by tiles, recognised in one call (frt_pipeline_run_photo_tiled, frt_tiles.cpp): the work list the select kernel
    //      leaves (kept boxes / sources / landmarks / positions, faces per pass), the faces' flags, embeddings and matches, and the packed
    //      records.  Grown on demand under images_mu, used again by later calls, freed with the pipeline.
    struct TiledFaces {
        DevBuf<frt_bbox> boxes;                    // [max_out]
        DevBuf<int32_t> src, keep_pos, pass_count, idx;
        DevBuf<int> n_kept, valid;
        PinnedBuf<int> h_n_kept;                   // the one host read between detection and the first recogniser pass
        DevBuf<float> ldm, embeds, sim;            // [max_out][10], [max_out][512], [max_out]
        DevBuf<uint8_t> crops;                     // [kept][112][112][3], calls that ask for crops
        DevBuf<frt_face_result> results;           // [max_out]
    } tiled_faces;

    // ---- hipGraph replay.  A step is ~150 dependent launches; eager dispatch costs 3.1 us per dependent kernel on this part,
    //      a graph replay 1.8 us (tools/ubench/launch_gap.hip).  Each call is two graphs - the detector part on det_stream, the
    //      rest on `stream` - so the cross-call overlap of the two streams survives; the fork/join events stay ordinary stream
    //      operations between the graph launches.  A part is keyed by everything baked into its nodes (buffers, batch, slot,
    //      mode, gallery generation); first sighting of a key runs eagerly (lazy one-time setup inside the launchers), the second
    //      is captured, later ones replay.  Off while the profiling hooks record events (frt_profile_enable).
    //      OPT-IN (frt_pipeline_set_graph(p, 1); FRT_PIPELINE_GRAPH=1 only in tuning builds): on the benchmark step the replay measured
    //      4.41 ms against 4.39 ms eager - the launches are queued far enough ahead that the per-dispatch cost hides behind the previous kernel.
    //      Part 2 (match + pack) of a call merged from several submit tickets packs each ticket's records with its own frame count from
    //      zero, so its key also carries the ticket split (nsub, sub_n): a call split 1 + 2 must not replay the graph of one split 2 + 1.
    //      Parts 0 (detector) and 1 (crop + recogniser) see only the call's frames as a whole and keep nsub = 0.
    struct GraphKey {
        int part;
        const void *frames, *results, *embeds;
        int n, slot, align;
        unsigned gallery_gen;
        int nsub = 0;  // part 2 of a merged call: its tickets' frame counts; 0 for everything else
        int sub_n[MAXSUB] = {};
        int flip = 0;  // part 1: the recogniser's flip mode (frt_embedder_set_flip), whose launches the graph holds; 0 for everything else
        bool operator==(const GraphKey &o) const {
            if (nsub != o.nsub || flip != o.flip) return false;
            for (int j = 0; j < nsub; ++j)
                if (sub_n[j] != o.sub_n[j]) return false;
            return part == o.part && frames == o.frames && results == o.results && embeds == o.embeds && n == o.n && slot == o.slot && align == o.align &&
                   gallery_gen == o.gallery_gen;
        }
    };
    struct GraphEntry {
        GraphKey key;
        int seen = 0;
        hipGraphExec_t exec = nullptr;
        unsigned long used = 0;  // tick of the last sighting (least-recently-used eviction)
    };
    std::vector<GraphEntry> graphs;
    bool use_graphs = false;
    // a steady pipelined workload cycles through NSLOT keys of stage 0, up to 2 * NSLOT (slot, activation set) pairs of stage 1 and NSLOT of
    // stage 2: the cache holds them all (a smaller one evicted every key before it recurred - nothing was ever replayed).  Merged calls add one
    // stage-2 key per ticket split seen at a slot; the least recently used keys make room for them
    static constexpr size_t GRAPH_CAP = 4 * NSLOT + 8;
    unsigned long graph_tick = 0;
    long graphs_captured = 0, graphs_replayed = 0;
    void drop_graphs() {
        for (GraphEntry &e : graphs)
            if (e.exec) (void)hipGraphExecDestroy(e.exec);
        graphs.clear();
    }
    template <typename Body>
    void run_part(const GraphKey &key, hipStream_t st, bool capturable, Body body);

    // ---- stream-overlap self-check.  The three-stage pipeline only overlaps when its stage streams (and the caller's joining stream)
    //      sit on different hardware queues: ROCm maps streams round-robin onto GPU_MAX_HW_QUEUES (4) queues per priority level, a
    //      queue is in-order, and one extra stream created before the pipeline has been seen to cost 7 % - 2.5x.
    //      Measured, not assumed: one 150 us single-wave spin kernel per stream, started together; `ratio` = elapsed / 150 us is ~1 when
    //      they run side by side and ~n when n streams share a queue.
    std::string warning;      // last self-check verdict ("" = fine); frt_pipeline_check_overlap returns it through frt_last_error
    float overlap_ratio = 0.f;
    float check_streams(const std::vector<hipStream_t> &sts, double us = 150.0);
    float blocked_by_wait(hipStream_t j, hipStream_t x, hipStream_t g);
    void self_check(bool with_caller);

    void ensure_stream() {
        if (!stream) {
            if (!own_stream) HIPCHK(hipStreamCreate(&own_stream));
            stream = own_stream;
        }
    }

    // ---- a call's way through (frt_pipeline.cpp).  Lock order: async_mu -> run_mu -> object mutexes (ObjLocks); all but submit() and wait(),
    //      which take the pipeline's mutexes themselves, are called with run_mu held.
    void run(const Request &r);                                // D now; E + M now (later_stages) or with the next calls (pend)
    void later_stages(const CallRec *c, int nc, bool pipe3);
    void flush_pending();                                      // the pending calls' later stages; object mutexes held
    void lock_run(const Request &r);                           // object mutexes + run()
    void run_dev(const Request &r);                            // frt_pipeline_run_dev / _run_dev_after
    void start_held();                                         // the held submits go out as ONE call
    void flush();                                              // held + pending
    void drain(bool checked = true);                           // wait for the stage streams and `stream`; needs no mutex
    void quiesce();                                            // flush(), then drain()
    long submit(const uint8_t *frames, int n_frames, frt_face_result *results, float *embeds_out, bool synchronous = false, uint8_t *crops_host = nullptr);
    void wait(long ticket);
};

// The gate's thresholds, checked as every "Face quality" entry point checks them before any device work (frt_quality.cpp): null gives the
// defaults, under which nothing can be flagged; a negative min_size / max_clipped, a NaN or min_mean > max_mean raises FRT_ERR_INVALID.
frt_quality_options quality_checked_options(const frt_quality_options *options, const char *who);
