// libfrt.so: the pipeline's C ABI (frt_pipeline_*): device-resident calls, the asynchronous host boundary, pairing / merging of calls.
// All device work is hand-written HIP (kernels_*.hip); there is no CPU fallback anywhere in this file: without a HIP
// device every entry point that needs one fails with FRT_ERR_DEVICE.
#include "frt_pipeline.hpp"

// ------------------------------------------------------------------------------------------------ a call's stages: graph replay, D, E + M
template <typename Body>
void frt_pipeline::run_part(const GraphKey &key, hipStream_t st, bool capturable, Body body) {
    if (!use_graphs || g_prof_kind != 0 || !capturable) return body(st);
    GraphEntry *e = nullptr;
    for (GraphEntry &g : graphs)
        if (g.key == key) e = &g;
    if (!e) {
        if (graphs.size() >= GRAPH_CAP) {  // callers that never repeat their buffers: bounded memory - the least recently seen key goes
            size_t lru = 0;
            for (size_t i = 1; i < graphs.size(); ++i)
                if (graphs[i].used < graphs[lru].used) lru = i;
            if (graphs[lru].exec) (void)hipGraphExecDestroy(graphs[lru].exec);
            graphs.erase(graphs.begin() + (long)lru);
        }
        graphs.push_back(GraphEntry{key, 0, nullptr, 0});
        e = &graphs.back();
    }
    e->used = ++graph_tick;
    if (e->exec) {
        HIPCHK(hipGraphLaunch(e->exec, st));
        ++graphs_replayed;
        return;
    }
    if (e->seen++ == 0) return body(st);
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    try {
        body(st);
    } catch (...) {
        (void)hipStreamEndCapture(st, &g);
        if (g) (void)hipGraphDestroy(g);
        throw;
    }
    HIPCHK(hipStreamEndCapture(st, &g));
    const hipError_t ie = hipGraphInstantiate(&e->exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ie != hipSuccess) {
        e->exec = nullptr;
        HIPCHK(ie);
    }
    ++graphs_captured;
    HIPCHK(hipGraphLaunch(e->exec, st));
}

void frt_pipeline::run(const Request &r) {
    ensure_stream();
    hipStream_t s = stream;
    const DetGeom &g = det->g;
    const int n = r.n, F = n * max_faces;
    // Three-stage software pipeline over consecutive calls (stage-profiling mode and overlap off: everything serially on `s`):
    //   D  detector of call b+1          (fp32 / split-fp16 MFMA + latency-bound stencils)
    //   E  crop + recogniser of call b   (fp16 MFMA / LDS bound)
    //   M  match + pack of call b-1      (HBM bound: streams the 1 GB fp16 shadow gallery)
    // The caller's stream only JOINS: it waits for M of this call, so everything the caller enqueues after the call sees the
    // results, exactly as if the call had run on that stream.  Boxes, embeddings and validity flags live in NSLOT slots.
    // Profiled calls (frt_profile_enable 1 or 2) run serially on `s`: HIP events around a launch only measure the kernel when
    // no other stream competes for the dispatch (with four streams in flight the bracketed time was 2.7x the kernel time).
    const bool pipe3 = overlap && g_prof_kind == 0 && !r.serial;
    // pairing: this call's later stages wait for the next call - or run together with the waiting call's
    const int gcap = std::min({group < 0 ? (int)MAXG : group, F_cap / F, emb->max_batch / F});  // calls of this size one pass can take
    const bool pairable = pipe3 && gcap >= 2 && (group > 0 || (group < 0 && (r.nsub || adaptive_dev)));
    if (npend && !(pairable && pend[0].n == n)) flush_pending();
    const unsigned call = seq++;
    const int slot = (int)(call % NSLOT);
    if (pipe3 && serial_pending) {  // a serial call used the shared detector / recogniser buffers on `s`: order the stages behind it
        HIPCHK(hipStreamWaitEvent(det_stream, ev_serial, 0));
        HIPCHK(hipStreamWaitEvent(emb_stream, ev_serial, 0));
        HIPCHK(hipStreamWaitEvent(emb_stream2, ev_serial, 0));
        serial_pending = false;
    }
    hipStream_t ds = pipe3 ? det_stream : s;
    if (pipe3 && call >= (unsigned)NSLOT) {
        // slot buffers are free again once M of the call NSLOT back is done.  NB the frames must be valid when the call is made:
        // making D wait for prior work on `s` would serialise the stages.
        HIPCHK(hipStreamWaitEvent(ds, ev_done[slot], 0));
    }
    // frt_pipeline_submit: the frames arrive on the copy stream; frt_pipeline_run_dev_after: the caller's producer (upload / decode / resize on
    // any stream) signals this event
    if (r.after) HIPCHK(hipStreamWaitEvent(ds, r.after, 0));  // (crop + recogniser follow the detector through ev_det[slot])
    if (input_sync && pipe3) {  // safe mode: everything queued on the caller's stream before this call happens-before the stages
        HIPCHK(hipEventRecord(ev_input, s));
        HIPCHK(hipStreamWaitEvent(ds, ev_input, 0));
    }
    const CallRec cur{r, call, slot};
    const int akey = (align ? 1 : 0) | (cur.crops ? 2 : 0);
    run_part(GraphKey{0, r.frames, nullptr, nullptr, n, slot, akey, 0u}, ds, !r.serial, [&](hipStream_t st) {
        det->forward_frames(r.frames, n, (size_t)g.frame_w * 3, (size_t)g.frame_w * g.frame_h * 3, st);
        det->postprocess(n, st, slot_boxes[slot], slot_nout[slot], slot_landmarks[slot]);  // straight into this call's slot
    });
    HIPCHK(hipEventRecord(det->ev_busy, ds));  // object-level detector calls wait for this (frt_detector::wait_idle)
    det->busy = true;
    if (pipe3) HIPCHK(hipEventRecord(ev_det[slot], ds));
    if (pairable) {
        // adaptive: hold this call back only while earlier recogniser passes are still in flight; fixed groups: always
        const bool hold = group > 0 || npend > 0 || (recogniser_busy() && (!cur.nsub || tickets_running() >= HOLD_MIN));
        if (hold) {
            pend[npend++] = cur;  // nothing else is queued for this call now (the caller's stream joins with the last partner's call)
            if (npend == gcap || (group < 0 && npend >= 2 && !recogniser_busy())) flush_pending();
            return;
        }
    }
    later_stages(&cur, 1, pipe3);
}

// the waiting calls' crop + recogniser + match: the group is complete, or the missing partners never came
void frt_pipeline::flush_pending() {
    if (!npend) return;
    CallRec grp[MAXG];
    const int n = npend;
    for (int i = 0; i < n; ++i) grp[i] = pend[i];
    npend = 0;
    try {
        later_stages(grp, n, true);  // (a call is only ever deferred in the three-stream mode: its detector stage sits on det_stream)
    } catch (...) {
        // the held calls are lost; their tickets must not be answered from a staging set's STALE "results have left" event: mark them
        // failed and re-arm the event behind whatever did get queued, so that frt_pipeline_wait returns - with the error
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < grp[i].nsub; ++j) {
                grp[i].sub[j].ab->failed = true;
                (void)hipEventRecord(grp[i].sub[j].ab->ev_out, stream);
            }
        throw;
    }
}

// E and M of one call, or of up to MAXG consecutive calls as ONE recogniser pass and ONE match call (pairing)
void frt_pipeline::later_stages(const CallRec *c, int nc, bool pipe3) {
    hipStream_t s = stream;
    const DetGeom &g = det->g;
    int Fc[MAXG] = {}, Ftot = 0;
    for (int i = 0; i < nc; ++i) {
        Fc[i] = c[i].n * max_faces;
        Ftot += Fc[i];
    }
    (nc >= 2 ? paired_passes : single_passes) += 1;
    const int eset = (pipe3 && Ftot <= emb->max_batch) ? (int)(epass++ & 1u) : 0;  // activation set / stream of this recogniser pass
    hipStream_t es = pipe3 ? (eset ? emb_stream2 : emb_stream) : s;
    // match + pack follow the recogniser pass on ITS stream (they overlap the other set's pass and the next detector pass): a stream
    // of their own measured 0.6 % slower and is one more stream competing for the four hardware queues
    hipStream_t ms = es;
    float *chw = eset ? d_chw2 : d_chw;
    // embeddings and validity flags of the pass: the first call's slot (the calls of a group fit one slot together: run() checked)
    float *emb_slot = slot_embeds[c[0].slot];
    int *valid = slot_valid[c[0].slot];
    for (int i = 0; i < nc; ++i) {
        if (pipe3 && c[i].call >= (unsigned)NSLOT) HIPCHK(hipStreamWaitEvent(es, ev_done[c[i].slot], 0));
        if (pipe3) HIPCHK(hipStreamWaitEvent(es, ev_det[c[i].slot], 0));
    }
    // (a call that was held back or waiting for a partner reaches this point after its submit: a live gallery edit in between - the first
    //  rows of an empty gallery above all - may have left the matcher without scratch for this pipeline; a no-op otherwise)
    if (mat && mat->N > 0) mat->ensure_queries(F_cap);
    const bool have_gallery = mat && mat->N > 0;
    const unsigned gen = mat ? mat->generation : 0u;
    const int akey = (align ? 1 : 0) | (c[0].crops ? 2 : 0);
    // (a pass on activation set k follows the previous pass on the same set: ordered by its stream)
    auto stage_e = [&](hipStream_t st) {
        int f_off = 0;
        for (int i = 0; i < nc; ++i) {
            const int sl = c[i].slot;
            if (align) {
                ProfScope ps(2, "align_faces", (double)Fc[i] * 112 * 112 * 3, st);
                launch_align_faces(c[i].frames, g.frame_h, g.frame_w, (size_t)g.frame_w * 3, (size_t)g.frame_w * g.frame_h * 3, slot_landmarks[sl],
                                   slot_nout[sl], max_faces, Fc[i], 0, c[i].crops, chw + (size_t)f_off * 3 * 112 * 112, valid + f_off, st);
            } else {
                ProfScope ps(2, "crop_faces", (double)Fc[i] * 112 * 112 * 3, st);
                launch_crop_faces(c[i].frames, g.frame_h, g.frame_w, (size_t)g.frame_w * 3, (size_t)g.frame_w * g.frame_h * 3, slot_boxes[sl],
                                  slot_nout[sl], max_faces, Fc[i], 0, 112, 112, c[i].crops, chw + (size_t)f_off * 3 * 112 * 112, valid + f_off, st);
            }
            f_off += Fc[i];
        }
        for (int f0 = 0; f0 < Ftot; f0 += emb->max_batch) {
            const int nf = std::min(emb->max_batch, Ftot - f0);
            emb->forward(eset, chw + (size_t)f0 * 3 * 112 * 112, nf, valid + f0, emb_slot + (size_t)f0 * 512, st);
        }
    };
    // (the fp32 pass is never captured: its single activation set is handed from pass to pass through the host-tracked event f32.done,
    //  which must be a real record on every pass - and a graph captured in one precision must not be replayed in the other)
    if (nc == 1 && !emb->fp32_mode) {
        GraphKey key{1, c[0].frames, nullptr, nullptr, c[0].n, c[0].slot, akey, (unsigned)eset};
        key.flip = emb->flip ? 1 : 0;  // (a graph captured in one mode never replays in the other)
        run_part(key, es, !c[0].serial, stage_e);
    } else {
        stage_e(es);
    }
    HIPCHK(hipEventRecord(emb->ev_busy[eset], es));
    emb->busy[eset] = true;
    if (pipe3) {
        HIPCHK(hipEventRecord(ev_emb[c[0].slot], es));
        HIPCHK(hipStreamWaitEvent(ms, ev_emb[c[0].slot], 0));
    }
    // consecutive calls' match stages sit on DIFFERENT streams (their recogniser passes') but share the matcher's scratch and this
    // pipeline's d_idx / d_sim: each one starts behind the previous one's end (they rarely meet: 0.3 ms every 3.3 ms, half a
    // period apart - which is exactly why an unordered pair showed up as one failing equality test in several hundred)
    // (the serial branch too: an object-level frt_matcher_top1_dev / topk_dev on another stream shares d_partial / the pair lists with this stage)
    if (mat && mat->busy) HIPCHK(hipStreamWaitEvent(ms, mat->ev_busy, 0));
    auto stage_m = [&](hipStream_t st) {
        if (have_gallery) mat->top1_dev(emb_slot, Ftot, d_idx, d_sim, st);
        int f_off = 0;
        for (int i = 0; i < nc; ++i) {
            const int sl = c[i].slot;
            {
                ProfScope ps(2, "pack_results", (double)Fc[i], st);
                // one launch per ticket of the call (merged submits): a ticket's records count ITS frames from zero
                const int np = c[i].nsub > 1 ? c[i].nsub : 1;
                for (int j = 0, fr = 0; j < np; ++j) {
                    const int nf = c[i].nsub > 1 ? c[i].sub[j].n : c[i].n, o = fr * max_faces;
                    launch_pack_results(slot_boxes[sl] + o, slot_nout[sl] + fr, valid + f_off + o, have_gallery ? d_idx + f_off + o : nullptr,
                                        have_gallery ? d_sim + f_off + o : nullptr, max_faces, nf * max_faces, c[i].results + o, st);
                    fr += nf;
                }
            }
            if (c[i].embeds)
                HIPCHK(hipMemcpyAsync(c[i].embeds, emb_slot + (size_t)f_off * 512, sizeof(float) * 512 * Fc[i], hipMemcpyDeviceToDevice, st));
            f_off += Fc[i];
        }
    };
    if (nc == 1) {
        GraphKey key{2, nullptr, c[0].results, c[0].embeds, c[0].n, c[0].slot, akey, gen};
        if (c[0].nsub > 1) {  // (stage_m packs a single-ticket call as one launch whatever its nsub: 0 and 1 are the same graph)
            key.nsub = c[0].nsub;
            for (int j = 0; j < c[0].nsub; ++j) key.sub_n[j] = c[0].sub[j].n;
        }
        run_part(key, ms, !c[0].serial, stage_m);
    } else {
        stage_m(ms);
    }
    if (mat) {
        HIPCHK(hipEventRecord(mat->ev_busy, ms));
        mat->busy = true;
    }
    if (pipe3) {
        for (int i = 0; i < nc; ++i) HIPCHK(hipEventRecord(ev_done[c[i].slot], ms));
        HIPCHK(hipStreamWaitEvent(s, ev_done[c[0].slot], 0));  // the caller's stream joins here
    } else if (overlap) {
        HIPCHK(hipEventRecord(ev_serial, s));
        serial_pending = true;
    }
    // calls that came through frt_pipeline_submit: their downloads follow the join
    for (int i = 0; i < nc; ++i) {
        size_t o = 0;  // face slots in front of this ticket inside the call's device blocks (c[i].results / .embeds / .crops)
        for (int j = 0; j < c[i].nsub; ++j) {
            const Sub &t = c[i].sub[j];
            const size_t nf = (size_t)t.n * max_faces;
            HIPCHK(hipMemcpyAsync(t.h_results, c[i].results + o, sizeof(frt_face_result) * nf, hipMemcpyDeviceToHost, s));
            if (t.h_embeds) HIPCHK(hipMemcpyAsync(t.h_embeds, c[i].embeds + o * 512, sizeof(float) * 512 * nf, hipMemcpyDeviceToHost, s));
            if (t.h_crops) HIPCHK(hipMemcpyAsync(t.h_crops, c[i].crops + o * 112 * 112 * 3, nf * 112 * 112 * 3, hipMemcpyDeviceToHost, s));
            o += nf;
        }
        // "results have left" only behind the LAST download of the call: the first ticket's staging set carries every ticket's data
        for (int j = 0; j < c[i].nsub; ++j) HIPCHK(hipEventRecord(c[i].sub[j].ab->ev_out, s));
    }
}

// ------------------------------------------------------------------------------------------------ host boundary: hold, merge, flush
// det->mu, emb->mu and (when there is a matcher) mat->mu, in that order, behind async_mu and run_mu
namespace {
struct ObjLocks {
    std::lock_guard<std::mutex> d, e;  // (members are locked in declaration order: d, e, then m - that IS the lock order)
    std::unique_lock<std::mutex> m;
    explicit ObjLocks(frt_pipeline *p) : d(p->det->mu), e(p->emb->mu) {
        if (p->mat) m = std::unique_lock<std::mutex>(p->mat->mu);
    }
};
}  // namespace

void frt_pipeline::lock_run(const Request &r) {
    ObjLocks l(this);
    if (mat && mat->N > 0) mat->ensure_queries(F_cap);
    run(r);
}

void frt_pipeline::run_dev(const Request &r) {
    start_held();  // (submits held back at the host boundary go first)
    if (r.n < 1 || r.n > max_frames) raise(FRT_ERR_CAPACITY, "pipeline: more frames than max_frames");
    lock_run(r);
}

// The held submits (merged at the host boundary) go out as ONE call.  Never throws: a failure is left on the tickets
// (AsyncBuf::failed, reported by frt_pipeline_wait) - the caller of the moment may be somebody else's submit or wait.
void frt_pipeline::start_held() {
    if (!held.base) return;
    const Held h = held;
    held = Held{};
    try {
        lock_run(h);
        merged_calls += h.nsub > 1;
        merged_tickets += h.nsub > 1 ? h.nsub : 0;
    } catch (const std::exception &e) {
        held_error = e.what();
        for (int j = 0; j < h.nsub; ++j) {
            h.sub[j].ab->failed = true;
            (void)hipEventRecord(h.sub[j].ab->ev_out, stream);
        }
    }
}

// the held call, then the later stages of the calls that are waiting for a partner (pairing)
void frt_pipeline::flush() {
    start_held();  // (takes the object mutexes itself)
    if (!npend) return;
    ObjLocks l(this);
    flush_pending();
}

// Wait for the stage streams and `stream`.  (A null `stream` is skipped: synchronising it would wait on the legacy default stream, on which the
// blocking stage streams - synchronised just before - have left nothing of this pipeline's.)  unchecked: frt_pipeline_destroy - every stream
// is waited for whatever the others answer
void frt_pipeline::drain(bool checked) {
    for (hipStream_t st : {det_stream, emb_stream, emb_stream2, stream}) {
        if (!st) continue;
        const hipError_t e = hipStreamSynchronize(st);
        if (checked) HIPCHK(e);
    }
}

// Nothing of this pipeline's is held back, queued or running after this.
void frt_pipeline::quiesce() {
    flush();
    drain();
}

// queue one batch through a staging set; caller holds neither mutex
long frt_pipeline::submit(const uint8_t *frames, int n_frames, frt_face_result *results, float *embeds_out, bool synchronous, uint8_t *crops_host) {
    if (n_frames < 1 || n_frames > max_frames) raise(FRT_ERR_CAPACITY, "pipeline: more frames than max_frames");
    use_device(det->device);
    std::lock_guard<std::mutex> lk(async_mu);   // staging sets + ticket order
    std::lock_guard<std::mutex> lr(run_mu);     // the stage enqueue itself (shared with frt_pipeline_run_dev)
    ensure_stream();
    ensure_async();
    const long ticket = next_ticket;
    AsyncBuf &b = abuf[ticket % NBUF];
    if (b.ticket >= 0) {
        // (a ticket that is still held back has no "results have left" event yet: its set's event is its previous occupant's)
        if (holds(b.ticket)) start_held();
        if (is_pending(b.ticket)) flush();
        wait_event_spinning(b.ev_out);  // the staging set is free once its previous batch has left
    }
    b.failed = false;
    hipStream_t s = stream;
    const size_t fbytes = (size_t)det->g.frame_h * det->g.frame_w * 3;
    const Sub me{&b, results, embeds_out, crops_host, n_frames, ticket};
    // ---- adaptive merging at the host boundary (frt_pipeline::Held): join the held call, or become one when the detector is busy
    auto join = [&] {  // this ticket's frames behind the held ones, in the FIRST ticket's staging set
        AsyncBuf &hb = *held.base;
        HIPCHK(hipMemcpyAsync(hb.d_frames + fbytes * (size_t)held.n, frames, fbytes * n_frames, hipMemcpyHostToDevice, copy_stream));
        HIPCHK(hipEventRecord(hb.ev_h2d, copy_stream));
        held.sub[held.nsub++] = me;
        held.n += n_frames;
        if (embeds_out) held.embeds = hb.d_embeds;
        if (crops_host) held.crops = hb.d_crops;
        b.ticket = ticket;
        next_ticket = ticket + 1;
    };
    if (held.base) {
        if (can_join(n_frames)) {
            join();
            if (held.nsub == MAXSUB || 2 * held.n > max_frames || held_must_go()) start_held();
            return ticket;
        }
        start_held();  // cannot join: first in, first out
    }
    if (may_hold(n_frames)) {
        held.base = &b;
        held.frames = b.d_frames;
        held.results = b.d_results;
        held.after = b.ev_h2d;  // recorded behind the last ticket's upload
        join();
        return ticket;
    }
    // A synchronous call that finds nothing else in flight (the reference's request / reply shape: one frame, one caller) has nothing to
    // overlap with: upload, detector, recogniser, match and download go down ONE stream - no stream-to-stream event hand-overs on its
    // critical path (5 of them otherwise; one 4-face call 1.02 -> 0.94 ms, profiles/r03/r03u_sync_overlap.txt).  Calls that arrive while
    // another is in flight take the stage streams as before (and are ordered behind this one through ev_serial).
    bool lone = synchronous && overlap && !npend && !held.base;
    for (int i = 0; lone && i < NBUF; ++i)
        if (abuf[i].ticket >= 0 && i != (int)(ticket % NBUF) && hipEventQuery(abuf[i].ev_out) != hipSuccess) lone = false;
    if (lone) {
        HIPCHK(hipMemcpyAsync(b.d_frames, frames, fbytes * n_frames, hipMemcpyHostToDevice, s));
    } else {
        HIPCHK(hipMemcpyAsync(b.d_frames, frames, fbytes * n_frames, hipMemcpyHostToDevice, copy_stream));
        HIPCHK(hipEventRecord(b.ev_h2d, copy_stream));  // (Request::after)
        // the stages that read the frames (detector, crop) wait for the copy; the caller's stream does not
    }
    // the downloads and the "results have left" event are queued by the pipeline behind this call's match stage - now, or (pairing) with the next call
    lock_run({b.d_frames, n_frames, b.d_results, embeds_out ? b.d_embeds : nullptr, crops_host ? b.d_crops : nullptr, lone ? nullptr : b.ev_h2d, lone, 1, {me}});
    b.ticket = ticket;
    next_ticket = ticket + 1;
    return ticket;
}

void frt_pipeline::wait(long ticket) {
    use_device(det->device);
    hipEvent_t ev = nullptr;
    {
        std::lock_guard<std::mutex> lk(async_mu);
        if (ticket < 0 || ticket >= next_ticket) raise(FRT_ERR_INVALID, "pipeline: unknown ticket");
        AsyncBuf &b = abuf[ticket % NBUF];
        if (b.ticket > ticket) return;  // its staging set was reused, which submit only does after that batch completed
        {
            std::lock_guard<std::mutex> lr(run_mu);
            // submits merged at the host boundary: one of its tickets is being waited for, or the detector has gone idle
            if (held.base && (holds(ticket) || held_must_go())) start_held();
            // pairing: the partners that would share its recogniser pass have not come; adaptive pairing: calls held back behind a busy
            // recogniser go out as soon as a waiting caller finds it idle (they would be running by now had they not been held)
            if (is_pending(ticket) || (npend && group < 0 && !recogniser_busy())) flush();
        }
        ev = b.ev_out;
    }
    wait_event_spinning(ev);
    {
        std::lock_guard<std::mutex> lk(async_mu);
        AsyncBuf &b = abuf[ticket % NBUF];
        if (b.ticket == ticket && b.failed)
            raise(FRT_ERR_DEVICE, "pipeline: the held stages of this call could not be queued" + (held_error.empty() ? std::string() : ": " + held_error));
    }
    emb->check_se_error();
}

extern "C" {

// ------------------------------------------------------------------------------------------------------------ pipeline
int frt_pipeline_create(frt_detector *d, frt_embedder *e, frt_matcher *m, int max_frames, frt_pipeline **out) {
    return guarded([&] {
        if (!d || !e || !out) raise(FRT_ERR_INVALID, "null argument");
        *out = nullptr;
        if (max_frames < 1 || max_frames > d->max_batch) raise(FRT_ERR_CAPACITY, "pipeline: max_frames exceeds det_maxBatchSize");
        if (d->device != e->device || (m && m->device != d->device)) raise(FRT_ERR_INVALID, "pipeline: objects live on different devices");
        use_device(d->device);
        std::unique_ptr<frt_pipeline> p(new frt_pipeline);
        p->det = d; p->emb = e; p->mat = m;
        p->max_frames = max_frames;
        p->max_faces = d->g.max_faces;
        p->F_cap = max_frames * p->max_faces;
        // the pipeline's own join stream is created on first use: ROCm maps streams onto 4 hardware queues round-robin and streams that
        // share a queue serialise, so a stream nobody uses (callers usually pass theirs) should not take a slot among the stage streams
        p->stream = nullptr;
        // the stage streams are created at the highest stream priority: ROCm keeps a separate hardware-queue pool per priority, so they
        // never share a queue with the caller's (normal priority) stream, whose queue holds the pending joins of the batches in flight
        // (run-time switches: frt_pipeline_set_overlap / _set_graph / _check_overlap)
        int prio_lo = 0, prio_hi = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        // hipStreamDefault (blocking), not hipStreamNonBlocking: a gallery reload between calls (hipFree / hipMalloc / synchronous
        // hipMemcpy on the legacy default stream) is then ordered against the stages still in flight without the caller
        // synchronising anything (tests/test_gpu_pipeline.py::test_gallery_reload_between_pipelined_calls); non-blocking
        // streams also measured 1 % slower
        p->copy_prio = prio_hi;
        auto mk = [&](hipStream_t *st) { HIPCHK(hipStreamCreateWithPriority(st, hipStreamDefault, prio_hi)); };
        mk(&p->det_stream);
        mk(&p->emb_stream);
        mk(&p->emb_stream2);
        // recogniser passes of consecutive calls run on two streams with two activation sets
        e->ensure_alt();
        p->d_chw2 = p->arena.alloc<float>((size_t)max_frames * d->g.max_faces * 3 * 112 * 112);
        const size_t F = (size_t)p->F_cap;
        HIPCHK(hipEventCreateWithFlags(&p->ev_serial, hipEventDisableTiming));
        for (int i = 0; i < frt_pipeline::NSLOT; ++i) {
            HIPCHK(hipEventCreateWithFlags(&p->ev_det[i], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&p->ev_emb[i], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&p->ev_done[i], hipEventDisableTiming));
            p->slot_embeds[i] = p->arena.alloc<float>(F * 512);
            p->slot_valid[i] = p->arena.alloc<int>(F);
            p->slot_boxes[i] = p->arena.alloc<frt_bbox>(F);
            p->slot_nout[i] = p->arena.alloc<int>((size_t)max_frames);
            if (d->has_landmarks) p->slot_landmarks[i] = p->arena.alloc<float>(F * 10);
        }
        HIPCHK(hipEventCreateWithFlags(&p->ev_input, hipEventDisableTiming));
        p->d_chw = p->arena.alloc<float>(F * 3 * 112 * 112);
        p->d_sim = p->arena.alloc<float>(F);
        p->d_idx = p->arena.alloc<int32_t>(F);
        p->self_check(false);  // create-time self-check of the stage streams (~1 ms)
        *out = p.release();
    });
}

void frt_pipeline_destroy(frt_pipeline *p) {
    if (!p) return;
    (void)hipSetDevice(p->det->device);
    try {  // pairing / merging: calls still waiting for partners run now - a submitted batch is never dropped
        std::lock_guard<std::mutex> lk(p->run_mu);
        p->flush();
    } catch (...) {
    }
    p->drain(false);
    p->drop_graphs();
    p->release_images();
    if (p->own_stream) (void)hipStreamDestroy(p->own_stream);
    if (p->det_stream) (void)hipStreamDestroy(p->det_stream);
    if (p->emb_stream) (void)hipStreamDestroy(p->emb_stream);
    if (p->emb_stream2) (void)hipStreamDestroy(p->emb_stream2);
    if (p->ev_serial) (void)hipEventDestroy(p->ev_serial);
    if (p->ev_input) (void)hipEventDestroy(p->ev_input);
    if (p->copy_stream) {
        (void)hipStreamSynchronize(p->copy_stream);
        (void)hipStreamDestroy(p->copy_stream);
    }
    for (frt_pipeline::AsyncBuf &b : p->abuf) {
        if (b.ev_h2d) (void)hipEventDestroy(b.ev_h2d);
        if (b.ev_out) (void)hipEventDestroy(b.ev_out);
    }
    for (int i = 0; i < frt_pipeline::NSLOT; ++i) {
        if (p->ev_det[i]) (void)hipEventDestroy(p->ev_det[i]);
        if (p->ev_emb[i]) (void)hipEventDestroy(p->ev_emb[i]);
        if (p->ev_done[i]) (void)hipEventDestroy(p->ev_done[i]);
    }
    p->arena.release();
    delete p;
}

int frt_pipeline_run_dev_after(frt_pipeline *p, const void *frames_dev, int n_frames, void *results_dev, void *embeds_dev, void *ready_event) {
    return guarded([&] {
        if (!p || !frames_dev || !results_dev) raise(FRT_ERR_INVALID, "null argument");
        use_device(p->det->device);
        std::lock_guard<std::mutex> lk(p->run_mu);
        p->run_dev({reinterpret_cast<const uint8_t *>(frames_dev), n_frames, reinterpret_cast<frt_face_result *>(results_dev),
                    reinterpret_cast<float *>(embeds_dev), nullptr, reinterpret_cast<hipEvent_t>(ready_event)});
    });
}

int frt_pipeline_run_dev(frt_pipeline *p, const void *frames_dev, int n_frames, void *results_dev, void *embeds_dev) {
    return frt_pipeline_run_dev_after(p, frames_dev, n_frames, results_dev, embeds_dev, nullptr);
}

int frt_pipeline_check_overlap(frt_pipeline *p, float *ratio_out) {
    int rc = guarded([&] {
        if (!p) raise(FRT_ERR_INVALID, "null argument");
        use_device(p->det->device);
        std::lock_guard<std::mutex> la(p->async_mu);  // same order as submit(): async_mu, then run_mu
        std::lock_guard<std::mutex> lk(p->run_mu);
        p->quiesce();
        p->ensure_stream();
        p->ensure_async();  // the upload stream of frt_pipeline_submit / run takes part
        p->self_check(true);
        if (ratio_out) *ratio_out = p->overlap_ratio;
    });
    if (rc == FRT_OK && p && !p->warning.empty()) frthost::last_error() = p->warning;  // FRT_OK + a message: a warning, not a failure
    return rc;
}

int frt_pipeline_set_input_sync(frt_pipeline *p, int enable) {
    return guarded([&] {
        if (!p) raise(FRT_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(p->run_mu);
        p->input_sync = enable != 0;
    });
}

int frt_pipeline_sync(frt_pipeline *p) {
    return guarded([&] {
        if (!p) raise(FRT_ERR_INVALID, "null argument");
        use_device(p->det->device);
        {
            std::lock_guard<std::mutex> lk(p->run_mu);
            p->flush();
        }
        p->drain();  // (without run_mu: other threads' calls go on being queued while this one waits)
        p->emb->check_se_error();
    });
}

int frt_pipeline_set_stream(frt_pipeline *p, void *hip_stream) {
    return guarded([&] {
        if (!p) raise(FRT_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(p->run_mu);
        use_device(p->det->device);
        p->quiesce();
        p->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : p->own_stream;  // null own_stream: created at the next run
    });
}

int frt_pipeline_set_overlap(frt_pipeline *p, int enable) {
    return guarded([&] {
        if (!p) raise(FRT_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(p->run_mu);
        use_device(p->det->device);
        p->quiesce();
        p->overlap = enable != 0;
        p->seq = 0;
        p->drop_graphs();
    });
}

int frt_pipeline_set_graph(frt_pipeline *p, int enable) {
    return guarded([&] {
        if (!p) raise(FRT_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(p->run_mu);
        use_device(p->det->device);
        p->quiesce();
        p->use_graphs = enable != 0;
        p->drop_graphs();
    });
}

int frt_pipeline_set_align(frt_pipeline *p, int enable) {
    return guarded([&] {
        if (!p) raise(FRT_ERR_INVALID, "null argument");
        if (enable && !p->det->has_landmarks) raise(FRT_ERR_FORMAT, "pipeline: alignment needs a detector blob with the LandmarkHead");
        std::lock_guard<std::mutex> lk(p->run_mu);
        use_device(p->det->device);
        p->quiesce();
        p->align = enable != 0;
    });
}

int frt_pipeline_set_pairing(frt_pipeline *p, int enable) {
    return guarded([&] {
        if (!p) raise(FRT_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(p->run_mu);
        use_device(p->det->device);
        p->flush();
        p->group = enable < 0 ? -1 : (enable == 0 ? 0 : std::min(std::max(enable, 2), (int)frt_pipeline::MAXG));
        p->adaptive_dev = enable == -2;
        p->merge_submits = enable != -3;
    });
}

int frt_pipeline_merge_stats(frt_pipeline *p, long *merged_calls, long *merged_tickets) {
    return guarded([&] {
        if (!p) raise(FRT_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(p->run_mu);
        if (merged_calls) *merged_calls = p->merged_calls;
        if (merged_tickets) *merged_tickets = p->merged_tickets;
    });
}

int frt_pipeline_graph_stats(frt_pipeline *p, long *captured, long *replayed) {
    return guarded([&] {
        if (!p) raise(FRT_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(p->run_mu);
        if (captured) *captured = p->graphs_captured;
        if (replayed) *replayed = p->graphs_replayed;
    });
}

int frt_pipeline_pairing_stats(frt_pipeline *p, long *paired_passes, long *single_passes) {
    return guarded([&] {
        if (!p) raise(FRT_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(p->run_mu);
        if (paired_passes) *paired_passes = p->paired_passes;
        if (single_passes) *single_passes = p->single_passes;
    });
}

// Synchronous host entry point.  Thread-safe: every call takes its own staging set (device frames / results / embeddings) under the
// pipeline's mutexes, so concurrent callers (the reference's Crow server is .multithreaded(), src/app.cpp:367) never share a buffer;
// with several threads calling, their batches overlap in the stage pipeline exactly like submit()/wait() batches do.
int frt_pipeline_run(frt_pipeline *p, const uint8_t *frames, int n_frames, frt_face_result *results, float *embeds_out) {
    return guarded([&] {
        if (!p || !frames || !results) raise(FRT_ERR_INVALID, "null argument");
        p->wait(p->submit(frames, n_frames, results, embeds_out, true));
    });
}

int frt_pipeline_submit(frt_pipeline *p, const uint8_t *frames, int n_frames, frt_face_result *results, float *embeds_out, long *ticket_out) {
    return guarded([&] {
        if (!p || !frames || !results || !ticket_out) raise(FRT_ERR_INVALID, "null argument");
        *ticket_out = p->submit(frames, n_frames, results, embeds_out);
    });
}

int frt_pipeline_submit_crops(frt_pipeline *p, const uint8_t *frames, int n_frames, frt_face_result *results, float *embeds_out, uint8_t *crops_out,
                              long *ticket_out) {
    return guarded([&] {
        if (!p || !frames || !results || !ticket_out) raise(FRT_ERR_INVALID, "null argument");
        *ticket_out = p->submit(frames, n_frames, results, embeds_out, false, crops_out);
    });
}

int frt_pipeline_wait(frt_pipeline *p, long ticket) {
    return guarded([&] {
        if (!p) raise(FRT_ERR_INVALID, "null argument");
        p->wait(ticket);
    });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ stream-overlap self-check
float frt_pipeline::check_streams(const std::vector<hipStream_t> &sts, double us) {
    std::vector<hipEvent_t> a(sts.size()), b(sts.size());
    for (size_t i = 0; i < sts.size(); ++i) {
        HIPCHK(hipEventCreate(&a[i]));
        HIPCHK(hipEventCreate(&b[i]));
        HIPCHK(hipStreamSynchronize(sts[i]));
    }
    for (size_t i = 0; i < sts.size(); ++i) launch_spin(5.0, sts[i]);  // first use of the kernel: code load off the clock
    for (size_t i = 0; i < sts.size(); ++i) HIPCHK(hipStreamSynchronize(sts[i]));
    float worst = 0.f;
    for (int rep = 0; rep < 3; ++rep) {  // best of three: a late host thread inflates a run, nothing deflates it
        for (size_t i = 0; i < sts.size(); ++i) {
            HIPCHK(hipEventRecord(a[i], sts[i]));
            launch_spin(us, sts[i]);
            HIPCHK(hipEventRecord(b[i], sts[i]));
        }
        for (size_t i = 0; i < sts.size(); ++i) HIPCHK(hipEventSynchronize(b[i]));
        float span = 0.f;  // first start -> last end
        for (size_t i = 0; i < sts.size(); ++i) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, a[0], b[i]));
            span = std::max(span, ms);
        }
        const float r = span * 1e3f / (float)us;
        worst = rep == 0 ? r : std::min(worst, r);
    }
    for (size_t i = 0; i < sts.size(); ++i) {
        (void)hipEventDestroy(a[i]);
        (void)hipEventDestroy(b[i]);
    }
    return worst;
}
// Does a wait that is PENDING on stream `j` hold up work on stream `x`?  That is what sharing a hardware queue means for this
// pipeline: kernels of two streams multiplexed onto one queue may still run side by side, but a queue is in-order, so the caller's
// stream - on which every call leaves "wait for the end of my match stage" - blocks whatever stream shares its queue until that
// call has finished, and consecutive calls serialise.  Test: a 400 us probe kernel on `g`, an event behind it that `j` waits for,
// then a 20 us probe on `x`: finished long before the gate opens (ratio << 1) or only behind it (>= 1).
float frt_pipeline::blocked_by_wait(hipStream_t j, hipStream_t x, hipStream_t g) {
    hipEvent_t e0, gate, xb;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&gate));
    HIPCHK(hipEventCreate(&xb));
    for (hipStream_t st : {j, x, g}) HIPCHK(hipStreamSynchronize(st));
    float worst = 0.f;
    for (int rep = 0; rep < 2; ++rep) {
        HIPCHK(hipEventRecord(e0, g));
        launch_spin(400.0, g);
        HIPCHK(hipEventRecord(gate, g));
        HIPCHK(hipStreamWaitEvent(j, gate, 0));
        launch_spin(20.0, x);
        HIPCHK(hipEventRecord(xb, x));
        HIPCHK(hipEventSynchronize(xb));
        HIPCHK(hipStreamSynchronize(j));
        HIPCHK(hipStreamSynchronize(g));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, xb));
        const float r = ms / 0.4f;
        worst = rep == 0 ? r : std::min(worst, r);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(gate);
    (void)hipEventDestroy(xb);
    return worst;
}

void frt_pipeline::self_check(bool with_caller) {
    std::vector<hipStream_t> sts = {det_stream, emb_stream, emb_stream2};
    std::vector<const char *> names = {"detector", "recogniser", "recogniser-2"};
    if (with_caller) {
        if (stream) {
            sts.push_back(stream);
            names.push_back("caller");
        }
        if (copy_stream) {
            sts.push_back(copy_stream);
            names.push_back("upload");
        }
    }
    overlap_ratio = check_streams({det_stream, emb_stream, emb_stream2});
    warning.clear();
    if (with_caller && stream) {  // the hazard proper: a pending join on the caller's stream must not hold up a pipeline stream
        std::string held;
        struct X {
            hipStream_t st;
            const char *name;
            hipStream_t gate_on;
        } xs[] = {{copy_stream, "upload", emb_stream2}, {det_stream, "detector", emb_stream2}, {emb_stream, "recogniser", emb_stream2},
                  {emb_stream2, "recogniser-2", emb_stream}};
        for (const X &x : xs) {
            if (!x.st) continue;
            const float r = blocked_by_wait(stream, x.st, x.gate_on);
            if (r > 0.8f) held += std::string(held.empty() ? "" : ", ") + x.name;
        }
        if (!held.empty()) {
            char buf[768];
            snprintf(buf, sizeof(buf),
                     "frt_pipeline: a wait pending on the caller's stream holds up the pipeline's %s stream(s) - they share a hardware queue, so "
                     "every call's final join blocks the next call and consecutive batches serialise (measured: 4-frame step 0.78 -> 1.65 ms).  "
                     "Hand the pipeline another stream (a newly created one lands on another queue) and check again; see INTEGRATION.md "
                     "'Streams and hardware queues'.",
                     held.c_str());
            warning = buf;
            overlap_ratio = std::max(overlap_ratio, 2.0f);
            if (!getenv("FRT_QUIET")) fprintf(stderr, "[libfrt] warning: %s\n", buf);
            return;
        }
    }
    if (overlap_ratio > 1.5f) {
        // which two?  pairwise probes (only on the failing path: 3 x 150 us per pair)
        std::string pairs;
        for (size_t i = 0; i < sts.size(); ++i)
            for (size_t j = i + 1; j < sts.size(); ++j)
                if (check_streams({sts[i], sts[j]}) > 1.5f) pairs += std::string(pairs.empty() ? "" : ", ") + names[i] + " + " + names[j];
        char buf[768];
        snprintf(buf, sizeof(buf),
                 "frt_pipeline: %zu streams of the stage pipeline do not run side by side (150 us probe kernels took %.2fx as long together as "
                 "alone; sharing a hardware queue: %s): consecutive batches will not overlap.  Create the pipeline - and hand it the "
                 "caller's stream - before the process's other HIP streams (RCCL, codec, copy streams) are created or first used, keep "
                 "GPU_MAX_HW_QUEUES at its default 4, see INTEGRATION.md 'Streams and hardware queues'.",
                 sts.size(), overlap_ratio, pairs.empty() ? "?" : pairs.c_str());
        warning = buf;
        if (!getenv("FRT_QUIET")) fprintf(stderr, "[libfrt] warning: %s\n", buf);
    }
}
