// libfrt.so: whole photos of any sizes (include/frt.h "Whole photos of any sizes"): frt_resize_images, frt_enrol_select_dev,
// frt_pipeline_run_images, frt_pipeline_enrol_images (and its quality-gated twin, include/frt.h "Face quality") - the ragged front end of the pipeline.  A batch is cut into chunks of at most
// max_frames photos (frt_plan_face_chunks); per chunk the photos are packed into pinned memory, uploaded and resized into a device frame
// buffer on the ingest stream, and handed to the pipeline's run_dev path with the resize's event as the call's "frames are ready" event.
// Two staging sets: chunk i + 1 uploads and resizes while chunk i runs, and the pipeline's own stage overlap carries across chunks.
// All device work is hand-written HIP; there is no CPU fallback: without a HIP device every entry point that needs one fails.
#include "frt_pipeline.hpp"

namespace {

using ImageStage = frt_pipeline::ImageStage;

size_t desc_header(int max_images) { return ((size_t)max_images * sizeof(frt_face_desc) + 255) & ~(size_t)255; }

// staging of the image route, allocated on first use (under images_mu); both crop buffers only for the first call that asks for crops.  A
// failed allocation leaves no half-built stage behind: everything is released and the next call starts over.
void ensure_image_stage(frt_pipeline *p, size_t need, bool crops) {
    ImageStage &is = p->images;
    const DetGeom &g = p->det->g;
    const size_t F = (size_t)p->F_cap, hdr = desc_header(p->max_frames);
    try {
        if (!is.built) {
            // beside the pipeline's upload stream: the stage streams' priority class (a pool of hardware queues of its own, see ensure_async)
            HIPCHK(hipStreamCreateWithPriority(&is.ingest, hipStreamNonBlocking, p->copy_prio));
            HIPCHK(hipEventCreateWithFlags(&is.finished, hipEventDisableTiming));
            is.h_count.reserve(1);
            is.d_count.reserve(1);
            for (int b = 0; b < ImageStage::NSET; ++b) {
                HIPCHK(hipEventCreateWithFlags(&is.uploaded[b], hipEventDisableTiming));
                HIPCHK(hipEventCreateWithFlags(&is.ready[b], hipEventDisableTiming));
                HIPCHK(hipEventCreateWithFlags(&is.done[b], hipEventDisableTiming));
                is.d_frames[b].reserve((size_t)p->max_frames * g.frame_h * g.frame_w * 3);
                is.d_results[b].reserve(F);
                is.d_embeds[b].reserve(F * 512);
                is.h_results[b].reserve(F);
                is.h_embeds[b].reserve(F * 512);
            }
            is.built = true;
        }
        for (int b = 0; b < ImageStage::NSET; ++b) {
            if (crops) is.d_crops[b].reserve(F * 112 * 112 * 3);
            if (crops) is.h_crops[b].reserve(F * 112 * 112 * 3);
            is.pack[b].reserve(hdr, need);  // (both sets idle: every call ends with its work complete)
        }
    } catch (...) {
        p->release_images();
        throw;
    }
}

// The chunks of one call through the pipeline, under images_mu.  Per chunk, with run_mu held and behind the pipeline stream's join of the
// chunk's call, `queued(chunk, set, stream)` adds the call's own device work (downloads into the set's pinned staging / the selection
// kernel); `collect(chunk, set)` runs on the host once that work is complete - after the NEXT chunk has been enqueued, so the host copy
// into the caller's memory never holds the device up.
template <typename Queued, typename Collect>
void run_image_chunks(frt_pipeline *p, const frt_face_image *images, const std::vector<frt_face_desc> &desc, const std::vector<frt_face_chunk> &chunks,
                      bool want_embeds, bool want_crops, Queued queued, Collect collect) {
    ImageStage &is = p->images;
    const DetGeom &g = p->det->g;
    const size_t hdr = desc_header(p->max_frames);
    size_t need = 0;
    for (const frt_face_chunk &c : chunks) need = std::max(need, c.bytes);
    ensure_image_stage(p, need, want_crops);
    bool used[ImageStage::NSET] = {false, false};
    auto stage = [&](size_t ci) {  // pack, upload, resize: chunk ci's frames into set ci & 1
        const int b = (int)(ci & 1);
        const frt_face_chunk &c = chunks[ci];
        if (used[b]) wait_event_spinning(is.uploaded[b]);  // the pinned buffer is rewritten only after its upload
        std::memcpy(is.pack[b].h.get(), &desc[(size_t)c.first], (size_t)c.count * sizeof(frt_face_desc));
        pack_face_images(images, desc.data(), c.first, c.count, is.pack[b].h.get() + hdr);
        // the frame buffer only after the stages of the chunk that used it last (the arena: behind that chunk's resize on this stream)
        if (used[b]) HIPCHK(hipStreamWaitEvent(is.ingest, is.done[b], 0));
        HIPCHK(hipMemcpyAsync(is.pack[b].d.get(), is.pack[b].h.get(), hdr + c.bytes, hipMemcpyHostToDevice, is.ingest));
        HIPCHK(hipEventRecord(is.uploaded[b], is.ingest));
        {
            ProfScope ps(2, "images_resize", (double)c.count * g.frame_h * g.frame_w, is.ingest);
            launch_images_resize(is.pack[b].d.get() + hdr, reinterpret_cast<const frt_face_desc *>(is.pack[b].d.get()), c.count, g.frame_h, g.frame_w,
                                 is.d_frames[b].get(), is.ingest);
        }
        HIPCHK(hipEventRecord(is.ready[b], is.ingest));
        used[b] = true;
    };
    auto enqueue = [&](size_t ci) {
        const int b = (int)(ci & 1);
        const frt_face_chunk &c = chunks[ci];
        std::lock_guard<std::mutex> lk(p->run_mu);
        frt_pipeline::Request r;
        r.frames = is.d_frames[b].get();
        r.n = c.count;
        r.results = is.d_results[b].get();
        r.embeds = want_embeds ? is.d_embeds[b].get() : nullptr;
        r.crops = want_crops ? is.d_crops[b].get() : nullptr;
        r.after = is.ready[b];
        p->run_dev(r);
        // A pairing mode that holds run_dev calls (frt_pipeline_set_pairing 1 .. 4 or -2) parks a chunk that could share a recogniser pass:
        // its later stages, and the pipeline stream's join, would come with a later call.  The chunk's own work below reads its results
        // behind that join, and its staging set is reused two chunks on, so whatever is held or pending goes out now, as
        // frt_pipeline_sync does.  (Default mode: run_dev calls are never held and this is a no-op.)
        p->flush();
        queued(c, b, p->stream);
        HIPCHK(hipEventRecord(is.done[b], p->stream));
    };
    try {
        stage(0);
        for (size_t ci = 0; ci < chunks.size(); ++ci) {
            enqueue(ci);
            if (ci + 1 < chunks.size()) stage(ci + 1);
            if (ci > 0) {
                wait_event_spinning(is.done[(ci - 1) & 1]);
                collect(chunks[ci - 1], (int)((ci - 1) & 1));
            }
        }
        const size_t last = chunks.size() - 1;
        wait_event_spinning(is.done[last & 1]);
        collect(chunks[last], (int)(last & 1));
    } catch (...) {  // leave nothing in flight that reads or writes the staging of a call that has returned
        (void)hipStreamSynchronize(is.ingest);
        p->drain(false);
        throw;
    }
    p->emb->check_se_error();
}

std::vector<frt_face_chunk> plan_images(frt_pipeline *p, std::vector<frt_face_desc> &desc) {
    return frt_plan_face_chunks(desc.data(), (int)desc.size(), p->max_frames, FRT_FACES_STAGE_CAP);
}

}  // namespace

void frt_pipeline::release_images() {
    ImageStage &is = images;
    if (is.ingest) {
        (void)hipStreamSynchronize(is.ingest);
        (void)hipStreamDestroy(is.ingest);
    }
    if (is.finished) (void)hipEventDestroy(is.finished);
    if (is.q_up) (void)hipEventDestroy(is.q_up);
    for (int b = 0; b < ImageStage::NSET; ++b)
        for (hipEvent_t ev : {is.uploaded[b], is.ready[b], is.done[b]})
            if (ev) (void)hipEventDestroy(ev);
    is = ImageStage{};  // every buffer goes: the next call starts over
}

extern "C" {

int frt_resize_images(const frt_face_image *images, int n, uint8_t *out, int out_rows, int out_cols, int device) {
    return guarded([&] {
        check_face_images(images, n, "resizeImages");
        if (out_rows < 1 || out_cols < 1 || (size_t)out_rows * (size_t)out_cols > (size_t)INT32_MAX - 256)
            raise(FRT_ERR_INVALID, "resizeImages: bad output size");
        if (n == 0) return;
        if (!out) raise(FRT_ERR_INVALID, "resizeImages: null output");
        std::vector<frt_face_desc> desc = face_descs(images, n);
        const std::vector<frt_face_chunk> chunks = frt_plan_face_chunks(desc.data(), n, n, SIZE_MAX);  // one chunk: one arena, one launch
        const size_t hdr = desc_header(n), px = (size_t)n * out_rows * out_cols * 3;
        std::vector<uint8_t> pack(hdr + chunks[0].bytes);
        std::memcpy(pack.data(), desc.data(), (size_t)n * sizeof(frt_face_desc));
        pack_face_images(images, desc.data(), 0, n, pack.data() + hdr);
        if (device >= 0) use_device(device);
        Arena a;
        struct Guard {
            Arena &a;
            ~Guard() { a.release(); }
        } guard{a};
        uint8_t *d_pack = a.alloc<uint8_t>(pack.size());
        uint8_t *d_out = a.alloc<uint8_t>(px);
        HIPCHK(hipMemcpy(d_pack, pack.data(), pack.size(), hipMemcpyHostToDevice));
        launch_images_resize(d_pack + hdr, reinterpret_cast<const frt_face_desc *>(d_pack), n, out_rows, out_cols, d_out, nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy(out, d_out, px, hipMemcpyDeviceToHost));
    });
}

int frt_enrol_select_dev(const void *results_dev, const void *embeds_dev, int n_frames, int max_faces, void *status_dev, void *face_dev,
                         void *rows_dev, void *count_dev, void *hip_stream) {
    return guarded([&] {
        if (n_frames < 0 || max_faces < 1) raise(FRT_ERR_INVALID, "enrolSelect: n_frames < 0 or max_faces < 1");
        if (n_frames == 0) return;
        if (!results_dev || !embeds_dev || !status_dev || !rows_dev || !count_dev) raise(FRT_ERR_INVALID, "enrolSelect: null argument");
        if (((uintptr_t)embeds_dev | (uintptr_t)rows_dev) & 15) raise(FRT_ERR_INVALID, "enrolSelect: embeds_dev and rows_dev must be 16-byte aligned");
        launch_enrol_select(reinterpret_cast<const frt_face_result *>(results_dev), reinterpret_cast<const float *>(embeds_dev), n_frames, max_faces,
                            reinterpret_cast<int32_t *>(status_dev), reinterpret_cast<frt_face_result *>(face_dev), reinterpret_cast<float *>(rows_dev),
                            reinterpret_cast<int32_t *>(count_dev), reinterpret_cast<hipStream_t>(hip_stream));
        HIPCHK(hipGetLastError());
    });
}

int frt_pipeline_run_images(frt_pipeline *p, const frt_face_image *images, int n, frt_face_result *results, float *embeds_out, uint8_t *crops_out) {
    return guarded([&] {
        check_face_images(images, n, "runImages");
        if (!p) raise(FRT_ERR_INVALID, "runImages: null pipeline");
        if (n == 0) return;
        if (!results) raise(FRT_ERR_INVALID, "runImages: null results");
        std::vector<frt_face_desc> desc = face_descs(images, n);
        const std::vector<frt_face_chunk> chunks = plan_images(p, desc);
        std::lock_guard<std::mutex> li(p->images_mu);
        use_device(p->det->device);
        ImageStage &is = p->images;
        const size_t K = (size_t)p->max_faces;
        run_image_chunks(
            p, images, desc, chunks, embeds_out != nullptr, crops_out != nullptr,
            [&](const frt_face_chunk &c, int b, hipStream_t s) {
                const size_t nf = (size_t)c.count * K;
                HIPCHK(hipMemcpyAsync(is.h_results[b].get(), is.d_results[b].get(), nf * sizeof(frt_face_result), hipMemcpyDeviceToHost, s));
                if (embeds_out) HIPCHK(hipMemcpyAsync(is.h_embeds[b].get(), is.d_embeds[b].get(), nf * 512 * sizeof(float), hipMemcpyDeviceToHost, s));
                if (crops_out) HIPCHK(hipMemcpyAsync(is.h_crops[b].get(), is.d_crops[b].get(), nf * 112 * 112 * 3, hipMemcpyDeviceToHost, s));
            },
            [&](const frt_face_chunk &c, int b) {
                const size_t nf = (size_t)c.count * K, o = (size_t)c.first * K;
                for (size_t f = 0; f < nf; ++f) {  // the chunk-local frame index gets the chunk's base
                    results[o + f] = is.h_results[b].get()[f];
                    results[o + f].frame += c.first;
                }
                if (embeds_out) std::memcpy(embeds_out + o * 512, is.h_embeds[b].get(), nf * 512 * sizeof(float));
                if (crops_out) std::memcpy(crops_out + o * 112 * 112 * 3, is.h_crops[b].get(), nf * 112 * 112 * 3);
            });
    });
}

}  // extern "C"

namespace {

// frt_pipeline_enrol_images and frt_pipeline_enrol_images_gated.  gate null: the first, as it always was - no crops, no quality launch,
// the selection without records.  gate set (its ranges checked by the caller, before anything here): every chunk also leaves its crops,
// the quality launch and the gated selection follow its stages on the pipeline stream, and quality_out (may be null) gets slot 0's
// record of every photo.
void enrol_images(frt_pipeline *p, const frt_face_image *images, int n, const int32_t *labels, const frt_quality_options *gate, int32_t *status_out,
                  frt_face_result *faces_out, struct frt_face_quality *quality_out, float *embeds_out, int *first_row_out, int *n_enrolled_out) {
    {  // (a scope of its own, indented as the entry point's guarded block was: what the ungated call runs reads as it did)
        check_face_images(images, n, "enrolImages");
        if (!p) raise(FRT_ERR_INVALID, "enrolImages: null pipeline");
        if (n > 65536) raise(FRT_ERR_CAPACITY, "enrolImages: more than 65536 images in one call");
        if (n > 0 && !status_out) raise(FRT_ERR_INVALID, "enrolImages: null status_out");
        for (int i = 0; labels && i < n; ++i)
            if (labels[i] < 0) raise(FRT_ERR_INVALID, "enrolImages: image " + std::to_string(i) + ": negative label");
        frt_matcher *m = p->mat;
        if (!m) raise(FRT_ERR_INVALID, "enrolImages: the pipeline has no matcher");
        int rows = 0;
        {  // what the edit will refuse is refused before any device work (the add below checks again: the gallery may change in between)
            std::lock_guard<std::mutex> lm(m->mu);
            rows = m->N;
            if (m->D != 512) raise(FRT_ERR_INVALID, "enrolImages: the gallery does not hold 512-column rows (frt_matcher_init or gallery_begin + commit first)");
            if (m->N > 0 && m->labelled != (labels != nullptr))
                raise(FRT_ERR_INVALID, m->labelled ? "enrolImages: the gallery is labelled (one label per image)"
                                                   : "enrolImages: the gallery has no labels (frt_matcher_set_labels first)");
        }
        if (n_enrolled_out) *n_enrolled_out = 0;
        if (first_row_out) *first_row_out = rows;
        if (n == 0) return;
        std::vector<frt_face_desc> desc = face_descs(images, n);
        const std::vector<frt_face_chunk> chunks = plan_images(p, desc);
        std::lock_guard<std::mutex> li(p->images_mu);
        use_device(p->det->device);
        ImageStage &is = p->images;
        // one call's status words, faces and dense rows
        is.d_rows.reserve((size_t)n * 512);
        is.d_status.reserve((size_t)n);
        is.d_face.reserve((size_t)n);
        is.h_status.reserve((size_t)n);
        is.h_face.reserve((size_t)n);
        const size_t K = (size_t)p->max_faces;
        for (int b = 0; gate && b < ImageStage::NSET; ++b) {
            is.d_quality[b].reserve((size_t)p->F_cap);
            if (quality_out) is.h_quality[b].reserve((size_t)p->F_cap);
        }
        bool first_chunk = true;
        run_image_chunks(
            p, images, desc, chunks, true, gate != nullptr,
            [&](const frt_face_chunk &c, int b, hipStream_t s) {  // after each chunk the selection kernel appends to the one dense buffer
                if (first_chunk) HIPCHK(hipMemsetAsync(is.d_count.get(), 0, sizeof(int32_t), s));
                first_chunk = false;
                if (gate) {  // every slot of the chunk is scored; the selection reads slot 0's record of each photo
                    ProfScope ps(2, "face_quality", (double)c.count * K, s);
                    launch_face_quality(is.d_crops[b].get(), is.d_results[b].get(), c.count * (int)K, *gate, is.d_quality[b].get(), s);
                }
                {
                    ProfScope ps(2, "enrol_select", (double)c.count, s);
                    launch_enrol_select(is.d_results[b].get(), is.d_embeds[b].get(), c.count, p->max_faces, is.d_status.get() + c.first,
                                        is.d_face.get() + c.first, is.d_rows.get(), is.d_count.get(), s, gate ? is.d_quality[b].get() : nullptr);
                }
                if (gate && quality_out)
                    HIPCHK(hipMemcpyAsync(is.h_quality[b].get(), is.d_quality[b].get(), (size_t)c.count * K * sizeof(struct frt_face_quality), hipMemcpyDeviceToHost, s));
            },
            [&](const frt_face_chunk &c, int b) {
                if (!gate || !quality_out) return;
                for (int i = 0; i < c.count; ++i) quality_out[c.first + i] = is.h_quality[b].get()[(size_t)i * K];  // slot 0 of photo i
            });
        {  // status, faces and the count come down once, behind the last chunk's selection, into pinned memory: the copies are asynchronous
           // and run_mu is held for the enqueue alone
            std::lock_guard<std::mutex> lk(p->run_mu);
            p->ensure_stream();
            hipStream_t s = p->stream;
            HIPCHK(hipMemcpyAsync(is.h_count.get(), is.d_count.get(), sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(is.h_status.get(), is.d_status.get(), (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            if (faces_out) HIPCHK(hipMemcpyAsync(is.h_face.get(), is.d_face.get(), (size_t)n * sizeof(frt_face_result), hipMemcpyDeviceToHost, s));
            HIPCHK(hipEventRecord(is.finished, s));
        }
        wait_event_spinning(is.finished);
        const int count = *is.h_count.get();
        if (count < 0 || count > n) raise(FRT_ERR_DEVICE, "enrolImages: the selection returned an impossible count");
        std::memcpy(status_out, is.h_status.get(), (size_t)n * sizeof(int32_t));
        if (faces_out) {
            std::memcpy(faces_out, is.h_face.get(), (size_t)n * sizeof(frt_face_result));
            for (const frt_face_chunk &c : chunks)  // the chunk-local frame index gets the chunk's base
                for (int i = c.first; i < c.first + c.count; ++i) faces_out[i].frame += c.first;
        }
        if (count == 0) return;  // no acceptable photo: no edit
        if (embeds_out) HIPCHK(hipMemcpy(embeds_out, is.d_rows.get(), (size_t)count * 512 * sizeof(float), hipMemcpyDeviceToHost));
        std::vector<int32_t> accepted;
        if (labels) {
            for (int i = 0; i < n; ++i)
                if (status_out[i] == FRT_ENROL_OK) accepted.push_back(labels[i]);
            if ((int)accepted.size() != count) raise(FRT_ERR_DEVICE, "enrolImages: status words and row count disagree");
        }
        // one edit: all accepted rows or none (it takes the matcher's lock itself, checks the gallery's state again and says where the rows went)
        const int first = matcher_add_rows_dev(m, is.d_rows.get(), labels ? accepted.data() : nullptr, count);
        if (first_row_out) *first_row_out = first;
        if (n_enrolled_out) *n_enrolled_out = count;
    }
}

}  // namespace

extern "C" {

int frt_pipeline_enrol_images(frt_pipeline *p, const frt_face_image *images, int n, const int32_t *labels, int32_t *status_out,
                              frt_face_result *faces_out, float *embeds_out, int *first_row_out, int *n_enrolled_out) {
    return guarded([&] { enrol_images(p, images, n, labels, nullptr, status_out, faces_out, nullptr, embeds_out, first_row_out, n_enrolled_out); });
}

int frt_pipeline_enrol_images_gated(frt_pipeline *p, const frt_face_image *images, int n, const int32_t *labels, const frt_quality_options *options,
                                    int32_t *status_out, frt_face_result *faces_out, struct frt_face_quality *quality_out, float *embeds_out,
                                    int *first_row_out, int *n_enrolled_out) {
    return guarded([&] {
        const frt_quality_options gate = quality_checked_options(options, "enrolImages");
        enrol_images(p, images, n, labels, &gate, status_out, faces_out, quality_out, embeds_out, first_row_out, n_enrolled_out);
    });
}

}  // extern "C"
