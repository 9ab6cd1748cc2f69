// Face quality, host side (include/frt.h "Face quality"): the option checks that run before any device work, the launch behind device and
// host pointers, the gated selection's device entry point and frt_pipeline_run_quality.  The kernel is in kernels_quality.hip; the gated
// enrolment shares its body with frt_pipeline_enrol_images (frt_images.cpp).
#include <cmath>

#include "frt_pipeline.hpp"

frt_quality_options quality_checked_options(const frt_quality_options *options, const char *who) {
    frt_quality_options o{0, 0.f, 0.f, 0.f, 255.f, 112 * 112, 0.f};  // nothing can be flagged
    if (!options) return o;
    o = *options;
    const std::string w(who);
    if (o.min_size < 0) raise(FRT_ERR_INVALID, w + ": quality options: min_size < 0");
    if (o.max_clipped < 0) raise(FRT_ERR_INVALID, w + ": quality options: max_clipped < 0");
    if (std::isnan(o.min_sharpness) || std::isnan(o.min_luma_var) || std::isnan(o.min_mean) || std::isnan(o.max_mean) || std::isnan(o.min_score))
        raise(FRT_ERR_INVALID, w + ": quality options: a threshold is NaN");
    if (o.min_mean > o.max_mean) raise(FRT_ERR_INVALID, w + ": quality options: min_mean > max_mean");
    return o;
}

namespace {

constexpr int QUALITY_MAX_FACES = 1 << 20;
constexpr size_t CROP_BYTES = 112 * 112 * 3;

// what both forms of the launch check, in the header's order; -> false: n == 0, nothing to do
bool check_call(int n, const frt_quality_options *options, frt_quality_options &opt, const char *who) {
    if (n < 0 || n > QUALITY_MAX_FACES) raise(FRT_ERR_CAPACITY, std::string(who) + ": n outside 0 .. 1048576");
    opt = quality_checked_options(options, who);
    return n > 0;
}

}  // namespace

extern "C" {

int frt_face_quality_dev(const void *crops_dev, const void *results_dev, int n, const frt_quality_options *options, void *quality_dev, void *hip_stream) {
    return guarded([&] {
        frt_quality_options opt;
        if (!check_call(n, options, opt, "faceQuality")) return;
        if (!crops_dev || !quality_dev) raise(FRT_ERR_INVALID, "faceQuality: null argument");
        if ((uintptr_t)crops_dev & 15) raise(FRT_ERR_INVALID, "faceQuality: crops_dev must be 16-byte aligned");
        if (((uintptr_t)quality_dev & 7) || ((uintptr_t)results_dev & 3)) raise(FRT_ERR_INVALID, "faceQuality: quality_dev must be 8-byte, results_dev 4-byte aligned");
        hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
        ProfScope ps(2, "face_quality", (double)n, s);
        launch_face_quality(reinterpret_cast<const uint8_t *>(crops_dev), reinterpret_cast<const frt_face_result *>(results_dev), n, opt,
                            reinterpret_cast<struct frt_face_quality *>(quality_dev), s);
        HIPCHK(hipGetLastError());
    });
}

int frt_face_quality(const uint8_t *crops, const frt_face_result *results, int n, const frt_quality_options *options, struct frt_face_quality *quality_out,
                     int device) {
    return guarded([&] {
        frt_quality_options opt;
        if (!check_call(n, options, opt, "faceQuality")) return;
        if (!crops || !quality_out) raise(FRT_ERR_INVALID, "faceQuality: null argument");
        if (device >= 0) use_device(device);
        const size_t F = (size_t)n;
        DevBuf<uint8_t> d_crops;
        DevBuf<frt_face_result> d_results;
        DevBuf<struct frt_face_quality> d_quality;
        d_crops.reserve(F * CROP_BYTES);
        if (results) d_results.reserve(F);
        d_quality.reserve(F);
        HIPCHK(hipMemcpy(d_crops.get(), crops, F * CROP_BYTES, hipMemcpyHostToDevice));
        if (results) HIPCHK(hipMemcpy(d_results.get(), results, F * sizeof(frt_face_result), hipMemcpyHostToDevice));
        {
            ProfScope ps(2, "face_quality", (double)n, nullptr);
            launch_face_quality(d_crops.get(), results ? d_results.get() : nullptr, n, opt, d_quality.get(), nullptr);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpy(quality_out, d_quality.get(), F * sizeof(struct frt_face_quality), hipMemcpyDeviceToHost));  // (the one synchronisation)
    });
}

int frt_enrol_select_gated_dev(const void *results_dev, const void *embeds_dev, int n_frames, int max_faces, void *status_dev, void *face_dev,
                               void *rows_dev, void *count_dev, void *hip_stream, const void *quality_dev) {
    return guarded([&] {  // frt_enrol_select_dev's checks, word for word
        if (n_frames < 0 || max_faces < 1) raise(FRT_ERR_INVALID, "enrolSelect: n_frames < 0 or max_faces < 1");
        if (n_frames == 0) return;
        if (!results_dev || !embeds_dev || !status_dev || !rows_dev || !count_dev) raise(FRT_ERR_INVALID, "enrolSelect: null argument");
        if (((uintptr_t)embeds_dev | (uintptr_t)rows_dev) & 15) raise(FRT_ERR_INVALID, "enrolSelect: embeds_dev and rows_dev must be 16-byte aligned");
        if ((uintptr_t)quality_dev & 7) raise(FRT_ERR_INVALID, "enrolSelect: quality_dev must be 8-byte aligned");
        launch_enrol_select(reinterpret_cast<const frt_face_result *>(results_dev), reinterpret_cast<const float *>(embeds_dev), n_frames, max_faces,
                            reinterpret_cast<int32_t *>(status_dev), reinterpret_cast<frt_face_result *>(face_dev), reinterpret_cast<float *>(rows_dev),
                            reinterpret_cast<int32_t *>(count_dev), reinterpret_cast<hipStream_t>(hip_stream),
                            reinterpret_cast<const struct frt_face_quality *>(quality_dev));
        HIPCHK(hipGetLastError());
    });
}

int frt_pipeline_run_quality(frt_pipeline *p, const uint8_t *frames, int n_frames, const frt_quality_options *options, frt_face_result *results,
                             struct frt_face_quality *quality_out, float *embeds_out, uint8_t *crops_out) {
    return guarded([&] {
        if (!p || !frames || !results || !quality_out) raise(FRT_ERR_INVALID, "runQuality: null argument");
        const frt_quality_options opt = quality_checked_options(options, "runQuality");
        if (n_frames < 1 || n_frames > p->max_frames) raise(FRT_ERR_CAPACITY, "runQuality: n_frames outside 1 .. max_frames");
        std::lock_guard<std::mutex> li(p->images_mu);  // the staging below is the image stage's: images_mu -> run_mu -> object mutexes
        use_device(p->det->device);
        frt_pipeline::ImageStage &is = p->images;
        const size_t frame_bytes = (size_t)p->det->g.frame_h * p->det->g.frame_w * 3, F = (size_t)n_frames * p->max_faces;
        if (!is.q_up) HIPCHK(hipEventCreateWithFlags(&is.q_up, hipEventDisableTiming));
        // (idle: every call that uses this staging ends with its work complete)
        is.q_frames.reserve((size_t)n_frames * frame_bytes);
        is.q_results.reserve(F);
        is.q_embeds.reserve(F * 512);
        is.q_crops.reserve(F * CROP_BYTES);
        is.q_quality.reserve(F);
        std::lock_guard<std::mutex> lr(p->run_mu);
        p->ensure_stream();
        hipStream_t s = p->stream;
        try {
            HIPCHK(hipMemcpyAsync(is.q_frames.get(), frames, n_frames * frame_bytes, hipMemcpyHostToDevice, s));
            HIPCHK(hipEventRecord(is.q_up, s));
            frt_pipeline::Request r;
            r.frames = is.q_frames.get();
            r.n = n_frames;
            r.results = is.q_results.get();
            r.embeds = is.q_embeds.get();
            r.crops = is.q_crops.get();
            r.after = is.q_up;
            p->run_dev(r);
            p->flush();  // (a pairing mode that holds run_dev calls: the join must be on the stream before the quality launch reads the crops)
            {
                ProfScope ps(2, "face_quality", (double)F, s);
                launch_face_quality(is.q_crops.get(), is.q_results.get(), (int)F, opt, is.q_quality.get(), s);
                HIPCHK(hipGetLastError());
            }
            HIPCHK(hipMemcpyAsync(results, is.q_results.get(), F * sizeof(frt_face_result), hipMemcpyDeviceToHost, s));
            if (embeds_out) HIPCHK(hipMemcpyAsync(embeds_out, is.q_embeds.get(), F * 512 * sizeof(float), hipMemcpyDeviceToHost, s));
            if (crops_out) HIPCHK(hipMemcpyAsync(crops_out, is.q_crops.get(), F * CROP_BYTES, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(quality_out, is.q_quality.get(), F * sizeof(struct frt_face_quality), hipMemcpyDeviceToHost, s));
            sync_stream_spinning(s);
        } catch (...) {  // leave nothing in flight that reads or writes the staging of a call that has returned
            p->drain(false);
            throw;
        }
        p->emb->check_se_error();
    });
}

}  // extern "C"
