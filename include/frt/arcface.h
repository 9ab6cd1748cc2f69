// Drop-in for /root/reference/src/arcface.h: getCroppedFaces, struct CroppedFace and class ArcFaceIR50 with the reference's
// public surface (src/arcface.h:11-39).  Differences, all deliberate:
//   * featureMatching() returns an object-owned, reused buffer (the reference leaks new float[F*N] per call, arcface.cpp:194);
//   * forward() with rec_maxBatchSize >= 2 implements the evident intent (the reference's batched branch overflows m_embed);
//   * initKnownEmbeds() frees the previous gallery (the reference leaks it on every /reload);
//   * crop + resize + normalise run in one HIP kernel; CroppedFace.face still holds the u8 BGR 112x112 crop (app.cpp:329)
//     and CroppedFace.faceMat the fp32 planar RGB tensor, like after the reference's preprocessFaces().
#ifndef FRT_ARCFACE_H
#define FRT_ARCFACE_H

#include <algorithm>
#include <array>
#include <cassert>
#include <cstring>
#include <iterator>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include <tuple>
#include <utility>

#include "coalesce.h"
#include "common.h"
#include "cvlite.h"
#include "matmul.h"
#include "tracker.h"

struct CroppedFace {
    cv::Mat face;     // u8 BGR crop
    cv::Mat faceMat;  // getCroppedFaces: same u8 crop; after ArcFaceIR50::forward: CV_32FC1 [3*112 x 112] planar RGB
    int x1, y1, x2, y2;
};

// Extension (include/frt.h "Face quality"): the record and the gate's thresholds under their C++ names.  The defaults flag nothing; there
// are no recommended thresholds - measure on your own faces first.
struct FaceQuality : frt_face_quality {
    FaceQuality() : frt_face_quality() {}
    bool passes() const { return present != 0 && flags == 0; }
};
struct QualityOptions : frt_quality_options {
    QualityOptions() {
        min_size = 0;
        min_sharpness = min_luma_var = min_mean = min_score = 0.f;
        max_mean = 255.f;
        max_clipped = 112 * 112;
    }
};

// src/arcface.cpp:3-17 (ROI = cols [y1,y2) x rows [x1,x2); INTER_CUBIC to resize_w x resize_h)
inline void getCroppedFaces(cv::Mat frame, std::vector<struct Bbox> &outputBbox, int resize_w, int resize_h, std::vector<struct CroppedFace> &croppedFaces) {
    croppedFaces.clear();
    const int n = (int)outputBbox.size();
    if (!n) return;
    std::vector<unsigned char> crops((size_t)n * resize_h * resize_w * 3);
    checkFrtStatus(frt_crop_faces(frame.data, frame.rows, frame.cols, (size_t)frame.step, reinterpret_cast<const frt_bbox *>(outputBbox.data()), n,
                                  resize_w, resize_h, crops.data(), -1));
    for (int i = 0; i < n; ++i) {
        CroppedFace c;
        c.faceMat = cv::Mat(resize_h, resize_w, CV_8UC3, &crops[(size_t)i * resize_h * resize_w * 3]).clone();
        c.face = c.faceMat.clone();
        c.x1 = outputBbox[i].x1;
        c.y1 = outputBbox[i].y1;
        c.x2 = outputBbox[i].x2;
        c.y2 = outputBbox[i].y2;
        croppedFaces.push_back(c);
    }
}

// `static int classCount` of the reference (src/arcface.h:39, defined once in src/arcface.cpp:19).  This shell is header-only and
// the reference includes arcface.h from two translation units (src/app.cpp:3 and src/db.cpp via src/db.h:8), so the definition
// has to be ODR-safe in C++11 (no inline variables): a static data member of a class TEMPLATE may be defined in a header, and
// ArcFaceIR50 inherits it - `ArcFaceIR50::classCount` / `recognizer.classCount` keep working unchanged.
template <class Tag = void>
struct ArcFaceIR50Statics {
    static int classCount;  // process-wide, as in the reference
};
template <class Tag>
int ArcFaceIR50Statics<Tag>::classCount = 0;

// engineFile (config.json's rec_engine) may be any of the six recogniser blobs weights_io.py exports: IR-50 (the reference's network),
// IR-100, IR-152 and their SE variants (--kind ir50 | ir100 | ir152 | ir_se50 | ir_se100 | ir_se152).  The depth is read from the
// blob; the class keeps the reference's name and API for all of them.
class ArcFaceIR50 : public ArcFaceIR50Statics<> {
  public:
    ArcFaceIR50(TRTLogger gLogger, const std::string engineFile, int frameWidth, int frameHeight, std::string inputName, std::string outputName,
                std::vector<int> inputShape, int outputDim, int maxBatchSize, int maxFacesPerScene, float knownPersonThreshold, int device = 0)
        : croppedFaces(this), h_(nullptr), m_id(frtdetail::nextObjectId()), m_frameWidth(frameWidth), m_frameHeight(frameHeight), m_OUTPUT_D(outputDim),
          m_maxBatchSize(maxBatchSize), m_maxFacesPerScene(maxFacesPerScene), m_knownPersonThresh(knownPersonThreshold), matmul(device), m_templates(device) {
        (void)gLogger;
        (void)inputName;
        (void)outputName;
        assert(inputShape.size() == 3);  // src/arcface.cpp:25
        m_INPUT_C = inputShape[0];
        m_INPUT_H = inputShape[1];
        m_INPUT_W = inputShape[2];
        // FRT_COALESCE=<frames>: the recogniser must be able to take the faces of a coalesced batch in one pass
        const int envFrames = frtdetail::coalesceEnv().frames;
        const int devBatch = std::max(maxBatchSize, envFrames * maxFacesPerScene);
        checkFrtStatus(frt_embedder_create(engineFile.c_str(), m_INPUT_C, m_INPUT_H, m_INPUT_W, outputDim, devBatch, device, &h_));
        std::cout << "[INFO] Loading ArcFace Engine...\n";
        croppedFaces.reserve((size_t)maxFacesPerScene);
        m_device = device;
        m_devBatch = devBatch;
        if (envFrames > 0) {
            m_auto = true;
            try {
                frtdetail::autoLink(false, frtdetail::Pending{device, frameWidth, frameHeight, devBatch, nullptr, h_, matmul.handle(), &m_link});
            } catch (...) {
                frt_embedder_destroy(h_);
                throw;
            }
        }
    }
    ~ArcFaceIR50() {
        frtdetail::autoUnlink(false, &m_link);
        if (std::shared_ptr<frtdetail::CoalesceLink> l = link()) l->shutdown();  // the coalescer borrows this object's embedder and matcher (waits for calls inside it)
        if (m_photoPipe) frt_pipeline_destroy(m_photoPipe);  // (enrolImages' pipeline borrows them too)
        frt_embedder_destroy(h_);
        frtdetail::retireObject(m_id);  // every thread drops its per-thread state of this object (page-locked similarity buffers) on its next access
    }
    // Opt-in request coalescing (include/frt/coalesce.h): findFace() calls of concurrent request threads on `detector` share one device
    // batch - detector, crop, recogniser, top-1 - and this object's forward() / featureMatching() / getOutputs() on the same thread, frame
    // and boxes answer from what that batch computed.  maxFrames 0: the detector's maxBatchSize (construct both objects with room:
    // detector maxBatchSize >= maxFrames, recogniser maxBatchSize >= maxFrames * maxFacesPerScene).  FRT_COALESCE=<frames>[:<window_us>]
    // in the environment does all of this without a code change.
    template <class Detector>
    void coalesceWith(Detector &detector, int maxFrames = 0, int windowUs = 100) {
        std::shared_ptr<frtdetail::CoalesceLink> l = frtdetail::makeLink(detector.handle(), h_, matmul.handle(), maxFrames, windowUs);
        if (std::shared_ptr<frtdetail::CoalesceLink> old = link()) old->shutdown();
        std::atomic_store(&m_link, l);
        detector.attachCoalescer(l);
    }
    // Extension (round 5): fp32 end-to-end recogniser (BASELINE configs[1]'s "fp32"; see frt_embedder_set_precision).  Default: fp16 MFMA.
    void setPrecisionFp32(bool on) { checkFrtStatus(frt_embedder_set_precision(h_, on ? 1 : 0)); }
    // Extension: flip-augmented embeddings, normalize(pre(face) + pre(mirrored face)), on every path through this object (see
    // frt_embedder_set_flip).  Gallery and probes must be embedded in the same mode: switching means re-enrolling.  Default: off.
    void setFlipAugment(bool on) { checkFrtStatus(frt_embedder_set_flip(h_, on ? 1 : 0)); }
    bool flipAugment() const {
        int on = 0;
        checkFrtStatus(frt_embedder_get_flip(h_, &on));
        return on != 0;
    }
    ArcFaceIR50(const ArcFaceIR50 &) = delete;
    ArcFaceIR50 &operator=(const ArcFaceIR50 &) = delete;

    // src/arcface.cpp:105-114: BGR->RGB, (x-127.5)*0.0078125, planar; output becomes CV_32FC1 [3*H x W]
    void preprocessFace(cv::Mat &face, cv::Mat &output) {
        cv::Mat tight = face.isContinuous() ? face : face.clone();
        output = cv::Mat(3 * m_INPUT_H, m_INPUT_W, CV_32FC1);
        checkFrtStatus(frt_embedder_preprocess_face(h_, tight.data, output.ptr<float>(0)));
    }
    void doInference(float *input, float *output) { checkFrtStatus(frt_embedder_infer(h_, input, 1, output)); }                          // arcface.cpp:131-137
    void doInference(float *input, float *output, int batchSize) { checkFrtStatus(frt_embedder_infer(h_, input, batchSize, output)); }  // arcface.cpp:139-148

    // Gallery management (src/arcface.cpp:150-164, :233-236).  The reference keeps a host array m_knownEmbeds (new float[num*D], never
    // freed) and uploads it in initMatMul; here every row goes straight into libfrt's pinned staging chunks and on to the device
    // while the caller (Database::getEmbeddings, src/db.cpp:316-346) fetches the next one - no second 2 GB host copy, no leak on
    // /reload, and the previous gallery stays searchable until initMatMul() swaps the new one in.
    void addEmbedding(const std::string className, float embedding[]) {  // arcface.cpp:150-154 (copies immediately: db.cpp:339 passes a blob pointer)
        matmul.galleryAppend(embedding, 1);
        classNames.push_back(className);
        classCount++;
    }
    void addEmbedding(const std::string className, std::vector<float> embedding) {  // arcface.cpp:156-160
        assert((int)embedding.size() == m_OUTPUT_D);
        matmul.galleryAppend(embedding.data(), 1);
        classNames.push_back(className);
        classCount++;
    }
    // Extension: bulk enrolment (one call for n rows; db.cpp:339's loop collapses to this)
    void addEmbeddings(const std::vector<std::string> &names, const float *embeddings) {
        matmul.galleryAppend(embeddings, (int)names.size());
        classNames.insert(classNames.end(), names.begin(), names.end());
        classCount += (int)names.size();
    }
    // Extension: live enrolment - what /insert/face and /delete/user (src/app.cpp:131-229) need so that nobody has to post /reload
    // (src/app.cpp:354-365).  The rows go to / leave the gallery the matcher is answering from (frt_matcher_gallery_add / _remove: the rows
    // already there stay on the device) and classNames / classCount move with them; the next featureMatching() sees the change.  Not for
    // use between initKnownEmbeds() and initMatMul(): a load in progress replaces the gallery at its commit.
    void enrolEmbedding(const std::string &className, const float embedding[]) { enrolEmbeddings(std::vector<std::string>(1, className), embedding); }
    void enrolEmbedding(const std::string &className, const std::vector<float> &embedding) {
        assert((int)embedding.size() == m_OUTPUT_D);
        enrolEmbedding(className, embedding.data());
    }
    void enrolEmbeddings(const std::vector<std::string> &names, const float *embeddings) {
        if (matmul.numRows() == 0 && classNames.empty()) {  // never loaded (or emptied): an empty gallery of this width first
            matmul.galleryBegin(0, m_OUTPUT_D);
            matmul.galleryCommit();
        }
        if (m_labelsSet && matmul.numRows() > 0) {  // the matcher carries labels (matchTopIdentities was used): the new rows bring theirs
            std::vector<int> labels;
            for (size_t i = 0; i < names.size(); ++i) labels.push_back(internLabel(names[i]));
            matmul.galleryAddLabeled(embeddings, labels.data(), (int)names.size());
        } else {
            matmul.galleryAdd(embeddings, (int)names.size());
            m_labelsSet = false;  // (an emptied gallery became unlabelled by the plain add)
        }
        classNames.insert(classNames.end(), names.begin(), names.end());
        classCount += (int)names.size();
    }
    // Extension: enrolEmbeddings from the face images themselves - /insert/face with api_imgIsCropped (src/app.cpp:148-162) and the gen
    // loop (src/app.cpp:79-97) for n images of any sizes (8UC3) in one call: resize + preprocessFace + inference on the device, and the
    // embeddings go into the live gallery device to device, as ONE edit (frt_embedder_enrol_faces).  classNames / classCount / labels move
    // as in enrolEmbeddings.  embeddingsOut (may be null): [n x outputDim], what db.insertFace stores.  At most 65536 images per call.
    void enrolFaces(const std::vector<std::string> &names, const std::vector<cv::Mat> &faces, float *embeddingsOut = nullptr) {
        assert(names.size() == faces.size());
        if (matmul.numRows() == 0 && classNames.empty()) {
            matmul.galleryBegin(0, m_OUTPUT_D);
            matmul.galleryCommit();
        }
        const std::vector<frt_face_image> imgs = faceImages(faces);
        const bool labelled = m_labelsSet && matmul.numRows() > 0;
        std::vector<int> labels;
        for (size_t i = 0; labelled && i < names.size(); ++i) labels.push_back(internLabel(names[i]));
        int first = 0;
        checkFrtStatus(frt_embedder_enrol_faces(h_, matmul.handle(), imgs.data(), (int)imgs.size(), labelled ? labels.data() : nullptr, embeddingsOut, &first));
        if (!labelled) m_labelsSet = false;
        classNames.insert(classNames.end(), names.begin(), names.end());
        classCount += (int)names.size();
    }
    // Extension: /insert/face WITHOUT api_imgIsCropped (src/app.cpp:163-187) for n whole photos of any sizes (8UC3) in one call: each photo is
    // stretched to the frame size (cv::resize, INTER_LINEAR), detected and cropped on the device; a photo with exactly one face is embedded
    // and enrolled, the others are refused as the handler refuses them - status[i] = FRT_ENROL_OK (1), FRT_ENROL_MANY (2: ret = 2),
    // FRT_ENROL_NONE (3: ret = 3) or FRT_ENROL_EMPTY_ROI (4).  The accepted rows enter the live gallery device to device as ONE edit
    // (frt_pipeline_enrol_images); classNames / classCount / labels move as in enrolFaces, by the accepted names only.  embeddingsOut (may be
    // null; room for [n x outputDim]): the rows added, in image order - what db.insertFace stores.  The object keeps one pipeline, created at
    // the first call for the detector's maxBatchSize frames (the recogniser needs maxBatchSize >= that x maxFacesPerScene for one pass per
    // chunk; smaller works, in several passes); the detector must outlive this object or the next call with another detector.
    // With labels in use (matchTopIdentities) every name is interned before the call, as enrolFaces does - the labels must exist when the
    // photos go in - so the name of a refused photo keeps a label that no row carries yet; answers do not change, a later enrolment of that
    // name reuses it.
    template <class Detector>
    void enrolImages(Detector &detector, const std::vector<std::string> &names, const std::vector<cv::Mat> &images, std::vector<int> &status,
                     float *embeddingsOut = nullptr) {
        enrolPhotos(detector, names, images, status, nullptr, nullptr, embeddingsOut);
    }
    // Extension: enrolImages with the quality gate at the door (frt_pipeline_enrol_images_gated): a photo whose one face carries a quality
    // flag under `quality` comes back FRT_ENROL_LOW_QUALITY (5) and is not enrolled; qualityOut[i] is the face's record (all zero without a
    // valid face).  A default-constructed QualityOptions flags nothing.
    template <class Detector>
    void enrolImages(Detector &detector, const std::vector<std::string> &names, const std::vector<cv::Mat> &images, std::vector<int> &status,
                     const QualityOptions &quality, std::vector<FaceQuality> &qualityOut, float *embeddingsOut = nullptr) {
        qualityOut.assign(images.size(), FaceQuality());
        enrolPhotos(detector, names, images, status, &quality, qualityOut.data(), embeddingsOut);
    }
    // Extension: the quality records of croppedFaces - the u8 crops forward() left - in one launch (frt_face_quality).  boxes: the
    // outputBbox forward() was given (size and score come from them, and SMALL / LOW_SCORE are evaluated); null: crops alone.
    std::vector<FaceQuality> faceQuality(const QualityOptions &options = QualityOptions(), const std::vector<struct Bbox> *boxes = nullptr) {
        const size_t n = croppedFaces.size(), bytes = (size_t)112 * 112 * 3;
        std::vector<FaceQuality> out(n);
        if (!n) return out;
        if (boxes && boxes->size() != n) throw std::logic_error("faceQuality: one box per cropped face");
        std::vector<unsigned char> crops(n * bytes);
        std::vector<frt_face_result> recs(boxes ? n : 0);
        for (size_t i = 0; i < n; ++i) {
            const cv::Mat &f = croppedFaces[i].face;
            if (f.rows != 112 || f.cols != 112 || f.type() != CV_8UC3) throw std::logic_error("faceQuality: a cropped face is not 112 x 112 8UC3");
            for (int r = 0; r < 112; ++r) std::memcpy(&crops[i * bytes + (size_t)r * 112 * 3], f.data + (size_t)r * f.step, 112 * 3);
            if (boxes) {
                frt_face_result rec = frt_face_result();
                rec.box.x1 = (*boxes)[i].x1;
                rec.box.y1 = (*boxes)[i].y1;
                rec.box.x2 = (*boxes)[i].x2;
                rec.box.y2 = (*boxes)[i].y2;
                rec.box.score = (*boxes)[i].score;
                rec.valid = 1;
                recs[i] = rec;
            }
        }
        checkFrtStatus(::frt_face_quality(crops.data(), boxes ? recs.data() : nullptr, (int)n, &options, out.data(), m_device));
        return out;
    }
    // Extension: a large photo by tiles, recognised in one call (include/frt.h "Recognising a large photo by tiles"): what
    // detector.findFaceTiled(photo, options, maxOut), this object's forward on the boxes with min(x2 - x1, y2 - y1) >= minFace and matchTop1
    // return, with the photo uploaded once and everything between the stages left on the device.  photo is CV_8UC3 of ANY size.  Returns the
    // kept boxes in PHOTO coordinates, best first; names / sims: per box the best gallery row's className and its similarity - "" and 0 for a
    // box whose ROI is empty and for an empty gallery (valid, when asked for, tells the two apart).  Uses enrolImages' pipeline (created at
    // the first call of either); passes are this object's maxBatchSize faces.
    template <class Detector>
    std::vector<struct Bbox> recognizeTiled(Detector &detector, cv::Mat &photo, std::vector<std::string> &names, std::vector<float> &sims,
                                            const frt_tile_options *options = nullptr, int minFace = 0, int maxOut = 256,
                                            std::vector<int> *valid = nullptr, std::vector<int> *sources = nullptr) {
        photoPipe(detector);
        const size_t cap = (size_t)std::max(maxOut, 1);
        std::vector<frt_face_result> res(cap);
        std::vector<int32_t> src(cap);
        int n = 0;
        checkFrtStatus(frt_pipeline_run_photo_tiled(m_photoPipe, photo.data, photo.rows, photo.cols, (size_t)photo.step, options, minFace, maxOut,
                                                    res.data(), nullptr, nullptr, nullptr, src.data(), &n));
        std::vector<struct Bbox> out((size_t)n);
        names.assign((size_t)n, std::string());
        sims.assign((size_t)n, 0.f);
        if (valid) valid->assign((size_t)n, 0);
        for (int i = 0; i < n; ++i) {
            const frt_face_result &r = res[(size_t)i];
            std::memcpy(&out[(size_t)i], &r.box, sizeof(frt_bbox));
            if (valid) (*valid)[(size_t)i] = r.valid;
            if (r.match_idx >= 0 && (size_t)r.match_idx < classNames.size()) {
                names[(size_t)i] = classNames[(size_t)r.match_idx];
                sims[(size_t)i] = r.match_sim;
            }
        }
        if (sources) sources->assign(src.begin(), src.begin() + n);
        return out;
    }
    // Extension: the /inference loop for video (include/frt.h "Face tracker"): the current frames of several streams (each CV_8UC3 of the
    // frame size; frame i belongs to stream streamIds[i], empty: to stream i) go through detector -> crop -> recogniser -> match as one
    // pipeline call, and the tracker follows the faces on the device.  Returns the pipeline's records [frames x maxFacesPerScene]; tracks
    // receives one record per face slot (a stable track_id, age, hits, confirmed), names the className of the row the TRACK's running
    // template matches best - as getOutputs names rows - and "" for a face without a track, without an embedding yet, or with an empty
    // gallery; sims (may be null) the template's similarity.  Uses enrolImages' pipeline; the tracker's maxFaces must be maxFacesPerScene.
    template <class Detector>
    std::vector<frt_face_result> trackFaces(Detector &detector, FaceTracker &tracker, const std::vector<cv::Mat> &frames, const std::vector<int> &streamIds,
                                            std::vector<frt_track_result> &tracks, std::vector<std::string> &names, std::vector<float> *sims = nullptr) {
        photoPipe(detector);
        const size_t n = frames.size(), slots = n * (size_t)tracker.maxFaces(), rowBytes = (size_t)m_frameWidth * 3;
        std::vector<uint8_t> packed(n * (size_t)m_frameHeight * rowBytes);
        for (size_t i = 0; i < n; ++i) {
            if (frames[i].rows != m_frameHeight || frames[i].cols != m_frameWidth) throw std::logic_error("trackFaces: a frame is not frameHeight x frameWidth");
            for (int r = 0; r < m_frameHeight; ++r)
                std::memcpy(&packed[(i * (size_t)m_frameHeight + (size_t)r) * rowBytes], frames[i].data + (size_t)r * (size_t)frames[i].step, rowBytes);
        }
        std::vector<frt_face_result> res(slots);
        tracks.assign(slots, frt_track_result());
        const std::vector<int32_t> ids(streamIds.begin(), streamIds.end());
        checkFrtStatus(frt_pipeline_run_tracked(m_photoPipe, tracker.handle(), packed.data(), (int)n, ids.empty() ? nullptr : ids.data(), res.data(),
                                                tracks.data(), nullptr, nullptr));
        names.assign(slots, std::string());
        if (sims) sims->assign(slots, 0.f);
        for (size_t i = 0; i < slots; ++i) {
            const frt_track_result &t = tracks[i];
            if (t.match_idx >= 0 && (size_t)t.match_idx < classNames.size()) {
                names[i] = classNames[(size_t)t.match_idx];
                if (sims) (*sims)[i] = t.match_sim;
            }
        }
        return res;
    }
    // trackFaces with the gate in front of the recogniser (include/frt.h "Gate"): a face that a confirmed track follows is neither cropped
    // nor embedded nor matched - its record keeps the box and has valid 0 -, and its name is its track's as above.  gate receives one record
    // per face slot (embedded, and why, or followed); nEmbed (may be null) how many faces went through the recogniser.  The options have no
    // defaults.
    template <class Detector>
    std::vector<frt_face_result> trackFaces(Detector &detector, FaceTracker &tracker, const frt_track_gate_options &options, const std::vector<cv::Mat> &frames,
                                            const std::vector<int> &streamIds, std::vector<frt_track_result> &tracks, std::vector<frt_track_gate> &gate,
                                            std::vector<std::string> &names, std::vector<float> *sims = nullptr, int *nEmbed = nullptr) {
        photoPipe(detector);
        const size_t n = frames.size(), slots = n * (size_t)tracker.maxFaces(), rowBytes = (size_t)m_frameWidth * 3;
        std::vector<uint8_t> packed(n * (size_t)m_frameHeight * rowBytes);
        for (size_t i = 0; i < n; ++i) {
            if (frames[i].rows != m_frameHeight || frames[i].cols != m_frameWidth) throw std::logic_error("trackFaces: a frame is not frameHeight x frameWidth");
            for (int r = 0; r < m_frameHeight; ++r)
                std::memcpy(&packed[(i * (size_t)m_frameHeight + (size_t)r) * rowBytes], frames[i].data + (size_t)r * (size_t)frames[i].step, rowBytes);
        }
        std::vector<frt_face_result> res(slots);
        tracks.assign(slots, frt_track_result());
        gate.assign(slots, frt_track_gate());
        const std::vector<int32_t> ids(streamIds.begin(), streamIds.end());
        int32_t embedded = 0;
        checkFrtStatus(frt_pipeline_run_tracked_gated(m_photoPipe, tracker.handle(), &options, packed.data(), (int)n, ids.empty() ? nullptr : ids.data(),
                                                      res.data(), tracks.data(), gate.data(), nullptr, nullptr, nullptr, &embedded));
        if (nEmbed) *nEmbed = embedded;
        names.assign(slots, std::string());
        if (sims) sims->assign(slots, 0.f);
        for (size_t i = 0; i < slots; ++i) {
            const frt_track_result &t = tracks[i];
            if (t.match_idx >= 0 && (size_t)t.match_idx < classNames.size()) {
                names[i] = classNames[(size_t)t.match_idx];
                if (sims) (*sims)[i] = t.match_sim;
            }
        }
        return res;
    }
    // every row of that name, as /delete/user removes every face of the user; the rows behind them close up in order (the order a
    // /reload would read them in: src/db.cpp:316-346).  Returns how many there were.
    int removeClass(const std::string &className) {
        std::vector<int> rows;
        for (size_t i = 0; i < classNames.size(); ++i)
            if (classNames[i] == className) rows.push_back((int)i);
        if (rows.empty()) return 0;
        matmul.galleryRemove(rows.data(), (int)rows.size());
        if (m_labelsFromCluster) {
            // clusterGallery's labels are ROW INDICES of the gallery as it was: the rows have moved, and a person whose first row has just
            // gone would keep the removed className.  The matcher goes back to no labels; the next ranked call interns classNames again.
            matmul.setLabels(nullptr, 0);
            forgetLabels();
        }
        classNames.erase(std::remove(classNames.begin(), classNames.end(), className), classNames.end());
        classCount -= (int)rows.size();
        return (int)rows.size();
    }
    void initKnownEmbeds(int num) { matmul.galleryBegin(num, m_OUTPUT_D); }  // arcface.cpp:162
    void initMatMul() {                                                       // arcface.cpp:164
        matmul.galleryCommit();
        forgetLabels();  // the commit replaced the gallery; matchTopIdentities sets the labels of the new one when it is next used
    }
    void resetEmbeddings() {                                                  // arcface.cpp:233-236
        classCount = 0;
        classNames.clear();
        forgetLabels();
    }

    // src/arcface.cpp:166-187
    void forward(cv::Mat image, std::vector<struct Bbox> outputBbox) {
        const int n = (int)outputBbox.size();
        State &s = st();
        s.croppedFaces.clear();
        s.top_valid = s.from_record = false;
        s.embeds.assign((size_t)std::max(n, 1) * m_OUTPUT_D, 0.f);
        if (!n) return;
        if (forwardFromRecord(s, image, outputBbox)) return;  // a coalesced findFace() of this thread already computed everything
        std::vector<unsigned char> crops((size_t)n * m_INPUT_H * m_INPUT_W * 3);
        checkFrtStatus(frt_embedder_forward(h_, image.data, image.rows, image.cols, (size_t)image.step, reinterpret_cast<const frt_bbox *>(outputBbox.data()), n,
                                            s.embeds.data(), crops.data()));
        for (int i = 0; i < n; ++i) {
            CroppedFace c;
            c.face = cv::Mat(m_INPUT_H, m_INPUT_W, CV_8UC3, &crops[(size_t)i * m_INPUT_H * m_INPUT_W * 3]).clone();
            preprocessFace(c.face, c.faceMat);
            c.x1 = outputBbox[i].x1;
            c.y1 = outputBbox[i].y1;
            c.x2 = outputBbox[i].x2;
            c.y2 = outputBbox[i].y2;
            croppedFaces.push_back(c);
        }
    }
    // Optional alignment mode (no reference counterpart): forward() with the 5-point similarity warp instead of the bbox crop.
    void forwardAligned(cv::Mat image, std::vector<struct Bbox> outputBbox, const std::vector<std::array<float, 10>> &landmarks) {
        const int n = (int)landmarks.size();
        State &s = st();
        s.croppedFaces.clear();
        s.top_valid = s.from_record = false;
        s.embeds.assign((size_t)std::max(n, 1) * m_OUTPUT_D, 0.f);
        if (!n) return;
        std::vector<unsigned char> crops((size_t)n * m_INPUT_H * m_INPUT_W * 3);
        checkFrtStatus(frt_embedder_forward_aligned(h_, image.data, image.rows, image.cols, (size_t)image.step, landmarks[0].data(), n, s.embeds.data(),
                                                    crops.data()));
        for (int i = 0; i < n; ++i) {
            CroppedFace c;
            c.face = cv::Mat(m_INPUT_H, m_INPUT_W, CV_8UC3, &crops[(size_t)i * m_INPUT_H * m_INPUT_W * 3]).clone();
            preprocessFace(c.face, c.faceMat);
            c.x1 = c.y1 = c.x2 = c.y2 = 0;
            if ((size_t)i < outputBbox.size()) {
                c.x1 = outputBbox[(size_t)i].x1;
                c.y1 = outputBbox[(size_t)i].y1;
                c.x2 = outputBbox[(size_t)i].x2;
                c.y2 = outputBbox[(size_t)i].y2;
            }
            croppedFaces.push_back(c);
        }
    }
    // Extension: forward() for face images instead of a frame and boxes - what /recognize does for one pre-cropped face (src/app.cpp:254-267:
    // cv::resize to 112x112 when the size differs, the box 0,0,112,112, forward), for n images of any sizes (8UC3) in one call
    // (frt_embedder_embed_faces: resize + preprocessFace in one kernel, recogniser passes of maxBatchSize faces while the next images
    // upload).  Leaves what forward() leaves - embeddings and croppedFaces with the resized face - so featureMatching / getOutputs /
    // matchTop1 / matchTopIdentities follow unchanged.
    void forwardFaces(const std::vector<cv::Mat> &faces) {
        const int n = (int)faces.size();
        State &s = st();
        s.croppedFaces.clear();
        s.top_valid = s.from_record = false;
        s.embeds.assign((size_t)std::max(n, 1) * m_OUTPUT_D, 0.f);
        if (!n) return;
        const std::vector<frt_face_image> imgs = faceImages(faces);
        const size_t px = (size_t)m_INPUT_H * m_INPUT_W;
        std::vector<unsigned char> crops((size_t)n * px * 3);
        checkFrtStatus(frt_embedder_embed_faces(h_, imgs.data(), n, s.embeds.data(), crops.data()));
        for (int i = 0; i < n; ++i) {
            CroppedFace c;
            c.face = cv::Mat(m_INPUT_H, m_INPUT_W, CV_8UC3, &crops[(size_t)i * px * 3]).clone();
            // faceMat as preprocessFace() leaves it; both steps are exact in binary floating point, so this loop is the device kernel's output
            c.faceMat = cv::Mat(3 * m_INPUT_H, m_INPUT_W, CV_32FC1);
            float *t = c.faceMat.ptr<float>(0);
            const unsigned char *p = c.face.data;
            for (size_t k = 0; k < px; ++k)
                for (int ch = 0; ch < 3; ++ch) t[(size_t)ch * px + k] = ((float)p[k * 3 + (size_t)(2 - ch)] - 127.5f) * 0.0078125f;
            c.x1 = 0;
            c.y1 = 0;
            c.x2 = m_INPUT_H;  // bbox.x2 = recInputShape[1], bbox.y2 = recInputShape[2] (src/app.cpp:263-264)
            c.y2 = m_INPUT_W;
            croppedFaces.push_back(c);
        }
    }
    // src/arcface.cpp:189-201.  Throws a const char* exactly like the reference (handlers catch const char*, app.cpp:276,341).
    // The [F x N] matrix lands in a page-locked buffer (one DMA instead of a staged pageable copy: 4 MB per face at N = 1M), and the
    // row-wise first maximum is computed on the device in the same call - the same accumulators, bit for bit - so that getOutputs()
    // on THIS buffer is O(F) instead of the reference's O(F*N) host scan.  setMaterializeSimilarities(false) skips the matrix
    // altogether for callers that, like src/app.cpp:309-310, only ever hand the pointer on to getOutputs (the buffer then holds
    // stale values; default: on, the reference's contract).
    float *featureMatching() {
        State &s = st();
        if (classNames.size() > 0 && s.croppedFaces.size() > 0) {
            const size_t n = s.croppedFaces.size();
            const size_t need = std::max<size_t>(m_materialize ? n * (size_t)classCount * sizeof(float) : 0, sizeof(float));
            if (need > s.out_cap) {
                frt_pinned_free(s.out);
                s.out = nullptr;
                s.out_cap = 0;
                void *p = nullptr;
                checkFrtStatus(frt_pinned_alloc(need, matmul.device(), &p));
                s.out = static_cast<float *>(p);
                s.out_cap = need;
            }
            // coalesced request, matrix not wanted: the batch's match stage already holds this frame's first maxima
            if (s.from_record && s.top_valid && !m_materialize) return s.out;
            s.top_idx.resize(n);
            s.top_sim.resize(n);
            s.top_valid = false;
            matmul.calculateTop1(s.embeds.data(), (int)n, m_materialize ? s.out : nullptr, s.top_idx.data(), s.top_sim.data());
            s.top_valid = true;
        } else {
            throw "Feature matching: No faces in database or no faces found";
        }
        return s.out;
    }
    void setMaterializeSimilarities(bool on) { m_materialize = on; }
    // src/arcface.cpp:203-217: first maximum per row (std::max_element), no threshold here
    std::tuple<std::vector<std::string>, std::vector<float>> getOutputs(float *output_sims) {
        std::vector<std::string> names;
        std::vector<float> sims;
        State &s = st();
        float *const m_out = s.out;
        const std::vector<int> &m_top_idx = s.top_idx;
        const std::vector<float> &m_top_sim = s.top_sim;
        bool fast = output_sims == m_out && s.top_valid && m_top_idx.size() == croppedFaces.size();  // the matrix featureMatching() just produced
        // the device maxima are only a shortcut for LOCAL, in-range rows: "no row wins" (-1: a row of NaNs - std::max_element answers 0 there)
        // and indices shifted by a shard's row offset go through the host scan below (or answer row 0 when no matrix was materialised)
        for (size_t i = 0; fast && i < m_top_idx.size(); ++i)
            if (m_top_idx[i] < 0 || (size_t)m_top_idx[i] >= classNames.size() || m_top_idx[i] >= classCount) fast = false;
        if (fast) {
            for (size_t i = 0; i < croppedFaces.size(); ++i) {
                names.push_back(classNames[(size_t)m_top_idx[i]]);
                sims.push_back(m_top_sim[i]);
            }
            return std::make_tuple(names, sims);
        }
        if (output_sims == m_out && !m_materialize) {  // nothing to scan: the reference's answer for a row without a maximum is element 0
            for (size_t i = 0; i < croppedFaces.size(); ++i) {
                const int k = i < m_top_idx.size() ? m_top_idx[i] : -1;
                const bool ok = k >= 0 && (size_t)k < classNames.size();
                names.push_back(classNames[ok ? (size_t)k : 0]);
                sims.push_back(i < m_top_sim.size() ? m_top_sim[i] : 0.f);
            }
            return std::make_tuple(names, sims);
        }
        for (size_t i = 0; i < croppedFaces.size(); ++i) {
            const float *row = output_sims + i * (size_t)classCount;
            const int argmax = (int)std::distance(row, std::max_element(row, row + classCount));
            names.push_back(classNames[(size_t)argmax]);
            sims.push_back(row[argmax]);
        }
        return std::make_tuple(names, sims);
    }
    // Extension: featureMatching + getOutputs fused on the device (no F x N matrix, no host scan).
    std::tuple<std::vector<std::string>, std::vector<float>> matchTop1() {
        State &s = st();
        if (classNames.empty() || s.croppedFaces.empty()) throw "Feature matching: No faces in database or no faces found";
        const int n = (int)s.croppedFaces.size();
        std::vector<int> idx((size_t)n);
        std::vector<float> sims((size_t)n);
        if (s.from_record && s.top_valid && (int)s.top_idx.size() == n) {  // coalesced request: computed by the batch's match stage
            idx = s.top_idx;
            sims = s.top_sim;
        } else {
            matmul.top1(s.embeds.data(), n, idx.data(), sims.data());
        }
        std::vector<std::string> names;
        for (int i = 0; i < n; ++i) {
            const int k = idx[(size_t)i];  // -1: no row won (NaN similarities); the reference's max_element answers element 0
            names.push_back(classNames[(k >= 0 && (size_t)k < classNames.size()) ? (size_t)k : 0]);
        }
        return std::make_tuple(names, sims);
    }
    // Extension: the k best IDENTITIES per cropped face of the calling thread - up to k (className, similarity) pairs, best first, every
    // class at most once with the similarity of its best row (the reference's gallery holds one row per FACE of a user: USER 1-N FACE,
    // src/db.cpp:316-346, so the k best rows can be one user k times).  Entry 0 is matchTop1's answer.  classNames are interned into labels
    // in first-appearance order and handed to the matcher on first use - a process that never asks pays nothing - and enrolEmbedding(s) /
    // removeClass / initMatMul keep them in step from then on.  1 <= k <= 16; k exact scans per call, or one screened search (frt.h).
    std::vector<std::vector<std::pair<std::string, float>>> matchTopIdentities(int k) {
        State &s = st();
        if (classNames.empty() || s.croppedFaces.empty()) throw "Feature matching: No faces in database or no faces found";
        const int n = (int)s.croppedFaces.size();
        ensureLabels();
        std::vector<int> labels((size_t)n * k), idx((size_t)n * k);
        std::vector<float> sims((size_t)n * k);
        matmul.topkLabels(s.embeds.data(), n, k, labels.data(), idx.data(), sims.data());
        std::vector<std::vector<std::pair<std::string, float>>> out((size_t)n);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < k; ++j) {
                const int l = labels[(size_t)i * k + j];
                if (l >= 0 && (size_t)l < m_labelNames.size()) out[(size_t)i].push_back(std::make_pair(m_labelNames[(size_t)l], sims[(size_t)i * k + j]));
            }
        return out;
    }
    // Extension: the k best PERSONS per cropped face of the calling thread by TEMPLATE similarity - up to k (className, similarity) pairs, best
    // first.  A second matcher owned by this object holds one row per className: the re-normalised sum of that class's rows
    // (frt_matcher_build_templates), so a call scans one row per person instead of one per photo, and one poor enrolment photo moves a
    // person's score less than it moves matchTopIdentities' best-photo score.  The templates are built at the first call and again whenever
    // frt_matcher_generation of the row gallery has moved since (enrolEmbedding(s), enrolFaces, enrolImages, removeClass, initMatMul); the
    // search itself is a plain top-k on the template gallery.  1 <= k <= 16.  A process that never calls this pays nothing.
    std::vector<std::vector<std::pair<std::string, float>>> matchTemplates(int k) {
        State &s = st();
        if (classNames.empty() || s.croppedFaces.empty()) throw "Feature matching: No faces in database or no faces found";
        const int n = (int)s.croppedFaces.size();
        ensureTemplates();
        std::vector<int> idx((size_t)n * k);
        std::vector<float> sims((size_t)n * k);
        m_templates.topk(s.embeds.data(), n, k, idx.data(), sims.data());
        std::vector<std::vector<std::pair<std::string, float>>> out((size_t)n);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < k; ++j) {
                const int r = idx[(size_t)i * k + j];
                if (r >= 0 && (size_t)r < m_templateLabels.size()) out[(size_t)i].push_back(std::make_pair(labelName(m_templateLabels[(size_t)r]), sims[(size_t)i * k + j]));
            }
        return out;
    }
    // Extension: what enrolment needs to find a mislabelled or poor photo - per className, in first-appearance order, (name, rows of that
    // name, the lowest similarity of one of its rows to the name's own template, the gallery row that has it).  Builds the templates as
    // matchTemplates does.
    std::vector<std::tuple<std::string, int, float, int>> auditTemplates() {
        std::vector<std::tuple<std::string, int, float, int>> out;
        if (classNames.empty()) return out;
        ensureTemplates();
        for (size_t i = 0; i < m_templateLabels.size(); ++i)
            out.push_back(std::make_tuple(labelName(m_templateLabels[i]), m_templateRows[i], m_templateMinSim[i], m_templateMinRow[i]));
        return out;
    }
    // Extension: which gallery rows are the same PERSON, without looking at classNames (the reference allows one person under two USR_IDs:
    // /insert/face never looks at the gallery).  Single-linkage clustering on the device (frt_matcher_cluster): rows whose exact similarity is
    // >= threshold are joined, the result is one label per gallery row = the smallest row of its group.  install: the groups become the
    // matcher's labels, so matchTopIdentities, matchTemplates and auditTemplates rank and audit PERSONS from then on, each named by the
    // className of its first row, until initMatMul / resetEmbeddings / removeClass go back to classNames (a removal shifts the rows the labels
    // name, so it drops the grouping: call clusterGallery again afterwards).  A row enrolled after the install gets a NEW label named by its
    // className even when that name is already a person's: the grouping is by similarity, and only a new clusterGallery call revises it.
    std::vector<int> clusterGallery(float threshold, bool install = false) {
        std::vector<int> labels;
        matmul.cluster(threshold, labels, install);
        if (install) {
            forgetLabels();
            m_labelNames = classNames;  // a label is a row index: its name is that row's
            m_labelNames.resize(labels.size());
            m_labelsSet = m_labelsFromCluster = !labels.empty();
        }
        return labels;
    }
    // Extension: how well the gallery's persons separate, and where knownPersonThreshold / clusterGallery's threshold should sit
    // (frt_matcher_separation): per gallery row, in row order, (its className, the similarity of the best OTHER row of its person, the
    // similarity of the best row of any other person, that row's className) - -inf where there is no such row, and then an empty name.
    // Persons are classNames, or clusterGallery's groups after an install.  thresholds (at most 64): counts (may be null) becomes
    // [thresholds.size() x 2] = rows that would be "unknown" from the rest of their person (sim < t) | rows that would be accepted as somebody
    // else (sim >= t).  stats (may be null): rows with a genuine candidate, with an impostor candidate, closer to another person than to
    // their own, screened chunks, exact chunks.  Above the largest impostor similarity clusterGallery joins no two persons.
    std::vector<std::tuple<std::string, float, float, std::string>> gallerySeparation(const std::vector<float> &thresholds = std::vector<float>(),
                                                                                      std::vector<long long> *counts = nullptr, long long *stats = nullptr) {
        std::vector<std::tuple<std::string, float, float, std::string>> out;
        if (classNames.empty()) {
            if (counts) counts->assign(thresholds.size() * 2, 0);
            for (int i = 0; stats && i < 5; ++i) stats[i] = 0;
            return out;
        }
        ensureLabels();
        std::vector<float> genSim, impSim;
        std::vector<int> genRow, impRow;
        matmul.separation(genSim, genRow, impSim, impRow, thresholds, counts, stats);
        for (size_t i = 0; i < genSim.size() && i < classNames.size(); ++i) {
            const int r = impRow[i];
            out.push_back(std::make_tuple(classNames[i], genSim[i], impSim[i], (r >= 0 && (size_t)r < classNames.size()) ? classNames[(size_t)r] : std::string()));
        }
        return out;
    }
    // src/arcface.cpp:219-231: drawing only, not on the hot path (not even called by app.cpp); real OpenCV required.
    void visualize(cv::Mat &image, std::vector<std::string> names, std::vector<float> sims) {
#ifdef FRT_HAVE_OPENCV
        for (size_t i = 0; i < croppedFaces.size(); ++i) {
            const CroppedFace &c = croppedFaces[i];
            const float fontScaler = static_cast<float>(c.x2 - c.x1) / static_cast<float>(m_frameWidth);
            const cv::Scalar color = sims[i] >= m_knownPersonThresh ? cv::Scalar(0, 255, 0) : cv::Scalar(0, 0, 255);
            cv::rectangle(image, cv::Point(c.y1, c.x1), cv::Point(c.y2, c.x2), color, 2, 8, 0);
            cv::putText(image, names[i] + " " + std::to_string(sims[i]), cv::Point(c.y1 + 2, c.x2 - 3), cv::FONT_HERSHEY_DUPLEX, 0.1 + 2 * fontScaler, color, 1);
        }
#else
        (void)image;
        (void)names;
        (void)sims;
#endif
    }
    const float *embeddings() const { return st().embeds.data(); }
    frt_embedder *handle() { return h_; }
    MatMul &matcher() { return matmul; }
    bool coalescing() const {
        std::shared_ptr<frtdetail::CoalesceLink> l = link();
        return l && l->alive();
    }

  private:
    // What a call leaves behind for the next call of the same request - per calling THREAD (include/frt/coalesce.h): the reference keeps
    // it in the object and shares the object between its server's threads.
    // labels of matchTopIdentities: className <-> label, in first-appearance order; m_labelsSet: the matcher holds the labels of classNames
    // both enrolImages: quality null is frt_pipeline_enrol_images, else the gated call
    template <class Detector>
    void enrolPhotos(Detector &detector, const std::vector<std::string> &names, const std::vector<cv::Mat> &images, std::vector<int> &status,
                     const frt_quality_options *quality, FaceQuality *qualityOut, float *embeddingsOut) {
        assert(names.size() == images.size());
        if (matmul.numRows() == 0 && classNames.empty()) {
            matmul.galleryBegin(0, m_OUTPUT_D);
            matmul.galleryCommit();
        }
        photoPipe(detector);
        const std::vector<frt_face_image> imgs = faceImages(images);
        const bool labelled = m_labelsSet && matmul.numRows() > 0;
        std::vector<int> labels;
        for (size_t i = 0; labelled && i < names.size(); ++i) labels.push_back(internLabel(names[i]));
        std::vector<int32_t> st(images.size(), 0);
        int first = 0, enrolled = 0;
        if (quality)
            checkFrtStatus(frt_pipeline_enrol_images_gated(m_photoPipe, imgs.data(), (int)imgs.size(), labelled ? labels.data() : nullptr, quality, st.data(),
                                                           nullptr, qualityOut, embeddingsOut, &first, &enrolled));
        else
            checkFrtStatus(frt_pipeline_enrol_images(m_photoPipe, imgs.data(), (int)imgs.size(), labelled ? labels.data() : nullptr, st.data(), nullptr,
                                                     embeddingsOut, &first, &enrolled));
        status.assign(st.begin(), st.end());
        if (!labelled && enrolled > 0) m_labelsSet = false;
        for (size_t i = 0; i < names.size(); ++i)
            if (st[i] == FRT_ENROL_OK) classNames.push_back(names[i]);
        classCount += enrolled;
    }
    // the pipeline of enrolImages / recognizeTiled: created at the first call, again when the detector is another one
    template <class Detector>
    void photoPipe(Detector &detector) {
        if (m_photoPipe && m_photoDet != detector.handle()) {
            frt_pipeline_destroy(m_photoPipe);
            m_photoPipe = nullptr;
        }
        if (!m_photoPipe) {
            int maxBatch = 1;
            checkFrtStatus(frt_detector_geometry(detector.handle(), nullptr, nullptr, &maxBatch, nullptr, nullptr));
            checkFrtStatus(frt_pipeline_create(detector.handle(), h_, matmul.handle(), maxBatch, &m_photoPipe));
            m_photoDet = detector.handle();
        }
    }
    static std::vector<frt_face_image> faceImages(const std::vector<cv::Mat> &faces) {  // row-strided Mats (ROIs) go as they are, not copied
        std::vector<frt_face_image> imgs(faces.size());
        for (size_t i = 0; i < faces.size(); ++i) {
            imgs[i].bgr = faces[i].data;
            imgs[i].rows = faces[i].rows;
            imgs[i].cols = faces[i].cols;
            imgs[i].row_stride = (size_t)faces[i].step;
        }
        return imgs;
    }
    int internLabel(const std::string &name) {
        std::map<std::string, int>::iterator it = m_labelOf.find(name);
        if (it != m_labelOf.end()) return it->second;
        const int l = (int)m_labelNames.size();
        m_labelOf[name] = l;
        m_labelNames.push_back(name);
        return l;
    }
    void forgetLabels() {
        m_labelsSet = false;
        m_labelsFromCluster = false;
        m_labelOf.clear();
        m_labelNames.clear();
    }
    void ensureLabels() {
        if (m_labelsSet) return;
        forgetLabels();
        std::vector<int> labels;
        for (size_t i = 0; i < classNames.size(); ++i) labels.push_back(internLabel(classNames[i]));
        matmul.setLabels(labels.data(), (int)labels.size());
        m_labelsSet = true;
    }
    // the template gallery follows the row gallery: rebuilt when that one's generation has moved (the labels first - setting them moves it too)
    void ensureTemplates() {
        ensureLabels();
        if (m_templatesBuilt && m_templateGen == frt_matcher_generation(matmul.handle())) return;
        int identities = 0, maxRows = 0;
        matmul.labelsInfo(identities, maxRows);
        m_templateLabels.assign((size_t)identities, 0);
        m_templateRows.assign((size_t)identities, 0);
        m_templateMinRow.assign((size_t)identities, 0);
        m_templateMinSim.assign((size_t)identities, 0.f);
        m_templatesBuilt = false;
        matmul.buildTemplates(&m_templates, m_templateLabels.data(), m_templateRows.data(), m_templateMinSim.data(), m_templateMinRow.data());
        m_templateGen = frt_matcher_generation(matmul.handle());
        m_templatesBuilt = true;
    }
    std::string labelName(int l) const { return (l >= 0 && (size_t)l < m_labelNames.size()) ? m_labelNames[(size_t)l] : std::string(); }
    bool m_templatesBuilt = false;
    unsigned m_templateGen = 0;
    std::vector<int> m_templateLabels, m_templateRows, m_templateMinRow;  // per template row (identity), from the last build
    std::vector<float> m_templateMinSim;
    frt_pipeline *m_photoPipe = nullptr;  // enrolImages: created at its first call, for m_photoDet
    frt_detector *m_photoDet = nullptr;
    bool m_labelsSet = false;
    bool m_labelsFromCluster = false;  // the labels are clusterGallery's row indices, not interned classNames
    std::map<std::string, int> m_labelOf;
    std::vector<std::string> m_labelNames;

    struct State {
        std::vector<struct CroppedFace> croppedFaces;
        std::vector<float> embeds;
        float *out = nullptr;  // page-locked [F x N] similarity matrix (reused; the reference leaks new float[F*N] per call)
        size_t out_cap = 0;
        bool top_valid = false, from_record = false;
        std::vector<int> top_idx;
        std::vector<float> top_sim;
        ~State() { frt_pinned_free(out); }
    };
    State &st() const { return frtdetail::perThread<State>(m_id); }
    static std::vector<struct CroppedFace> &croppedFacesOf(const ArcFaceIR50 *o) { return o->st().croppedFaces; }

  public:
    // `std::vector<struct CroppedFace> croppedFaces` of the reference (src/arcface.h:37), one per calling thread
    frtdetail::PerThreadVector<struct CroppedFace, ArcFaceIR50, &ArcFaceIR50::croppedFacesOf> croppedFaces;
    // static int classCount: inherited from ArcFaceIR50Statics<> above (src/arcface.h:39, arcface.cpp:19)

  private:
    // forward() of a frame this thread's coalesced findFace() has just analysed: same frame bytes (pointer, size, sampled fingerprint),
    // same boxes, every ROI non-empty -> embeddings, crops and first maxima come from the record
    std::shared_ptr<frtdetail::CoalesceLink> link() const { return std::atomic_load(&m_link); }
    // FRT_COALESCE: the detector of an auto-linked pair was destroyed (its destructor shut the coalescer down) - wait for a new partner
    void relinkIfOrphaned() {
        if (!m_auto) return;
        std::shared_ptr<frtdetail::CoalesceLink> l = link();
        if (!l || l->alive()) return;
        std::lock_guard<std::mutex> lk(m_relink);
        l = link();
        if (!l || l->alive()) return;
        std::atomic_store(&m_link, std::shared_ptr<frtdetail::CoalesceLink>());
        try {
            frtdetail::autoLink(false, frtdetail::Pending{m_device, m_frameWidth, m_frameHeight, m_devBatch, nullptr, h_, matmul.handle(), &m_link});
        } catch (...) {  // (a partner exists but the coalescer could not be built: stay on the plain path)
        }
    }
    bool forwardFromRecord(State &s, const cv::Mat &image, const std::vector<struct Bbox> &boxes) {
        relinkIfOrphaned();
        std::shared_ptr<frtdetail::CoalesceLink> lnk = link();
        if (!lnk) return false;
        frtdetail::FrameRecord &fr = frtdetail::frameRecord();
        const size_t n = boxes.size();
        if (fr.link != lnk.get() || fr.data != image.data || fr.rows != image.rows || fr.cols != image.cols || fr.boxes.size() != n ||
            m_INPUT_H != 112 || m_INPUT_W != 112 || m_OUTPUT_D != 512)
            return false;
        for (size_t i = 0; i < n; ++i)
            if (std::memcmp(&fr.boxes[i], &boxes[i], sizeof(Bbox)) != 0 || !fr.res[i].valid) return false;
        if (fr.print != frtdetail::framePrint(image.data, image.rows, image.cols, (size_t)image.step)) return false;
        s.embeds.assign(fr.embeds.begin(), fr.embeds.begin() + (long)(n * 512));
        bool matched = true;
        s.top_idx.resize(n);
        s.top_sim.resize(n);
        for (size_t i = 0; i < n; ++i) {
            CroppedFace c;
            c.face = cv::Mat(112, 112, CV_8UC3, &fr.crops[i * 112 * 112 * 3]).clone();
            // faceMat = the recogniser's input tensor as preprocessFace() leaves it (src/arcface.cpp:105-114): planar RGB, (x - 127.5) / 128 -
            // both steps are exact in binary floating point, so this host loop IS the device kernel's output, bit for bit
            c.faceMat = cv::Mat(3 * 112, 112, CV_32FC1);
            float *t = c.faceMat.ptr<float>(0);
            const unsigned char *px = c.face.data;
            for (int k = 0; k < 112 * 112; ++k)
                for (int ch = 0; ch < 3; ++ch) t[ch * 112 * 112 + k] = ((float)px[k * 3 + (2 - ch)] - 127.5f) * 0.0078125f;
            c.x1 = boxes[i].x1;
            c.y1 = boxes[i].y1;
            c.x2 = boxes[i].x2;
            c.y2 = boxes[i].y2;
            s.croppedFaces.push_back(c);
            s.top_idx[i] = fr.res[i].match_idx;
            s.top_sim[i] = fr.res[i].match_sim;
            if (fr.res[i].match_idx < 0) matched = false;  // the batch ran without a gallery
        }
        // the batch's (row index, similarity) pairs name rows of the gallery it ran against: after addEmbedding / initKnownEmbeds / initMatMul
        // they would index a different classNames - featureMatching / getOutputs then take the device path with these embeddings
        if (!fr.galleryGen || fr.galleryGen != frt_matcher_generation(matmul.handle())) matched = false;
        s.from_record = true;
        s.top_valid = matched;
        return true;
    }
    frt_embedder *h_;
    uint64_t m_id;
    int m_frameWidth, m_frameHeight, m_INPUT_C, m_INPUT_H, m_INPUT_W, m_OUTPUT_D, m_maxBatchSize, m_maxFacesPerScene;
    float m_knownPersonThresh;
    bool m_materialize = true;
    bool m_auto = false;
    int m_device = 0, m_devBatch = 0;
    std::mutex m_relink;
    std::vector<std::string> classNames;
    MatMul matmul;
    MatMul m_templates;  // matchTemplates / auditTemplates: one row per className, created (and built) at their first use
    std::shared_ptr<frtdetail::CoalesceLink> m_link;
};

#endif  // FRT_ARCFACE_H
