// struct frt_embedder: the object behind frt_embedder_* (include/frt.h).  Internal header of libfrt.so.
#pragma once
#include "frt_arc_launches.hpp"
#include "frt_internal.hpp"

struct frt_embedder {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    // end of the last pipeline recogniser pass on each activation set (see frt_detector::wait_idle)
    hipEvent_t ev_busy[2] = {nullptr, nullptr};
    bool busy[2] = {false, false};
    void wait_idle(hipStream_t s) {
        for (int i = 0; i < 2; ++i)
            if (busy[i]) HIPCHK(hipStreamWaitEvent(s, ev_busy[i], 0));
    }
    Arena arena;
    int max_batch = 1;
    bool se = false;
    frt::ArcLayout layout;     // backbone read from the blob (frt::arc_layout): IR-50 / 100 / 152, with or without SE
    float stream_scale = 1.f;  // residual-stream conditioning factor of the fp16 path (a power of two; 1 except for deep IR blobs, build())
    std::vector<ArcUnit> units;
    float *in_w, *in_s0, *in_b0, *in_slope, *in_s1, *in_b1;
    half_t *in_wh = nullptr;
    half_t *wfc;
    float *fc_bias, *bn_s, *bn_b;
    // activations.  Two sets: the pipeline runs the recogniser passes of two consecutive calls concurrently on two streams, one set each;
    // everything else uses set 0.  Set 1 is allocated on demand (288 GB of HBM: 1.2 GB more is not a concern).
    struct ActSet {
        half_t *Y[2] = {nullptr, nullptr}, *Z[2] = {nullptr, nullptr}, *T = nullptr, *SC = nullptr, *RES = nullptr;
        float *se_pool = nullptr;   // IR-SE: SE_SPLIT partial sums per (face, channel) ...
        int *se_counter = nullptr;  // ... and behind them [max_batch] arrival counters + [max_batch] gate-ready flags (zero between launches)
        float *se_gate = nullptr, *fc_partial = nullptr;  // fc_partial [FC_SPLITS][max(max_batch, 2)][512]
        float *pair = nullptr;      // flip mode: the network input of a sub-pass [max_batch][3][112][112] (set_flip)
    } act[2];
    bool has_alt = false;  // act[1] is allocated
    void alloc_act_set(ActSet &a);
    // what a unit's launches touch when its input sits at parity `cur` of the set
    ArcUnitBuffers unit_buffers(const ActSet &a, int cur) const {
        return {a.Z[cur], a.Y[cur], a.T, a.SC, a.RES, a.Y[cur ^ 1], a.Z[cur ^ 1], a.se_pool, a.se_gate, a.se_counter, max_batch, d_se_error, zeros};
    }
    void ensure_alt();
    // ---- flip-augmented embeddings (frt_embedder_set_flip; kernels_arc_flip.hip): normalize(pre(x) + pre(mirror x)).  forward() then runs
    //      sub-passes of max_batch / 2 faces: pair-up into `pair`, the unchanged network on twice the faces, pair finalize
    bool flip = false;
    void set_flip(bool on);  // allocates the pair-up scratch of every activation set that exists (never forward(): it may run inside a capture)
    // the network up to the Linear's slice sums: chw_dev [F][3][112][112] -> partial [FC_SPLITS][F][512]
    void run_network(const ActSet &A, const float *chw_dev, int F, float *partial, hipStream_t s);
    float *d_in = nullptr;  // [max_batch][3][112][112]
    float *d_out = nullptr;
    half_t *zeros = nullptr;
    int se_epoch = 0;  // launch counter of the fused SE tails (their gate-ready flags carry the launch number)
    bool se_fused = true;        // IR-SE: run the SE tail inside conv2's epilogue where the strip kernels allow it
                                 // (frt_embedder_set_se_fused(e, 0): always the stand-alone pool + gate + apply launches)
    int *h_se_error = nullptr;   // error word of the fused tail's cross-workgroup hand-over (pinned, mapped; 0 = fine)
    int *d_se_error = nullptr;   // ... its device address
    void check_se_error() {      // after a host synchronisation: a timed-out hand-over must not pass as a result
        if (h_se_error && *reinterpret_cast<volatile int *>(h_se_error) != 0) {
            *h_se_error = 0;
            raise(FRT_ERR_DEVICE, "IR-SE: the fused SE tail's cross-workgroup hand-over timed out (embeddings of that pass are invalid); "
                                  "frt_embedder_set_se_fused(e, 0) selects the stand-alone tail");
        }
    }
    uint8_t *d_crops = nullptr;
    int *d_valid = nullptr;
    frt_bbox *d_boxes = nullptr;
    float *d_lm = nullptr;  // landmark staging of forward_aligned [max_batch][10]
    DevBuf<uint8_t> d_frame;  // the caller's frame of frt_embedder_forward / _forward_aligned: grows to fit
    // ---- face images instead of frames (frt_embedder_embed_faces / _enrol_faces), allocated on first use: chunk i + 1 is packed into one
    //      pinned buffer and uploaded on `copy` into one arena while chunk i's prepare kernel and network pass run on `stream`
    struct FaceStage {
        hipStream_t copy = nullptr;
        PackPair pack[2];  // pinned: [max_batch] descriptors, then the chunk's images with the row strides removed; the same bytes on the device
        hipEvent_t uploaded[2] = {nullptr, nullptr};  // pack[b].h may be rewritten
        hipEvent_t read[2] = {nullptr, nullptr};      // pack[b].d may be rewritten: the prepare kernel that read it is done
        DevBuf<float> d_embeds;  // one enrolment call's embeddings [n][512]
    } faces;
    static constexpr int FC_SPLITS = 49;
    double flops_per_face = 0;

    // ---- fp32 end-to-end mode (frt_embedder_set_precision(e, 1); kernels_arc_f32.hip): its own weights and activation buffers, built on
    //      first use from the blob the object was created from
    typedef Arc32Weights F32Unit;  // [Cout][tap][Cin] fp32 in conv32_kernel's fragment order
    struct F32 {
        std::vector<void *> owned;   // device allocations of this mode
        std::vector<F32Unit> units;
        float *wfc = nullptr;        // [512][hw * 512 + c]
        float *A[2] = {nullptr, nullptr}, *T = nullptr, *SCb = nullptr, *RES = nullptr, *gate = nullptr, *fc_out = nullptr;  // fc_out [max(chunk, 2)][512]
        float *pair = nullptr;       // flip mode: the network input of a sub-pass [chunk][3][112][112]
        int chunk = 0;               // faces per pass of this path
        hipEvent_t done = nullptr;   // end of the last pass: one activation set, so passes on different streams run one after the other
        bool busy = false;
    } f32;
    bool fp32_mode = false;
    std::string blob_path;
    void build_f32();
    void forward_f32(const float *chw_dev, int F, const int *valid_dev, float *out_dev, hipStream_t s);

    void build(const frt::Blob &b);
    void warm_strip_tables();
    // chw_dev [F][3][112][112] -> out_dev [F][512] on activation set `set`; F <= max_batch
    void forward(int set, const float *chw_dev, int F, const int *valid_dev, float *out_dev, hipStream_t s);
};

// every argument of a face-image / photo entry point that can be checked on the host, before any device work; the images' descriptors;
// images [first, first + count) packed behind `arena` at their descriptors' offsets (frt_embedder.cpp; shared with frt_images.cpp)
void check_face_images(const frt_face_image *faces, int n, const char *what);
std::vector<frt_face_desc> face_descs(const frt_face_image *faces, int n);
void pack_face_images(const frt_face_image *faces, const frt_face_desc *desc, int first, int count, uint8_t *arena);
