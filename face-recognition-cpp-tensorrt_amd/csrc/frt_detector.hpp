// struct frt_detector: the object behind frt_detector_* (include/frt.h).  Internal header of libfrt.so.
#pragma once
#include <variant>

#include "frt_internal.hpp"

struct DetLayout {
    int family = 0;  // blob kind: 1 RetinaFace mobilenet0.25, 4 Slim, 5 RFB
    int levels = 0;  // pyramid levels of the anchor table
    bool has_landmarks = false;
};
DetLayout det_layout(const frt::Blob &b);  // throws on a blob that is no detector, or a Slim / RFB blob with a missing / misshapen / extra tensor

struct frt_detector {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    // The pipeline's detector stage keeps running on the pipeline's stream after frt_pipeline_run_dev / submit returned (the
    // object mutex is only held while work is enqueued).  Object-level entry points share d_input, the activations and the
    // candidate buffers with it: they order their stream behind the end of the last such stage (one event wait).
    hipEvent_t ev_busy = nullptr;
    bool busy = false;
    void wait_idle(hipStream_t s) {
        if (busy) HIPCHK(hipStreamWaitEvent(s, ev_busy, 0));
    }
    Arena arena;
    DetGeom g{};
    int max_batch = 1;
    // One launch of the network.  An op is the argument struct of the kernel family that runs it; the kinds that run up to three problems in
    // one launch (one per pyramid level, or the parallel RFB branches) keep the count of live problems next to them.
    struct Conv3Op {      // n same-shaped 3x3 convs (launch_conv3x3_multi); n == 1: a single conv
        Conv3Args p[3];
        int n;
    };
    struct HeadsOp {      // mnet0.25 bbox / class / landmark heads of n levels
        HeadArgs p[3];
        int n;
    };
    struct SlimHeadsOp {  // Slim / RFB heads of levels 0 .. n-1 (kernels_det_slim.hip)
        SlimHeadsArgs a;
        int n;
    };
    struct RfbConvOp {    // n 3x3 convs of BasicRFB on the same map
        RfbConvMulti a;
        int n;
    };
    // DwPwArgs: a conv_dw block or a plain 1x1 conv; DenseHeadArgs: Slim / RFB head of level 3; RfbProjArgs / RfbTailArgs: BasicRFB's 1x1 convs
    using Op = std::variant<DwPwArgs, Conv3Op, HeadsOp, SlimHeadsOp, DenseHeadArgs, RfbProjArgs, RfbConvOp, RfbTailArgs>;
    // The leading ops a fused kernel may stand in for.  c: op 0 when it is a single 3x3 conv (launch_det_conv1_u8); d1, d2: ops 1 and 2 when c
    // is set and both are DwPwArgs (launch_det_stem: ops 0 - 2).  Null otherwise.  The kernels' launchers decide from the arguments whether they apply.
    struct Stem {
        Conv3Args *c = nullptr;
        DwPwArgs *d1 = nullptr, *d2 = nullptr;
    };
    Stem stem();
    int family = 1;  // blob kind: 1 mnet0.25, 4 Slim, 5 RFB
    float *d_tmp = nullptr;  // depthwise intermediate of the split conv_dw path
    float *d_wave_zeros = nullptr;  // zeros for dwpw_wave_kernel (input rows outside the image)
    std::vector<Op> ops;
    // op i at a batch of n frames: "set the batch, launch", once per kind of op.  forward() runs the network through it, and so does
    // tests/cpp/det_op_check.cpp, which launches every op alone.
    void run_op(size_t i, int n, hipStream_t s) {
        std::visit([&](auto &a) { run(a, n, s); }, ops[i]);
    }
    double flops_per_frame = 0;
    uint8_t *d_frames = nullptr;
    float *d_input = nullptr, *d_loc = nullptr, *d_conf = nullptr;
    Candidate *d_cand = nullptr;
    int *d_cand_count = nullptr, *d_nout = nullptr;
    uint8_t *d_dead = nullptr;
    frt_bbox *d_boxes = nullptr;
    // optional alignment mode: present only when the blob carries the LandmarkHead (the reference trims it away)
    bool has_landmarks = false;
    float *d_ldm = nullptr;        // raw head output [B][A][10]
    int *d_kept_anchor = nullptr;  // [B][max_faces]
    float *d_landmarks = nullptr;  // decoded, frame coordinates [B][max_faces][10]
    // large photos by tiles (frt_tiles.cpp): buffers that grow on demand, sized by the photo and its plan
    struct Tiled {
        DevBuf<uint8_t> photo;  // a frt_face_desc (launch_images_resize's, for the overview) in front of the photo's tightly packed bytes
        DevBuf<frt_tile> tiles;
        DevBuf<frt_bbox> boxes;  // [n_tiles][max_faces], tile coordinates
        DevBuf<int32_t> n_boxes;
        DevBuf<float> ldm;       // [n_tiles][max_faces][10]
        TileMergeScratch merge;
        DevBuf<float> ldm_out;   // [max_out][10]
    } tiled;

  private:
    static void run(DwPwArgs &a, int n, hipStream_t s) {
        a.B = n;
        launch_dwpw(a, s);
    }
    static void run(Conv3Op &o, int n, hipStream_t s) {
        for (int k = 0; k < o.n; ++k) o.p[k].B = n;
        launch_conv3x3_multi(o.p, o.n, s);
    }
    static void run(HeadsOp &o, int n, hipStream_t s) {
        for (int k = 0; k < o.n; ++k) o.p[k].B = n;
        launch_heads_multi(o.p, o.n, s);
    }
    static void run(SlimHeadsOp &o, int n, hipStream_t s) {
        o.a.B = n;
        launch_slim_heads(o.a, o.n, s);
    }
    static void run(DenseHeadArgs &a, int n, hipStream_t s) {
        a.B = n;
        launch_dense_head(a, s);
    }
    static void run(RfbProjArgs &a, int n, hipStream_t s) {
        a.B = n;
        launch_rfb_proj(a, s);
    }
    static void run(RfbConvOp &o, int n, hipStream_t s) {
        o.a.B = n;
        launch_rfb_conv(o.a, o.n, s);
    }
    static void run(RfbTailArgs &a, int n, hipStream_t s) {
        a.B = n;
        launch_rfb_tail(a, s);
    }

  public:
    void build(const frt::Blob &b);
    // the builders of one op's arguments: weights uploaded in every layout their kernels may use, flops_per_frame advanced
    DwPwArgs dwpw_op(const float *in, float *out, const std::vector<float> &w, const std::vector<float> &bias, const std::vector<float> &w2,
                     const std::vector<float> &bias2, int cin, int cout, int h, int w_, int oh, int ow, int stride);
    DwPwArgs pw_op(const float *in, float *out, const std::vector<float> &w2, const std::vector<float> &bias2, int cin, int cout, int h, int w_,
                   const float *add, int add_h, int add_w);
    Conv3Args conv3_op(const float *in, float *out, const std::vector<float> &w, const std::vector<float> &bias, int cin, int cout, int h, int w_,
                       int stride, int ctotal, int coff);
    void build_slim(const frt::Blob &b, bool rfb);  // kinds 4 / 5 (net_slim.py, net_rfb.py)
    void forward(int n, hipStream_t s, int first_op = 0);  // d_input -> d_loc/d_conf; ops before first_op already ran (forward_frames)
    // preprocess + forward; when the letterbox is the identity the stem kernel or the first conv reads the u8 frames and d_input is never written
    void forward_frames(const uint8_t *frames_dev, int n, size_t row_stride, size_t frame_stride, hipStream_t s);
    void postprocess(int n, hipStream_t s, frt_bbox *boxes_out = nullptr, int *nout_out = nullptr, float *landmarks_out = nullptr);  // d_loc/d_conf -> boxes (default: d_boxes/d_nout/d_landmarks)
    void preprocess(const uint8_t *frames_dev, int n, size_t row_stride, size_t frame_stride, hipStream_t s);
};

