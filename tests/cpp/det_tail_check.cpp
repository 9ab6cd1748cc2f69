// Runs the launches between the detector's heads and the recogniser's input ONE AT A TIME (candidate compaction, NMS, landmark decode, the two
// face cutters, the result records), or chained, through the launchers libfrt.so exports, on buffers whose every byte the test controls.
// tests/det_tail_ref.py writes the case directory and holds the references; tests/test_gpu_det_tail.py compares.  This program knows nothing
// about expected values.
//
//   det_tail_check DIR     run DIR/ops.txt on the current device; stops at the first HIP error (exit 1)
//
// DIR/ops.txt is a list of operations, one per line, on NAMED device buffers (read by run_ops, check_common.hpp, which owns case / buf / rbuf /
// load / dump / end; this file holds the launches and their size checks).  Every buffer is allocated with kGuard bytes in front and behind;
// the guards and every byte the case does not load are filled with the pattern 0x5a (as a float about 1.5e16, as an int 1515870810).  Numbers
// are decimal; floats travel as their 32-bit pattern (decimal); "-" is a null pointer.
//   case ID                            begins a case
//   buf NAME BYTES FILE|-              a buffer the launches may write (FILE: DIR/FILE is loaded at its start; it may be shorter than BYTES)
//   rbuf NAME BYTES FILE               an input: at `end` every byte of it must still be what was loaded
//   load NAME FILE                     DIR/FILE over the start of an existing buffer (an rbuf: the whole of it), nothing else touched
//   geom FAMILY LEVELS IN_W IN_H FRAME_W FRAME_H NMS_BITS BBOX_BITS MAX_FACES   det_geometry(...): the DetGeom of the launches that follow
//   dump_geom FILE                     the DetGeom's bytes -> DIR/FILE
//   decode CONF B CAND COUNT           launch_decode
//   nms CAND LOC COUNT B DEAD OUT NOUT KEPT|-      launch_nms
//   landmarks LDM KEPT NOUT B OUT      launch_landmark_decode
//   crop FRAMES NFRAMES FH FW ROW_STRIDE FRAME_STRIDE BOXES NBOXES|- MAX_FACES F SHARED OH OW CROPS|- CHW VALID    launch_crop_faces
//   align FRAMES NFRAMES FH FW ROW_STRIDE FRAME_STRIDE LM NBOXES|- MAX_FACES F SHARED CROPS|- CHW VALID            launch_align_faces
//   pack BOXES NBOXES VALID IDX|- SIM|- MAX_FACES F OUT               launch_pack_results
//   dump NAME FILE                     the buffer's bytes (without guards) -> DIR/FILE
//   end                                "ID\t<changed guard bytes + changed rbufs>" -> DIR/results.txt; frees every buffer
// Every launch is checked against the sizes of the buffers it is given before it runs, and followed by hipDeviceSynchronize and hipGetLastError.
#define CHECK_PROGRAM "det_tail_check"
#include "check_common.hpp"
#include "frt_kernels.h"

// (csrc/frt_internal.hpp declares it among the host library's internals, which this program does not need)
void launch_pack_results(const frt_bbox *boxes, const int *n_boxes, const int *valid, const int32_t *idx, const float *sim, int max_faces, int F,
                         frt_face_result *out, hipStream_t s);

using namespace check;

constexpr size_t kCountStride = 32;  // ints between the frames' candidate counters (kernels_post.hip)

int main(int argc, char **argv) {
    DetGeom g{};
    bool have_geom = false;
    auto launch = [&](const OpLine &l) -> bool {
        const std::string &op = l.op;
        auto I = [&](size_t i) { return l.I(i); };
        auto S = [&](size_t i) -> const std::string & { return l.S(i); };
        auto need_geom = [&](long long B) {
            if (!have_geom) die(op + ": no geom");
            if (B < 1 || B > 65535) die(op + ": bad frame count");
        };
        // frames of `fh` rows of `fw` pixels, `rs` bytes from row to row and `fs` from frame to frame: the bytes the cutters may read
        auto frame_bytes = [&](long long n, long long fh, long long fw, long long rs, long long fs) -> size_t {
            if (n < 1 || fh < 1 || fw < 1 || rs < fw * 3 || fs < fh * rs) die(op + ": bad frame layout");
            return (size_t)((n - 1) * fs + (fh - 1) * rs + fw * 3);
        };
        auto slots_ok = [&](long long n, long long maxf, long long F, long long shared) {
            if (maxf < 1 || F < 1 || F > 65535) die(op + ": bad slot count");
            if (!shared && F > n * maxf) die(op + ": more face slots than the frames hold");
        };
        if (op == "geom") {
            if (I(1) < 1 || I(1) > DET_MAX_LEVELS || I(2) < 8 || I(3) < 8 || I(4) < 1 || I(5) < 1 || I(8) < 1) die("geom: bad arguments");
            g = det_geometry((int)I(0), (int)I(1), (int)I(2), (int)I(3), (int)I(4), (int)I(5), from_bits(I(6)), from_bits(I(7)), (int)I(8));
            have_geom = true;
        } else if (op == "dump_geom") {
            write_file(g_dir + "/" + S(0), &g, sizeof(g));
        } else if (op == "decode") {
            const long long B = I(1);
            need_geom(B);
            launch_decode(nullptr, ptr<float>(S(0), (size_t)B * g.A * 8), (int)B, g, ptr<Candidate>(S(2), (size_t)B * g.A * sizeof(Candidate)),
                          ptr<int>(S(3), ((size_t)(B - 1) * kCountStride + 1) * 4), nullptr);
            sync_and_check();
        } else if (op == "nms") {
            const long long B = I(3);
            need_geom(B);
            // the candidate count is read from the device's own counter: a case that injects one keeps it <= A (checked here, before the launch)
            std::vector<int> cc((size_t)(B - 1) * kCountStride + 1);
            int *d_count = ptr<int>(S(2), cc.size() * 4);
            HIPCHK(hipMemcpy(cc.data(), d_count, cc.size() * 4, hipMemcpyDeviceToHost));
            for (long long f = 0; f < B; ++f)
                if (cc[(size_t)f * kCountStride] < 0 || cc[(size_t)f * kCountStride] > g.A) die("nms: a candidate count outside [0, A]: not launched");
            launch_nms(ptr<Candidate>(S(0), (size_t)B * g.A * sizeof(Candidate)), ptr<float>(S(1), (size_t)B * g.A * 16), d_count, (int)B, g,
                       ptr<uint8_t>(S(4), (size_t)B * g.A), ptr<frt_bbox>(S(5), (size_t)B * g.max_faces * sizeof(frt_bbox)), ptr<int>(S(6), (size_t)B * 4),
                       ptr<int>(S(7), (size_t)B * g.max_faces * 4), nullptr);
            sync_and_check();
        } else if (op == "landmarks") {
            const long long B = I(3);
            need_geom(B);
            launch_landmark_decode(ptr<float>(S(0), (size_t)B * g.A * 40), ptr<int>(S(1), (size_t)B * g.max_faces * 4), ptr<int>(S(2), (size_t)B * 4), (int)B, g,
                                   ptr<float>(S(4), (size_t)B * g.max_faces * 40), nullptr);
            sync_and_check();
        } else if (op == "crop") {
            const long long n = I(1), fh = I(2), fw = I(3), rs = I(4), fs = I(5), maxf = I(8), F = I(9), shared = I(10), oh = I(11), ow = I(12);
            slots_ok(n, maxf, F, shared);
            if (oh < 1 || ow < 1) die("crop: bad output size");
            launch_crop_faces(ptr<uint8_t>(S(0), frame_bytes(n, fh, fw, rs, fs)), (int)fh, (int)fw, (size_t)rs, (size_t)fs, ptr<frt_bbox>(S(6), (size_t)F * sizeof(frt_bbox)),
                              ptr<int>(S(7), (size_t)((F + maxf - 1) / maxf) * 4), (int)maxf, (int)F, (int)shared, (int)oh, (int)ow, ptr<uint8_t>(S(13), (size_t)F * oh * ow * 3),
                              ptr<float>(S(14), (size_t)F * oh * ow * 12), ptr<int>(S(15), (size_t)F * 4), nullptr);
            sync_and_check();
        } else if (op == "align") {
            const long long n = I(1), fh = I(2), fw = I(3), rs = I(4), fs = I(5), maxf = I(8), F = I(9), shared = I(10);
            slots_ok(n, maxf, F, shared);
            launch_align_faces(ptr<uint8_t>(S(0), frame_bytes(n, fh, fw, rs, fs)), (int)fh, (int)fw, (size_t)rs, (size_t)fs, ptr<float>(S(6), (size_t)F * 40),
                               ptr<int>(S(7), (size_t)((F + maxf - 1) / maxf) * 4), (int)maxf, (int)F, (int)shared, ptr<uint8_t>(S(11), (size_t)F * 112 * 112 * 3),
                               ptr<float>(S(12), (size_t)F * 112 * 112 * 12), ptr<int>(S(13), (size_t)F * 4), nullptr);
            sync_and_check();
        } else if (op == "pack") {
            const long long maxf = I(5), F = I(6);
            if (maxf < 1 || F < 1) die("pack: bad slot count");
            launch_pack_results(ptr<frt_bbox>(S(0), (size_t)F * sizeof(frt_bbox)), ptr<int>(S(1), (size_t)((F + maxf - 1) / maxf) * 4), ptr<int>(S(2), (size_t)F * 4),
                                ptr<int32_t>(S(3), (size_t)F * 4), ptr<float>(S(4), (size_t)F * 4), (int)maxf, (int)F,
                                ptr<frt_face_result>(S(7), (size_t)F * sizeof(frt_face_result)), nullptr);
            sync_and_check();
        } else {
            return false;
        }
        return true;
    };
    return run_ops(argc, argv, launch, [] {});
}
