// Face quality through the drop-in shell: ArcFaceIR50::faceQuality over croppedFaces after forward(), and the enrolImages overload with the
// quality gate.  Compiled with g++ -std=c++11 like application code.  Usage:
//   quality_demo <det.frtw> <rec.frtw> <frame.bin (u8 BGR [frameHeight][frameWidth][3])> <frameWidth> <frameHeight> <maxFacesPerScene>
//                <min_sharpness>
// Prints per face of the frame     face <i> <sum_y> <sum_y2> <sum_lap> <sum_lap2> <n_dark> <n_bright> <size> <sharpness bits> <flags> <passes>
// and, the frame enrolled as a photo under the gate,     enrol <status> <flags of its face> <classCount>.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "frt/arcface.h"
#include "frt/retinaface.h"

static_assert(sizeof(FaceQuality) == 56 && sizeof(QualityOptions) == sizeof(frt_quality_options), "the shells add nothing to the C records");

static std::vector<char> slurp(const char *p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
    if (argc != 8) return 2;
    TRTLogger gLogger;
    const int frameW = std::atoi(argv[4]), frameH = std::atoi(argv[5]), maxFaces = std::atoi(argv[6]);
    std::vector<char> bytes = slurp(argv[3]);
    if (bytes.size() != (size_t)frameH * frameW * 3) return 2;
    std::vector<std::string> detOutputs = {"output_det0", "output_det1"};
    std::vector<int> detInputShape = {3, frameH, frameW}, recInputShape = {3, 112, 112};
    RetinaFace detector(gLogger, argv[1], frameW, frameH, "input_det", detOutputs, detInputShape, 1, maxFaces, 0.4f, 0.02f);
    ArcFaceIR50 recognizer(gLogger, argv[2], frameW, frameH, "input", "output", recInputShape, 512, maxFaces, maxFaces, 0.65f);
    cv::Mat frame(frameH, frameW, CV_8UC3, bytes.data(), (size_t)frameW * 3);

    QualityOptions opt;
    opt.min_sharpness = (float)std::atof(argv[7]);
    std::vector<struct Bbox> boxes = detector.findFace(frame);
    recognizer.forward(frame, boxes);
    const std::vector<FaceQuality> q = recognizer.faceQuality(opt, &boxes);
    if (q.size() != boxes.size() || recognizer.faceQuality().size() != boxes.size()) return 3;
    for (size_t i = 0; i < q.size(); ++i) {
        unsigned sbits;
        std::memcpy(&sbits, &q[i].sharpness, 4);
        std::printf("face %d %u %u %d %llu %u %u %d %u %u %d\n", (int)i, q[i].sum_y, q[i].sum_y2, q[i].sum_lap, (unsigned long long)q[i].sum_lap2, q[i].n_dark,
                    q[i].n_bright, q[i].size, sbits, q[i].flags, q[i].passes() ? 1 : 0);
    }
    std::vector<int> status;
    std::vector<FaceQuality> enrolQuality;
    recognizer.enrolImages(detector, std::vector<std::string>(1, "someone"), std::vector<cv::Mat>(1, frame), status, opt, enrolQuality);
    if (status.size() != 1 || enrolQuality.size() != 1) return 3;
    std::printf("enrol %d %u %d\n", status[0], enrolQuality[0].flags, ArcFaceIR50::classCount);
    return 0;
}
