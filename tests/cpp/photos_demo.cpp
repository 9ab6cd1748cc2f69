// Whole photos instead of frames through the drop-in shell: ArcFaceIR50::enrolImages - /insert/face without api_imgIsCropped for a ragged
// batch.  Compiled with g++ -std=c++11 like application code.  Usage:
//   photos_demo <det.frtw> <rec.frtw> <photos.bin> <gallery.bin (fp32 [n][512])> <n> <names.txt (n lines)> <enrol_names.txt>
//               <frameWidth> <frameHeight> <det maxBatchSize> <maxFacesPerScene> <embeds_out.bin>
// photos.bin: int32 count, then per image int32 rows, cols, row_stride followed by rows * row_stride bytes (u8 BGR; a stride above
// cols * 3 is a row-strided cv::Mat, passed as it is).  enrol_names.txt: one name per photo.
// Enrols all photos in ONE enrolImages call and prints   status <i> <status>   per photo,   enrolled <count> <gallery rows>   and
//   row <j> <gallery row its embedding matches best> <similarity>   for every row added; the rows added go to embeds_out.bin as raw fp32.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "frt/arcface.h"
#include "frt/retinaface.h"

static std::vector<char> slurp(const char *p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static std::vector<std::string> lines(const char *p) {
    std::vector<std::string> out;
    std::ifstream f(p);
    std::string line;
    while (std::getline(f, line)) out.push_back(line);
    return out;
}

int main(int argc, char **argv) {
    if (argc != 13) return 2;
    TRTLogger gLogger;
    const int n = std::atoi(argv[5]), frameW = std::atoi(argv[8]), frameH = std::atoi(argv[9]), maxFrames = std::atoi(argv[10]),
              maxFaces = std::atoi(argv[11]);
    std::vector<char> pb = slurp(argv[3]), gb = slurp(argv[4]);
    const std::vector<std::string> names = lines(argv[6]), enrolNames = lines(argv[7]);
    if (gb.size() != (size_t)n * 512 * sizeof(float) || (int)names.size() != n || pb.size() < 4) return 2;
    std::vector<cv::Mat> photos;
    {
        size_t at = 0;
        int32_t count = 0, hdr[3];
        std::memcpy(&count, &pb[at], 4);
        at += 4;
        for (int i = 0; i < count; ++i) {
            if (at + 12 > pb.size()) return 2;
            std::memcpy(hdr, &pb[at], 12);
            at += 12;
            if (at + (size_t)hdr[0] * hdr[2] > pb.size()) return 2;
            photos.push_back(cv::Mat(hdr[0], hdr[1], CV_8UC3, &pb[at], (size_t)hdr[2]));
            at += (size_t)hdr[0] * hdr[2];
        }
    }
    if (photos.size() != enrolNames.size() || photos.empty()) return 2;
    const float *g = reinterpret_cast<const float *>(gb.data());
    std::vector<std::string> detOutputs = {"output_det0", "output_det1"};
    std::vector<int> detInputShape = {3, frameH, frameW}, recInputShape = {3, 112, 112};
    RetinaFace detector(gLogger, argv[1], frameW, frameH, "input_det", detOutputs, detInputShape, maxFrames, maxFaces, 0.4f, 0.6f);
    ArcFaceIR50 recognizer(gLogger, argv[2], frameW, frameH, "input", "output", recInputShape, 512, maxFrames * maxFaces, maxFaces, 0.65f);
    recognizer.initKnownEmbeds(n);
    for (int i = 0; i < n; ++i) recognizer.addEmbedding(names[(size_t)i], const_cast<float *>(g + (size_t)i * 512));
    recognizer.initMatMul();
    std::vector<int> status;
    std::vector<float> enrolled(photos.size() * 512);
    recognizer.enrolImages(detector, enrolNames, photos, status, enrolled.data());
    if (status.size() != photos.size()) return 3;
    int ok = 0;
    for (size_t i = 0; i < status.size(); ++i) {
        std::printf("status %d %d\n", (int)i, status[i]);
        ok += status[i] == FRT_ENROL_OK;
    }
    if (recognizer.matcher().numRows() != n + ok || recognizer.classCount != n + ok) return 3;
    std::printf("enrolled %d %d\n", ok, recognizer.matcher().numRows());
    if (ok > 0) {  // the rows are where the call says they are
        std::vector<int32_t> idx((size_t)ok);
        std::vector<float> sim((size_t)ok);
        checkFrtStatus(frt_matcher_top1(recognizer.matcher().handle(), enrolled.data(), ok, idx.data(), sim.data()));
        for (int j = 0; j < ok; ++j) std::printf("row %d %d %.9g\n", j, (int)idx[(size_t)j], sim[(size_t)j]);
    }
    std::ofstream out(argv[12], std::ios::binary);
    out.write(reinterpret_cast<const char *>(enrolled.data()), (std::streamsize)((size_t)ok * 512 * sizeof(float)));
    // a second call with the refused photos alone: no acceptable photo, so no edit
    std::vector<cv::Mat> refused;
    std::vector<std::string> refusedNames;
    for (size_t i = 0; i < status.size(); ++i)
        if (status[i] != FRT_ENROL_OK) {
            refused.push_back(photos[i]);
            refusedNames.push_back(enrolNames[i]);
        }
    if (!refused.empty()) {
        std::vector<int> again;
        recognizer.enrolImages(detector, refusedNames, refused, again);
        for (size_t i = 0; i < again.size(); ++i)
            if (again[i] == FRT_ENROL_OK) return 3;
        if (recognizer.matcher().numRows() != n + ok || recognizer.classCount != n + ok) return 3;
    }
    return out.good() ? 0 : 3;
}
