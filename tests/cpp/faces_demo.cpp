// Face images instead of frames through the drop-in shell: ArcFaceIR50::forwardFaces + matchTopIdentities, and enrolFaces.  Compiled with
// g++ -std=c++11 like application code.  Usage:
//   faces_demo <rec.frtw> <faces.bin> <gallery.bin (fp32 [n][512])> <n> <names.txt (n lines)> <k> <enrol_names.txt> <maxBatchSize>
// faces.bin: int32 count, then per image int32 rows, cols, row_stride followed by rows * row_stride bytes (u8 BGR; a stride above
// cols * 3 is a row-strided cv::Mat, passed as it is).  enrol_names.txt: one name per image.
// Prints, per image,   forward <i> <entries> { <name> <sim> } x entries    after forwardFaces + matchTopIdentities on the loaded gallery,
// then enrols all images under the enrol names in ONE enrolFaces call and prints the same lines with "enrol" in front.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "frt/arcface.h"

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
    if (argc != 9) return 2;
    TRTLogger gLogger;
    const int n = std::atoi(argv[4]), k = std::atoi(argv[6]), maxBatch = std::atoi(argv[8]);
    std::vector<char> fb = slurp(argv[2]), gb = slurp(argv[3]);
    const std::vector<std::string> names = lines(argv[5]), enrolNames = lines(argv[7]);
    if (gb.size() != (size_t)n * 512 * sizeof(float) || (int)names.size() != n || fb.size() < 4) return 2;
    std::vector<cv::Mat> faces;
    {
        size_t at = 0;
        int32_t count = 0, hdr[3];
        std::memcpy(&count, &fb[at], 4);
        at += 4;
        for (int i = 0; i < count; ++i) {
            if (at + 12 > fb.size()) return 2;
            std::memcpy(hdr, &fb[at], 12);
            at += 12;
            if (at + (size_t)hdr[0] * hdr[2] > fb.size()) return 2;
            faces.push_back(cv::Mat(hdr[0], hdr[1], CV_8UC3, &fb[at], (size_t)hdr[2]));
            at += (size_t)hdr[0] * hdr[2];
        }
    }
    if (faces.size() != enrolNames.size() || faces.empty()) return 2;
    const float *g = reinterpret_cast<const float *>(gb.data());
    std::vector<int> recInputShape = {3, 112, 112};
    ArcFaceIR50 recognizer(gLogger, argv[1], 640, 480, "input", "output", recInputShape, 512, maxBatch, 4, 0.65f);
    recognizer.initKnownEmbeds(n);
    for (int i = 0; i < n; ++i) recognizer.addEmbedding(names[(size_t)i], const_cast<float *>(g + (size_t)i * 512));
    recognizer.initMatMul();
    auto match = [&](const char *tag) -> int {
        recognizer.forwardFaces(faces);
        if (recognizer.croppedFaces.size() != faces.size()) return 3;
        for (size_t i = 0; i < faces.size(); ++i) {  // the state forward() leaves: the resized face, its tensor, the box /recognize builds
            const CroppedFace &c = recognizer.croppedFaces[i];
            if (c.face.rows != 112 || c.face.cols != 112 || c.faceMat.rows != 3 * 112 || c.x1 != 0 || c.y1 != 0 || c.x2 != 112 || c.y2 != 112) return 3;
            if (faces[i].rows == 112 && faces[i].cols == 112 && faces[i].isContinuous() && std::memcmp(c.face.data, faces[i].data, 112 * 112 * 3) != 0) return 3;
        }
        std::vector<std::vector<std::pair<std::string, float>>> ids = recognizer.matchTopIdentities(k);
        std::vector<std::string> top1;
        std::vector<float> sims1;
        std::tie(top1, sims1) = recognizer.matchTop1();
        if (ids.size() != faces.size()) return 3;
        for (size_t i = 0; i < ids.size(); ++i) {
            if (ids[i].empty() || (int)ids[i].size() > k || ids[i][0].first != top1[i] || ids[i][0].second != sims1[i]) return 3;
            std::printf("%s %d %d", tag, (int)i, (int)ids[i].size());
            for (size_t a = 0; a < ids[i].size(); ++a) std::printf(" %s %.9g", ids[i][a].first.c_str(), ids[i][a].second);
            std::printf("\n");
        }
        return 0;
    };
    if (match("forward")) return 3;
    std::vector<float> enrolled(faces.size() * 512);
    recognizer.enrolFaces(enrolNames, faces, enrolled.data());
    if (recognizer.matcher().numRows() != n + (int)faces.size() || recognizer.classCount != n + (int)faces.size()) return 3;
    if (std::memcmp(enrolled.data(), recognizer.embeddings(), enrolled.size() * sizeof(float)) != 0) return 3;  // same images, same passes
    if (match("enrol")) return 3;
    return 0;
}
