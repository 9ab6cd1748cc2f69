// A large photo by tiles, recognised in one call, through the drop-in shell: ArcFaceIR50::recognizeTiled.  Compiled with g++ -std=c++11 like
// application code.  Usage:
//   tiled_faces_demo <det.frtw> <rec.frtw> <photo.bin (u8 BGR, rows * row_stride bytes)> <rows> <cols> <row_stride> <frameWidth> <frameHeight>
//                    <det maxBatchSize> <maxFacesPerScene> <rec maxBatchSize> <gallery.bin (fp32 [n][512])> <n> <names.txt (n lines)>
//                    <overlap> <overview> <metric> <drop_cut> <merge threshold> <minFace> <maxOut>
// Prints   face <x1> <y1> <x2> <y2> <score bits> <source index> <valid> <name> <similarity bits>   per kept face, best first, then the same
// call with the default options and no gate as   default <count>.
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

int main(int argc, char **argv) {
    if (argc != 22) return 2;
    TRTLogger gLogger;
    const int rows = std::atoi(argv[4]), cols = std::atoi(argv[5]), stride = std::atoi(argv[6]), frameW = std::atoi(argv[7]),
              frameH = std::atoi(argv[8]), maxFrames = std::atoi(argv[9]), maxFaces = std::atoi(argv[10]), recBatch = std::atoi(argv[11]),
              n = std::atoi(argv[13]);
    std::vector<char> bytes = slurp(argv[3]), gb = slurp(argv[12]);
    if (bytes.size() != (size_t)rows * stride || gb.size() != (size_t)n * 512 * sizeof(float)) return 2;
    std::vector<std::string> names;
    {
        std::ifstream f(argv[14]);
        std::string line;
        while (std::getline(f, line)) names.push_back(line);
    }
    if ((int)names.size() != n) return 2;
    cv::Mat photo(rows, cols, CV_8UC3, bytes.data(), (size_t)stride);
    std::vector<std::string> detOutputs = {"output_det0", "output_det1"};
    std::vector<int> detInputShape = {3, frameH, frameW}, recInputShape = {3, 112, 112};
    RetinaFace detector(gLogger, argv[1], frameW, frameH, "input_det", detOutputs, detInputShape, maxFrames, maxFaces, 0.4f, 0.02f);
    ArcFaceIR50 recognizer(gLogger, argv[2], frameW, frameH, "input", "output", recInputShape, 512, recBatch, maxFaces, 0.65f);
    const float *g = reinterpret_cast<const float *>(gb.data());
    recognizer.initKnownEmbeds(n);
    for (int i = 0; i < n; ++i) recognizer.addEmbedding(names[(size_t)i], const_cast<float *>(g + (size_t)i * 512));
    recognizer.initMatMul();
    frt_tile_options opt;
    opt.overlap_rows = opt.overlap_cols = std::atoi(argv[15]);
    opt.overview = std::atoi(argv[16]);
    opt.metric = std::atoi(argv[17]);
    opt.drop_cut = std::atoi(argv[18]);
    opt.merge_threshold = (float)std::atof(argv[19]);
    std::vector<std::string> who;
    std::vector<float> sims;
    std::vector<int> valid, sources;
    std::vector<struct Bbox> boxes = recognizer.recognizeTiled(detector, photo, who, sims, &opt, std::atoi(argv[20]), std::atoi(argv[21]), &valid, &sources);
    if (boxes.size() != who.size() || boxes.size() != sims.size() || boxes.size() != valid.size() || boxes.size() != sources.size()) return 3;
    for (size_t i = 0; i < boxes.size(); ++i) {
        unsigned bits, sbits;
        std::memcpy(&bits, &boxes[i].score, 4);
        std::memcpy(&sbits, &sims[i], 4);
        std::printf("face %d %d %d %d %u %d %d %s %u\n", boxes[i].x1, boxes[i].y1, boxes[i].x2, boxes[i].y2, bits, sources[i], valid[i],
                    who[i].empty() ? "-" : who[i].c_str(), sbits);
    }
    std::printf("default %d\n", (int)recognizer.recognizeTiled(detector, photo, who, sims).size());
    return 0;
}
