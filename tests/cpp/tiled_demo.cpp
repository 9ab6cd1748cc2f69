// Large photos by tiles through the drop-in shell: RetinaFace::findFaceTiled.  Compiled with g++ -std=c++11 like application code.  Usage:
//   tiled_demo <det.frtw> <photo.bin (u8 BGR, rows * row_stride bytes)> <rows> <cols> <row_stride> <frameWidth> <frameHeight>
//              <det maxBatchSize> <maxFacesPerScene> <overlap> <overview> <metric> <drop_cut> <maxOut>
// Prints   box <x1> <y1> <x2> <y2> <score bits> <source index>   per face, best first, then the same call with the default options as
//   default <count>.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "frt/retinaface.h"

int main(int argc, char **argv) {
    if (argc != 15) return 2;
    TRTLogger gLogger;
    const int rows = std::atoi(argv[3]), cols = std::atoi(argv[4]), stride = std::atoi(argv[5]), frameW = std::atoi(argv[6]),
              frameH = std::atoi(argv[7]), maxFrames = std::atoi(argv[8]), maxFaces = std::atoi(argv[9]);
    std::ifstream f(argv[2], std::ios::binary);
    std::vector<char> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (bytes.size() != (size_t)rows * stride) return 2;
    cv::Mat photo(rows, cols, CV_8UC3, bytes.data(), (size_t)stride);
    std::vector<std::string> detOutputs = {"output_det0", "output_det1"};
    std::vector<int> detInputShape = {3, frameH, frameW};
    RetinaFace detector(gLogger, argv[1], frameW, frameH, "input_det", detOutputs, detInputShape, maxFrames, maxFaces, 0.4f, 0.02f);
    frt_tile_options opt;
    opt.overlap_rows = opt.overlap_cols = std::atoi(argv[10]);
    opt.overview = std::atoi(argv[11]);
    opt.metric = std::atoi(argv[12]);
    opt.drop_cut = std::atoi(argv[13]);
    opt.merge_threshold = -1.f;
    std::vector<int> sources;
    std::vector<struct Bbox> boxes = detector.findFaceTiled(photo, &opt, std::atoi(argv[14]), nullptr, &sources);
    if (boxes.size() != sources.size()) return 3;
    for (size_t i = 0; i < boxes.size(); ++i) {
        unsigned bits;
        std::memcpy(&bits, &boxes[i].score, 4);
        std::printf("box %d %d %d %d %u %d\n", boxes[i].x1, boxes[i].y1, boxes[i].x2, boxes[i].y2, bits, sources[i]);
    }
    std::printf("default %d\n", (int)detector.findFaceTiled(photo).size());
    return 0;
}
