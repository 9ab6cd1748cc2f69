// Faces followed across the frames of video streams through the drop-in shell: FaceTracker + ArcFaceIR50::trackFaces.  Compiled with
// g++ -std=c++11 like application code.  Usage:
//   track_demo <det.frtw> <rec.frtw> <frames.bin (u8 BGR [calls][frames][frameHeight][frameWidth][3])> <calls> <frames per call> <frameWidth>
//              <frameHeight> <maxFacesPerScene> <rec maxBatchSize> <gallery.bin (fp32 [n][512])> <n> <names.txt (n lines)> <maxTracks>
// Every call carries the next frame of each stream (frame i of a call is stream i).  Prints per call and face slot
//   track <call> <frame> <face slot> <x1> <y1> <x2> <y2> <track id> <track slot> <age> <hits> <n_embeds> <confirmed> <name> <similarity bits>
// and at the end, per stream,   stream <i> <next_id> <tick> <dropped> <live tracks>.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "frt/arcface.h"
#include "frt/retinaface.h"
#include "frt/tracker.h"

static std::vector<char> slurp(const char *p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
    if (argc != 14) return 2;
    TRTLogger gLogger;
    const int calls = std::atoi(argv[4]), perCall = std::atoi(argv[5]), frameW = std::atoi(argv[6]), frameH = std::atoi(argv[7]),
              maxFaces = std::atoi(argv[8]), recBatch = std::atoi(argv[9]), n = std::atoi(argv[11]), maxTracks = std::atoi(argv[13]);
    std::vector<char> bytes = slurp(argv[3]), gb = slurp(argv[10]);
    const size_t frameBytes = (size_t)frameH * frameW * 3;
    if (bytes.size() != (size_t)calls * perCall * frameBytes || gb.size() != (size_t)n * 512 * sizeof(float)) return 2;
    std::vector<std::string> names;
    {
        std::ifstream f(argv[12]);
        std::string line;
        while (std::getline(f, line)) names.push_back(line);
    }
    if ((int)names.size() != n) return 2;
    std::vector<std::string> detOutputs = {"output_det0", "output_det1"};
    std::vector<int> detInputShape = {3, frameH, frameW}, recInputShape = {3, 112, 112};
    RetinaFace detector(gLogger, argv[1], frameW, frameH, "input_det", detOutputs, detInputShape, perCall, maxFaces, 0.4f, 0.02f);
    ArcFaceIR50 recognizer(gLogger, argv[2], frameW, frameH, "input", "output", recInputShape, 512, recBatch, maxFaces, 0.65f);
    const float *g = reinterpret_cast<const float *>(gb.data());
    recognizer.initKnownEmbeds(n);
    for (int i = 0; i < n; ++i) recognizer.addEmbedding(names[(size_t)i], const_cast<float *>(g + (size_t)i * 512));
    recognizer.initMatMul();
    FaceTracker tracker(perCall, maxTracks, maxFaces);
    for (int c = 0; c < calls; ++c) {
        std::vector<cv::Mat> frames;
        for (int i = 0; i < perCall; ++i)
            frames.push_back(cv::Mat(frameH, frameW, CV_8UC3, bytes.data() + ((size_t)c * perCall + (size_t)i) * frameBytes, (size_t)frameW * 3));
        std::vector<frt_track_result> tracks;
        std::vector<std::string> who;
        std::vector<float> sims;
        std::vector<frt_face_result> res = recognizer.trackFaces(detector, tracker, frames, std::vector<int>(), tracks, who, &sims);
        if (res.size() != (size_t)perCall * maxFaces || tracks.size() != res.size() || who.size() != res.size() || sims.size() != res.size()) return 3;
        for (size_t k = 0; k < res.size(); ++k) {
            unsigned sbits;
            std::memcpy(&sbits, &sims[k], 4);
            const frt_track_result &t = tracks[k];
            std::printf("track %d %d %d %d %d %d %d %d %d %d %d %d %d %s %u\n", c, (int)(k / (size_t)maxFaces), (int)(k % (size_t)maxFaces), res[k].box.x1,
                        res[k].box.y1, res[k].box.x2, res[k].box.y2, t.track_id, t.slot, t.age, t.hits, t.n_embeds, t.confirmed,
                        who[k].empty() ? "-" : who[k].c_str(), sbits);
        }
    }
    for (int s = 0; s < perCall; ++s) {
        int counters[3];
        std::vector<frt_track_state> slots = tracker.tracks(s, counters);
        int live = 0;
        for (size_t i = 0; i < slots.size(); ++i) live += slots[i].live != 0;
        std::printf("stream %d %d %d %d %d\n", s, counters[0], counters[1], counters[2], live);
    }
    return 0;
}
