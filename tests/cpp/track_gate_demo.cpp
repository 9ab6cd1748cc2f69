// Faces followed across the frames of video streams with the gate in front of the recogniser, through the drop-in shell: FaceTracker::gate
// and the ArcFaceIR50::trackFaces overload that takes frt_track_gate_options.  Compiled with g++ -std=c++11 like application code.  Usage:
//   track_gate_demo <det.frtw> <rec.frtw> <frames.bin (u8 BGR [calls][frames][frameHeight][frameWidth][3])> <calls> <frames per call>
//                   <frameWidth> <frameHeight> <maxFacesPerScene> <rec maxBatchSize> <gallery.bin (fp32 [n][512])> <n> <names.txt (n lines)>
//                   <maxTracks> <refresh> <min_embeds> <skip_iou>
// Every call carries the next frame of each stream (frame i of a call is stream i).  Prints per call and face slot
//   gate <call> <frame> <face slot> <x1> <y1> <x2> <y2> <valid> <decision> <peek slot> <overlap bits> <why> <track id> <hits> <n_embeds> <name>
// per call   embedded <call> <n_embed> <embedded by the gate alone on the same boxes AFTER the update>,
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
    if (argc != 17) return 2;
    TRTLogger gLogger;
    const int calls = std::atoi(argv[4]), perCall = std::atoi(argv[5]), frameW = std::atoi(argv[6]), frameH = std::atoi(argv[7]),
              maxFaces = std::atoi(argv[8]), recBatch = std::atoi(argv[9]), n = std::atoi(argv[11]), maxTracks = std::atoi(argv[13]);
    frt_track_gate_options options;  // no defaults: the caller says all three
    options.refresh = std::atoi(argv[14]);
    options.min_embeds = std::atoi(argv[15]);
    options.skip_iou = (float)std::atof(argv[16]);
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
        std::vector<frt_track_gate> gate;
        std::vector<std::string> who;
        int nEmbed = -1;
        std::vector<frt_face_result> res = recognizer.trackFaces(detector, tracker, options, frames, std::vector<int>(), tracks, gate, who, nullptr, &nEmbed);
        if (res.size() != (size_t)perCall * maxFaces || tracks.size() != res.size() || gate.size() != res.size() || who.size() != res.size()) return 3;
        std::vector<frt_bbox> boxes(res.size());
        for (size_t k = 0; k < res.size(); ++k) {
            unsigned obits;
            std::memcpy(&obits, &gate[k].ovr, 4);
            boxes[k] = res[k].box;
            std::printf("gate %d %d %d %d %d %d %d %d %d %d %u %d %d %d %d %s\n", c, (int)(k / (size_t)maxFaces), (int)(k % (size_t)maxFaces), res[k].box.x1,
                        res[k].box.y1, res[k].box.x2, res[k].box.y2, res[k].valid, gate[k].decision, gate[k].slot, obits, gate[k].why, tracks[k].track_id,
                        tracks[k].hits, tracks[k].n_embeds, who[k].empty() ? "-" : who[k].c_str());
        }
        // the gate alone, on the boxes the call returned and the state it left: what the NEXT call would embed if nothing moved
        std::vector<int> list, passCount;
        std::vector<frt_track_gate> again = tracker.gate(boxes, options, list, std::vector<int>(), std::vector<int>(), recBatch, &passCount);
        if (again.size() != res.size() || passCount.size() != (res.size() + (size_t)recBatch - 1) / (size_t)recBatch) return 3;
        std::printf("embedded %d %d %d\n", c, nEmbed, (int)list.size());
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
