// Live enrolment through the drop-in shell: what /insert/face and /delete/user (src/app.cpp:131-229) become when nobody has to post
// /reload.  Compiled with g++ -std=c++11 like application code.  Usage:
//   enrol_demo <rec.frtw> <face.bin (u8 BGR 112x112x3)> <gallery.bin (fp32 [n][512])> <n> <emb.bin (fp32 [512]: the embedding to enrol)>
// The gallery rows are named "u<i>".  After every step the face is matched again (forward -> featureMatching -> getOutputs, and matchTop1)
// and one line is printed:   step <k> <classCount> <name> <sim> <return value of the step>
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "frt/arcface.h"

static std::vector<char> slurp(const char *p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
    if (argc != 6) return 2;
    TRTLogger gLogger;
    const int n = std::atoi(argv[4]);
    std::vector<char> fb = slurp(argv[2]), gb = slurp(argv[3]), eb = slurp(argv[5]);
    if (fb.size() != 112 * 112 * 3 || gb.size() != (size_t)n * 512 * sizeof(float) || eb.size() != 512 * sizeof(float)) return 2;
    const float *g = reinterpret_cast<const float *>(gb.data()), *e = reinterpret_cast<const float *>(eb.data());
    std::vector<int> recInputShape = {3, 112, 112};
    ArcFaceIR50 recognizer(gLogger, argv[1], 640, 480, "input", "output", recInputShape, 512, 1, 4, 0.65f);
    cv::Mat frame(112, 112, CV_8UC3, fb.data());
    int step = 0;
    auto match = [&](int ret) -> int {
        std::vector<struct Bbox> outputBbox;
        Bbox bbox;
        bbox.x1 = 0;
        bbox.y1 = 0;
        bbox.x2 = 112;
        bbox.y2 = 112;
        bbox.score = 1;
        outputBbox.push_back(bbox);
        recognizer.forward(frame, outputBbox);
        float *output_sims = recognizer.featureMatching();
        std::vector<std::string> names, names2;
        std::vector<float> sims, sims2;
        std::tie(names, sims) = recognizer.getOutputs(output_sims);
        std::tie(names2, sims2) = recognizer.matchTop1();
        if (names.size() != 1 || names2 != names || sims2[0] != sims[0]) return 3;
        std::printf("step %d %d %s %.9g %d\n", step++, ArcFaceIR50::classCount, names[0].c_str(), sims[0], ret);
        return 0;
    };
    // 0: enrol into a recogniser that never loaded a gallery
    recognizer.enrolEmbedding("first", g);
    if (match(0)) return 3;
    // 1: the ordinary load replaces it (src/db.cpp:326-340)
    recognizer.resetEmbeddings();
    recognizer.initKnownEmbeds(n);
    for (int i = 0; i < n; ++i) recognizer.addEmbedding("u" + std::to_string(i), const_cast<float *>(g + (size_t)i * 512));
    recognizer.initMatMul();
    if (match(0)) return 3;
    // 2: /insert/face
    recognizer.enrolEmbedding("alice", e);
    if (match(0)) return 3;
    // 3: a second user with the same face: the first one keeps winning
    recognizer.enrolEmbedding("bob", std::vector<float>(e, e + 512));
    if (match(0)) return 3;
    // 4: /delete/user alice -> bob, one row further down
    int r = recognizer.removeClass("alice");
    if (match(r)) return 3;
    // 5: a user in front of them (and an unknown one: nothing happens)
    r = recognizer.removeClass("u0") + recognizer.removeClass("nobody");
    if (match(r)) return 3;
    // 6: bulk enrolment, two rows of one user
    std::vector<float> two(e, e + 512);
    two.insert(two.end(), g + 512, g + 1024);
    recognizer.enrolEmbeddings(std::vector<std::string>(2, "carol"), two.data());
    if (match(0)) return 3;
    // 7: bob and both rows of carol leave
    r = recognizer.removeClass("bob") + recognizer.removeClass("carol");
    if (match(r)) return 3;
    // the reference-named methods keep their behaviour: addEmbedding outside a load throws
    try {
        recognizer.addEmbedding("late", const_cast<float *>(e));
        return 4;
    } catch (const std::exception &) {
    } catch (const char *) {
    }
    return 0;
}
