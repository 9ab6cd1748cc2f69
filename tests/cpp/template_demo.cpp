// The template gallery through the drop-in shell: ArcFaceIR50::matchTemplates / auditTemplates on a gallery whose classNames repeat (several
// faces per user), and the rebuild after enrolEmbeddings / removeClass.  Compiled with g++ -std=c++11 like application code.  Usage:
//   template_demo <rec.frtw> <face.bin (u8 BGR 112x112x3)> <gallery.bin (fp32 [n][512])> <n> <names.txt (n lines)> <k> <emb.bin (fp32 [512])>
// After every step the face is matched again and the gallery audited:
//   step <s> <entries> { <name> <sim> } x entries
//   audit <s> <names> { <name> <n_rows> <min_sim> <min_row> } x names
//   0  the ordinary load (initKnownEmbeds / addEmbedding / initMatMul)
//   1  enrolEmbeddings: the embedding itself as one more row of the user of row 55, and row 7 again under the new name "zed"
//   2  removeClass of the user of row 10
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "frt/arcface.h"

static std::vector<char> slurp(const char *p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
    if (argc != 8) return 2;
    TRTLogger gLogger;
    const int n = std::atoi(argv[4]), k = std::atoi(argv[6]);
    std::vector<char> fb = slurp(argv[2]), gb = slurp(argv[3]), eb = slurp(argv[7]);
    if (fb.size() != 112 * 112 * 3 || gb.size() != (size_t)n * 512 * sizeof(float) || eb.size() != 512 * sizeof(float) || n < 56) return 2;
    std::vector<std::string> names;
    {
        std::ifstream f(argv[5]);
        std::string line;
        while (std::getline(f, line)) names.push_back(line);
    }
    if ((int)names.size() != n) return 2;
    const float *g = reinterpret_cast<const float *>(gb.data()), *e = reinterpret_cast<const float *>(eb.data());
    std::vector<int> recInputShape = {3, 112, 112};
    ArcFaceIR50 recognizer(gLogger, argv[1], 640, 480, "input", "output", recInputShape, 512, 1, 4, 0.65f);
    cv::Mat frame(112, 112, CV_8UC3, fb.data());
    int step = 0;
    auto match = [&]() -> int {
        std::vector<struct Bbox> outputBbox;
        Bbox bbox;
        bbox.x1 = 0;
        bbox.y1 = 0;
        bbox.x2 = 112;
        bbox.y2 = 112;
        bbox.score = 1;
        outputBbox.push_back(bbox);
        recognizer.forward(frame, outputBbox);
        std::vector<std::vector<std::pair<std::string, float>>> ids = recognizer.matchTemplates(k);
        // one face; no class twice; a second call without an edit in between answers the same from the templates it has
        if (ids.size() != 1 || ids[0].empty() || (int)ids[0].size() > k || recognizer.matchTemplates(k) != ids) return 3;
        for (size_t a = 0; a < ids[0].size(); ++a)
            for (size_t b = a + 1; b < ids[0].size(); ++b)
                if (ids[0][a].first == ids[0][b].first) return 3;
        // the row gallery still answers as before: the best photo's user
        std::vector<std::string> top1;
        std::vector<float> sims1;
        std::tie(top1, sims1) = recognizer.matchTop1();
        if (top1.size() != 1) return 3;
        std::printf("step %d %d", step, (int)ids[0].size());
        for (size_t a = 0; a < ids[0].size(); ++a) std::printf(" %s %.9g", ids[0][a].first.c_str(), ids[0][a].second);
        std::printf("\n");
        std::vector<std::tuple<std::string, int, float, int>> audit = recognizer.auditTemplates();
        std::printf("audit %d %d", step++, (int)audit.size());
        for (size_t a = 0; a < audit.size(); ++a)
            std::printf(" %s %d %.9g %d", std::get<0>(audit[a]).c_str(), std::get<1>(audit[a]), std::get<2>(audit[a]), std::get<3>(audit[a]));
        std::printf("\n");
        return 0;
    };
    recognizer.initKnownEmbeds(n);
    for (int i = 0; i < n; ++i) recognizer.addEmbedding(names[(size_t)i], const_cast<float *>(g + (size_t)i * 512));
    recognizer.initMatMul();
    if (match()) return 3;
    std::vector<float> two(e, e + 512);
    two.insert(two.end(), g + 7 * 512, g + 8 * 512);
    std::vector<std::string> who;
    who.push_back(names[55]);
    who.push_back("zed");
    recognizer.enrolEmbeddings(who, two.data());
    if (match()) return 3;
    if (recognizer.removeClass(names[10]) < 1) return 3;
    if (match()) return 3;
    return 0;
}
