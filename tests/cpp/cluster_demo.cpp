// Clustering through the drop-in shells: MatMul::cluster and ArcFaceIR50::clusterGallery on a photo dump enrolled under one name per row.
// Compiled with g++ -std=c++11 like application code.  Usage:
//   cluster_demo <rec.frtw> <gallery.bin (fp32 [n][512])> <n> <threshold (%.9g)>
// Prints
//   matmul <clusters> <edges> <screened chunks> <dense chunks>
//   labels <n labels>                     MatMul::cluster, nothing installed (the matcher stays unlabelled)
//   shell <n labels>                      ArcFaceIR50::clusterGallery(threshold, true)
//   person <name> <rows>                  one line per entry of auditTemplates() afterwards, in its order
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "frt/arcface.h"

static std::vector<char> slurp(const char *p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static void print_labels(const char *what, const std::vector<int> &labels) {
    std::printf("%s", what);
    for (size_t i = 0; i < labels.size(); ++i) std::printf(" %d", labels[i]);
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    TRTLogger gLogger;
    const int n = std::atoi(argv[3]);
    const float t = std::strtof(argv[4], nullptr);
    std::vector<char> gb = slurp(argv[2]);
    if (n < 1 || gb.size() != (size_t)n * 512 * sizeof(float)) return 2;
    float *g = reinterpret_cast<float *>(gb.data());
    {
        MatMul mm;
        mm.init(g, n, 512);
        std::vector<int> labels;
        long long stats[4] = {-1, -1, -1, -1};
        mm.cluster(t, labels, false, stats);
        int identities = -1, maxRows = -1;
        mm.labelsInfo(identities, maxRows);
        if ((int)labels.size() != n || identities != 0) return 3;  // nothing was installed
        std::printf("matmul %lld %lld %lld %lld\n", stats[0], stats[1], stats[2], stats[3]);
        print_labels("labels", labels);
        std::vector<int> again;
        mm.cluster(t, again);
        if (again != labels) return 3;
    }
    std::vector<int> recInputShape = {3, 112, 112};
    ArcFaceIR50 recognizer(gLogger, argv[1], 640, 480, "input", "output", recInputShape, 512, 1, 4, 0.65f);
    recognizer.resetEmbeddings();
    recognizer.initKnownEmbeds(n);
    for (int i = 0; i < n; ++i) recognizer.addEmbedding("u" + std::to_string(i), g + (size_t)i * 512);
    recognizer.initMatMul();
    const std::vector<int> labels = recognizer.clusterGallery(t, true);
    print_labels("shell", labels);
    const std::vector<std::tuple<std::string, int, float, int>> audit = recognizer.auditTemplates();
    for (size_t i = 0; i < audit.size(); ++i) std::printf("person %s %d\n", std::get<0>(audit[i]).c_str(), std::get<1>(audit[i]));
    return 0;
}
