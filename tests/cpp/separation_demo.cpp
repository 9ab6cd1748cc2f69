// Separation through the drop-in shells: MatMul::separation on a labelled gallery and ArcFaceIR50::gallerySeparation on the same rows
// enrolled under one name per label.  Compiled with g++ -std=c++11 like application code.  Usage:
//   separation_demo <rec.frtw> <gallery.bin (fp32 [n][512])> <labels.bin (int32 [n])> <n> <threshold (%.9g)> [<threshold> ...]
// Prints
//   stats <5 values>                       MatMul::separation
//   gen_sim / imp_sim <n values, %.9g>     gen_row / imp_row <n values>
//   counts <2 values per threshold>
//   row <name> <gen_sim> <imp_sim> <name of the impostor row, - for none>     one line per row from gallerySeparation, then
//   shell_stats <5 values> and shell_counts <...>
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "frt/arcface.h"

static std::vector<char> slurp(const char *p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

template <typename T>
static void print_all(const char *what, const char *fmt, const T *v, size_t n) {
    std::printf("%s", what);
    for (size_t i = 0; i < n; ++i) {
        std::printf(" ");
        std::printf(fmt, v[i]);
    }
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 6) return 2;
    TRTLogger gLogger;
    const int n = std::atoi(argv[4]);
    std::vector<float> thr;
    for (int a = 5; a < argc; ++a) thr.push_back(std::strtof(argv[a], nullptr));
    std::vector<char> gb = slurp(argv[2]), lb = slurp(argv[3]);
    if (n < 1 || gb.size() != (size_t)n * 512 * sizeof(float) || lb.size() != (size_t)n * sizeof(int)) return 2;
    float *g = reinterpret_cast<float *>(gb.data());
    const int *labels = reinterpret_cast<const int *>(lb.data());
    {
        MatMul mm;
        mm.init(g, n, 512);
        mm.setLabels(labels, n);
        std::vector<float> genSim, impSim;
        std::vector<int> genRow, impRow;
        std::vector<long long> counts;
        long long stats[5] = {-1, -1, -1, -1, -1};
        mm.separation(genSim, genRow, impSim, impRow, thr, &counts, stats);
        if ((int)genSim.size() != n || counts.size() != thr.size() * 2) return 3;
        print_all("stats", "%lld", stats, 5);
        print_all("gen_sim", "%.9g", genSim.data(), genSim.size());
        print_all("gen_row", "%d", genRow.data(), genRow.size());
        print_all("imp_sim", "%.9g", impSim.data(), impSim.size());
        print_all("imp_row", "%d", impRow.data(), impRow.size());
        print_all("counts", "%lld", counts.data(), counts.size());
        std::vector<float> g2, i2;
        std::vector<int> gr2, ir2;
        mm.separation(g2, gr2, i2, ir2);  // the sweep and the statistics are optional
        if (gr2 != genRow || ir2 != impRow) return 3;
    }
    std::vector<int> recInputShape = {3, 112, 112};
    ArcFaceIR50 recognizer(gLogger, argv[1], 640, 480, "input", "output", recInputShape, 512, 1, 4, 0.65f);
    recognizer.resetEmbeddings();
    recognizer.initKnownEmbeds(n);
    for (int i = 0; i < n; ++i) recognizer.addEmbedding("p" + std::to_string(labels[i]), g + (size_t)i * 512);
    recognizer.initMatMul();
    std::vector<long long> counts;
    long long stats[5] = {-1, -1, -1, -1, -1};
    const std::vector<std::tuple<std::string, float, float, std::string>> rows = recognizer.gallerySeparation(thr, &counts, stats);
    for (size_t i = 0; i < rows.size(); ++i)
        std::printf("row %s %.9g %.9g %s\n", std::get<0>(rows[i]).c_str(), std::get<1>(rows[i]), std::get<2>(rows[i]),
                    std::get<3>(rows[i]).empty() ? "-" : std::get<3>(rows[i]).c_str());
    print_all("shell_stats", "%lld", stats, 5);
    print_all("shell_counts", "%lld", counts.data(), counts.size());
    return 0;
}
