// Host-only check of csrc/frt_faces.hpp: the chunk planner of the face-image route (frt_embedder_embed_faces / _enrol_faces).
// Every plan is checked against the rule itself - each chunk is the longest prefix of the remaining images with at most max_batch faces
// and at most cap packed bytes, an image larger than cap alone - and against the layout the prepare kernel relies on: the offsets tile
// each chunk without gaps or overlap, every image is in exactly one chunk, in order.  Prints "face chunks ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "frt_faces.hpp"

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);     \
            std::exit(1);                                          \
        }                                                          \
    } while (0)

struct Dim {
    int rows, cols;
};

static std::vector<frt_face_chunk> plan(const std::vector<Dim> &dims, int max_batch, size_t cap, std::vector<frt_face_desc> &desc) {
    desc.assign(dims.size(), frt_face_desc{0xdeadbeefu, 0, 0});
    for (size_t i = 0; i < dims.size(); ++i) {
        desc[i].rows = dims[i].rows;
        desc[i].cols = dims[i].cols;
    }
    const std::vector<frt_face_chunk> chunks = frt_plan_face_chunks(desc.data(), (int)dims.size(), max_batch, cap);
    // the rule and the layout, for any input
    int next = 0;
    for (size_t c = 0; c < chunks.size(); ++c) {
        const frt_face_chunk &k = chunks[c];
        CHECK(k.first == next && k.count >= 1 && k.count <= max_batch);  // consecutive, in order, nothing skipped or repeated
        size_t at = 0;
        for (int i = k.first; i < k.first + k.count; ++i) {
            CHECK(desc[(size_t)i].rows == dims[(size_t)i].rows && desc[(size_t)i].cols == dims[(size_t)i].cols);
            CHECK(desc[(size_t)i].offset == at);  // tiles the chunk: each image starts where the one before it ends
            at += frt_face_bytes(dims[(size_t)i].rows, dims[(size_t)i].cols);
        }
        CHECK(k.bytes == at);
        CHECK(k.bytes <= cap || k.count == 1);  // over the cap only as one image alone
        next = k.first + k.count;
        if (next < (int)dims.size() && k.count < max_batch)  // ended early: the next image did not fit
            CHECK(k.bytes + frt_face_bytes(dims[(size_t)next].rows, dims[(size_t)next].cols) > cap);
    }
    CHECK(next == (int)dims.size());
    return chunks;
}

int main() {
    std::vector<frt_face_desc> desc;
    const size_t big = FRT_FACES_STAGE_CAP, face = 112 * 112 * 3;
    CHECK(big >= ((size_t)64 << 20));
    // n = 0
    CHECK(plan(std::vector<Dim>(), 4, big, desc).empty());
    // n < max_batch, n = max_batch, n = max_batch + 1 under the real cap: full passes and one remainder, the chunking of frt_embedder_infer
    {
        std::vector<frt_face_chunk> c = plan(std::vector<Dim>(3, Dim{112, 112}), 4, big, desc);
        CHECK(c.size() == 1 && c[0].count == 3 && c[0].bytes == 3 * face);
        c = plan(std::vector<Dim>(4, Dim{112, 112}), 4, big, desc);
        CHECK(c.size() == 1 && c[0].count == 4);
        c = plan(std::vector<Dim>(5, Dim{112, 112}), 4, big, desc);
        CHECK(c.size() == 2 && c[0].count == 4 && c[1].first == 4 && c[1].count == 1 && desc[4].offset == 0);
        c = plan(std::vector<Dim>(5, Dim{112, 112}), 1, big, desc);
        CHECK(c.size() == 5);
    }
    // ragged sizes, 11 images in passes of 4: 4 + 4 + 3
    {
        const std::vector<Dim> dims = {{1, 1}, {1, 7}, {9, 1}, {56, 56}, {112, 112}, {224, 224}, {448, 448}, {113, 111}, {37, 201}, {333, 500}, {50, 61}};
        const std::vector<frt_face_chunk> c = plan(dims, 4, big, desc);
        CHECK(c.size() == 3 && c[0].count == 4 && c[1].count == 4 && c[2].count == 3);
        CHECK(desc[1].offset == 3 && desc[2].offset == 3 + 21 && desc[3].offset == 3 + 21 + 27);
    }
    // twelve 1080 x 1920 frames, passes of 16: the cap (64 MiB) ends the first chunk after ten of them
    {
        const std::vector<frt_face_chunk> c = plan(std::vector<Dim>(12, Dim{1080, 1920}), 16, big, desc);
        CHECK(c.size() == 2 && c[0].count == 10 && c[1].count == 2 && c[0].bytes == (size_t)10 * 1080 * 1920 * 3);
    }
    // a cap that ends a chunk early, exactly at the cap and one byte below it
    {
        std::vector<frt_face_chunk> c = plan(std::vector<Dim>(6, Dim{10, 10}), 4, 900, desc);  // 300 bytes each
        CHECK(c.size() == 2 && c[0].count == 3 && c[1].count == 3);
        c = plan(std::vector<Dim>(6, Dim{10, 10}), 4, 899, desc);
        CHECK(c.size() == 3 && c[0].count == 2 && c[1].count == 2 && c[2].count == 2);
    }
    // an image larger than the cap is a chunk of its own, wherever it stands
    {
        const std::vector<Dim> dims = {{10, 10}, {100, 100}, {10, 10}, {10, 10}, {100, 100}};
        const std::vector<frt_face_chunk> c = plan(dims, 8, 1000, desc);
        CHECK(c.size() == 4 && c[0].count == 1 && c[1].count == 1 && c[1].bytes == 30000 && c[2].count == 2 && c[3].count == 1);
        const std::vector<frt_face_chunk> first = plan(std::vector<Dim>{{100, 100}, {10, 10}}, 8, 1000, desc);
        CHECK(first.size() == 2 && first[0].bytes == 30000 && first[1].bytes == 300);
    }
    // sizes whose byte counts pass 2^32: 64-bit arithmetic throughout
    {
        const std::vector<Dim> dims = {{40000, 40000}, {40000, 40000}, {1, 1}};
        const std::vector<frt_face_chunk> c = plan(dims, 4, (size_t)1 << 40, desc);
        CHECK(c.size() == 1 && c[0].bytes == (size_t)2 * 40000 * 40000 * 3 + 3 && desc[2].offset == (uint64_t)2 * 40000 * 40000 * 3);
    }
    // a pseudo-random sweep: the invariants in plan() hold for every (sizes, max_batch, cap)
    {
        unsigned s = 12345;
        for (int t = 0; t < 2000; ++t) {
            std::vector<Dim> dims;
            s = s * 1664525u + 1013904223u;
            const int n = (int)((s >> 16) % 40);
            for (int i = 0; i < n; ++i) {
                s = s * 1664525u + 1013904223u;
                dims.push_back(Dim{1 + (int)((s >> 8) % 300), 1 + (int)((s >> 20) % 300)});
            }
            s = s * 1664525u + 1013904223u;
            plan(dims, 1 + (int)((s >> 16) % 9), 1 + (size_t)((s >> 4) % 400000), desc);
        }
    }
    std::printf("face chunks ok\n");
    return 0;
}
