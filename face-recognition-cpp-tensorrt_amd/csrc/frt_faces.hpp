// Face images instead of frames (frt_preprocess_faces / frt_embedder_embed_faces / _enrol_faces): where every image of a ragged batch lies
// in the packed byte arena the prepare kernel reads, and how a batch is cut into the chunks that are staged, uploaded and embedded one
// after the other.  Plain C++ (no HIP types), so the host-only test (tests/cpp/face_chunks_test.cpp) includes it as it is.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

// one face of the arena: tightly packed u8 BGR [rows][cols][3] at byte `offset` (what ragged_resize_kernel reads per grid row)
struct frt_face_desc {
    uint64_t offset;
    int32_t rows, cols;
};

// faces [first, first + count) of the batch; `bytes` = their packed size = the arena a pass over this chunk needs
struct frt_face_chunk {
    int first, count;
    size_t bytes;
};

// staging byte cap of the embedder's face route.  128 faces of 250x250 are 24 MB, so batches of ordinary face images are cut by max_batch
// alone: chunks of exactly max_batch faces and one remainder, the chunking frt_embedder_infer uses.
constexpr size_t FRT_FACES_STAGE_CAP = (size_t)64 << 20;

inline size_t frt_face_bytes(int32_t rows, int32_t cols) { return (size_t)rows * (size_t)cols * 3; }

// Cuts the n images of desc (rows / cols set by the caller, both >= 1) into consecutive chunks: each is the longest prefix of the remaining
// images with at most max_batch faces and at most cap packed bytes; an image larger than cap is a chunk of its own (the staging grows to
// fit it).  Sets every desc[i].offset to the image's byte offset inside ITS chunk.
inline std::vector<frt_face_chunk> frt_plan_face_chunks(frt_face_desc *desc, int n, int max_batch, size_t cap) {
    std::vector<frt_face_chunk> chunks;
    if (max_batch < 1) max_batch = 1;
    int i = 0;
    while (i < n) {
        frt_face_chunk c = {i, 0, 0};
        while (i < n && c.count < max_batch) {
            const size_t b = frt_face_bytes(desc[i].rows, desc[i].cols);
            if (c.count > 0 && (b > cap || c.bytes > cap - b)) break;
            desc[i].offset = c.bytes;
            c.bytes += b;
            ++c.count;
            ++i;
        }
        chunks.push_back(c);
    }
    return chunks;
}
