// libfrt.so: large photos by tiles (include/frt.h, "Large photos by tiles") - the plan on the host, the cut and the merge behind host
// pointers, and frt_detector_find_faces_tiled, which strings them around the detector with one upload and one synchronisation.
// Device work: kernels_tiles.hip (cut, merge), kernels_image.hip (the overview's resize); no CPU fallback.
#include "frt_detector.hpp"

namespace {

constexpr int MAX_TILES = 4096, MAX_CANDIDATES = 16384, MAX_OUT = 16384;
constexpr size_t PHOTO_HDR = 256;  // the overview's frt_face_desc lies in front of the photo's bytes

// origins along one axis of length L: tile T, overlap V
std::vector<int> axis_origins(int L, int T, int V) {
    if (L <= T) return {0};
    const int S = T - V, n = (L - T + S - 1) / S + 1;
    std::vector<int> o((size_t)n);
    for (int i = 0; i < n; ++i) o[(size_t)i] = std::min((long)i * S, (long)L - T);
    return o;
}
long axis_count(int L, int T, int V) { return L <= T ? 1 : ((long)L - T + (T - V) - 1) / (T - V) + 1; }

frt_tile_options default_options(int tile_rows, int tile_cols) { return frt_tile_options{tile_rows / 4, tile_cols / 4, 1, 1, 1, -1.f}; }

void check_photo(int rows, int cols, int tile_rows, int tile_cols) {
    if (rows < 1) raise(FRT_ERR_INVALID, "tiles: rows < 1");
    if (cols < 1) raise(FRT_ERR_INVALID, "tiles: cols < 1");
    if (tile_rows < 1 || tile_cols < 1) raise(FRT_ERR_INVALID, "tiles: tile size < 1");
}
void check_overlap(const frt_tile_options &o, int tile_rows, int tile_cols) {
    if (o.overlap_rows < 0 || o.overlap_rows >= tile_rows) raise(FRT_ERR_INVALID, "tiles: overlap_rows outside 0 <= overlap < tile_rows");
    if (o.overlap_cols < 0 || o.overlap_cols >= tile_cols) raise(FRT_ERR_INVALID, "tiles: overlap_cols outside 0 <= overlap < tile_cols");
}
void check_metric(const frt_tile_options &o) {
    if (o.metric != 0 && o.metric != 1) raise(FRT_ERR_INVALID, "tiles: metric must be 0 (IoU) or 1 (intersection over the smaller area)");
}

// the plan; FRT_ERR_CAPACITY past 4096 tiles (checked on the counts, before anything is built)
std::vector<frt_tile> plan(int rows, int cols, int tile_rows, int tile_cols, const frt_tile_options &o) {
    const long total = axis_count(rows, tile_rows, o.overlap_rows) * axis_count(cols, tile_cols, o.overlap_cols) + (o.overview ? 1 : 0);
    if (total > MAX_TILES) raise(FRT_ERR_CAPACITY, "tiles: more than 4096 tiles per photo");
    const std::vector<int> ro = axis_origins(rows, tile_rows, o.overlap_rows), co = axis_origins(cols, tile_cols, o.overlap_cols);
    std::vector<frt_tile> t;
    t.reserve((size_t)total);
    for (int r : ro)
        for (int c : co) t.push_back(frt_tile{r, c, std::min(tile_rows, rows - r), std::min(tile_cols, cols - c), 0});
    if (o.overview) t.push_back(frt_tile{0, 0, rows, cols, 1});
    return t;
}

// photo (host) -> dst: a frt_face_desc at byte 0, the tightly packed bytes at PHOTO_HDR.  Asynchronous on s: desc, like the photo, is read
// until the caller's synchronisation.
void upload_photo(DevBuf<uint8_t> &dst, frt_face_desc &desc, const uint8_t *bgr, int rows, int cols, size_t row_stride, hipStream_t s) {
    const size_t tight = (size_t)cols * 3;
    dst.reserve(PHOTO_HDR + (size_t)rows * tight);
    desc = frt_face_desc{0, rows, cols};
    HIPCHK(hipMemcpyAsync(dst.get(), &desc, sizeof(desc), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpy2DAsync(dst.get() + PHOTO_HDR, tight, bgr, row_stride, tight, rows, hipMemcpyHostToDevice, s));
}

// tiles [first, first + n) of the plan (tiles_dev: the whole plan) -> out [n][tile_rows][tile_cols][3]
void cut_chunk(const uint8_t *photo_buf, int rows, int cols, const std::vector<frt_tile> &tiles, const frt_tile *tiles_dev, int first, int n,
               int tile_rows, int tile_cols, uint8_t *out, hipStream_t s) {
    ProfScope ps(2, "tiles_cut", (double)n * tile_rows * tile_cols * 3, s);
    launch_cut_tiles(photo_buf + PHOTO_HDR, rows, cols, (size_t)cols * 3, tiles_dev + first, n, tile_rows, tile_cols, out, s);
    for (int i = 0; i < n; ++i)
        if (tiles[(size_t)(first + i)].kind == 1)
            launch_images_resize(photo_buf + PHOTO_HDR, reinterpret_cast<const frt_face_desc *>(photo_buf), 1, tile_rows, tile_cols,
                                 out + (size_t)i * tile_rows * tile_cols * 3, s);
}

void check_tiles(const frt_tile *tiles, int n_tiles) {
    if (n_tiles < 1) raise(FRT_ERR_INVALID, "tiles: n_tiles < 1");
    if (n_tiles > MAX_TILES) raise(FRT_ERR_CAPACITY, "tiles: more than 4096 tiles per photo");
    for (int i = 0; i < n_tiles; ++i)
        if ((tiles[i].kind != 0 && tiles[i].kind != 1) || tiles[i].row0 < 0 || tiles[i].col0 < 0)
            raise(FRT_ERR_INVALID, "tiles: tile " + std::to_string(i) + " has a kind other than 0 / 1 or a negative origin");
}

}  // namespace

extern "C" {

int frt_tile_plan(int rows, int cols, int tile_rows, int tile_cols, const frt_tile_options *options, frt_tile *tiles_out, int capacity,
                  int *n_tiles_out) {
    return guarded([&] {
        if (!options || !n_tiles_out || (!tiles_out && capacity > 0)) raise(FRT_ERR_INVALID, "null argument");
        check_photo(rows, cols, tile_rows, tile_cols);
        check_overlap(*options, tile_rows, tile_cols);
        if (capacity < 0) raise(FRT_ERR_INVALID, "tiles: capacity < 0");
        const std::vector<frt_tile> t = plan(rows, cols, tile_rows, tile_cols, *options);
        *n_tiles_out = (int)t.size();
        if ((int)t.size() > capacity) raise(FRT_ERR_CAPACITY, "tiles: the plan has more tiles than tiles_out holds");
        std::copy(t.begin(), t.end(), tiles_out);
    });
}

int frt_cut_tiles(const uint8_t *bgr, int rows, int cols, size_t row_stride, const frt_tile *tiles, int n_tiles, int tile_rows, int tile_cols,
                  uint8_t *out, int device) {
    return guarded([&] {
        if (!bgr || !tiles || !out) raise(FRT_ERR_INVALID, "null argument");
        check_photo(rows, cols, tile_rows, tile_cols);
        if (row_stride < (size_t)cols * 3) raise(FRT_ERR_INVALID, "tiles: row_stride < cols * 3");
        check_tiles(tiles, n_tiles);
        if (device >= 0) use_device(device);
        DevBuf<uint8_t> photo, frames;
        DevBuf<frt_tile> td;
        const std::vector<frt_tile> tv(tiles, tiles + n_tiles);
        const size_t bytes = (size_t)n_tiles * tile_rows * tile_cols * 3;
        frames.reserve(bytes);
        td.reserve((size_t)n_tiles);
        frt_face_desc desc;
        upload_photo(photo, desc, bgr, rows, cols, row_stride, nullptr);
        HIPCHK(hipMemcpyAsync(td.get(), tiles, sizeof(frt_tile) * n_tiles, hipMemcpyHostToDevice, nullptr));
        cut_chunk(photo.get(), rows, cols, tv, td.get(), 0, n_tiles, tile_rows, tile_cols, frames.get(), nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy(out, frames.get(), bytes, hipMemcpyDeviceToHost));
    });
}

int frt_merge_boxes(const frt_bbox *boxes, const int32_t *n_boxes, const frt_tile *tiles, int n_tiles, int slots, int photo_rows,
                    int photo_cols, int tile_rows, int tile_cols, const frt_tile_options *options, int max_out, frt_bbox *out,
                    int32_t *src_out, int *n_out, int device) {
    return guarded([&] {
        if (!boxes || !n_boxes || !tiles || !options || !out || !src_out || !n_out) raise(FRT_ERR_INVALID, "null argument");
        check_photo(photo_rows, photo_cols, tile_rows, tile_cols);
        check_metric(*options);
        if (slots < 1) raise(FRT_ERR_INVALID, "tiles: slots < 1");
        if (!(options->merge_threshold >= 0.f)) raise(FRT_ERR_INVALID, "tiles: frt_merge_boxes has no detector to take a threshold from: merge_threshold must be >= 0");
        check_tiles(tiles, n_tiles);
        if ((long)n_tiles * slots > MAX_CANDIDATES) raise(FRT_ERR_CAPACITY, "tiles: n_tiles * slots exceeds 16384 candidates");
        if (max_out < 1 || max_out > MAX_OUT) raise(FRT_ERR_CAPACITY, "tiles: max_out outside 1 .. 16384");
        if (device >= 0) use_device(device);
        const int M = n_tiles * slots;
        DevBuf<frt_bbox> db;
        DevBuf<int32_t> dn;
        DevBuf<frt_tile> dt;
        TileMergeScratch sc;
        db.reserve((size_t)M);
        dn.reserve((size_t)n_tiles);
        dt.reserve((size_t)n_tiles);
        TileMergeArgs a{db.get(), dn.get(), dt.get(), n_tiles, slots, photo_rows, photo_cols, tile_rows, tile_cols, options->metric,
                        options->drop_cut ? 1 : 0, options->merge_threshold};
        sc.bind(a, M, max_out);
        HIPCHK(hipMemcpyAsync(db.get(), boxes, sizeof(frt_bbox) * M, hipMemcpyHostToDevice, nullptr));
        HIPCHK(hipMemcpyAsync(dn.get(), n_boxes, sizeof(int32_t) * n_tiles, hipMemcpyHostToDevice, nullptr));
        HIPCHK(hipMemcpyAsync(dt.get(), tiles, sizeof(frt_tile) * n_tiles, hipMemcpyHostToDevice, nullptr));
        {
            ProfScope ps(2, "tiles_merge", (double)M, nullptr);
            launch_tile_merge(a, nullptr);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, a.out, sizeof(frt_bbox) * max_out, hipMemcpyDeviceToHost, nullptr));
        HIPCHK(hipMemcpyAsync(src_out, a.src_out, sizeof(int32_t) * max_out, hipMemcpyDeviceToHost, nullptr));
        HIPCHK(hipMemcpyAsync(n_out, a.n_out, sizeof(int), hipMemcpyDeviceToHost, nullptr));
        HIPCHK(hipStreamSynchronize(nullptr));
    });
}

int frt_detector_find_faces_tiled(frt_detector *d, const uint8_t *bgr, int rows, int cols, size_t row_stride, const frt_tile_options *options,
                                  int max_out, frt_bbox *out, float *landmarks_out, int32_t *src_out, int *n_out) {
    return guarded([&] {
        if (!d || !bgr || !out || !n_out) raise(FRT_ERR_INVALID, "null argument");
        const int T_r = d->g.frame_h, T_c = d->g.frame_w, slots = d->g.max_faces;
        check_photo(rows, cols, T_r, T_c);
        if (row_stride < (size_t)cols * 3) raise(FRT_ERR_INVALID, "tiles: row_stride < cols * 3");
        frt_tile_options o = options ? *options : default_options(T_r, T_c);
        check_overlap(o, T_r, T_c);
        check_metric(o);
        if (landmarks_out && !d->has_landmarks) raise(FRT_ERR_FORMAT, "findFaceTiled: the detector blob has no LandmarkHead (trimmed export)");
        if (!(o.merge_threshold >= 0.f)) o.merge_threshold = d->g.nms_thr;
        const std::vector<frt_tile> tiles = plan(rows, cols, T_r, T_c, o);
        const int n_tiles = (int)tiles.size();
        if ((long)n_tiles * slots > MAX_CANDIDATES) raise(FRT_ERR_CAPACITY, "tiles: n_tiles * max_faces exceeds 16384 candidates");
        if (max_out < 1 || max_out > MAX_OUT) raise(FRT_ERR_CAPACITY, "tiles: max_out outside 1 .. 16384");
        const int M = n_tiles * slots;

        std::lock_guard<std::mutex> lk(d->mu);
        use_device(d->device);
        hipStream_t s = d->stream;
        d->wait_idle(s);
        frt_detector::Tiled &t = d->tiled;
        t.tiles.reserve((size_t)n_tiles);
        t.boxes.reserve((size_t)M);
        t.n_boxes.reserve((size_t)n_tiles);
        if (d->has_landmarks) {
            t.ldm.reserve((size_t)M * 10);  // (postprocess decodes them for every chunk of a blob with the head, wanted or not)
            t.ldm_out.reserve((size_t)max_out * 10);
        }
        TileMergeArgs a{t.boxes.get(), t.n_boxes.get(), t.tiles.get(), n_tiles, slots, rows, cols, T_r, T_c, o.metric, o.drop_cut ? 1 : 0, o.merge_threshold};
        t.merge.bind(a, M, max_out);
        frt_face_desc desc;
        upload_photo(t.photo, desc, bgr, rows, cols, row_stride, s);
        HIPCHK(hipMemcpyAsync(t.tiles.get(), tiles.data(), sizeof(frt_tile) * n_tiles, hipMemcpyHostToDevice, s));
        const size_t tight = (size_t)T_c * 3;
        for (int first = 0; first < n_tiles; first += d->max_batch) {
            const int n = std::min(d->max_batch, n_tiles - first);
            cut_chunk(t.photo.get(), rows, cols, tiles, t.tiles.get(), first, n, T_r, T_c, d->d_frames, s);
            d->forward_frames(d->d_frames, n, tight, (size_t)T_r * tight, s);
            d->postprocess(n, s, t.boxes.get() + (size_t)first * slots, t.n_boxes.get() + first,
                           d->has_landmarks ? t.ldm.get() + (size_t)first * slots * 10 : nullptr);
        }
        {
            ProfScope ps(2, "tiles_merge", (double)M, s);
            launch_tile_merge(a, s);
            if (landmarks_out) launch_tile_landmarks(t.ldm.get(), t.tiles.get(), a.src_out, a.n_out, slots, max_out, rows, cols, T_r, T_c, t.ldm_out.get(), s);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, a.out, sizeof(frt_bbox) * max_out, hipMemcpyDeviceToHost, s));
        if (src_out) HIPCHK(hipMemcpyAsync(src_out, a.src_out, sizeof(int32_t) * max_out, hipMemcpyDeviceToHost, s));
        if (landmarks_out) HIPCHK(hipMemcpyAsync(landmarks_out, t.ldm_out.get(), sizeof(float) * 10 * max_out, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(n_out, a.n_out, sizeof(int), hipMemcpyDeviceToHost, s));
        sync_stream_spinning(s);
    });
}

}  // extern "C"
