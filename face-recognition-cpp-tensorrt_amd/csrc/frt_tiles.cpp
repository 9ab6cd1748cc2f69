// libfrt.so: large photos by tiles (include/frt.h, "Large photos by tiles") - the plan on the host, the cut and the merge behind host
// pointers, and frt_detector_find_faces_tiled, which strings them around the detector with one upload and one synchronisation.
// "Recognising a large photo by tiles": frt_select_faces (the work list of the recogniser out of the merged list, behind host pointers) and
// frt_pipeline_run_photo_tiled, which goes on from the merged list to crops, embeddings and matches on the pipeline's three objects.
// Device work: kernels_tiles.hip (cut, merge, select), kernels_image.hip (the overview's resize, crop, align); no CPU fallback.
#include "frt_pipeline.hpp"

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

// What frt_detector_find_faces_tiled and frt_pipeline_run_photo_tiled check alike once they have a detector, before any device work: the
// options with their defaults filled in, and the plan
struct TiledPlan {
    frt_tile_options o;
    std::vector<frt_tile> tiles;
};
TiledPlan plan_tiled(const frt_detector *d, int rows, int cols, const frt_tile_options *options, bool landmarks, int max_out) {
    const int T_r = d->g.frame_h, T_c = d->g.frame_w;
    TiledPlan tp;
    tp.o = options ? *options : default_options(T_r, T_c);
    check_overlap(tp.o, T_r, T_c);
    check_metric(tp.o);
    if (landmarks && !d->has_landmarks) raise(FRT_ERR_FORMAT, "findFaceTiled: the detector blob has no LandmarkHead (trimmed export)");
    if (!(tp.o.merge_threshold >= 0.f)) tp.o.merge_threshold = d->g.nms_thr;
    tp.tiles = plan(rows, cols, T_r, T_c, tp.o);
    if ((long)tp.tiles.size() * d->g.max_faces > MAX_CANDIDATES) raise(FRT_ERR_CAPACITY, "tiles: n_tiles * max_faces exceeds 16384 candidates");
    if (max_out < 1 || max_out > MAX_OUT) raise(FRT_ERR_CAPACITY, "tiles: max_out outside 1 .. 16384");
    return tp;
}

// The tiled detection of one photo, queued on s and left on the device: upload, cut + detector + post-processing per chunk of max_batch
// tiles, one merge -> a.out / a.src_out / a.n_out (and, with landmarks, d->tiled.ldm_out [max_out][10]); the photo stays in d->tiled.photo
// behind PHOTO_HDR.  The caller holds d->mu, has ordered s behind the detector's last stage (wait_idle), and keeps tp and desc alive until
// it has synchronised s: the uploads read them.
TileMergeArgs enqueue_tiled(frt_detector *d, const uint8_t *bgr, int rows, int cols, size_t row_stride, const TiledPlan &tp, frt_face_desc &desc,
                            int max_out, bool landmarks, hipStream_t s) {
    const int T_r = d->g.frame_h, T_c = d->g.frame_w, slots = d->g.max_faces;
    const int n_tiles = (int)tp.tiles.size(), M = n_tiles * slots;
    const frt_tile_options &o = tp.o;
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
    upload_photo(t.photo, desc, bgr, rows, cols, row_stride, s);
    HIPCHK(hipMemcpyAsync(t.tiles.get(), tp.tiles.data(), sizeof(frt_tile) * n_tiles, hipMemcpyHostToDevice, s));
    const size_t tight = (size_t)T_c * 3;
    for (int first = 0; first < n_tiles; first += d->max_batch) {
        const int n = std::min(d->max_batch, n_tiles - first);
        cut_chunk(t.photo.get(), rows, cols, tp.tiles, t.tiles.get(), first, n, T_r, T_c, d->d_frames, s);
        d->forward_frames(d->d_frames, n, tight, (size_t)T_r * tight, s);
        d->postprocess(n, s, t.boxes.get() + (size_t)first * slots, t.n_boxes.get() + first,
                       d->has_landmarks ? t.ldm.get() + (size_t)first * slots * 10 : nullptr);
    }
    {
        ProfScope ps(2, "tiles_merge", (double)M, s);
        launch_tile_merge(a, s);
        if (landmarks) launch_tile_landmarks(t.ldm.get(), t.tiles.get(), a.src_out, a.n_out, slots, max_out, rows, cols, T_r, T_c, t.ldm_out.get(), s);
    }
    HIPCHK(hipGetLastError());
    return a;
}

void check_select(int n, int max_batch) {
    if (n < 0 || n > MAX_OUT) raise(FRT_ERR_CAPACITY, "selectFaces: n outside 0 .. 16384");
    if (max_batch < 1) raise(FRT_ERR_INVALID, "selectFaces: max_batch < 1");
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
        check_photo(rows, cols, d->g.frame_h, d->g.frame_w);
        if (row_stride < (size_t)cols * 3) raise(FRT_ERR_INVALID, "tiles: row_stride < cols * 3");
        const TiledPlan tp = plan_tiled(d, rows, cols, options, landmarks_out != nullptr, max_out);

        std::lock_guard<std::mutex> lk(d->mu);
        use_device(d->device);
        hipStream_t s = d->stream;
        d->wait_idle(s);
        frt_face_desc desc;
        const TileMergeArgs a = enqueue_tiled(d, bgr, rows, cols, row_stride, tp, desc, max_out, landmarks_out != nullptr, s);
        HIPCHK(hipMemcpyAsync(out, a.out, sizeof(frt_bbox) * max_out, hipMemcpyDeviceToHost, s));
        if (src_out) HIPCHK(hipMemcpyAsync(src_out, a.src_out, sizeof(int32_t) * max_out, hipMemcpyDeviceToHost, s));
        if (landmarks_out) HIPCHK(hipMemcpyAsync(landmarks_out, d->tiled.ldm_out.get(), sizeof(float) * 10 * max_out, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(n_out, a.n_out, sizeof(int), hipMemcpyDeviceToHost, s));
        sync_stream_spinning(s);
    });
}

int frt_select_faces(const frt_bbox *boxes, const int32_t *src, const float *landmarks, int n, int min_face, int max_batch, frt_bbox *boxes_out,
                     int32_t *src_out, float *landmarks_out, int32_t *keep_pos_out, int32_t *pass_count_out, int *n_kept_out, int device) {
    return guarded([&] {
        check_select(n, max_batch);
        if (!n_kept_out || (n > 0 && (!boxes || !boxes_out || !keep_pos_out || !pass_count_out || (src && !src_out) || (landmarks && !landmarks_out))))
            raise(FRT_ERR_INVALID, "selectFaces: null argument");
        if (device >= 0) use_device(device);
        const size_t cap = (size_t)n, passes = (cap + (size_t)max_batch - 1) / (size_t)max_batch;
        DevBuf<frt_bbox> db, dbk;
        DevBuf<int32_t> dsrc, dsk, dpos, dpass;
        DevBuf<float> dl, dlk;
        DevBuf<int> dn;  // [0] the list's length, [1] the kept count
        db.reserve(std::max<size_t>(cap, 1));
        dbk.reserve(std::max<size_t>(cap, 1));
        dpos.reserve(std::max<size_t>(cap, 1));
        dpass.reserve(std::max<size_t>(passes, 1));
        dn.reserve(2);
        if (src) {
            dsrc.reserve(std::max<size_t>(cap, 1));
            dsk.reserve(std::max<size_t>(cap, 1));
        }
        if (landmarks) {
            dl.reserve(std::max<size_t>(cap * 10, 1));
            dlk.reserve(std::max<size_t>(cap * 10, 1));
        }
        HIPCHK(hipMemcpyAsync(dn.get(), &n, sizeof(int), hipMemcpyHostToDevice, nullptr));
        if (n > 0) {
            HIPCHK(hipMemcpyAsync(db.get(), boxes, sizeof(frt_bbox) * cap, hipMemcpyHostToDevice, nullptr));
            if (src) HIPCHK(hipMemcpyAsync(dsrc.get(), src, sizeof(int32_t) * cap, hipMemcpyHostToDevice, nullptr));
            if (landmarks) HIPCHK(hipMemcpyAsync(dl.get(), landmarks, sizeof(float) * 10 * cap, hipMemcpyHostToDevice, nullptr));
        }
        {
            ProfScope ps(2, "tile_faces_select", (double)n, nullptr);
            launch_tile_faces_select(db.get(), dsrc.get(), dl.get(), dn.get(), n, min_face, max_batch, dbk.get(), dsk.get(), dlk.get(), dpos.get(),
                                     dn.get() + 1, dpass.get(), nullptr);
        }
        HIPCHK(hipGetLastError());
        if (n > 0) {
            HIPCHK(hipMemcpyAsync(boxes_out, dbk.get(), sizeof(frt_bbox) * cap, hipMemcpyDeviceToHost, nullptr));
            HIPCHK(hipMemcpyAsync(keep_pos_out, dpos.get(), sizeof(int32_t) * cap, hipMemcpyDeviceToHost, nullptr));
            HIPCHK(hipMemcpyAsync(pass_count_out, dpass.get(), sizeof(int32_t) * passes, hipMemcpyDeviceToHost, nullptr));
            if (src) HIPCHK(hipMemcpyAsync(src_out, dsk.get(), sizeof(int32_t) * cap, hipMemcpyDeviceToHost, nullptr));
            if (landmarks) HIPCHK(hipMemcpyAsync(landmarks_out, dlk.get(), sizeof(float) * 10 * cap, hipMemcpyDeviceToHost, nullptr));
        }
        HIPCHK(hipMemcpyAsync(n_kept_out, dn.get() + 1, sizeof(int), hipMemcpyDeviceToHost, nullptr));
        HIPCHK(hipStreamSynchronize(nullptr));
    });
}

int frt_pipeline_run_photo_tiled(frt_pipeline *p, const uint8_t *bgr, int rows, int cols, size_t row_stride, const frt_tile_options *options,
                                 int min_face, int max_out, frt_face_result *results, float *landmarks_out, float *embeds_out, uint8_t *crops_out,
                                 int32_t *src_out, int *n_out) {
    return guarded([&] {
        // ---- what can be checked without the pipeline (the overlap's upper bound and the candidate count need the detector's tile)
        if (!bgr || !results || !n_out) raise(FRT_ERR_INVALID, "runPhotoTiled: null argument");
        check_photo(rows, cols, 1, 1);
        if (row_stride < (size_t)cols * 3) raise(FRT_ERR_INVALID, "tiles: row_stride < cols * 3");
        if (options) {
            if (options->overlap_rows < 0) raise(FRT_ERR_INVALID, "tiles: overlap_rows outside 0 <= overlap < tile_rows");
            if (options->overlap_cols < 0) raise(FRT_ERR_INVALID, "tiles: overlap_cols outside 0 <= overlap < tile_cols");
            check_metric(*options);
        }
        if (max_out < 1 || max_out > MAX_OUT) raise(FRT_ERR_CAPACITY, "tiles: max_out outside 1 .. 16384");
        if (!p) raise(FRT_ERR_INVALID, "runPhotoTiled: null pipeline");
        frt_detector *d = p->det;
        frt_embedder *e = p->emb;
        frt_matcher *m = p->mat;
        const TiledPlan tp = plan_tiled(d, rows, cols, options, landmarks_out != nullptr, max_out);

        // ---- images_mu -> run_mu -> detector, embedder, matcher: held to the end, the call's buffers are the objects' own
        std::lock_guard<std::mutex> li(p->images_mu);
        std::lock_guard<std::mutex> lr(p->run_mu);
        use_device(d->device);
        p->flush();  // whatever a pairing mode holds or has pending goes first (takes the object mutexes itself)
        std::lock_guard<std::mutex> ld(d->mu), le(e->mu);
        std::unique_lock<std::mutex> lm;
        if (m) lm = std::unique_lock<std::mutex>(m->mu);
        const bool align = p->align;  // (frt_pipeline_set_align refuses a detector without the LandmarkHead)
        const bool want_ldm = align || landmarks_out != nullptr;
        if (m && m->N > 0 && m->D != 512) raise(FRT_ERR_INVALID, "runPhotoTiled: the gallery does not hold 512-column rows");
        const int B = e->max_batch, passes_cap = (max_out + B - 1) / B;
        frt_pipeline::TiledFaces &t = p->tiled_faces;
        const size_t cap = (size_t)max_out;
        t.boxes.reserve(cap);
        t.src.reserve(cap);
        t.keep_pos.reserve(cap);
        t.pass_count.reserve((size_t)passes_cap);
        t.idx.reserve(cap);
        t.sim.reserve(cap);
        t.valid.reserve(cap);
        t.n_kept.reserve(1);
        t.h_n_kept.reserve(1);
        if (want_ldm) t.ldm.reserve(cap * 10);
        t.embeds.reserve(cap * 512);
        t.results.reserve(cap);

        hipStream_t s = d->stream;
        try {
            d->wait_idle(s);
            e->wait_idle(s);
            frt_face_desc desc;
            const TileMergeArgs a = enqueue_tiled(d, bgr, rows, cols, row_stride, tp, desc, max_out, want_ldm, s);
            {
                ProfScope ps(2, "tile_faces_select", (double)max_out, s);
                launch_tile_faces_select(a.out, a.src_out, want_ldm ? d->tiled.ldm_out.get() : nullptr, a.n_out, max_out, min_face, B, t.boxes.get(),
                                         t.src.get(), t.ldm.get(), t.keep_pos.get(), t.n_kept.get(), t.pass_count.get(), s);
            }
            HIPCHK(hipGetLastError());
            // the one host read in front of the recogniser: how many passes to queue
            HIPCHK(hipMemcpyAsync(t.h_n_kept.get(), t.n_kept.get(), sizeof(int), hipMemcpyDeviceToHost, s));
            sync_stream_spinning(s);
            const int kept = *t.h_n_kept.get();
            if (kept < 0 || kept > max_out) raise(FRT_ERR_DEVICE, "runPhotoTiled: the selection returned an impossible count");
            if (crops_out && kept > 0) t.crops.reserve((size_t)kept * 112 * 112 * 3);
            const uint8_t *photo = d->tiled.photo.get() + PHOTO_HDR;
            const size_t tight = (size_t)cols * 3;
            constexpr size_t CROP = (size_t)112 * 112 * 3;
            for (int f0 = 0, j = 0; f0 < kept; f0 += B, ++j) {  // passes cut as frt_embedder_forward cuts them
                const int nf = std::min(B, kept - f0);
                uint8_t *crops = crops_out ? t.crops.get() + (size_t)f0 * CROP : nullptr;
                if (align) {
                    ProfScope ps(2, "align_faces", (double)nf * CROP, s);
                    launch_align_faces(photo, rows, cols, tight, 0, t.ldm.get() + (size_t)f0 * 10, t.pass_count.get() + j, B, nf, 1, crops, e->d_in,
                                       t.valid.get() + f0, s);
                } else {
                    ProfScope ps(2, "crop_faces", (double)nf * CROP, s);
                    launch_crop_faces(photo, rows, cols, tight, 0, t.boxes.get() + f0, t.pass_count.get() + j, B, nf, 1, 112, 112, crops, e->d_in,
                                      t.valid.get() + f0, s);
                }
                e->forward(0, e->d_in, nf, t.valid.get() + f0, t.embeds.get() + (size_t)f0 * 512, s);
            }
            const bool have_gallery = m && m->N > 0 && kept > 0;
            if (have_gallery) {
                m->wait_idle(s);
                m->ensure_queries(kept);
                m->top1_dev(t.embeds.get(), kept, t.idx.get(), t.sim.get(), s);
                HIPCHK(hipEventRecord(m->ev_busy, s));
                m->busy = true;
            }
            {
                ProfScope ps(2, "pack_results", (double)max_out, s);
                launch_pack_results(t.boxes.get(), t.n_kept.get(), t.valid.get(), have_gallery ? t.idx.get() : nullptr,
                                    have_gallery ? t.sim.get() : nullptr, max_out, max_out, t.results.get(), s);
            }
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(results, t.results.get(), sizeof(frt_face_result) * cap, hipMemcpyDeviceToHost, s));
            if (src_out) HIPCHK(hipMemcpyAsync(src_out, t.src.get(), sizeof(int32_t) * cap, hipMemcpyDeviceToHost, s));
            if (landmarks_out) HIPCHK(hipMemcpyAsync(landmarks_out, t.ldm.get(), sizeof(float) * 10 * cap, hipMemcpyDeviceToHost, s));
            if (embeds_out && kept > 0) HIPCHK(hipMemcpyAsync(embeds_out, t.embeds.get(), sizeof(float) * 512 * kept, hipMemcpyDeviceToHost, s));
            if (crops_out && kept > 0) HIPCHK(hipMemcpyAsync(crops_out, t.crops.get(), (size_t)kept * CROP, hipMemcpyDeviceToHost, s));
            sync_stream_spinning(s);
            *n_out = kept;
        } catch (...) {  // leave nothing in flight that reads the caller's photo or writes the caller's arrays
            (void)hipStreamSynchronize(s);
            throw;
        }
        e->check_se_error();
    });
}

}  // extern "C"
