// struct frt_matcher: the object behind frt_matcher_* (include/frt.h).  Internal header of libfrt.so.
#pragma once
#include "frt_internal.hpp"

#include <unordered_map>

struct frt_matcher {
    unsigned generation = 0;  // bumped whenever gallery pointers / sizes / offsets change (invalidates captured graphs)
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    hipEvent_t ev_busy = nullptr;  // end of the last pipeline match stage that used this object's scratch (see wait_idle)
    bool busy = false;
    float *d_gallery = nullptr;  // fp32 rows [N][D]; null when the gallery is STORED as fp16 (store16)
    int N = 0, D = 0;
    int row_offset = 0;  // global index of local row 0 (sharded galleries)
    // scratch (grown on demand)
    float *d_q = nullptr, *d_sim = nullptr, *d_full = nullptr, *d_kth = nullptr;
    int32_t *d_idx = nullptr;
    static constexpr int KCAP = 16;  // d_sim / d_idx hold [q_cap][KCAP] (top-k lists of the host entry point)
    MatchPartial *d_partial = nullptr;
    int q_cap = 0;
    size_t full_cap = 0;
    int blocks = 0;
    // screened search (shadow gallery; see kernels_match.hip).  Off for small galleries and for widths the coarse kernel is not
    // instantiated for (anything but 64 / 128 / 256 / 512).
    half_t *d_g16 = nullptr;   // fp16 shadow of d_gallery, or the fp16-STORED gallery itself
    uint8_t *d_g8 = nullptr;   // int8 shadow of d_gallery (round 4: fp32-stored galleries with 512 columns take this instead of the fp16 shadow)
    float *d_g8_scale = nullptr;
    float gerr = 0.f;          // largest quantisation error norm of the int8 rows (part of the screening bound)
    bool store16 = false;      // current gallery is fp16-stored
    bool want16 = false;       // storage mode of the NEXT init / gallery_begin (frt_matcher_set_storage)
    float gmax_norm = 0.f;
    bool screen = false;
    bool screen_on = true;     // frt_matcher_set_screening: false = every top-1 call takes the exact fp32 scan (the shadow gallery stays resident)
    ScreenScratch scr{};
    // ---- live edits (frt_matcher_gallery_reserve / add / remove; frt_matcher.cpp).  The stored rows, the shadow and every scratch buffer
    //      sized by rows, tiles or blocks are allocated for cap_rows >= N rows, so an add inside the capacity allocates nothing.
    int cap_rows = 0;       // rows the stored buffer (d_gallery, or d_g16 when store16) holds
    int shadow_rows = 0;    // rows the shadow buffers (d_g8 + d_g8_scale, or the fp16 shadow of an fp32 gallery) hold; 0 = none.  They outlive
                            // `screen` (a gallery that fell below the threshold keeps the allocation; its contents are then stale)
    int reserve_rows = 0;   // floor of the next allocation (frt_matcher_gallery_reserve)
    int scratch_rows = 0;   // cap_rows when d_partial / the tile-sized screening scratch were allocated
    long edit_stats[4] = {};  // rows_uploaded, rows_moved, shadow_rows_rebuilt, reallocations
    int *d_edit_bits = nullptr;     // [2]: largest error norm^2 / row norm^2 of the rows an edit converted (float bit patterns)
    float *d_edit_stage = nullptr;  // fp16 storage: fp32 landing buffer of host rows in front of the conversion kernel
    size_t edit_stage_floats = 0;
    void *d_bounce = nullptr;       // BOUNCE_BYTES of the chunked compaction
    int *d_keys = nullptr;          // the hole keys of a removal (frt_holes.h)
    size_t keys_cap = 0;
    // ---- identities (frt_matcher_set_labels / gallery_add_labeled / topk_labels): one int32 label >= 0 per row, on the device for the label
    //      test of the identity passes and mirrored on the host, where the edits and the per-label row counts are kept.
    bool labelled = false;
    int32_t *d_labels = nullptr;  // [labels_cap], allocated for cap_rows like the rows: a labelled add inside the capacity allocates nothing
    int labels_cap = 0;
    std::vector<int32_t> h_labels;               // [N] while labelled
    std::unordered_map<int32_t, int> label_rows;  // label -> rows that carry it (its size = number of identities)
    int max_rows_per_label = 0;   // M of the screening bound: never below the true maximum; a remove leaves it alone (an over-estimate is only slower)
    int32_t *d_lab = nullptr;     // [q_cap][KCAP] label lists of the host entry point (allocated with d_idx / d_sim)
    static constexpr size_t BOUNCE_BYTES = (size_t)32 << 20;
    static constexpr int SCREEN_MIN_ROWS = 32768;
    // the coarse scan runs one persistent workgroup per CU and each needs a tile of its own: scr.wgmax is [FRT_MATCH_COARSE_WG][F], read in full
    static_assert(SCREEN_MIN_ROWS / 128 >= FRT_MATCH_COARSE_WG, "a screened gallery has at least one 128-row tile per coarse workgroup");
    void bind_scratch() { blocks = match_top1_blocks(N, 0); }
    void drop_labels() {  // back to an unlabelled gallery (the device allocation is kept for the next labels)
        labelled = false;
        h_labels.clear();
        label_rows.clear();
        max_rows_per_label = 0;
    }
    // d_labels holds at least `rows` labels; the first `keep` survive a move
    void ensure_label_room(int rows, int keep, hipStream_t s) {
        if (rows <= labels_cap) return;
        int32_t *nl = nullptr;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&nl), (size_t)rows * sizeof(int32_t)));
        if (keep > 0 && d_labels) {
            hipError_t e = hipMemcpyAsync(nl, d_labels, (size_t)keep * sizeof(int32_t), hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) {
                (void)hipFree(nl);
                HIPCHK(e);
            }
        }
        if (d_labels) (void)hipFree(d_labels);
        d_labels = nl;
        labels_cap = rows;
    }
    // count `n` more labels into label_rows / max_rows_per_label
    void count_labels(const int32_t *l, int n) {
        for (int i = 0; i < n; ++i) max_rows_per_label = std::max(max_rows_per_label, ++label_rows[l[i]]);
    }
    void free_screen_scratch() {
        for (void *p : {(void *)scr.tilemax, (void *)scr.wgmax, scr.pairs, (void *)scr.ctl, (void *)scr.qkey})
            if (p) (void)hipFree(p);
        scr = ScreenScratch{};
    }
    // the rows the exact kernels read, typed: fn(const float *) for an fp32-stored gallery, fn(const half_t *) for an fp16-stored one
    template <typename Fn>
    void with_rows(Fn &&fn) const {
        if (store16) fn(static_cast<const half_t *>(d_g16));
        else fn(static_cast<const float *>(d_gallery));
    }
    ScreenScratch screen_scratch() const {  // scr + the shadow the coarse scan reads
        ScreenScratch w = scr;
        w.g8 = d_g8;
        w.g8_scale = d_g8_scale;
        w.gerr = gerr;
        return w;
    }
    // Object-level entry points share the scratch buffers with the pipeline's match stage, which keeps running on the pipeline's
    // stream after frt_pipeline_run_dev / submit returned: order this object's stream behind it (one event wait, no host sync).
    void wait_idle(hipStream_t s) {
        if (busy) HIPCHK(hipStreamWaitEvent(s, ev_busy, 0));
    }

    // ---- streaming gallery load (frt_matcher_gallery_begin / append / commit == initKnownEmbeds / addEmbedding / initMatMul,
    //      src/db.cpp:316-346): rows are copied into pinned staging chunks as they arrive (the caller's pointer may be SQLite's
    //      blob buffer) and every full chunk goes to the device with an asynchronous copy while the next one fills.  The previous
    //      gallery stays live (and searchable) until commit swaps the pointers.
    struct Load {
        static constexpr int NCH = 3;
        static constexpr int CH_ROWS = 4096;   // x 512 floats = 8 MB per chunk
        bool active = false;
        bool f16 = false;
        int cap = 0, D = 0, rows = 0, fill = 0, cur = 0;
        int alloc = 0;  // rows allocated: cap, or the matcher's reserve_rows when that is more
        float *d_new32 = nullptr;
        half_t *d_new16 = nullptr;
        float *h_stage[NCH] = {};
        float *d_stage[NCH] = {};   // fp16 storage only: fp32 landing buffers in front of the conversion kernel
        hipEvent_t ev[NCH] = {};
        bool pending[NCH] = {};
        size_t stage_floats = 0;
        hipStream_t s = nullptr;
    } ld;
    void load_release_staging() {
        for (int i = 0; i < Load::NCH; ++i) {
            if (ld.h_stage[i]) (void)hipHostFree(ld.h_stage[i]);
            if (ld.d_stage[i]) (void)hipFree(ld.d_stage[i]);
            if (ld.ev[i]) (void)hipEventDestroy(ld.ev[i]);
            ld.h_stage[i] = ld.d_stage[i] = nullptr;
            ld.ev[i] = nullptr;
            ld.pending[i] = false;
        }
        ld.stage_floats = 0;
    }
    void load_abort() {
        if (ld.s) (void)hipStreamSynchronize(ld.s);
        if (ld.d_new32) (void)hipFree(ld.d_new32);
        if (ld.d_new16) (void)hipFree(ld.d_new16);
        ld.d_new32 = nullptr;
        ld.d_new16 = nullptr;
        ld.active = false;
    }
    void load_begin(int cap, int cols) {
        if (ld.active) load_abort();
        // The load runs on the matcher's own stream.  NOT on a stream of its own: one more hipStreamCreateWithFlags(hipStreamNonBlocking)
        // stream in the process before the pipeline's stage streams exist changes how ROCm maps those onto hardware queues, and the
        // stages of consecutive calls stop overlapping (measured: batch-1 step 0.56 -> 1.39 ms, batch-32 step +10 %).
        ld.s = stream;
        const size_t need = (size_t)Load::CH_ROWS * cols;
        if (ld.stage_floats != need) {
            load_release_staging();
            for (int i = 0; i < Load::NCH; ++i) {
                HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&ld.h_stage[i]), need * sizeof(float), hipHostMallocDefault));
                HIPCHK(hipEventCreateWithFlags(&ld.ev[i], hipEventDisableTiming));
            }
            ld.stage_floats = need;
        }
        ld.f16 = want16;
        ld.cap = cap;
        ld.D = cols;
        ld.rows = ld.fill = ld.cur = 0;
        ld.alloc = cap > 0 ? std::max(cap, reserve_rows) : 0;
        if (cap > 0) {
            if (ld.f16) {
                HIPCHK(hipMalloc(reinterpret_cast<void **>(&ld.d_new16), gallery16_elems(ld.alloc, cols) * sizeof(half_t)));
                HIPCHK(hipMemsetAsync(ld.d_new16, 0, gallery16_elems(ld.alloc, cols) * sizeof(half_t), ld.s));  // fragment order, zero pad rows
                for (int i = 0; i < Load::NCH; ++i)
                    if (!ld.d_stage[i]) HIPCHK(hipMalloc(reinterpret_cast<void **>(&ld.d_stage[i]), need * sizeof(float)));
            } else {
                HIPCHK(hipMalloc(reinterpret_cast<void **>(&ld.d_new32), (size_t)ld.alloc * cols * sizeof(float)));
            }
        }
        ld.active = true;
    }
    void load_flush() {  // current chunk -> device
        if (!ld.fill) return;
        const int c = ld.cur;
        const size_t off = (size_t)(ld.rows - ld.fill) * ld.D, n = (size_t)ld.fill * ld.D;
        if (ld.f16) {
            HIPCHK(hipMemcpyAsync(ld.d_stage[c], ld.h_stage[c], n * sizeof(float), hipMemcpyHostToDevice, ld.s));
            launch_rows_to_half(ld.d_stage[c], (long)(ld.rows - ld.fill), (long)ld.fill, ld.D, ld.d_new16, ld.s);  // (chunks start on 128-row tiles)
        } else {
            HIPCHK(hipMemcpyAsync(ld.d_new32 + off, ld.h_stage[c], n * sizeof(float), hipMemcpyHostToDevice, ld.s));
        }
        HIPCHK(hipEventRecord(ld.ev[c], ld.s));
        ld.pending[c] = true;
        ld.cur = (c + 1) % Load::NCH;
        ld.fill = 0;
        if (ld.pending[ld.cur]) {  // the chunk about to be refilled must have left the host (and its landing buffer)
            HIPCHK(hipEventSynchronize(ld.ev[ld.cur]));
            ld.pending[ld.cur] = false;
        }
    }
    void load_append(const float *rows, int n) {
        if (!ld.active) raise(FRT_ERR_INVALID, "gallery_append: no load in progress (call frt_matcher_gallery_begin first)");
        if (n < 0 || (n > 0 && !rows)) raise(FRT_ERR_INVALID, "gallery_append: bad argument");
        if ((long)ld.rows + n > ld.cap) raise(FRT_ERR_CAPACITY, "gallery_append: more rows than gallery_begin reserved (initKnownEmbeds)");
        while (n > 0) {
            const int take = std::min(n, Load::CH_ROWS - ld.fill);
            std::memcpy(ld.h_stage[ld.cur] + (size_t)ld.fill * ld.D, rows, (size_t)take * ld.D * sizeof(float));
            ld.fill += take;
            ld.rows += take;
            rows += (size_t)take * ld.D;
            n -= take;
            if (ld.fill == Load::CH_ROWS) load_flush();
        }
    }
    // make the loaded rows THE gallery: swap pointers, rebuild the screening data, free the previous gallery
    void load_commit() {
        if (!ld.active) raise(FRT_ERR_INVALID, "gallery_commit: no load in progress");
        load_flush();
        HIPCHK(hipStreamSynchronize(ld.s));
        for (bool &p : ld.pending) p = false;
        HIPCHK(hipStreamSynchronize(stream));
        if (busy) HIPCHK(hipEventSynchronize(ev_busy));
        float *old32 = d_gallery;
        half_t *old16 = d_g16;
        if (d_g8) (void)hipFree(d_g8);  // (the streams were synchronised above: no scan is reading it)
        if (d_g8_scale) (void)hipFree(d_g8_scale);
        d_g8 = nullptr;
        d_g8_scale = nullptr;
        shadow_rows = 0;
        gerr = 0.f;
        drop_labels();  // a new gallery: its rows have no labels until frt_matcher_set_labels
        ++generation;
        N = ld.rows;
        D = ld.D;
        store16 = ld.f16;
        d_gallery = ld.rows > 0 ? ld.d_new32 : nullptr;
        d_g16 = ld.rows > 0 ? ld.d_new16 : nullptr;
        cap_rows = ld.rows > 0 ? ld.alloc : 0;
        if (ld.rows == 0) {  // empty gallery: nothing to keep
            if (ld.d_new32) (void)hipFree(ld.d_new32);
            if (ld.d_new16) (void)hipFree(ld.d_new16);
        }
        ld.d_new32 = nullptr;
        ld.d_new16 = nullptr;
        ld.active = false;
        if (old32) (void)hipFree(old32);  // (hipFree waits for the device: stages of earlier pipeline calls have finished with it)
        if (old16) (void)hipFree(old16);
        screen = N >= SCREEN_MIN_ROWS && match_screen_supported(D);
        gmax_norm = 0.f;
        if (N > 0 && (screen || store16)) build_screen_data();
        q_cap = 0;  // partial scratch depends on `blocks`
        if (d_partial) {
            (void)hipFree(d_partial);
            d_partial = nullptr;
        }
        bind_scratch();
    }
    // The screening data of the whole current gallery, on `stream`, synchronously: the int8 / fp16 shadow of fp32-stored rows (allocated for
    // cap_rows; rows from N on hold the value 0) with the largest row norm and quantisation error; fp16-stored rows are their own shadow.
    void build_screen_data() {
        const size_t cap_tiles = ((size_t)cap_rows + 127) / 128, n_tiles = ((size_t)N + 127) / 128;
        // fp32-stored galleries of 512 columns are screened through an INT8 shadow (half the bytes of the per-call scan; kernels_match.hip);
        // other widths through an fp16 shadow
        const bool use_i8 = screen && !store16 && D == 512;
        if (!d_edit_bits) HIPCHK(hipMalloc(reinterpret_cast<void **>(&d_edit_bits), 2 * sizeof(int)));
        HIPCHK(hipMemsetAsync(d_edit_bits, 0, 2 * sizeof(int), stream));
        if (store16) {
            launch_rows_norm(d_g16, 0, N, D, d_edit_bits + 1, stream);
        } else {
            if (shadow_rows < cap_rows) {
                if (d_g8) (void)hipFree(d_g8);
                if (d_g8_scale) (void)hipFree(d_g8_scale);
                if (d_g16) (void)hipFree(d_g16);
                d_g8 = nullptr;
                d_g8_scale = nullptr;
                d_g16 = nullptr;
                shadow_rows = 0;
                if (use_i8) {
                    HIPCHK(hipMalloc(reinterpret_cast<void **>(&d_g8), gallery8_bytes(cap_rows, D)));
                    HIPCHK(hipMalloc(reinterpret_cast<void **>(&d_g8_scale), cap_tiles * 128 * sizeof(float)));
                } else {
                    HIPCHK(hipMalloc(reinterpret_cast<void **>(&d_g16), gallery16_elems(cap_rows, D) * sizeof(half_t)));
                }
                shadow_rows = (int)(cap_tiles * 128);
            }
            if (use_i8) {
                launch_gallery_shadow8(d_gallery, N, D, d_g8, d_g8_scale, d_edit_bits, d_edit_bits + 1, stream);
                if (cap_tiles > n_tiles) {  // the tiles an add will fill later
                    HIPCHK(hipMemsetAsync(d_g8 + n_tiles * 128 * D, 0x80, (cap_tiles - n_tiles) * 128 * D, stream));
                    HIPCHK(hipMemsetAsync(d_g8_scale + n_tiles * 128, 0, (cap_tiles - n_tiles) * 128 * sizeof(float), stream));
                }
            } else {
                launch_gallery_shadow(d_gallery, N, D, d_g16, d_edit_bits + 1, stream);
                if (cap_tiles > n_tiles) HIPCHK(hipMemsetAsync(d_g16 + n_tiles * 128 * D, 0, (cap_tiles - n_tiles) * 128 * D * sizeof(half_t), stream));
            }
        }
        read_bounds(false);
    }
    // d_edit_bits -> gerr / gmax_norm.  merge: keep the larger of the old and the new value (an add: still upper bounds, and the exact
    // re-rank keeps the answers exact); a NaN - the mark of a non-finite row - sticks either way.
    void read_bounds(bool merge) {
        int bits[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(bits, d_edit_bits, sizeof(bits), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        float e2, n2;
        std::memcpy(&e2, &bits[0], 4);
        std::memcpy(&n2, &bits[1], 4);
        const float e = std::sqrt(e2), n = std::sqrt(n2);
        auto upper = [](float old, float nw) { return (old != old || nw <= old) ? old : nw; };
        gerr = merge ? upper(gerr, e) : e;
        gmax_norm = merge ? upper(gmax_norm, n) : n;
    }

    void ensure_queries(int F) {
        if (F <= q_cap && d_partial && scratch_rows >= cap_rows && (!screen || scr.tilemax)) return;
        const int cap = std::max(std::max(F, q_cap), 128);
        const int rows = std::max(cap_rows, N);
        ++generation;  // scratch buffers move
        if (d_q) (void)hipFree(d_q);
        if (d_sim) (void)hipFree(d_sim);
        if (d_idx) (void)hipFree(d_idx);
        if (d_lab) (void)hipFree(d_lab);
        if (d_kth) (void)hipFree(d_kth);
        if (d_partial) (void)hipFree(d_partial);
        d_q = d_sim = d_kth = nullptr;
        d_idx = d_lab = nullptr;
        d_partial = nullptr;
        free_screen_scratch();
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&d_q), (size_t)cap * D * sizeof(float)));
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&d_sim), (size_t)cap * KCAP * sizeof(float)));
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&d_idx), (size_t)cap * KCAP * sizeof(int32_t)));
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&d_lab), (size_t)cap * KCAP * sizeof(int32_t)));
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&d_kth), (size_t)cap * sizeof(float)));
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&d_partial), (size_t)match_top1_blocks(rows, 0) * cap * sizeof(MatchPartial)));  // [blocks][cap], blocks <= those of `rows`
        if (screen) {
            const size_t tiles = ((size_t)rows + 127) / 128;
            HIPCHK(hipMalloc(reinterpret_cast<void **>(&scr.tilemax), (size_t)cap * tiles * 4 * sizeof(float)));  // 4 coarse entries per tile (one per wave)
            scr.pair_cap = std::max(cap * FRT_MATCH_SEL_SUB, 8192);  // (a multiple of the FRT_MATCH_SEL_SUB sub-lists)
            HIPCHK(hipMalloc(reinterpret_cast<void **>(&scr.wgmax), (size_t)FRT_MATCH_COARSE_WG * cap * sizeof(float)));
            HIPCHK(hipMalloc(&scr.pairs, (size_t)scr.pair_cap * 8));
            HIPCHK(hipMalloc(reinterpret_cast<void **>(&scr.ctl), FRT_MATCH_CTL_WORDS * sizeof(int)));
            HIPCHK(hipMemset(scr.ctl, 0, FRT_MATCH_CTL_WORDS * sizeof(int)));
            HIPCHK(hipMalloc(reinterpret_cast<void **>(&scr.qkey), (size_t)cap * sizeof(unsigned long long)));
        }
        q_cap = cap;
        scratch_rows = rows;
        bind_scratch();
    }
    // queries_dev [F][D] -> idx_dev, sim_dev (device pointers)
    void top1_dev(const float *queries_dev, int F, int32_t *idx_dev, float *sim_dev, hipStream_t s) {
        ProfScope ps(2, "match_top1", 2.0 * D * (double)N * F, s);
        // the partial scratch is [blocks][F]
        if (screen && screen_on)  // (d_gallery == nullptr with fp16 storage: the exact re-rank then reads the stored fp16 rows)
            launch_match_screened(d_gallery, d_g16, N, D, queries_dev, F, 1, gmax_norm, screen_scratch(), d_kth, d_partial, blocks, idx_dev, sim_dev, row_offset, s);
        else
            with_rows([&](auto *g) { launch_match_top1(g, N, D, queries_dev, F, d_partial, blocks, idx_dev, sim_dev, row_offset, s); });
        HIPCHK(hipGetLastError());
    }
    // exact top-k lists [F][k] (idx_dev / sim_dev device pointers); queries fp32 on the device
    void topk_dev(const float *queries_dev, int F, int k, int32_t *idx_dev, float *sim_dev, hipStream_t s) {
        ProfScope ps(2, "match_topk", 2.0 * D * (double)N * F, s);
        launch_match_topk(d_gallery, d_g16, N, D, queries_dev, F, k, screen, gmax_norm, screen_scratch(), d_kth, d_partial, blocks, idx_dev, sim_dev, row_offset, s);
        HIPCHK(hipGetLastError());
    }
    // The selection count of a screened identity search, 0 = take the exact passes.  With at most M rows per label the best (k - 1) * M + 1
    // rows hold k identities, so the ((k - 1) * M + 1)-th largest coarse entry bounds the k-th identity's similarity the way the k-th largest
    // bounds the k-th row's; the kth kernel ranks up to match_topk_max() entries.
    int identity_kth_count(int k) const {
        if (!(screen && screen_on)) return 0;
        const long c = (long)(k - 1) * max_rows_per_label + 1;
        return c <= match_topk_max() ? (int)c : 0;
    }
    // exact top-k over identities [F][k] (label_dev / idx_dev / sim_dev device pointers); queries fp32 on the device
    void topk_labels_dev(const float *queries_dev, int F, int k, int32_t *label_dev, int32_t *idx_dev, float *sim_dev, hipStream_t s) {
        ProfScope ps(2, "match_topk_labels", 2.0 * D * (double)N * F, s);
        launch_match_topk_labels(d_gallery, d_g16, N, D, queries_dev, F, k, identity_kth_count(k), gmax_norm, screen_scratch(), d_kth, d_partial, blocks,
                                 d_labels, label_dev, idx_dev, sim_dev, row_offset, s);
        HIPCHK(hipGetLastError());
    }
};

// gallery_add_dev / gallery_add_labeled_dev (labels != nullptr) returning the index of the first new row (frt_matcher.cpp)
int matcher_add_rows_dev(frt_matcher *m, const void *rows_dev, const int32_t *labels, int n_rows);
