// struct frt_matcher: the object behind frt_matcher_* (include/frt.h).  Internal header of libfrt.so: the state, what must hold of it, and
// declarations; the bodies are in frt_matcher.cpp.  Every device and pinned buffer is a DevBuf / PinnedBuf member: frt_matcher_destroy sets
// the device, retires the stream and the events, and `delete` frees the rest.
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
    int N = 0, D = 0;
    int row_offset = 0;  // global index of local row 0 (sharded galleries)
    static constexpr int KCAP = 16;  // qs.sim / idx / lab hold [q_cap][KCAP] (top-k lists of the host entry point)
    static constexpr size_t BOUNCE_BYTES = (size_t)32 << 20;
    static constexpr int SCREEN_MIN_ROWS = 32768;
    // the coarse scan runs one persistent workgroup per CU and each needs a tile of its own: the wgmax scratch is [FRT_MATCH_COARSE_WG][F], read in full
    static_assert(SCREEN_MIN_ROWS / 128 >= FRT_MATCH_COARSE_WG, "a screened gallery has at least one 128-row tile per coarse workgroup");

    // ---- the stored rows and their shadow: one value, so a grown or a reloaded gallery is built aside and swapped in whole.  The stored rows,
    //      the shadow and every scratch buffer sized by rows, tiles or blocks are allocated for cap_rows >= N rows: an add inside the capacity
    //      allocates nothing (frt_matcher_gallery_reserve / add / remove).
    struct Gallery {
        DevBuf<float> rows32;     // fp32 rows [cap_rows][D]; empty when the gallery is STORED as fp16 (store16)
        DevBuf<half_t> rows16;    // fp16 shadow of rows32, or the fp16-STORED gallery itself
        DevBuf<uint8_t> g8;       // int8 shadow of rows32 (fp32-stored galleries with 512 columns take this instead of the fp16 shadow)
        DevBuf<float> g8_scale;
        int cap_rows = 0;       // rows the stored buffer (rows32, or rows16 when store16) holds
        int shadow_rows = 0;    // rows the shadow buffers (g8 + g8_scale, or the fp16 shadow of an fp32 gallery) hold; 0 = none.  They outlive
                                // `screen` (a gallery that fell below the threshold keeps the allocation; its contents are then stale)
        bool store16 = false;   // fp16-stored
        size_t cap_tiles() const { return ((size_t)cap_rows + 127) / 128; }
        void alloc_shadow(int D);                                // fp32 storage: a shadow for cap_rows rows, in place of any it has
        void pad_tiles(size_t n_tiles, int D, hipStream_t s);    // the tiles from n_tiles to cap_tiles hold the value 0 (what an add fills later)
    } gal;
    int reserve_rows = 0;   // floor of the next allocation (frt_matcher_gallery_reserve)
    bool want16 = false;    // storage mode of the NEXT init / gallery_begin (frt_matcher_set_storage)
    // screened search (shadow gallery; see kernels_match.hip).  Off for small galleries and for widths the coarse kernel is not
    // instantiated for (anything but 64 / 128 / 256 / 512).
    float gerr = 0.f;          // largest quantisation error norm of the int8 rows (part of the screening bound)
    float gmax_norm = 0.f;
    bool screen = false;
    bool screen_on = true;     // frt_matcher_set_screening: false = every top-1 call takes the exact fp32 scan (the shadow gallery stays resident)

    // ---- query scratch, freed and allocated together by ensure_queries for q_cap queries and scratch_rows rows
    struct Scratch {
        DevBuf<float> q, sim, kth;
        DevBuf<int32_t> idx, lab;          // (lab: the label lists of the host entry point)
        DevBuf<MatchPartial> partial;      // [blocks][q_cap]
        // the screening scratch (allocated while `screen`): what ScreenScratch views
        DevBuf<float> tilemax, wgmax;
        DevBuf<unsigned long long> pairs, qkey;  // (8 bytes per candidate pair)
        DevBuf<int> ctl;                   // zeroed when allocated
        int pair_cap = 0;
    } qs;
    int q_cap = 0;
    int scratch_rows = 0;   // cap_rows when qs.partial / the tile-sized screening scratch were allocated
    int blocks = 0;
    DevBuf<float> d_full;   // the full similarity matrix of frt_matcher_calculate

    // ---- live edits (frt_matcher.cpp)
    long edit_stats[4] = {};  // rows_uploaded, rows_moved, shadow_rows_rebuilt, reallocations
    DevBuf<int> d_edit_bits;       // [2]: largest error norm^2 / row norm^2 of the rows an edit converted (float bit patterns)
    DevBuf<float> d_edit_stage;    // fp16 storage: fp32 landing buffer of host rows in front of the conversion kernel
    DevBuf<uint8_t> d_bounce;      // BOUNCE_BYTES of the chunked compaction
    DevBuf<int> d_keys;            // the hole keys of a removal (frt_holes.h)
    // ---- clustering (frt_matcher_cluster): the union-find forest, one overflow flag per 128-row chunk, and the host form's results
    DevBuf<int32_t> d_parent, d_cluster_labels;
    DevBuf<int> d_cluster_ovf;
    DevBuf<long long> d_cluster_stats;  // [4]
    // ---- separation (frt_matcher_separation): the grouping (group_rows [N] | pos_ident [N] | group_off [I + 1]), one overflow flag per
    //      128-row chunk, and the arrays a caller did not ask for or the host form downloads (sim: gen [N] | imp [N]; row likewise;
    //      counts: stats [5] | counts [64][2])
    DevBuf<int> d_sep_groups, d_sep_ovf;
    DevBuf<float> d_sep_sim;
    DevBuf<int32_t> d_sep_row;
    DevBuf<long long> d_sep_counts;
    // ---- identities (frt_matcher_set_labels / gallery_add_labeled / topk_labels): one int32 label >= 0 per row, on the device for the label
    //      test of the identity passes and mirrored on the host, where the edits and the per-label row counts are kept.
    bool labelled = false;
    DevBuf<int32_t> d_labels;  // allocated for cap_rows like the rows: a labelled add inside the capacity allocates nothing
    std::vector<int32_t> h_labels;               // [N] while labelled
    std::unordered_map<int32_t, int> label_rows;  // label -> rows that carry it (its size = number of identities)
    int max_rows_per_label = 0;   // M of the screening bound: never below the true maximum; a remove leaves it alone (an over-estimate is only slower)

    void bind_scratch() { blocks = match_top1_blocks(N, 0); }
    void drop_labels() {  // back to an unlabelled gallery (the device allocation is kept for the next labels)
        labelled = false;
        h_labels.clear();
        label_rows.clear();
        max_rows_per_label = 0;
    }
    // d_labels holds at least `rows` labels; the first `keep` survive a move
    void ensure_label_room(int rows, int keep, hipStream_t s);
    // count `n` more labels into label_rows / max_rows_per_label
    void count_labels(const int32_t *l, int n) {
        for (int i = 0; i < n; ++i) max_rows_per_label = std::max(max_rows_per_label, ++label_rows[l[i]]);
    }
    // the rows the exact kernels read, typed: fn(const float *) for an fp32-stored gallery, fn(const half_t *) for an fp16-stored one
    template <typename Fn>
    void with_rows(Fn &&fn) const {
        if (gal.store16) fn(static_cast<const half_t *>(gal.rows16.get()));
        else fn(static_cast<const float *>(gal.rows32.get()));
    }
    ScreenScratch screen_scratch() const {  // the plain view the kernels take: the scratch + the shadow the coarse scan reads
        return {qs.tilemax.get(), qs.wgmax.get(), qs.pairs.get(), qs.pair_cap, qs.ctl.get(), qs.qkey.get(), gal.g8.get(), gal.g8_scale.get(), gerr};
    }
    // Object-level entry points share the scratch buffers with the pipeline's match stage, which keeps running on the pipeline's
    // stream after frt_pipeline_run_dev / submit returned: order this object's stream behind it (one event wait, no host sync).
    void wait_idle(hipStream_t s) {
        if (busy) HIPCHK(hipStreamWaitEvent(s, ev_busy, 0));
    }

    // ---- streaming gallery load (frt_matcher_gallery_begin / append / commit == initKnownEmbeds / addEmbedding / initMatMul,
    //      src/db.cpp:316-346): rows are copied into pinned staging chunks as they arrive (the caller's pointer may be SQLite's
    //      blob buffer) and every full chunk goes to the device with an asynchronous copy while the next one fills.  The previous
    //      gallery stays live (and searchable) until commit swaps the new one in.
    struct Load {
        static constexpr int NCH = 3;
        static constexpr int CH_ROWS = 4096;   // x 512 floats = 8 MB per chunk
        bool active = false;
        bool f16 = false;
        int cap = 0, D = 0, rows = 0, fill = 0, cur = 0;
        int alloc = 0;  // rows allocated: cap, or the matcher's reserve_rows when that is more
        DevBuf<float> new32;
        DevBuf<half_t> new16;
        PinnedBuf<float> h_stage[NCH];
        DevBuf<float> d_stage[NCH];   // fp16 storage only: fp32 landing buffers in front of the conversion kernel
        hipEvent_t ev[NCH] = {};
        bool pending[NCH] = {};
        size_t stage_floats = 0;      // floats per staging chunk once all NCH chunks and their events exist
        hipStream_t s = nullptr;
    } ld;
    void load_release_staging();
    void load_abort();  // waits for the load's stream, then drops the rows loaded so far
    void load_begin(int cap, int cols);
    void load_flush();  // current chunk -> device
    void load_append(const float *rows, int n);
    // make the loaded rows THE gallery: swap it in, rebuild the screening data, free the previous gallery
    void load_commit();
    // The screening data of the whole current gallery, on `stream`, synchronously: the int8 / fp16 shadow of fp32-stored rows (allocated for
    // cap_rows; rows from N on hold the value 0) with the largest row norm and quantisation error; fp16-stored rows are their own shadow.
    void build_screen_data();
    // d_edit_bits -> gerr / gmax_norm.  merge: keep the larger of the old and the new value (an add: still upper bounds, and the exact
    // re-rank keeps the answers exact); a NaN - the mark of a non-finite row - sticks either way.
    void read_bounds(bool merge);
    // scratch for F queries over the current capacity; ++generation when it moves
    void ensure_queries(int F);

    // queries_dev [F][D] -> idx_dev, sim_dev (device pointers)
    void top1_dev(const float *queries_dev, int F, int32_t *idx_dev, float *sim_dev, hipStream_t s) {
        ProfScope ps(2, "match_top1", 2.0 * D * (double)N * F, s);
        // the partial scratch is [blocks][F]
        if (screen && screen_on)  // (rows32 is null with fp16 storage: the exact re-rank then reads the stored fp16 rows)
            launch_match_screened(gal.rows32.get(), gal.rows16.get(), N, D, queries_dev, F, 1, gmax_norm, screen_scratch(), qs.kth.get(), qs.partial.get(), blocks,
                                  idx_dev, sim_dev, row_offset, s);
        else
            with_rows([&](auto *g) { launch_match_top1(g, N, D, queries_dev, F, qs.partial.get(), blocks, idx_dev, sim_dev, row_offset, s); });
        HIPCHK(hipGetLastError());
    }
    // exact top-k lists [F][k] (idx_dev / sim_dev device pointers); queries fp32 on the device
    void topk_dev(const float *queries_dev, int F, int k, int32_t *idx_dev, float *sim_dev, hipStream_t s) {
        ProfScope ps(2, "match_topk", 2.0 * D * (double)N * F, s);
        launch_match_topk(gal.rows32.get(), gal.rows16.get(), N, D, queries_dev, F, k, screen, gmax_norm, screen_scratch(), qs.kth.get(), qs.partial.get(), blocks,
                          idx_dev, sim_dev, row_offset, s);
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
        launch_match_topk_labels(gal.rows32.get(), gal.rows16.get(), N, D, queries_dev, F, k, identity_kth_count(k), gmax_norm, screen_scratch(), qs.kth.get(),
                                 qs.partial.get(), blocks, d_labels.get(), label_dev, idx_dev, sim_dev, row_offset, s);
        HIPCHK(hipGetLastError());
    }
};

// gallery_add_dev / gallery_add_labeled_dev (labels != nullptr) returning the index of the first new row (frt_matcher.cpp)
int matcher_add_rows_dev(frt_matcher *m, const void *rows_dev, const int32_t *labels, int n_rows);
