// libfrt.so: the matcher object's C ABI (frt_matcher_*, top-1 / top-k merges, pinned host memory).
// All device work is hand-written HIP (kernels_*.hip); there is no CPU fallback anywhere in this file: without a HIP
// device every entry point that needs one fails with FRT_ERR_DEVICE.
#include "frt_matcher.hpp"

#include "frt_holes.h"
#include "frt_templates.hpp"

// ------------------------------------------------------------------------------------------------------------- gallery storage
// fp32-stored galleries of 512 columns are screened through an INT8 shadow (half the bytes of the per-call scan; kernels_match.hip);
// other widths through an fp16 shadow
void frt_matcher::Gallery::alloc_shadow(int D) {
    g8.reset();
    g8_scale.reset();
    rows16.reset();
    shadow_rows = 0;
    if (D == 512) {
        g8.reserve(gallery8_bytes(cap_rows, D));
        g8_scale.reserve(cap_tiles() * 128);
    } else {
        rows16.reserve(gallery16_elems(cap_rows, D));
    }
    shadow_rows = (int)(cap_tiles() * 128);
}

// int8 rows of value 0 are bytes of 0x80 (biased) under a scale of 0; fp16 rows - a shadow or the stored rows themselves - are zeros
void frt_matcher::Gallery::pad_tiles(size_t n_tiles, int D, hipStream_t s) {
    if (cap_tiles() <= n_tiles) return;
    const size_t pad_rows = (cap_tiles() - n_tiles) * 128;
    if (g8) {
        HIPCHK(hipMemsetAsync(g8.get() + n_tiles * 128 * D, 0x80, pad_rows * D, s));
        HIPCHK(hipMemsetAsync(g8_scale.get() + n_tiles * 128, 0, pad_rows * sizeof(float), s));
    } else if (rows16) {
        HIPCHK(hipMemsetAsync(rows16.get() + n_tiles * 128 * D, 0, pad_rows * D * sizeof(half_t), s));
    }
}

void frt_matcher::build_screen_data() {
    d_edit_bits.reserve(2);
    int *bits = d_edit_bits.get();
    HIPCHK(hipMemsetAsync(bits, 0, 2 * sizeof(int), stream));
    if (gal.store16) {
        launch_rows_norm(gal.rows16.get(), 0, N, D, bits + 1, stream);
    } else {
        if (gal.shadow_rows < gal.cap_rows) gal.alloc_shadow(D);
        if (gal.g8) launch_gallery_shadow8(gal.rows32.get(), N, D, gal.g8.get(), gal.g8_scale.get(), bits, bits + 1, stream);
        else launch_gallery_shadow(gal.rows32.get(), N, D, gal.rows16.get(), bits + 1, stream);
        gal.pad_tiles(((size_t)N + 127) / 128, D, stream);  // the tiles an add will fill later
    }
    read_bounds(false);
}

void frt_matcher::read_bounds(bool merge) {
    int bits[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(bits, d_edit_bits.get(), sizeof(bits), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    float e2, n2;
    std::memcpy(&e2, &bits[0], 4);
    std::memcpy(&n2, &bits[1], 4);
    const float e = std::sqrt(e2), n = std::sqrt(n2);
    auto upper = [](float old, float nw) { return (old != old || nw <= old) ? old : nw; };
    gerr = merge ? upper(gerr, e) : e;
    gmax_norm = merge ? upper(gmax_norm, n) : n;
}

void frt_matcher::ensure_label_room(int rows, int keep, hipStream_t s) {
    if ((size_t)rows <= d_labels.capacity()) return;
    DevBuf<int32_t> nl;
    nl.reserve((size_t)rows);
    if (keep > 0 && d_labels) {
        hipError_t e = hipMemcpyAsync(nl.get(), d_labels.get(), (size_t)keep * sizeof(int32_t), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        HIPCHK(e);
    }
    d_labels = std::move(nl);
}

void frt_matcher::ensure_queries(int F) {
    if (F <= q_cap && qs.partial && scratch_rows >= gal.cap_rows && (!screen || qs.tilemax)) return;
    const size_t cap = (size_t)std::max(std::max(F, q_cap), 128);
    const int rows = std::max(gal.cap_rows, N);
    ++generation;  // scratch buffers move
    qs = Scratch{};  // everything goes before anything comes
    qs.q.reserve(cap * D);
    qs.sim.reserve(cap * KCAP);
    qs.idx.reserve(cap * KCAP);
    qs.lab.reserve(cap * KCAP);
    qs.kth.reserve(cap);
    qs.partial.reserve((size_t)match_top1_blocks(rows, 0) * cap);  // [blocks][cap], blocks <= those of `rows`
    if (screen) {
        const size_t tiles = ((size_t)rows + 127) / 128;
        qs.tilemax.reserve(cap * tiles * 4);  // 4 coarse entries per tile (one per wave)
        qs.pair_cap = std::max((int)cap * FRT_MATCH_SEL_SUB, 8192);  // (a multiple of the FRT_MATCH_SEL_SUB sub-lists)
        qs.wgmax.reserve((size_t)FRT_MATCH_COARSE_WG * cap);
        qs.pairs.reserve((size_t)qs.pair_cap);
        qs.ctl.reserve(FRT_MATCH_CTL_WORDS);
        HIPCHK(hipMemset(qs.ctl.get(), 0, FRT_MATCH_CTL_WORDS * sizeof(int)));
        qs.qkey.reserve(cap);
    }
    q_cap = (int)cap;
    scratch_rows = rows;
    bind_scratch();
}

// ------------------------------------------------------------------------------------------------------------- streaming load
void frt_matcher::load_release_staging() {
    for (int i = 0; i < Load::NCH; ++i) {
        ld.h_stage[i].reset();
        ld.d_stage[i].reset();
        if (ld.ev[i]) (void)hipEventDestroy(ld.ev[i]);
        ld.ev[i] = nullptr;
        ld.pending[i] = false;
    }
    ld.stage_floats = 0;
}

void frt_matcher::load_abort() {
    if (ld.s) (void)hipStreamSynchronize(ld.s);
    ld.new32.reset();
    ld.new16.reset();
    ld.active = false;
}

void frt_matcher::load_begin(int cap, int cols) {
    if (ld.active) load_abort();
    // The load runs on the matcher's own stream.  NOT on a stream of its own: one more hipStreamCreateWithFlags(hipStreamNonBlocking)
    // stream in the process before the pipeline's stage streams exist changes how ROCm maps those onto hardware queues, and the
    // stages of consecutive calls stop overlapping (measured: batch-1 step 0.56 -> 1.39 ms, batch-32 step +10 %).
    ld.s = stream;
    const size_t need = (size_t)Load::CH_ROWS * cols;
    if (ld.stage_floats != need) {
        load_release_staging();
        for (int i = 0; i < Load::NCH; ++i) {
            ld.h_stage[i].reserve(need);
            HIPCHK(hipEventCreateWithFlags(&ld.ev[i], hipEventDisableTiming));
        }
        ld.stage_floats = need;
    }
    ld.f16 = want16;
    ld.cap = cap;
    ld.D = cols;
    ld.rows = ld.fill = ld.cur = 0;
    ld.alloc = cap > 0 ? std::max(cap, reserve_rows) : 0;
    ld.new32.reset();  // (an aborted load left none; a committed one moved them out)
    ld.new16.reset();
    if (cap > 0) {
        if (ld.f16) {
            ld.new16.reserve(gallery16_elems(ld.alloc, cols));
            HIPCHK(hipMemsetAsync(ld.new16.get(), 0, gallery16_elems(ld.alloc, cols) * sizeof(half_t), ld.s));  // fragment order, zero pad rows
            for (int i = 0; i < Load::NCH; ++i) ld.d_stage[i].reserve(need);
        } else {
            ld.new32.reserve((size_t)ld.alloc * cols);
        }
    }
    ld.active = true;
}

void frt_matcher::load_flush() {
    if (!ld.fill) return;
    const int c = ld.cur;
    const size_t off = (size_t)(ld.rows - ld.fill) * ld.D, n = (size_t)ld.fill * ld.D;
    if (ld.f16) {
        HIPCHK(hipMemcpyAsync(ld.d_stage[c].get(), ld.h_stage[c].get(), n * sizeof(float), hipMemcpyHostToDevice, ld.s));
        launch_rows_to_half(ld.d_stage[c].get(), (long)(ld.rows - ld.fill), (long)ld.fill, ld.D, ld.new16.get(), ld.s);  // (chunks start on 128-row tiles)
    } else {
        HIPCHK(hipMemcpyAsync(ld.new32.get() + off, ld.h_stage[c].get(), n * sizeof(float), hipMemcpyHostToDevice, ld.s));
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

void frt_matcher::load_append(const float *rows, int n) {
    if (!ld.active) raise(FRT_ERR_INVALID, "gallery_append: no load in progress (call frt_matcher_gallery_begin first)");
    if (n < 0 || (n > 0 && !rows)) raise(FRT_ERR_INVALID, "gallery_append: bad argument");
    if ((long)ld.rows + n > ld.cap) raise(FRT_ERR_CAPACITY, "gallery_append: more rows than gallery_begin reserved (initKnownEmbeds)");
    while (n > 0) {
        const int take = std::min(n, Load::CH_ROWS - ld.fill);
        std::memcpy(ld.h_stage[ld.cur].get() + (size_t)ld.fill * ld.D, rows, (size_t)take * ld.D * sizeof(float));
        ld.fill += take;
        ld.rows += take;
        rows += (size_t)take * ld.D;
        n -= take;
        if (ld.fill == Load::CH_ROWS) load_flush();
    }
}

void frt_matcher::load_commit() {
    if (!ld.active) raise(FRT_ERR_INVALID, "gallery_commit: no load in progress");
    load_flush();
    HIPCHK(hipStreamSynchronize(ld.s));
    for (bool &p : ld.pending) p = false;
    HIPCHK(hipStreamSynchronize(stream));
    if (busy) HIPCHK(hipEventSynchronize(ev_busy));  // (the streams are synchronised: no scan is reading the gallery that goes)
    Gallery loaded;  // an empty load leaves an empty gallery: nothing to keep
    loaded.store16 = ld.f16;
    if (ld.rows > 0) {
        loaded.rows32 = std::move(ld.new32);
        loaded.rows16 = std::move(ld.new16);
        loaded.cap_rows = ld.alloc;
    }
    ld.new32.reset();
    ld.new16.reset();
    ld.active = false;
    gerr = 0.f;
    drop_labels();  // a new gallery: its rows have no labels until frt_matcher_set_labels
    ++generation;
    N = ld.rows;
    D = ld.D;
    std::swap(gal, loaded);
    loaded = Gallery{};  // the previous gallery, with the new pointers in place (hipFree waits for the device: stages of earlier pipeline calls have finished with it)
    screen = N >= SCREEN_MIN_ROWS && match_screen_supported(D);
    gmax_norm = 0.f;
    if (N > 0 && (screen || gal.store16)) build_screen_data();
    q_cap = 0;  // partial scratch depends on `blocks`
    qs.partial.reset();
    bind_scratch();
}

// ------------------------------------------------------------------------------------------------------------- live gallery edits
// Add and remove rows of the gallery the matcher is answering from (include/frt.h).  Every edit runs on the matcher's stream behind its
// in-flight match stages (wait_idle), holds the object's mutex - which the pipeline takes to queue a match stage - from start to end, and
// returns when its device work is complete: a match call sees the gallery of before or of after, never a mix.
namespace {

int round_up_tile(long rows) { return (int)((rows + 127) / 128 * 128); }

void edit_checks(frt_matcher *m, const char *what) {
    if (m->row_offset != 0) raise(FRT_ERR_INVALID, std::string(what) + ": a gallery with a row offset (a shard) is edited by reloading it");
}

// Room for `rows` rows: a new gallery value beside the live one + device copy + swap (both copies exist until the copy has run).  Counts
// as one reallocation when there were rows to carry over.
void grow(frt_matcher *m, int rows) {
    frt_matcher::Gallery &g = m->gal;
    if (rows <= g.cap_rows) return;
    hipStream_t s = m->stream;
    const int N = m->N, D = m->D;
    const size_t n_tiles = ((size_t)N + 127) / 128;
    const bool shadow = !g.store16 && m->screen && g.shadow_rows > 0;  // a valid shadow moves along; a stale one is dropped
    frt_matcher::Gallery ng;
    ng.store16 = g.store16;
    ng.cap_rows = round_up_tile(rows);
    if (m->labelled) m->ensure_label_room(ng.cap_rows, N, s);  // the labels move with the rows
    try {
        if (g.store16) {
            ng.rows16.reserve(gallery16_elems(ng.cap_rows, D));
            if (N > 0) HIPCHK(hipMemcpyAsync(ng.rows16.get(), g.rows16.get(), n_tiles * 128 * D * sizeof(half_t), hipMemcpyDeviceToDevice, s));
        } else {
            ng.rows32.reserve((size_t)ng.cap_rows * D);
            if (N > 0) HIPCHK(hipMemcpyAsync(ng.rows32.get(), g.rows32.get(), (size_t)N * D * sizeof(float), hipMemcpyDeviceToDevice, s));
            if (shadow) ng.alloc_shadow(D);
            if (ng.g8) {
                HIPCHK(hipMemcpyAsync(ng.g8.get(), g.g8.get(), n_tiles * 128 * D, hipMemcpyDeviceToDevice, s));
                HIPCHK(hipMemcpyAsync(ng.g8_scale.get(), g.g8_scale.get(), n_tiles * 128 * sizeof(float), hipMemcpyDeviceToDevice, s));
            } else if (shadow) {
                HIPCHK(hipMemcpyAsync(ng.rows16.get(), g.rows16.get(), n_tiles * 128 * D * sizeof(half_t), hipMemcpyDeviceToDevice, s));
            }
        }
        ng.pad_tiles(n_tiles, D, s);
        HIPCHK(hipStreamSynchronize(s));
    } catch (...) {
        (void)hipStreamSynchronize(s);  // before `ng` goes: a queued copy may still be writing into it
        throw;
    }
    std::swap(g, ng);  // the previous gallery is freed when `ng` leaves, with the new pointers in place
    if (N > 0) ++m->edit_stats[3];
}

// the tail of every edit: sizes, scratch, generation; the stream is idle when this returns
void finish_edit(frt_matcher *m, int new_n) {
    m->N = new_n;
    ++m->generation;
    m->bind_scratch();
    if (m->q_cap > 0 && new_n > 0) m->ensure_queries(m->q_cap);  // (a grown capacity, or screening that has just begun: a pipeline call that was
                                                                  //  queued before the edit runs its match stage without passing ensure_queries again)
    HIPCHK(hipStreamSynchronize(m->stream));
}

// labels: one per new row (host memory) for the labelled form, nullptr for the plain one.  A gallery with rows takes only the form that
// matches its state; an empty one takes either and becomes labelled or unlabelled by it.
void add_rows(frt_matcher *m, const void *rows, int n, bool on_device, const int32_t *labels = nullptr, bool labelled_form = false) {
    edit_checks(m, "gallery_add");
    if (n < 0 || (n > 0 && !rows) || (labelled_form && n > 0 && !labels)) raise(FRT_ERR_INVALID, "gallery_add: bad argument");
    if (m->D <= 0) raise(FRT_ERR_INVALID, "gallery_add: the number of columns is not known yet (frt_matcher_init or gallery_begin + commit first)");
    if (m->N > 0 && m->labelled != labelled_form)
        raise(FRT_ERR_INVALID, m->labelled ? "gallery_add: the gallery is labelled (frt_matcher_gallery_add_labeled)"
                                           : "gallery_add_labeled: the gallery has no labels (frt_matcher_set_labels first)");
    for (int i = 0; labelled_form && i < n; ++i)
        if (labels[i] < 0) raise(FRT_ERR_INVALID, "gallery_add_labeled: negative label");
    if (n == 0) return;
    if ((long)m->N + n > INT32_MAX - 128) raise(FRT_ERR_CAPACITY, "gallery_add: too many rows");
    hipStream_t s = m->stream;
    const int N = m->N, D = m->D, new_n = N + n;
    m->wait_idle(s);
    if (N == 0) m->drop_labels();  // (rows == 0: whatever labels the emptied gallery had are gone; grow then moves none)
    frt_matcher::Gallery &g = m->gal;
    if (new_n > g.cap_rows) grow(m, std::max(new_n, std::max((int)std::min((long)g.cap_rows * 3 / 2, (long)INT32_MAX - 128), m->reserve_rows)));
    if (labelled_form) {
        m->ensure_label_room(g.cap_rows, N, s);
        HIPCHK(hipMemcpyAsync(m->d_labels.get() + N, labels, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));  // (complete before finish_edit returns)
        m->h_labels.reserve((size_t)g.cap_rows);
    }
    const float *src32 = reinterpret_cast<const float *>(rows);  // the new rows as fp32 ON THE DEVICE (conversion source)
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (g.store16) {
        if (!on_device) {
            const size_t need = (size_t)n * D;
            m->d_edit_stage.reserve(need);
            HIPCHK(hipMemcpyAsync(m->d_edit_stage.get(), rows, need * sizeof(float), kind, s));
            src32 = m->d_edit_stage.get();
        }
        launch_rows_to_half(src32, N, n, D, g.rows16.get(), s);
    } else {
        HIPCHK(hipMemcpyAsync(g.rows32.get() + (size_t)N * D, rows, (size_t)n * D * sizeof(float), kind, s));
        src32 = g.rows32.get() + (size_t)N * D;
    }
    m->edit_stats[0] += n;
    const bool was_screen = m->screen;
    m->screen = new_n >= frt_matcher::SCREEN_MIN_ROWS && match_screen_supported(D);
    if (m->screen && !was_screen) {  // the gallery has grown across the screening threshold: the one add that builds the whole shadow
        m->N = new_n;
        try {
            m->build_screen_data();
        } catch (...) {
            m->N = N;
            m->screen = was_screen;
            throw;
        }
        if (!g.store16) m->edit_stats[2] += new_n;
    } else if (m->screen) {  // tail update: only the new rows are converted into their places
        int *bits = m->d_edit_bits.get();
        if (g.store16) {
            launch_rows_norm(g.rows16.get(), N, n, D, bits + 1, s);
            HIPCHK(hipMemsetAsync(bits, 0, sizeof(int), s));
        } else if (g.g8 && D == 512) {
            launch_gallery_shadow8_rows(src32, N, n, g.g8.get(), g.g8_scale.get(), bits, bits + 1, s);
            m->edit_stats[2] += n;
        } else {
            launch_rows_to_half(src32, N, n, D, g.rows16.get(), s);
            launch_rows_norm(g.rows32.get(), N, n, D, bits + 1, s);
            HIPCHK(hipMemsetAsync(bits, 0, sizeof(int), s));
            m->edit_stats[2] += n;
        }
        HIPCHK(hipGetLastError());
        m->read_bounds(true);
    }
    HIPCHK(hipGetLastError());
    if (labelled_form) {
        m->labelled = true;
        m->h_labels.insert(m->h_labels.end(), labels, labels + n);
        m->count_labels(labels, n);
    }
    finish_edit(m, new_n);
}

void remove_rows(frt_matcher *m, const int32_t *idx, int n_idx) {
    edit_checks(m, "gallery_remove");
    if (n_idx < 0 || (n_idx > 0 && !idx)) raise(FRT_ERR_INVALID, "gallery_remove: bad argument");
    std::vector<int> keys;
    if (!frt_hole_keys(idx, n_idx, m->N, keys)) raise(FRT_ERR_INVALID, "gallery_remove: row index out of range");
    if (keys.empty()) return;
    hipStream_t s = m->stream;
    const int N = m->N, D = m->D, nk = (int)keys.size(), new_n = N - nk, r0 = keys[0];
    const long tile0 = r0 >> 7, new_tiles = ((long)new_n + 127) / 128, old_tiles = ((long)N + 127) / 128;
    m->wait_idle(s);
    frt_matcher::Gallery &g = m->gal;
    m->d_bounce.reserve(frt_matcher::BOUNCE_BYTES);
    m->d_keys.reserve(keys.size());
    const int *d_keys = m->d_keys.get();
    HIPCHK(hipMemcpyAsync(m->d_keys.get(), keys.data(), keys.size() * sizeof(int), hipMemcpyHostToDevice, s));
    // the keys that fall into the destination rows [a, b): those in front of them all count, those behind them never do
    auto key_range = [&](long a, long b, int &lo, int &hi) {
        lo = (int)(std::lower_bound(keys.begin(), keys.end(), (int)a) - keys.begin());
        hi = (int)(std::upper_bound(keys.begin(), keys.end(), (int)(b - 1)) - keys.begin());
    };
    if (g.store16) {
        // whole destination tiles from the first hole's tile on; the gather also zeroes the padding of the new last tile
        const long chunk = std::max<long>(1, (long)(frt_matcher::BOUNCE_BYTES / ((size_t)128 * D * sizeof(half_t))));
        half_t *bounce = reinterpret_cast<half_t *>(m->d_bounce.get());
        for (long t = tile0; t < new_tiles; t += chunk) {
            const long nt = std::min(chunk, new_tiles - t);
            int lo, hi;
            key_range(t * 128, (t + nt) * 128, lo, hi);
            launch_gather_rows16(g.rows16.get(), D, t, nt, new_n, d_keys, lo, hi, bounce, s);
            HIPCHK(hipMemcpyAsync(g.rows16.get() + (size_t)t * 128 * D, bounce, (size_t)nt * 128 * D * sizeof(half_t), hipMemcpyDeviceToDevice, s));
        }
        if (old_tiles > new_tiles) HIPCHK(hipMemsetAsync(g.rows16.get() + (size_t)new_tiles * 128 * D, 0, (size_t)(old_tiles - new_tiles) * 128 * D * sizeof(half_t), s));
    } else {
        const long chunk = std::max<long>(1, (long)(frt_matcher::BOUNCE_BYTES / ((size_t)D * sizeof(float))));
        float *bounce = reinterpret_cast<float *>(m->d_bounce.get());
        for (long a = r0; a < new_n; a += chunk) {
            const long nr = std::min(chunk, (long)new_n - a);
            int lo, hi;
            key_range(a, a + nr, lo, hi);
            launch_gather_rows(g.rows32.get(), D, (int)a, (int)nr, d_keys, lo, hi, bounce, s);
            HIPCHK(hipMemcpyAsync(g.rows32.get() + (size_t)a * D, bounce, (size_t)nr * D * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
    }
    HIPCHK(hipGetLastError());
    if (new_n > r0) m->edit_stats[1] += new_n - r0;
    // Below the threshold a fresh matcher does not screen, and neither does this one (the shadow's allocation stays for the way back up).
    m->screen = new_n >= frt_matcher::SCREEN_MIN_ROWS && match_screen_supported(D);
    if (m->screen && !g.store16) {
        // the shadow from the first affected tile on, with the build's arithmetic; gerr / gmax_norm stay (maxima over a subset are no larger)
        const long first = tile0 * 128, n_re = std::max(0L, (long)new_n - first);
        if (g.g8 && D == 512) {
            HIPCHK(hipMemsetAsync(g.g8.get() + (size_t)first * D, 0x80, (size_t)(old_tiles - tile0) * 128 * D, s));
            HIPCHK(hipMemsetAsync(g.g8_scale.get() + first, 0, (size_t)(old_tiles - tile0) * 128 * sizeof(float), s));
            launch_gallery_shadow8_rows(g.rows32.get() + (size_t)first * D, (int)first, (int)n_re, g.g8.get(), g.g8_scale.get(), m->d_edit_bits.get(), m->d_edit_bits.get() + 1, s);
        } else {
            HIPCHK(hipMemsetAsync(g.rows16.get() + (size_t)first * D, 0, (size_t)(old_tiles - tile0) * 128 * D * sizeof(half_t), s));
            launch_rows_to_half(g.rows32.get() + (size_t)first * D, first, n_re, D, g.rows16.get(), s);
        }
        HIPCHK(hipGetLastError());
        m->edit_stats[2] += n_re;
    }
    if (m->labelled) {  // the labels close up with the rows: on the host mirror, then the moved tail goes back to the device
        for (int i = 0; i < nk; ++i) {
            auto it = m->label_rows.find(m->h_labels[(size_t)(keys[(size_t)i] + i)]);
            if (it != m->label_rows.end() && --it->second == 0) m->label_rows.erase(it);
        }
        for (int j = r0; j < new_n; ++j) m->h_labels[(size_t)j] = m->h_labels[(size_t)frt_hole_source_row(keys.data(), 0, nk, j)];
        m->h_labels.resize((size_t)new_n);
        if (new_n > r0)
            HIPCHK(hipMemcpyAsync(m->d_labels.get() + r0, m->h_labels.data() + r0, (size_t)(new_n - r0) * sizeof(int32_t), hipMemcpyHostToDevice, s));
        // max_rows_per_label stays: the true maximum cannot have grown, and an over-estimate only makes fewer calls screen
    }
    finish_edit(m, new_n);
}

// ------------------------------------------------------------------------------------------------------------- template gallery
// frt_matcher_build_templates (include/frt.h) with both mutexes held by the caller.  The grouping comes from src's host mirror of the labels,
// the pass over the rows runs on src's stream into buffers of this call, and dst takes the templates by the route every device row takes:
// emptied as a commit of zero rows empties a matcher (which also waits for its match stages), then ONE labelled add that allocates for I rows.
void build_templates(frt_matcher *src, frt_matcher *dst, int32_t *labels_out, int32_t *n_rows_out, float *min_sim_out, int32_t *min_row_out,
                     float *templates_out) {
    if (src->D <= 0) raise(FRT_ERR_INVALID, "build_templates: the source has no gallery yet (frt_matcher_init or gallery_begin + commit first)");
    if (src->N > 0 && !src->labelled) raise(FRT_ERR_INVALID, "build_templates: the source gallery has no labels (frt_matcher_set_labels)");
    if (dst && dst->row_offset != 0) raise(FRT_ERR_INVALID, "build_templates: the destination has a row offset (a shard); templates go to an unsharded matcher");
    use_device(src->device);
    const int N = src->N, D = src->D;
    std::vector<int32_t> ident_label;
    std::vector<int> off, rows;
    frt_template_groups(src->h_labels.data(), N, ident_label, off, rows);
    const int I = (int)ident_label.size();
    Arena mem;
    try {
        float *d_t = nullptr;
        if (I > 0) {
            hipStream_t s = src->stream;
            src->wait_idle(s);  // behind a match stage still reading src's scratch (it only reads the rows, as this pass does)
            int *d_off = mem.alloc<int>(off.size()), *d_rows = mem.alloc<int>(rows.size());
            d_t = mem.alloc<float>((size_t)I * D);
            float *d_sim = mem.alloc<float>((size_t)I);
            int32_t *d_row = mem.alloc<int32_t>((size_t)I);
            HIPCHK(hipMemcpyAsync(d_off, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice, s));
            {
                ProfScope ps(2, "template_build", (double)N * D * (src->gal.store16 ? 2 : 4) + (double)I * D * 4, s);  // work = bytes moved
                src->with_rows([&](auto *g) { launch_template_build(g, D, d_off, d_rows, I, src->row_offset, d_t, d_sim, d_row, s); });
                HIPCHK(hipGetLastError());
            }
            if (min_sim_out) HIPCHK(hipMemcpyAsync(min_sim_out, d_sim, (size_t)I * sizeof(float), hipMemcpyDeviceToHost, s));
            if (min_row_out) HIPCHK(hipMemcpyAsync(min_row_out, d_row, (size_t)I * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            if (templates_out) HIPCHK(hipMemcpyAsync(templates_out, d_t, (size_t)I * D * sizeof(float), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        for (int i = 0; i < I; ++i) {
            if (labels_out) labels_out[i] = ident_label[(size_t)i];
            if (n_rows_out) n_rows_out[i] = off[(size_t)i + 1] - off[(size_t)i];
        }
        if (dst) {
            dst->load_begin(0, D);
            try {
                dst->load_commit();
            } catch (...) {
                dst->load_abort();
                throw;
            }
            add_rows(dst, d_t, I, true, ident_label.data(), true);
        }
    } catch (...) {
        (void)hipStreamSynchronize(src->stream);
        mem.release();
        throw;
    }
    mem.release();
}

// What every host entry point that takes queries starts with (the caller holds m->mu): the queries are in d_q, on the returned stream
hipStream_t upload_queries(frt_matcher *m, const float *embeds, int F) {
    if (m->N <= 0 || F <= 0) raise(FRT_ERR_EMPTY, "Feature matching: No faces in database or no faces found");
    use_device(m->device);
    hipStream_t s = m->stream;
    m->wait_idle(s);
    m->ensure_queries(F);
    HIPCHK(hipMemcpyAsync(m->qs.q.get(), embeds, sizeof(float) * (size_t)F * m->D, hipMemcpyHostToDevice, s));
    return s;
}

// the full similarity matrix of the F queries in d_q -> outputs [F][N] on the host (queued on s; grows d_full)
void full_matrix_to_host(frt_matcher *m, int F, float *outputs, hipStream_t s) {
    const size_t need = (size_t)F * m->N;
    m->d_full.reserve(need);
    for (int f0 = 0; f0 < F; f0 += 128)
        m->with_rows([&](auto *g) { launch_match_full(g, m->N, m->D, m->qs.q.get() + (size_t)f0 * m->D, std::min(128, F - f0), m->d_full.get() + (size_t)f0 * m->N, s); });
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(outputs, m->d_full.get(), need * sizeof(float), hipMemcpyDeviceToHost, s));
}

// upload the queries, search, download k columns per query: the top-1 search (lists == false, k == 1) or the top-k lists.
// matrix_out != nullptr: the full matrix as well (the search runs under the tail of its download).  label_out != nullptr: the lists rank
// identities (frt_matcher_topk_labels) and their labels come back too.
void check_labelled(frt_matcher *m) {
    if (m->N > 0 && !m->labelled) raise(FRT_ERR_INVALID, "topk_labels: the gallery has no labels (frt_matcher_set_labels)");
}

void search_to_host(frt_matcher *m, const float *embeds, int F, bool lists, int k, int32_t *idx_out, float *sim_out, float *matrix_out = nullptr,
                    int32_t *label_out = nullptr) {
    std::lock_guard<std::mutex> lk(m->mu);
    if (label_out) check_labelled(m);
    hipStream_t s = upload_queries(m, embeds, F);
    if (matrix_out) full_matrix_to_host(m, F, matrix_out, s);
    const float *q = m->qs.q.get();
    int32_t *idx = m->qs.idx.get();
    float *sim = m->qs.sim.get();
    if (label_out) {
        m->topk_labels_dev(q, F, k, m->qs.lab.get(), idx, sim, s);
        HIPCHK(hipMemcpyAsync(label_out, m->qs.lab.get(), sizeof(int32_t) * (size_t)F * k, hipMemcpyDeviceToHost, s));
    } else if (lists) m->topk_dev(q, F, k, idx, sim, s);
    else m->top1_dev(q, F, idx, sim, s);
    HIPCHK(hipMemcpyAsync(idx_out, idx, sizeof(int32_t) * (size_t)F * k, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(sim_out, sim, sizeof(float) * (size_t)F * k, hipMemcpyDeviceToHost, s));
    sync_stream_spinning(s);
}

// What the three *_dev searches share (the caller holds m->mu): the scratch behind in-flight match stages on the caller's stream, fp16
// queries widened exactly into the query scratch, search(fp32 queries, stream), and the scratch marked in use until the search has run
template <typename Fn>
void search_dev(frt_matcher *m, const void *embeds_dev, int embeds_fp16, int F, void *hip_stream, Fn &&search) {
    if (m->N <= 0 || F <= 0) raise(FRT_ERR_EMPTY, "Feature matching: No faces in database or no faces found");
    use_device(m->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    m->wait_idle(s);
    m->ensure_queries(F);
    const float *q = reinterpret_cast<const float *>(embeds_dev);
    if (embeds_fp16) {
        launch_half_to_float(reinterpret_cast<const half_t *>(embeds_dev), (long)F * m->D, m->qs.q.get(), s);
        q = m->qs.q.get();
    }
    search(q, s);
    HIPCHK(hipEventRecord(m->ev_busy, s));
    m->busy = true;
}

// frt_matcher_set_labels with m->mu held by the caller
void set_labels(frt_matcher *m, const int32_t *labels, int n) {
    if (n == 0) {  // clear
        if (m->labelled) ++m->generation;
        m->drop_labels();
        return;
    }
    if (n != m->N) raise(FRT_ERR_INVALID, "set_labels: one label per gallery row");
    for (int i = 0; i < n; ++i)
        if (labels[i] < 0) raise(FRT_ERR_INVALID, "set_labels: negative label");
    use_device(m->device);
    hipStream_t s = m->stream;
    m->wait_idle(s);  // a match stage in flight may be reading the old labels
    HIPCHK(hipStreamSynchronize(s));
    if (m->busy) HIPCHK(hipEventSynchronize(m->ev_busy));
    m->ensure_label_room(std::max(m->gal.cap_rows, n), 0, s);
    HIPCHK(hipMemcpyAsync(m->d_labels.get(), labels, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    m->drop_labels();
    m->labelled = true;
    m->h_labels.reserve((size_t)std::max(m->gal.cap_rows, n));
    m->h_labels.assign(labels, labels + n);
    m->count_labels(labels, n);
    ++m->generation;
}

// ------------------------------------------------------------------------------------------------------------- clustering
// frt_matcher_cluster / _cluster_dev (include/frt.h) with m->mu held and N > 0: labels_dev [N] and stats_dev [4] are complete
// on `s` when the stream has run.  The gallery is walked in chunks of 128 stored rows used as queries; a chunk goes through the screen
// (coarse scan, absolute-threshold selection from the chunk's own tile on, edge re-rank + union) or through the dense pass (the chunk's
// full similarity matrix, at most DENSE_BYTES of it at a time, then the union over it).  A screened chunk whose pair list overflowed
// joined nothing; its flag lands in d_cluster_ovf, which the host reads once behind the walk to send those chunks through the dense pass.
// frt_profile_enable(3) brackets every chunk's stages (cluster_coarse / _select / _rerank / _dense); kind 2 the whole call.
constexpr size_t CLUSTER_DENSE_BYTES = (size_t)64 << 20;

void cluster(frt_matcher *m, float t, int32_t *labels_dev, long long *stats_dev, hipStream_t s) {
    const int N = m->N, D = m->D, chunks = (N + 127) / 128;
    m->wait_idle(s);
    m->ensure_queries(128);
    const int dense_q = (int)std::max<size_t>(1, std::min<size_t>(128, CLUSTER_DENSE_BYTES / sizeof(float) / (size_t)N));  // queries per dense launch
    m->d_full.reserve((size_t)dense_q * N);
    m->d_parent.reserve((size_t)std::max(m->gal.cap_rows, N));
    m->d_cluster_ovf.reserve((size_t)chunks);
    int32_t *parent = m->d_parent.get();
    ProfScope ps(2, "cluster", 2.0 * D * (double)N * N, s);
    launch_cluster_init(parent, N, stats_dev, s);
    // the chunk's queries: the stored fp32 rows where they lie; fp16 storage: widened into the query scratch
    auto chunk_queries = [&](int r0, int F) -> const float * {
        if (!m->gal.store16) return m->gal.rows32.get() + (size_t)r0 * D;
        launch_cluster_queries(m->gal.rows16.get(), r0, F, D, m->qs.q.get(), s);
        return m->qs.q.get();
    };
    auto dense_chunk = [&](int r0, int F) {
        const float *q = chunk_queries(r0, F);
        ProfScope p(3, "cluster_dense", 2.0 * D * (double)N * F, s);
        for (int f0 = 0; f0 < F; f0 += dense_q) {
            const int nf = std::min(dense_q, F - f0);
            m->with_rows([&](auto *g) { launch_match_full(g, N, D, q + (size_t)f0 * D, nf, m->d_full.get(), s); });
            launch_cluster_dense_union(m->d_full.get(), nf, N, r0 + f0, t, parent, stats_dev, s);
        }
    };
    const bool screened = m->screen && m->screen_on;
    const bool triangular = !getenv("FRT_CLUSTER_FULL_WALK");  // measurement only (tools/cluster_timing.py): every chunk scans from tile 0
    const int tiles = chunks;
    if (screened) prof_reserve(3, 3 * (size_t)chunks);
    long long n_screened = 0, n_dense = 0;
    for (int c = 0; c < chunks; ++c) {
        const int r0 = c * 128, F = std::min(128, N - r0);
        if (screened) {
            const float *q = chunk_queries(r0, F);
            // Triangular walk: rows j > i lie in tiles >= c, so the scan begins at the chunk's own tile - the shadow, its scales and the stored
            // fp16 rows are whole 128-row tiles of 128 * D elements each, and the coarse kernels number tiles from the pointer they are given.
            // They launch min(tiles, FRT_MATCH_COARSE_WG) workgroups and the selection reads FRT_MATCH_COARSE_WG rows of wgmax, so a tail
            // with fewer tiles than that is scanned from tile 0 like the whole gallery (the selection still lists tiles >= c only).
            const int origin = (triangular && tiles - c >= FRT_MATCH_COARSE_WG) ? c : 0;
            const size_t skip = (size_t)origin * 128 * D;
            const int Nl = N - origin * 128;
            ScreenScratch w = m->screen_scratch();
            if (w.g8) {
                w.g8 += skip;
                w.g8_scale += (size_t)origin * 128;
            }
            const half_t *g16 = m->gal.rows16 ? m->gal.rows16.get() + skip : nullptr;
            bool i8;
            {
                ProfScope p(3, "cluster_coarse", 2.0 * D * (double)Nl * F, s);
                i8 = launch_match_coarse(g16, Nl, D, q, F, w, s);
            }
            {
                ProfScope p(3, "cluster_select", 0.0, s);
                launch_match_select_threshold(Nl, D, q, F, t, c - origin, m->gmax_norm, w, i8, s);
            }
            ProfScope p(3, "cluster_rerank", 0.0, s);
            m->with_rows([&](auto *g) { launch_cluster_rerank_union(g, N, D, q, r0, origin, w, t, parent, stats_dev, m->d_cluster_ovf.get() + c, s); });
        } else {
            dense_chunk(r0, F);
        }
    }
    HIPCHK(hipGetLastError());
    if (screened) {
        std::vector<int> ovf((size_t)chunks);
        HIPCHK(hipMemcpyAsync(ovf.data(), m->d_cluster_ovf.get(), (size_t)chunks * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int c = 0; c < chunks; ++c)
            if (ovf[(size_t)c]) {
                dense_chunk(c * 128, std::min(128, N - c * 128));
                ++n_dense;
            }
        n_screened = chunks - n_dense;
    } else {
        n_dense = chunks;
    }
    launch_cluster_flatten(parent, N, labels_dev, stats_dev, n_screened, n_dense, s);
    HIPCHK(hipGetLastError());
}

void cluster_checks(frt_matcher *m, float threshold) {
    if (!std::isfinite(threshold)) raise(FRT_ERR_INVALID, "cluster: the threshold is not finite");
    if (m->row_offset != 0) raise(FRT_ERR_INVALID, "cluster: a gallery with a row offset (a shard) does not know its neighbours' rows");
}

// ------------------------------------------------------------------------------------------------------------- separation
// frt_matcher_separation / _separation_dev (include/frt.h) with m->mu held, N > 0 and labels: the four arrays [N], counts
// [n_thr][2] and stats [5] (device pointers, none null) are complete on `s` when the stream has run.  Genuine side: one launch over the
// identity -> rows grouping (uploaded as build_templates uploads it; the host waits once for the copies, so the vectors may go).  Impostor
// side: the gallery walked in chunks of 128 stored rows as queries, every chunk ONE label-excluded top-1 search whose taken labels are the
// chunk's own slice of the device labels - through the screen when topk_labels would screen k = 2 (identity_kth_count), else one
// label-excluded exact scan.  A screened chunk whose pair list overflowed is answered by the gated exact scan inside the same search; its
// flag lands in d_sep_ovf for the statistics.  frt_profile_enable(3) brackets the stages (separation_genuine / _coarse / _select / _rerank
// / _exact / _reduce); kind 2 the whole call.
void separation(frt_matcher *m, float *gen_sim, int32_t *gen_row, float *imp_sim, int32_t *imp_row, const float *thresholds, int n_thr, long long *counts,
                long long *stats, hipStream_t s) {
    const int N = m->N, D = m->D, chunks = (N + 127) / 128;
    m->wait_idle(s);
    m->ensure_queries(128);
    std::vector<int32_t> ident_label;
    std::vector<int> off, rows;
    frt_template_groups(m->h_labels.data(), N, ident_label, off, rows);
    const size_t I = ident_label.size();
    std::vector<int> pos_ident((size_t)N);
    for (size_t i = 0; i < I; ++i) std::fill(pos_ident.begin() + off[i], pos_ident.begin() + off[i + 1], (int)i);
    m->d_sep_groups.reserve(2 * (size_t)N + I + 1);
    m->d_sep_ovf.reserve((size_t)chunks);
    int *d_rows = m->d_sep_groups.get(), *d_pos = d_rows + N, *d_off = d_pos + N;
    HIPCHK(hipMemcpyAsync(d_rows, rows.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_pos, pos_ident.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_off, off.data(), (I + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    ProfScope ps(2, "separation", 2.0 * D * (double)N * N, s);
    const int kth_count = m->identity_kth_count(2);  // max_rows_per_label + 1 when the screen applies: the best M + 1 rows hold a row of another label
    const bool screened = kth_count > 0;
    prof_reserve(3, 3 * (size_t)chunks + 2);
    {
        ProfScope p(3, "separation_genuine", 0.0, s);
        m->with_rows([&](auto *g) { launch_separation_genuine(g, N, D, d_off, d_rows, d_pos, gen_sim, gen_row, s); });
    }
    const int32_t *labels = m->d_labels.get();
    for (int c = 0; c < chunks; ++c) {
        const int r0 = c * 128, F = std::min(128, N - r0);
        // the chunk's queries: the stored fp32 rows where they lie; fp16 storage: widened into the query scratch
        const float *q = m->qs.q.get();
        if (m->gal.store16) launch_cluster_queries(m->gal.rows16.get(), r0, F, D, m->qs.q.get(), s);
        else q = m->gal.rows32.get() + (size_t)r0 * D;
        if (screened) {
            const ScreenScratch w = m->screen_scratch();
            bool i8;
            {
                ProfScope p(3, "separation_coarse", 2.0 * D * (double)N * F, s);
                i8 = launch_match_coarse(m->gal.rows16.get(), N, D, q, F, w, s);
            }
            {
                ProfScope p(3, "separation_select", 0.0, s);
                launch_match_select_kth(N, D, q, F, kth_count, m->gmax_norm, w, m->qs.kth.get(), i8, s);
            }
            ProfScope p(3, "separation_rerank", 0.0, s);
            launch_match_top1_excluding(m->gal.rows32.get(), m->gal.rows16.get(), N, D, q, F, true, w, m->qs.partial.get(), m->blocks, labels, labels + r0,
                                        imp_row + r0, imp_sim + r0, m->d_sep_ovf.get() + c, s);
        } else {
            ProfScope p(3, "separation_exact", 2.0 * D * (double)N * F, s);
            launch_match_top1_excluding(m->gal.rows32.get(), m->gal.rows16.get(), N, D, q, F, false, m->screen_scratch(), m->qs.partial.get(), m->blocks, labels,
                                        labels + r0, imp_row + r0, imp_sim + r0, nullptr, s);
        }
    }
    HIPCHK(hipGetLastError());
    ProfScope p(3, "separation_reduce", 0.0, s);
    launch_separation_reduce(gen_sim, gen_row, imp_sim, imp_row, N, thresholds, n_thr, m->d_sep_ovf.get(), chunks, screened, counts, stats, s);
    HIPCHK(hipGetLastError());
}

void separation_checks(frt_matcher *m, const float *thresholds, int n_thr) {
    if (n_thr < 0 || n_thr > FRT_SEPARATION_MAX_THRESHOLDS || (n_thr > 0 && !thresholds)) raise(FRT_ERR_INVALID, "separation: n_thresholds must be in 0..64");
    for (int k = 0; k < n_thr; ++k)
        if (!std::isfinite(thresholds[k])) raise(FRT_ERR_INVALID, "separation: a threshold is not finite");
    if (m->row_offset != 0) raise(FRT_ERR_INVALID, "separation: a gallery with a row offset (a shard) does not know its neighbours' rows");
    if (m->N > 0 && !m->labelled) raise(FRT_ERR_INVALID, "separation: the gallery has no labels (frt_matcher_set_labels)");
}

// the shell of the gallery entry points: the object's lock and device around fn
template <typename Fn>
int with_gallery(frt_matcher *m, Fn &&fn) {
    return guarded([&] {
        if (!m) raise(FRT_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(m->mu);
        use_device(m->device);
        fn();
    });
}

}  // namespace

// frt_matcher_gallery_add_dev / _add_labeled_dev (labels != nullptr) for callers inside the library that need the index of the first new
// row from the edit itself (another thread's edit may follow before they could ask): takes m->mu; raises like the entry points
int matcher_add_rows_dev(frt_matcher *m, const void *rows_dev, const int32_t *labels, int n_rows) {
    std::lock_guard<std::mutex> lk(m->mu);
    use_device(m->device);
    const int first = m->N;
    add_rows(m, rows_dev, n_rows, true, labels, labels != nullptr);
    return first;
}

extern "C" {

// ------------------------------------------------------------------------------------------------------------- matcher
int frt_matcher_create(int device, frt_matcher **out) {
    return guarded([&] {
        if (!out) raise(FRT_ERR_INVALID, "null argument");
        *out = nullptr;
        use_device(device);
        std::unique_ptr<frt_matcher> m(new frt_matcher);
        m->device = device;
        HIPCHK(hipStreamCreate(&m->stream));
        HIPCHK(hipEventCreateWithFlags(&m->ev_busy, hipEventDisableTiming));
        *out = m.release();
    });
}

void frt_matcher_destroy(frt_matcher *m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    // an unfinished streaming load runs on m->stream (ld.s == stream): abort it while the stream still exists
    m->load_abort();
    m->load_release_staging();
    m->ld.s = nullptr;
    if (m->stream) {
        (void)hipStreamSynchronize(m->stream);
        (void)hipStreamDestroy(m->stream);
    }
    if (m->ev_busy) (void)hipEventDestroy(m->ev_busy);
    delete m;  // every buffer frees itself, on the device set above
}

static void check_gallery_shape(int num_row, int num_col) {
    if (num_row < 0) raise(FRT_ERR_INVALID, "MatMul::init: bad argument");
    if (num_col < 32 || num_col % 32) raise(FRT_ERR_INVALID, "MatMul::init: numCol must be a multiple of 32");
}

int frt_matcher_set_storage(frt_matcher *m, int fp16) {
    return guarded([&] {
        if (!m) raise(FRT_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(m->mu);
        m->want16 = fp16 != 0;
    });
}

int frt_matcher_set_screening(frt_matcher *m, int on) {
    return guarded([&] {
        if (!m) raise(FRT_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(m->mu);
        m->screen_on = on != 0;
    });
}

unsigned frt_matcher_generation(frt_matcher *m) {
    if (!m) return 0;
    std::lock_guard<std::mutex> lk(m->mu);
    return m->generation;
}

size_t frt_matcher_scan_bytes(frt_matcher *m) {
    if (!m) return 0;
    std::lock_guard<std::mutex> lk(m->mu);
    const size_t n = (size_t)m->N, d = (size_t)m->D;
    if (m->screen && m->screen_on) return (m->gal.g8 ? 1 : 2) * n * d;   // the coarse scan reads the shadow copy once per call
    return (m->gal.store16 ? 2 : 4) * n * d;
}

int frt_matcher_init(frt_matcher *m, const float *gallery, int num_row, int num_col) {
    return guarded([&] {
        if (!m || (num_row > 0 && !gallery)) raise(FRT_ERR_INVALID, "MatMul::init: bad argument");
        check_gallery_shape(num_row, num_col);
        std::lock_guard<std::mutex> lk(m->mu);
        use_device(m->device);
        // one path for every gallery load: pinned staging chunks + asynchronous copies (idempotent: the previous device copy is
        // freed at commit - the reference leaks it on every /reload)
        m->load_begin(num_row, num_col);
        try {
            m->load_append(gallery, num_row);
            m->load_commit();
        } catch (...) {
            m->load_abort();
            throw;
        }
    });
}

int frt_matcher_gallery_begin(frt_matcher *m, int row_capacity, int num_col) {
    return guarded([&] {
        if (!m) raise(FRT_ERR_INVALID, "null argument");
        check_gallery_shape(row_capacity, num_col);
        std::lock_guard<std::mutex> lk(m->mu);
        use_device(m->device);
        m->load_begin(row_capacity, num_col);
    });
}

int frt_matcher_gallery_append(frt_matcher *m, const void *rows, int n_rows) {
    return with_gallery(m, [&] {
        m->load_append(reinterpret_cast<const float *>(rows), n_rows);
    });
}

int frt_matcher_gallery_commit(frt_matcher *m) {
    return with_gallery(m, [&] {
        try {
            m->load_commit();
        } catch (...) {
            m->load_abort();
            throw;
        }
    });
}

int frt_matcher_gallery_reserve(frt_matcher *m, int row_capacity) {
    return guarded([&] {
        if (!m || row_capacity < 0 || row_capacity > INT32_MAX - 128) raise(FRT_ERR_INVALID, "gallery_reserve: bad argument");
        std::lock_guard<std::mutex> lk(m->mu);
        use_device(m->device);
        edit_checks(m, "gallery_reserve");
        m->reserve_rows = std::max(m->reserve_rows, row_capacity);
        if (m->N > 0 && row_capacity > m->gal.cap_rows) {  // a live gallery moves now; an empty matcher allocates with its first rows
            m->wait_idle(m->stream);
            grow(m, row_capacity);
            finish_edit(m, m->N);
        }
    });
}

int frt_matcher_gallery_add(frt_matcher *m, const float *rows, int n_rows) {
    return with_gallery(m, [&] {
        add_rows(m, rows, n_rows, false);
    });
}

int frt_matcher_gallery_add_dev(frt_matcher *m, const void *rows_dev, int n_rows) {
    return with_gallery(m, [&] {
        add_rows(m, rows_dev, n_rows, true);
    });
}

int frt_matcher_gallery_add_labeled(frt_matcher *m, const float *rows, const int32_t *labels, int n_rows) {
    return with_gallery(m, [&] {
        add_rows(m, rows, n_rows, false, labels, true);
    });
}

int frt_matcher_gallery_add_labeled_dev(frt_matcher *m, const void *rows_dev, const int32_t *labels, int n_rows) {
    return with_gallery(m, [&] {
        add_rows(m, rows_dev, n_rows, true, labels, true);
    });
}

int frt_matcher_set_labels(frt_matcher *m, const int32_t *labels, int n) {
    return guarded([&] {
        if (!m || n < 0 || (n > 0 && !labels)) raise(FRT_ERR_INVALID, "set_labels: bad argument");
        std::lock_guard<std::mutex> lk(m->mu);
        set_labels(m, labels, n);
    });
}

int frt_matcher_labels_info(frt_matcher *m, int *n_identities, int *max_rows_per_label) {
    return guarded([&] {
        if (!m || !n_identities || !max_rows_per_label) raise(FRT_ERR_INVALID, "labels_info: null argument");
        std::lock_guard<std::mutex> lk(m->mu);
        *n_identities = m->labelled ? (int)m->label_rows.size() : 0;
        *max_rows_per_label = m->labelled ? m->max_rows_per_label : 0;
    });
}

int frt_matcher_build_templates(frt_matcher *src, frt_matcher *dst, int32_t *labels_out, int32_t *n_rows_out, float *min_sim_out, int32_t *min_row_out,
                                float *templates_out) {
    return guarded([&] {
        if (!src) raise(FRT_ERR_INVALID, "build_templates: null source");
        if (src == dst) raise(FRT_ERR_INVALID, "build_templates: source and destination are the same matcher");
        if (dst && dst->device != src->device) raise(FRT_ERR_INVALID, "build_templates: the two matchers are on different devices");
        // both mutexes for the whole call, taken in address order (two concurrent builds over the same pair cannot deadlock)
        frt_matcher *first = src, *second = dst;
        if (dst && std::less<frt_matcher *>()(dst, src)) std::swap(first, second);
        std::unique_lock<std::mutex> lk1(first->mu), lk2;
        if (second) lk2 = std::unique_lock<std::mutex>(second->mu);
        build_templates(src, dst, labels_out, n_rows_out, min_sim_out, min_row_out, templates_out);
    });
}

int frt_matcher_cluster(frt_matcher *m, float threshold, int32_t *labels_out, int install_labels, long long stats_out[4]) {
    return with_gallery(m, [&] {
        cluster_checks(m, threshold);
        long long stats[4] = {0, 0, 0, 0};
        if (m->N > 0) {
            const int N = m->N;
            hipStream_t s = m->stream;
            m->d_cluster_labels.reserve((size_t)N);
            m->d_cluster_stats.reserve(4);
            cluster(m, threshold, m->d_cluster_labels.get(), m->d_cluster_stats.get(), s);
            std::vector<int32_t> own;
            int32_t *labels = labels_out;
            if (!labels && install_labels) {
                own.resize((size_t)N);
                labels = own.data();
            }
            if (labels) HIPCHK(hipMemcpyAsync(labels, m->d_cluster_labels.get(), (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(stats, m->d_cluster_stats.get(), sizeof(stats), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (install_labels) set_labels(m, labels, N);
        }
        for (int i = 0; stats_out && i < 4; ++i) stats_out[i] = stats[i];
    });
}

int frt_matcher_cluster_dev(frt_matcher *m, float threshold, void *labels_dev, void *stats_dev, void *hip_stream) {
    return with_gallery(m, [&] {
        cluster_checks(m, threshold);
        hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
        if (m->N <= 0) {
            if (stats_dev) HIPCHK(hipMemsetAsync(stats_dev, 0, 4 * sizeof(long long), s));
            return;
        }
        if (!labels_dev) raise(FRT_ERR_INVALID, "cluster_dev: null argument");
        long long *stats = reinterpret_cast<long long *>(stats_dev);
        if (!stats) {
            m->d_cluster_stats.reserve(4);
            stats = m->d_cluster_stats.get();
        }
        cluster(m, threshold, reinterpret_cast<int32_t *>(labels_dev), stats, s);
        HIPCHK(hipEventRecord(m->ev_busy, s));  // the caller's stream is still using the scratch
        m->busy = true;
    });
}

int frt_matcher_separation(frt_matcher *m, float *gen_sim_out, int32_t *gen_row_out, float *imp_sim_out, int32_t *imp_row_out, const float *thresholds,
                           int n_thresholds, long long *counts_out, long long stats_out[5]) {
    return with_gallery(m, [&] {
        separation_checks(m, thresholds, n_thresholds);
        long long res[5 + 2 * FRT_SEPARATION_MAX_THRESHOLDS] = {};  // stats | counts
        if (m->N > 0) {
            const size_t N = (size_t)m->N;
            hipStream_t s = m->stream;
            m->d_sep_sim.reserve(2 * N);
            m->d_sep_row.reserve(2 * N);
            m->d_sep_counts.reserve(5 + 2 * FRT_SEPARATION_MAX_THRESHOLDS);
            float *sim = m->d_sep_sim.get();
            int32_t *row = m->d_sep_row.get();
            long long *cnt = m->d_sep_counts.get();
            separation(m, sim, row, sim + N, row + N, thresholds, n_thresholds, cnt + 5, cnt, s);
            if (gen_sim_out) HIPCHK(hipMemcpyAsync(gen_sim_out, sim, N * sizeof(float), hipMemcpyDeviceToHost, s));
            if (gen_row_out) HIPCHK(hipMemcpyAsync(gen_row_out, row, N * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            if (imp_sim_out) HIPCHK(hipMemcpyAsync(imp_sim_out, sim + N, N * sizeof(float), hipMemcpyDeviceToHost, s));
            if (imp_row_out) HIPCHK(hipMemcpyAsync(imp_row_out, row + N, N * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(res, cnt, (5 + 2 * (size_t)n_thresholds) * sizeof(long long), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        for (int i = 0; stats_out && i < 5; ++i) stats_out[i] = res[i];
        for (int i = 0; counts_out && i < 2 * n_thresholds; ++i) counts_out[i] = res[5 + i];
    });
}

int frt_matcher_separation_dev(frt_matcher *m, void *gen_sim_dev, void *gen_row_dev, void *imp_sim_dev, void *imp_row_dev, const float *thresholds,
                               int n_thresholds, void *counts_dev, void *stats_dev, void *hip_stream) {
    return with_gallery(m, [&] {
        separation_checks(m, thresholds, n_thresholds);
        hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
        if (m->N <= 0) {
            if (stats_dev) HIPCHK(hipMemsetAsync(stats_dev, 0, 5 * sizeof(long long), s));
            if (counts_dev && n_thresholds > 0) HIPCHK(hipMemsetAsync(counts_dev, 0, 2 * (size_t)n_thresholds * sizeof(long long), s));
            return;
        }
        // what the caller did not ask for still feeds the reduction: it goes to the matcher's own buffers
        const size_t N = (size_t)m->N;
        if (!gen_sim_dev || !imp_sim_dev) m->d_sep_sim.reserve(2 * N);
        if (!gen_row_dev || !imp_row_dev) m->d_sep_row.reserve(2 * N);
        if (!counts_dev || !stats_dev) m->d_sep_counts.reserve(5 + 2 * FRT_SEPARATION_MAX_THRESHOLDS);
        float *gs = gen_sim_dev ? reinterpret_cast<float *>(gen_sim_dev) : m->d_sep_sim.get();
        float *is = imp_sim_dev ? reinterpret_cast<float *>(imp_sim_dev) : m->d_sep_sim.get() + N;
        int32_t *gr = gen_row_dev ? reinterpret_cast<int32_t *>(gen_row_dev) : m->d_sep_row.get();
        int32_t *ir = imp_row_dev ? reinterpret_cast<int32_t *>(imp_row_dev) : m->d_sep_row.get() + N;
        long long *stats = stats_dev ? reinterpret_cast<long long *>(stats_dev) : m->d_sep_counts.get();
        long long *counts = counts_dev ? reinterpret_cast<long long *>(counts_dev) : m->d_sep_counts.get() + 5;
        separation(m, gs, gr, is, ir, thresholds, n_thresholds, counts, stats, s);
        HIPCHK(hipEventRecord(m->ev_busy, s));  // the caller's stream is still using the scratch
        m->busy = true;
    });
}

int frt_matcher_gallery_remove(frt_matcher *m, const int32_t *idx, int n_idx) {
    return with_gallery(m, [&] {
        remove_rows(m, idx, n_idx);
    });
}

int frt_matcher_edit_stats(frt_matcher *m, long out[4]) {
    return guarded([&] {
        if (!m || !out) raise(FRT_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(m->mu);
        for (int i = 0; i < 4; ++i) out[i] = m->edit_stats[i];
    });
}

int frt_matcher_num_rows(const frt_matcher *m) { return m ? m->N : 0; }

int frt_matcher_set_row_offset(frt_matcher *m, int row_offset) {
    return guarded([&] {
        if (!m || row_offset < 0) raise(FRT_ERR_INVALID, "set_row_offset: bad argument");
        std::lock_guard<std::mutex> lk(m->mu);
        m->row_offset = row_offset;
        ++m->generation;
    });
}

int frt_matcher_calculate(frt_matcher *m, const float *embeds, int embed_count, float *outputs) {
    return guarded([&] {
        if (!m || !embeds || !outputs) raise(FRT_ERR_INVALID, "MatMul::calculate: null argument");
        std::lock_guard<std::mutex> lk(m->mu);
        hipStream_t s = upload_queries(m, embeds, embed_count);
        full_matrix_to_host(m, embed_count, outputs, s);
        sync_stream_spinning(s);
    });
}

int frt_matcher_calculate_top1(frt_matcher *m, const float *embeds, int embed_count, float *outputs, int32_t *idx_out, float *sim_out) {
    return guarded([&] {
        if (!m || !embeds || !idx_out || !sim_out) raise(FRT_ERR_INVALID, "calculate_top1: null argument");
        search_to_host(m, embeds, embed_count, false, 1, idx_out, sim_out, outputs);
    });
}

int frt_pinned_alloc(size_t bytes, int device, void **out) {
    return guarded([&] {
        if (!out) raise(FRT_ERR_INVALID, "null argument");
        *out = nullptr;
        if (device >= 0) use_device(device);
        *out = PinnedMem::alloc(bytes ? bytes : 1);
    });
}

void frt_pinned_free(void *p) {
    if (p) PinnedMem::free(p);
}

int frt_matcher_top1(frt_matcher *m, const float *embeds, int embed_count, int32_t *idx_out, float *sim_out) {
    return guarded([&] {
        if (!m || !embeds || !idx_out || !sim_out) raise(FRT_ERR_INVALID, "top1: null argument");
        search_to_host(m, embeds, embed_count, false, 1, idx_out, sim_out);
    });
}

/* device-resident queries (sharded-gallery path, dist.py: the all-gathered embeddings never visit the host) */
int frt_matcher_top1_dev(frt_matcher *m, const void *embeds_dev, int embed_count, void *idx_dev, void *sim_dev, void *hip_stream) {
    return guarded([&] {
        if (!m || !embeds_dev || !idx_dev || !sim_dev) raise(FRT_ERR_INVALID, "top1_dev: null argument");
        std::lock_guard<std::mutex> lk(m->mu);
        search_dev(m, embeds_dev, 0, embed_count, hip_stream, [&](const float *q, hipStream_t s) {
            m->top1_dev(q, embed_count, reinterpret_cast<int32_t *>(idx_dev), reinterpret_cast<float *>(sim_dev), s);
        });
    });
}

int frt_merge_top1(int n, const int32_t *idx_a, const float *sim_a, const int32_t *idx_b, const float *sim_b, int32_t *idx_out, float *sim_out) {
    return guarded([&] {
        if (n < 0 || !idx_a || !sim_a || !idx_b || !sim_b || !idx_out || !sim_out) raise(FRT_ERR_INVALID, "merge: bad argument");
        for (int i = 0; i < n; ++i) {
            const bool a_ok = idx_a[i] >= 0, b_ok = idx_b[i] >= 0;
            bool take_b = false;
            if (!a_ok)
                take_b = b_ok;
            else if (b_ok)
                take_b = (sim_b[i] > sim_a[i]) || (sim_b[i] == sim_a[i] && idx_b[i] < idx_a[i]);
            idx_out[i] = take_b ? idx_b[i] : idx_a[i];
            sim_out[i] = take_b ? sim_b[i] : sim_a[i];
        }
    });
}

static void check_k(int k) {
    if (k < 1 || k > match_topk_max() || k > frt_matcher::KCAP) raise(FRT_ERR_INVALID, "top-k: k must be in 1..16");
}

int frt_matcher_topk(frt_matcher *m, const float *embeds, int embed_count, int k, int32_t *idx_out, float *sim_out) {
    return guarded([&] {
        if (!m || !embeds || !idx_out || !sim_out) raise(FRT_ERR_INVALID, "topk: null argument");
        check_k(k);
        search_to_host(m, embeds, embed_count, true, k, idx_out, sim_out);
    });
}

int frt_matcher_topk_dev(frt_matcher *m, const void *embeds_dev, int embeds_fp16, int embed_count, int k, void *idx_dev, void *sim_dev, void *hip_stream) {
    return guarded([&] {
        if (!m || !embeds_dev || !idx_dev || !sim_dev) raise(FRT_ERR_INVALID, "topk_dev: null argument");
        check_k(k);
        std::lock_guard<std::mutex> lk(m->mu);
        search_dev(m, embeds_dev, embeds_fp16, embed_count, hip_stream, [&](const float *q, hipStream_t s) {
            m->topk_dev(q, embed_count, k, reinterpret_cast<int32_t *>(idx_dev), reinterpret_cast<float *>(sim_dev), s);
        });
    });
}

int frt_matcher_topk_labels(frt_matcher *m, const float *embeds, int embed_count, int k, int32_t *label_out, int32_t *idx_out, float *sim_out) {
    return guarded([&] {
        if (!m || !embeds || !label_out || !idx_out || !sim_out) raise(FRT_ERR_INVALID, "topk_labels: null argument");
        check_k(k);
        search_to_host(m, embeds, embed_count, true, k, idx_out, sim_out, nullptr, label_out);
    });
}

int frt_matcher_topk_labels_dev(frt_matcher *m, const void *embeds_dev, int embeds_fp16, int embed_count, int k, void *label_dev, void *idx_dev, void *sim_dev,
                                void *hip_stream) {
    return guarded([&] {
        if (!m || !embeds_dev || !label_dev || !idx_dev || !sim_dev) raise(FRT_ERR_INVALID, "topk_labels_dev: null argument");
        check_k(k);
        std::lock_guard<std::mutex> lk(m->mu);
        check_labelled(m);
        search_dev(m, embeds_dev, embeds_fp16, embed_count, hip_stream, [&](const float *q, hipStream_t s) {
            m->topk_labels_dev(q, embed_count, k, reinterpret_cast<int32_t *>(label_dev), reinterpret_cast<int32_t *>(idx_dev), reinterpret_cast<float *>(sim_dev), s);
        });
    });
}

int frt_merge_topk_labels(int shards, int n, int k, const int32_t *label_all, const int32_t *idx_all, const float *sim_all, int32_t *label_out,
                          int32_t *idx_out, float *sim_out) {
    return guarded([&] {
        if (shards < 1 || n < 0 || k < 1 || !label_all || !idx_all || !sim_all || !label_out || !idx_out || !sim_out)
            raise(FRT_ERR_INVALID, "merge_topk_labels: bad argument");
        std::vector<size_t> ent;  // the query's occupied entries in the result order; the first of every label is kept
        for (int q = 0; q < n; ++q) {
            ent.clear();
            for (int sh = 0; sh < shards; ++sh)
                for (int j = 0; j < k; ++j) {
                    const size_t e = ((size_t)sh * n + q) * k + j;
                    if (idx_all[e] >= 0) ent.push_back(e);
                }
            std::sort(ent.begin(), ent.end(), [&](size_t a, size_t b) { return sim_all[a] > sim_all[b] || (sim_all[a] == sim_all[b] && idx_all[a] < idx_all[b]); });
            int o = 0;
            for (size_t e : ent) {
                if (o == k) break;
                bool taken = false;
                for (int t = 0; t < o; ++t) taken = taken || label_out[(size_t)q * k + t] == label_all[e];
                if (taken) continue;
                label_out[(size_t)q * k + o] = label_all[e];
                idx_out[(size_t)q * k + o] = idx_all[e];
                sim_out[(size_t)q * k + o] = sim_all[e];
                ++o;
            }
            for (; o < k; ++o) {
                label_out[(size_t)q * k + o] = -1;
                idx_out[(size_t)q * k + o] = -1;
                sim_out[(size_t)q * k + o] = -INFINITY;
            }
        }
    });
}

int frt_merge_topk_labels_dev(int shards, int n, int k, const void *label_all_dev, const void *idx_all_dev, const void *sim_all_dev, void *label_out_dev,
                              void *idx_out_dev, void *sim_out_dev, void *hip_stream) {
    return guarded([&] {
        if (shards < 1 || n < 0 || k < 1 || !label_all_dev || !idx_all_dev || !sim_all_dev || !label_out_dev || !idx_out_dev || !sim_out_dev)
            raise(FRT_ERR_INVALID, "merge_topk_labels_dev: bad argument");
        if (n == 0) return;
        launch_merge_topk_labels(reinterpret_cast<const int32_t *>(label_all_dev), reinterpret_cast<const int32_t *>(idx_all_dev),
                                 reinterpret_cast<const float *>(sim_all_dev), shards, n, k, reinterpret_cast<int32_t *>(label_out_dev),
                                 reinterpret_cast<int32_t *>(idx_out_dev), reinterpret_cast<float *>(sim_out_dev), reinterpret_cast<hipStream_t>(hip_stream));
        HIPCHK(hipGetLastError());
    });
}

int frt_merge_topk(int shards, int n, int k, const int32_t *idx_all, const float *sim_all, int32_t *idx_out, float *sim_out) {
    return guarded([&] {
        if (shards < 1 || n < 0 || k < 1 || !idx_all || !sim_all || !idx_out || !sim_out) raise(FRT_ERR_INVALID, "merge_topk: bad argument");
        std::vector<int> pos((size_t)shards);
        for (int q = 0; q < n; ++q) {
            std::fill(pos.begin(), pos.end(), 0);
            for (int o = 0; o < k; ++o) {
                int best = -1, bi = 0;
                float bv = 0.f;
                for (int sh = 0; sh < shards; ++sh) {
                    while (pos[(size_t)sh] < k && idx_all[((size_t)sh * n + q) * k + pos[(size_t)sh]] < 0) ++pos[(size_t)sh];  // empty slots
                    if (pos[(size_t)sh] >= k) continue;
                    const size_t e = ((size_t)sh * n + q) * k + pos[(size_t)sh];
                    const float v = sim_all[e];
                    const int i = idx_all[e];
                    if (best < 0 || v > bv || (v == bv && i < bi)) {
                        best = sh;
                        bv = v;
                        bi = i;
                    }
                }
                if (best < 0) {
                    idx_out[(size_t)q * k + o] = -1;
                    sim_out[(size_t)q * k + o] = -INFINITY;
                } else {
                    idx_out[(size_t)q * k + o] = bi;
                    sim_out[(size_t)q * k + o] = bv;
                    ++pos[(size_t)best];
                }
            }
        }
    });
}

int frt_merge_topk_dev(int shards, int n, int k, const void *idx_all_dev, const void *sim_all_dev, void *idx_out_dev, void *sim_out_dev, void *hip_stream) {
    return guarded([&] {
        if (shards < 1 || n < 0 || k < 1 || !idx_all_dev || !sim_all_dev || !idx_out_dev || !sim_out_dev) raise(FRT_ERR_INVALID, "merge_topk_dev: bad argument");
        if (n == 0) return;
        launch_merge_topk(reinterpret_cast<const int32_t *>(idx_all_dev), reinterpret_cast<const float *>(sim_all_dev), shards, n, k,
                          reinterpret_cast<int32_t *>(idx_out_dev), reinterpret_cast<float *>(sim_out_dev), reinterpret_cast<hipStream_t>(hip_stream));
        HIPCHK(hipGetLastError());
    });
}

int frt_embeds_to_half_dev(const void *embeds_dev, size_t n_values, void *half_out_dev, void *hip_stream) {
    return guarded([&] {
        if (!embeds_dev || !half_out_dev || n_values % 8) raise(FRT_ERR_INVALID, "embeds_to_half: bad argument (n_values must be a multiple of 8)");
        if (n_values == 0) return;
        launch_float_to_half(reinterpret_cast<const float *>(embeds_dev), (long)n_values, reinterpret_cast<half_t *>(half_out_dev),
                             reinterpret_cast<hipStream_t>(hip_stream));
        HIPCHK(hipGetLastError());
    });
}


}  // extern "C"
