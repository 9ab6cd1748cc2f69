// Drop-in for /root/reference/src/matmul.h: class MatMul with the same public surface (src/matmul.h:17-21).
//   C = B x A^T : A = knownEmbeds [numRow x numCol] row-major (resident on the GPU), B = embeds [embedCount x numCol],
//   outputs[i*numRow + j] = <B_i, A_j>   (src/matmul.h:7-16)
#ifndef FRT_MATMUL_H
#define FRT_MATMUL_H

#include "common.h"

class MatMul {
  public:
    MatMul() : h_(nullptr), device_(0) {}
    explicit MatMul(int device) : h_(nullptr), device_(device) {}
    ~MatMul() { frt_matcher_destroy(h_); }
    MatMul(const MatMul &) = delete;
    MatMul &operator=(const MatMul &) = delete;

    void init(float *knownEmbeds, int numRow, int numCol) {
        ensure();
        checkFrtStatus(frt_matcher_init(h_, knownEmbeds, numRow, numCol));
    }
    void calculate(float *embeds, int embedCount, float *outputs) {
        ensure();
        checkFrtStatus(frt_matcher_calculate(h_, embeds, embedCount, outputs));
    }
    // Extension: calculate + the row-wise first maximum (what getOutputs computes from the matrix) in one call; outputs may be null
    void calculateTop1(float *embeds, int embedCount, float *outputs, int *idx, float *sim) {
        ensure();
        checkFrtStatus(frt_matcher_calculate_top1(h_, embeds, embedCount, outputs, idx, sim));
    }
    int device() const { return device_; }
    // Extension: streaming load (== initKnownEmbeds / addEmbedding x n / initMatMul without a host copy of the gallery): rows go
    // through pinned staging chunks to the device while the caller fetches the next ones (src/db.cpp:316-346)
    void galleryBegin(int rowCapacity, int numCol) {
        ensure();
        checkFrtStatus(frt_matcher_gallery_begin(h_, rowCapacity, numCol));
    }
    void galleryAppend(const float *rows, int n) { checkFrtStatus(frt_matcher_gallery_append(h_, rows, n)); }
    void galleryCommit() { checkFrtStatus(frt_matcher_gallery_commit(h_)); }
    int numRows() const { return frt_matcher_num_rows(h_); }
    // Extension: live edits of the gallery the object is answering from (frt_matcher_gallery_reserve / _add / _add_dev / _remove): no reload,
    // the rows already on the device stay there.  galleryAdd appends (new indices numRows() ...), galleryRemove closes the gaps in order.
    void galleryReserve(int rowCapacity) {
        ensure();
        checkFrtStatus(frt_matcher_gallery_reserve(h_, rowCapacity));
    }
    void galleryAdd(const float *rows, int n) {
        ensure();
        checkFrtStatus(frt_matcher_gallery_add(h_, rows, n));
    }
    void galleryAddDev(const void *rowsDev, int n) {
        ensure();
        checkFrtStatus(frt_matcher_gallery_add_dev(h_, rowsDev, n));
    }
    void galleryRemove(const int *rows, int n) {
        ensure();
        checkFrtStatus(frt_matcher_gallery_remove(h_, rows, n));
    }
    // Extension: identities (frt.h "Top-k over IDENTITIES").  One label >= 0 per row; topkLabels then returns, per query, the k best
    // IDENTITIES with the best row of each: labels / idx / sim are [embedCount x k], unused slots -1 / -1 / -inf.  init and galleryCommit
    // drop the labels; galleryRemove closes them up with the rows; a labelled gallery grows through galleryAddLabeled[Dev] only.
    void setLabels(const int *labels, int n) {
        ensure();
        checkFrtStatus(frt_matcher_set_labels(h_, labels, n));
    }
    void labelsInfo(int &identities, int &maxRowsPerLabel) {
        ensure();
        checkFrtStatus(frt_matcher_labels_info(h_, &identities, &maxRowsPerLabel));
    }
    void galleryAddLabeled(const float *rows, const int *labels, int n) {
        ensure();
        checkFrtStatus(frt_matcher_gallery_add_labeled(h_, rows, labels, n));
    }
    void galleryAddLabeledDev(const void *rowsDev, const int *labels, int n) {
        ensure();
        checkFrtStatus(frt_matcher_gallery_add_labeled_dev(h_, rowsDev, labels, n));
    }
    void topkLabels(const float *embeds, int embedCount, int k, int *labels, int *idx, float *sim) {
        ensure();
        checkFrtStatus(frt_matcher_topk_labels(h_, embeds, embedCount, k, labels, idx, sim));
    }
    // Extension: the template gallery (frt.h "Template gallery"): one row per identity of this labelled gallery - the re-normalised sum of
    // its rows - built on the device.  dst (may be null: an audit only) is replaced by the templates, labelled, in its own storage mode, and
    // is then matched like any gallery: its rows are persons.  labels / nRows / minSim / minRow are [identities] (labelsInfo), templates
    // [identities x numCol]; any of them may be null.  minRow names the row that agrees least with its own identity's template.
    void buildTemplates(MatMul *dst, int *labels = nullptr, int *nRows = nullptr, float *minSim = nullptr, int *minRow = nullptr, float *templates = nullptr) {
        ensure();
        checkFrtStatus(frt_matcher_build_templates(h_, dst ? dst->handle() : nullptr, labels, nRows, minSim, minRow, templates));
    }
    // Extension: group the rows into persons without any labels (frt.h "Group an UNLABELLED gallery"): single-linkage clustering on the
    // device at a similarity threshold.  labels[i] = the smallest row of i's component (rows i, j are joined iff their exact similarity is
    // >= threshold); stats (may be null) = clusters, joined pairs, screened chunks, dense chunks.  install: the labels become the gallery's
    // own, as setLabels(labels) would make them - photo dump -> cluster(t, labels, true) -> buildTemplates(&persons) never leaves the device.
    void cluster(float threshold, std::vector<int> &labels, bool install = false, long long *stats = nullptr) {
        ensure();
        labels.assign((size_t)numRows(), 0);
        checkFrtStatus(frt_matcher_cluster(h_, threshold, labels.empty() ? nullptr : labels.data(), install ? 1 : 0, stats));
    }
    // Extension: how well the labels separate (frt.h "Leave-one-out genuine / impostor scores"): for every row the best OTHER row of its own
    // label (genSim / genRow) and the best row of any other label (impSim / impRow) by the exact similarity, -inf / -1 without a candidate.
    // thresholds (at most 64): counts (may be null) becomes [thresholds.size() x 2] = rows with genSim < t | rows with impSim >= t.  stats
    // (may be null) = rows with a genuine candidate, with an impostor candidate, with impSim >= genSim, screened chunks, exact chunks.  The
    // largest impSim is the threshold above which cluster() merges no two labels.
    void separation(std::vector<float> &genSim, std::vector<int> &genRow, std::vector<float> &impSim, std::vector<int> &impRow,
                    const std::vector<float> &thresholds = std::vector<float>(), std::vector<long long> *counts = nullptr, long long *stats = nullptr) {
        ensure();
        const size_t n = (size_t)numRows();
        genSim.assign(n, 0.f);
        impSim.assign(n, 0.f);
        genRow.assign(n, -1);
        impRow.assign(n, -1);
        if (counts) counts->assign(thresholds.size() * 2, 0);
        checkFrtStatus(frt_matcher_separation(h_, n ? genSim.data() : nullptr, n ? genRow.data() : nullptr, n ? impSim.data() : nullptr,
                                              n ? impRow.data() : nullptr, thresholds.empty() ? nullptr : thresholds.data(), (int)thresholds.size(),
                                              (counts && !counts->empty()) ? counts->data() : nullptr, stats));
    }
    void topk(const float *embeds, int embedCount, int k, int *idx, float *sim) {
        ensure();
        checkFrtStatus(frt_matcher_topk(h_, embeds, embedCount, k, idx, sim));
    }
    // Extension: store the gallery rows as fp16 on the device (next init / galleryBegin); see frt_matcher_set_storage
    void setStorageFp16(bool on) {
        ensure();
        checkFrtStatus(frt_matcher_set_storage(h_, on ? 1 : 0));
    }
    // Extension: exact fp32 scan on every top-1 call instead of the screened one (same answers; see frt_matcher_set_screening)
    void setScreening(bool on) {
        ensure();
        checkFrtStatus(frt_matcher_set_screening(h_, on ? 1 : 0));
    }
    // Extension: fused argmax (what ArcFaceIR50::getOutputs computes from the full matrix), never materialises [n x numRow].
    void top1(float *embeds, int embedCount, int *idx, float *sim) {
        ensure();
        checkFrtStatus(frt_matcher_top1(h_, embeds, embedCount, idx, sim));
    }
    frt_matcher *handle() {
        ensure();
        return h_;
    }

  private:
    void ensure() {  // the reference constructs the cuBLASLt handle in the ctor; lazily here so a MatMul member costs nothing until used
        if (!h_) checkFrtStatus(frt_matcher_create(device_, &h_));
    }
    frt_matcher *h_;
    int device_;
};

using CosineSimilarityCalculator = MatMul;  // the name BASELINE.json:north_star uses for this class

#endif  // FRT_MATMUL_H
