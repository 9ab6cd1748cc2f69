// Grouping of a labelled gallery's rows by identity, for the template build (include/frt.h, frt_matcher_build_templates).
// Plain C++ (no HIP types), so the host-only test (tests/cpp/template_groups_test.cpp) includes it as it is.
//
// labels[n] (any int32 values) -> identities numbered in FIRST-APPEARANCE order (by the lowest row that carries the label):
//   ident_label[I]   the label of identity i
//   off[I + 1]       identity i owns rows[off[i] .. off[i + 1])
//   rows[n]          row indices, ascending inside every identity
// One pass for the label range, one counting pass and one filling pass; the rows of an identity come out ascending because the filling
// pass walks the rows in order.
#pragma once
#include <stdint.h>

#include <unordered_map>
#include <vector>

inline void frt_template_groups(const int32_t *labels, int n, std::vector<int32_t> &ident_label, std::vector<int> &off, std::vector<int> &rows) {
    // label -> identity: a table indexed by label - lo where the labels are dense enough for one of at most 4 n + 1024 entries (interned
    // labels 0 .. I - 1 are), a hash map otherwise.  A million labels group in a few milliseconds through the table, in tens through the map.
    int32_t lo = 0, hi = 0;
    for (int r = 0; r < n; ++r) {
        lo = (r == 0 || labels[r] < lo) ? labels[r] : lo;
        hi = (r == 0 || labels[r] > hi) ? labels[r] : hi;
    }
    const bool dense = (int64_t)hi - lo < (int64_t)4 * n + 1024;
    std::vector<int> table(dense && n > 0 ? (size_t)((int64_t)hi - lo + 1) : 0, -1);
    std::unordered_map<int32_t, int> map;
    std::vector<int> of_row((size_t)(n > 0 ? n : 0));
    ident_label.clear();
    off.assign(1, 0);
    for (int r = 0; r < n; ++r) {
        int *slot;
        if (dense) {
            slot = &table[(size_t)((int64_t)labels[r] - lo)];
        } else {
            slot = &map.insert(std::make_pair(labels[r], -1)).first->second;
        }
        if (*slot < 0) {  // the label's first row opens the next identity
            *slot = (int)ident_label.size();
            ident_label.push_back(labels[r]);
            off.push_back(0);
        }
        of_row[(size_t)r] = *slot;
        ++off[(size_t)*slot + 1];  // counts for now
    }
    for (size_t i = 1; i < off.size(); ++i) off[i] += off[i - 1];
    std::vector<int> next(off.begin(), off.end() - 1);
    rows.assign(of_row.size(), 0);
    for (int r = 0; r < n; ++r) rows[(size_t)next[(size_t)of_row[(size_t)r]]++] = r;
}
