// Order-preserving removal of gallery rows: the map from a row of the compacted gallery to the row it comes from.
// Plain C++ (host and device): no HIP types, so the host-only test (tests/cpp/hole_map_test.cpp) includes it as it is.
//
// holes = the removed row indices, sorted and distinct.  Row j of the compacted gallery is old row j + c(j), c(j) = the number of holes
// in front of it = the number of i with holes[i] - i <= j.  The keys holes[i] - i never decrease, so c(j) is one binary search.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FRT_HOLES_HD __host__ __device__
#else
#define FRT_HOLES_HD
#endif

// number of keys[lo .. hi) that are <= j, plus lo (the caller narrows [lo, hi) to the keys that can matter for its rows)
FRT_HOLES_HD inline int frt_holes_before(const int *keys, int lo, int hi, int j) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] <= j) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
FRT_HOLES_HD inline int frt_hole_source_row(const int *keys, int lo, int hi, int j) { return j + frt_holes_before(keys, lo, hi, j); }

#include <algorithm>
#include <vector>
// idx[n] (any order, duplicates count once) -> keys; false (keys untouched) when an index lies outside [0, N)
inline bool frt_hole_keys(const int32_t *idx, int n, int N, std::vector<int> &keys) {
    for (int i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= N) return false;
    std::vector<int> h(idx, idx + n);
    std::sort(h.begin(), h.end());
    h.erase(std::unique(h.begin(), h.end()), h.end());
    for (size_t i = 0; i < h.size(); ++i) h[i] -= (int)i;
    keys.swap(h);
    return true;
}
