// Host-only check of the removal map of frt_matcher_gallery_remove (csrc/frt_holes.h): for seeded random hole sets, every row of the
// compacted gallery must come from the row an order-preserving erase leaves there, with the search narrowed per chunk as the library does.
#include <cstdio>
#include <cstdlib>
#include <numeric>

#include "frt_holes.h"

static unsigned long long rng_state = 12345;
static unsigned rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(rng_state >> 33);
}

int main() {
    long checked = 0;
    for (int trial = 0; trial < 400; ++trial) {
        const int N = 1 + (int)(rnd() % 3000);
        int n_idx = (int)(rnd() % 5) == 0 ? N + (int)(rnd() % 50) : (int)(rnd() % (unsigned)(N / 4 + 2));
        if (trial == 0) n_idx = 0;
        std::vector<int32_t> idx((size_t)n_idx);
        for (int &v : idx) v = (int32_t)(rnd() % (unsigned)N);  // duplicates on purpose
        std::vector<int> keys;
        if (!frt_hole_keys(idx.data(), n_idx, N, keys)) return 1;
        // the model: erase, keeping the order
        std::vector<char> gone((size_t)N, 0);
        for (int v : idx) gone[(size_t)v] = 1;
        std::vector<int> want;
        for (int i = 0; i < N; ++i)
            if (!gone[(size_t)i]) want.push_back(i);
        if (keys.size() + want.size() != (size_t)N) return 2;
        const int nk = (int)keys.size(), chunk = 1 + (int)(rnd() % 700);
        for (int a = 0; a < (int)want.size(); a += chunk) {
            const int b = std::min(a + chunk, (int)want.size());
            const int lo = (int)(std::lower_bound(keys.begin(), keys.end(), a) - keys.begin());
            const int hi = (int)(std::upper_bound(keys.begin(), keys.end(), b - 1) - keys.begin());
            for (int j = a; j < b; ++j, ++checked) {
                if (frt_hole_source_row(keys.data(), lo, hi, j) != want[(size_t)j]) return 3;
                if (frt_hole_source_row(keys.data(), 0, nk, j) != want[(size_t)j]) return 4;
            }
        }
    }
    // rejected lists leave the keys alone
    std::vector<int> keys(1, 77);
    const int32_t bad1[2] = {3, 10}, bad2[1] = {-1};
    if (frt_hole_keys(bad1, 2, 10, keys) || frt_hole_keys(bad2, 1, 10, keys) || keys.size() != 1 || keys[0] != 77) return 5;
    std::printf("hole map ok %ld\n", checked);
    return 0;
}
