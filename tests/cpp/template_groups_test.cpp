// frt_template_groups (csrc/frt_templates.hpp), compiled for the host alone: seeded label arrays against a brute-force grouping.
// Identities are numbered by the lowest row that carries the label; the rows of an identity ascend.  Prints "template groups ok <cases>".
#include <cstdio>
#include <cstdlib>

#include "frt_templates.hpp"

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() {  // xorshift64*: the same arrays on every run
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return (unsigned)((g_state * 0x2545F4914F6CDD1Dull) >> 33);
}

static int check(const std::vector<int32_t> &labels, const char *what) {
    const int n = (int)labels.size();
    // brute force: walk the rows, a label not seen before opens the next identity; its rows are collected by a scan per identity
    std::vector<int32_t> want_label;
    for (int r = 0; r < n; ++r) {
        bool seen = false;
        for (size_t i = 0; i < want_label.size(); ++i) seen = seen || want_label[i] == labels[(size_t)r];
        if (!seen) want_label.push_back(labels[(size_t)r]);
    }
    std::vector<int> want_off(1, 0), want_rows;
    for (size_t i = 0; i < want_label.size(); ++i) {
        for (int r = 0; r < n; ++r)
            if (labels[(size_t)r] == want_label[i]) want_rows.push_back(r);
        want_off.push_back((int)want_rows.size());
    }
    std::vector<int32_t> got_label(3, 77);  // stale contents must not survive
    std::vector<int> got_off(5, 77), got_rows(2, 77);
    frt_template_groups(n ? labels.data() : NULL, n, got_label, got_off, got_rows);
    if (got_label != want_label || got_off != want_off || got_rows != want_rows) {
        std::printf("MISMATCH in %s (n = %d, identities %d / %d)\n", what, n, (int)got_label.size(), (int)want_label.size());
        return 1;
    }
    return 0;
}

int main() {
    int bad = 0, cases = 0;
    for (int trial = 0; trial < 40; ++trial) {
        const int n = 1 + (int)(rnd() % 700), ids = 1 + (int)(rnd() % 90);
        std::vector<int32_t> l((size_t)n);
        for (int r = 0; r < n; ++r) l[(size_t)r] = (int32_t)(rnd() % (unsigned)ids);  // interleaved identities
        bad += check(l, "interleaved");
        for (int r = 0; r < n; ++r) l[(size_t)r] = (int32_t)(2147483647LL - (long long)(rnd() % (unsigned)ids) * 24000000LL);  // large sparse values, INT32_MAX among them
        bad += check(l, "large sparse labels");
        cases += 2;
    }
    bad += check(std::vector<int32_t>(257, 5), "one identity holds all rows");
    std::vector<int32_t> distinct(300);
    for (int r = 0; r < 300; ++r) distinct[(size_t)r] = 299 - r;  // all distinct, descending values: the order is by row, not by value
    bad += check(distinct, "all labels distinct");
    bad += check(std::vector<int32_t>(), "no rows");
    std::vector<int32_t> blocks;
    for (int i = 0; i < 9; ++i) blocks.insert(blocks.end(), (size_t)(1 + i), (int32_t)(1000 - i));  // contiguous blocks of growing size
    bad += check(blocks, "contiguous blocks");
    cases += 4;
    if (bad) return 1;
    std::printf("template groups ok %d\n", cases);
    return 0;
}
