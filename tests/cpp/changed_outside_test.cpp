// changed_outside (check_common.hpp), the count every guard and margin check of the launch-alone programs rests on, on host arrays: no device.
// Prints one line per failed expectation and exits 1 if there was one.  tests/test_check_common.py runs it.
#define CHECK_PROGRAM "changed_outside_test"
#include "check_common.hpp"

int main() {
    using check::changed_outside;
    int bad = 0;
    auto expect = [&](const char *what, size_t got, size_t want) {
        if (got != want) printf("%s: %zu, expected %zu\n", what, got, want), ++bad;
    };
    constexpr size_t F = 5, L = 7, B = 3;  // front margin, logical range, back margin
    constexpr uint16_t fill = 0x5a5a;
    const std::vector<uint16_t> clean(F + L + B, fill);
    expect("clean", changed_outside(clean.data(), clean.size(), F, L, fill), 0);
    // one changed element at each end of each margin is counted; the first and the last logical element are not
    for (size_t i : {(size_t)0, F - 1, F + L, F + L + B - 1}) {
        std::vector<uint16_t> h = clean;
        h[i] ^= 1;
        expect("one margin element", changed_outside(h.data(), h.size(), F, L, fill), 1);
    }
    std::vector<uint16_t> h = clean;
    h[F] = h[F + L - 1] = 0;
    expect("first and last logical element", changed_outside(h.data(), h.size(), F, L, fill), 0);
    h[F - 1] = h[F + L] = 0;
    expect("both neighbours of the logical range", changed_outside(h.data(), h.size(), F, L, fill), 2);
    // a zero-length logical range: every element is outside
    h = clean;
    h[F] = 0;
    expect("zero-length range", changed_outside(h.data(), h.size(), F, 0, fill), 1);
    expect("zero-length range at 0, nothing held", changed_outside(clean.data(), clean.size(), 0, 0, (uint16_t)0), clean.size());
    // front only: the logical range ends the array, or slack follows it
    const std::vector<char> bytes(F + L, 0x5a);
    std::vector<char> g = bytes;
    g[F + L - 1] = 0;
    expect("front only, last logical byte", changed_outside(g.data(), g.size(), F, L, (char)0x5a), 0);
    g[0] = g[F - 1] = 1;
    expect("front only, both ends of the margin", changed_outside(g.data(), g.size(), F, L, (char)0x5a), 2);
    g = bytes;
    g[F + L - 1] = 0;
    expect("front only, slack behind a shorter range", changed_outside(g.data(), g.size(), F, L - 1, (char)0x5a), 1);
    if (!bad) printf("ok\n");
    return bad != 0;
}
