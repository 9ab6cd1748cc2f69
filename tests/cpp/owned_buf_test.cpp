// Owned<T, Mem> (csrc/frt_owned.hpp) on a counting malloc policy that can be told to throw on the k-th allocation.  Host only; built with
// ASan + UBSan by tests/test_templates_abi.py, so a double free, a use after free or a leak ends the run on its own.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>

#include "frt_owned.hpp"

namespace {

int g_allocs = 0, g_frees = 0, g_throw_at = 0;  // g_throw_at: the g_allocs value at which alloc throws (0 = never)

struct CountingMem {
    static void *alloc(size_t bytes) {
        if (++g_allocs == g_throw_at) throw std::bad_alloc();
        return std::malloc(bytes ? bytes : 1);
    }
    static void free(void *p) {
        ++g_frees;
        std::free(p);
    }
};
using Buf = Owned<int, CountingMem>;

int live() { return g_allocs - g_frees - (g_throw_at && g_allocs >= g_throw_at ? 1 : 0); }  // (a thrown allocation handed out no block)

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

}  // namespace

int main() {
    {
        Buf b;
        CHECK(!b && b.get() == nullptr && b.capacity() == 0);
        b.reserve(0);
        CHECK(g_allocs == 0 && !b);
        b.reserve(100);
        CHECK(b && b.capacity() == 100 && g_allocs == 1 && g_frees == 0);
        std::memset(b.get(), 0x5a, 100 * sizeof(int));  // (all 100 elements are there: ASan would say otherwise)
        // below and at the capacity: nothing is allocated and the pointer stays
        int *p = b.get();
        b.reserve(1);
        b.reserve(100);
        CHECK(b.get() == p && b.capacity() == 100 && g_allocs == 1 && g_frees == 0);
        // above: exactly one free and one allocation
        b.reserve(101);
        CHECK(b.capacity() == 101 && g_allocs == 2 && g_frees == 1 && live() == 1);
        b.get()[100] = 7;
        // a throwing allocation leaves an empty buffer and no live block
        g_throw_at = 3;
        bool thrown = false;
        try {
            b.reserve(1000);
        } catch (const std::bad_alloc &) {
            thrown = true;
        }
        CHECK(thrown && b.get() == nullptr && b.capacity() == 0 && !b && g_frees == 2 && live() == 0);
        b.reset();  // (of an empty buffer: nothing to free)
        CHECK(g_frees == 2);
        b.reserve(10);  // usable again after the failure
        CHECK(b && b.capacity() == 10 && live() == 1);
    }
    CHECK(live() == 0);
    {
        // move construction leaves the source empty
        Buf a;
        a.reserve(8);
        int *pa = a.get();
        const int frees = g_frees;
        Buf c(std::move(a));
        CHECK(c.get() == pa && c.capacity() == 8 && a.get() == nullptr && a.capacity() == 0 && g_frees == frees);
        // move assignment frees the target's old block and empties the source
        Buf d;
        d.reserve(4);
        d = std::move(c);
        CHECK(d.get() == pa && d.capacity() == 8 && c.get() == nullptr && c.capacity() == 0 && g_frees == frees + 1);
        Buf &self = d;
        d = std::move(self);  // self-assignment keeps the block
        CHECK(d.get() == pa && d.capacity() == 8 && g_frees == frees + 1);
        // swap exchanges blocks and capacities, frees nothing
        Buf e;
        e.reserve(2);
        int *pe = e.get();
        e.swap(d);
        CHECK(e.get() == pa && e.capacity() == 8 && d.get() == pe && d.capacity() == 2 && g_frees == frees + 1);
        // reset frees once and empties
        e.reset();
        CHECK(!e && e.capacity() == 0 && g_frees == frees + 2);
        // an aggregate of buffers is replaced whole by assigning a fresh one (how the matcher drops its query scratch)
        struct Pair {
            Buf x, y;
        } pr;
        pr.x.reserve(3);
        pr.y.reserve(5);
        pr = Pair{};
        CHECK(!pr.x && !pr.y && g_frees == frees + 4);
    }
    CHECK(live() == 0);  // after every object is gone (ASan's leak check at exit agrees)
    std::printf("owned buf ok: %d allocations, %d frees\n", g_allocs, g_frees);
    return 0;
}
