// Owned<T, Mem>: one block of T that frees itself.  Host-only and HIP-free: Mem is a policy with two static functions,
//   void *alloc(size_t bytes)   - throws on failure, never returns a block it did not get
//   void free(void *p)
// (frt_internal.hpp defines the device and the pinned policy; tests/cpp/owned_buf_test.cpp a counting malloc).
#pragma once
#include <cstddef>
#include <utility>

template <class T, class Mem>
class Owned {
    T *p_ = nullptr;
    size_t cap_ = 0;  // elements

  public:
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept { swap(o); }
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) {
            reset();
            swap(o);
        }
        return *this;
    }
    ~Owned() { reset(); }

    T *get() const { return p_; }
    size_t capacity() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }

    void reset() {
        if (p_) Mem::free(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // Grow and DISCARD: room for n elements, contents undefined after a growth.  The old block goes first (the two never exist side by
    // side), so an allocation that throws leaves an empty buffer, never a dangling one.
    void reserve(size_t n) {
        if (n <= cap_) return;
        reset();
        p_ = static_cast<T *>(Mem::alloc(n * sizeof(T)));
        cap_ = n;
    }
    void swap(Owned &o) noexcept {
        std::swap(p_, o.p_);
        std::swap(cap_, o.cap_);
    }
};
