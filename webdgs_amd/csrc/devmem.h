// DevMem<T>: the one owner of a block of device memory (wdgs_alloc / wdgs_free, api.hip).  Every device pointer an op struct owns is one of these,
// so an op's destructor frees what it holds and a create function that fails half way has nothing to undo by hand.  Pointer and element count
// change together: after a failed alloc() the handle is EMPTY, never a null pointer beside a stale capacity.
//
// Plain C++17 like alloc_cache.h, with no HIP call of its own: whoever includes it has declared hipStream_t (common.h through the HIP runtime;
// tests/cpp/devmem_test.cpp by hand, with a counting wdgs_alloc / wdgs_free of its own).  It never synchronises: when a free has to wait for the
// device stays the decision of the op that holds the handle.
#pragma once
#include <cstddef>

int wdgs_alloc(void** p, size_t bytes, bool zero, hipStream_t stream);
void wdgs_free(void* p);   // the counterpart of wdgs_alloc (api.hip: freed blocks are kept by size class)

namespace wdgs {

template <class T>
class DevMem {
public:
    DevMem() = default;
    ~DevMem() { reset(); }
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    DevMem(DevMem&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevMem& operator=(DevMem&& o) noexcept {
        if (this != &o) { reset(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }

    // Frees what the handle holds, then asks for `count` elements (zeroed on `stream` if `zero`).  Returns wdgs_alloc's status; the handle holds the
    // new block on success and nothing on failure.  (A request for 0 bytes yields a block: wdgs_alloc's rule.)
    int alloc(size_t count, bool zero, hipStream_t stream) {
        reset();
        void* q = nullptr;
        const int r = wdgs_alloc(&q, count * sizeof(T), zero, stream);
        if (r != 0) return r;   // (WDGS_OK == 0)
        p = static_cast<T*>(q);
        n = count;
        return r;
    }
    void reset() {
        if (p) wdgs_free(p);
        p = nullptr;
        n = 0;
    }
    // A block that came from wdgs_alloc elsewhere (optimizer state handed in by the host) becomes this handle's; release() hands it out again.
    void adopt(T* block, size_t count) { reset(); p = block; n = count; }
    T* release() { T* q = p; p = nullptr; n = 0; return q; }

    T* get() const { return p; }
    size_t count() const { return n; }
    explicit operator bool() const { return p != nullptr; }
    operator T*() const { return p; }   // kernel launch lines take the handle where they took the pointer

private:
    T* p = nullptr;
    size_t n = 0;
};

}  // namespace wdgs
