// rt_devbuf.h -- DevBuf<T>: the owner of one device allocation (pointer + capacity in elements): non-copyable, movable, freed by its destructor.
// It allocates and frees only through rt::dev_alloc / rt::dev_free (rt_kernels.hip defines them over the HIP runtime), so this header includes no
// HIP header and tests/devbuf_host_test.cpp runs the type over malloc / free under the sanitizers.  A second release function makes the same
// template the owner of a handle that is no device block (rt_host.h: page-locked memory, events, the scene's own stream).
#pragma once
#include <cstddef>
#include <utility>

namespace rt {
int dev_alloc(void **p, size_t bytes);   // 0, or a status code with *p == nullptr (the message is left for rt_last_error())
void dev_free(void *p);

template <class T, void (*Release)(void *) = dev_free>
struct DevBuf {
    T *p = nullptr; size_t cap = 0;      // cap: elements
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); p = std::exchange(o.p, nullptr); cap = std::exchange(o.cap, 0); } return *this; }
    ~DevBuf() { reset(); }
    void reset() { if (p) Release(p); p = nullptr; cap = 0; }
    // Room for `need` elements; the contents do not survive.  Nothing happens when need <= cap; otherwise the old block is released FIRST (the two
    // need not fit side by side), and a failed allocation leaves {nullptr, 0}.  Whoever may still have the old block in use on a stream waits for it
    // before calling (rt_host.h ensure()).
    int grow(size_t need) {
        if (need <= cap) return 0;
        reset();
        void *q = nullptr;
        if (int rc = dev_alloc(&q, need * sizeof(T))) return rc;
        p = static_cast<T *>(q); cap = need;
        return 0;
    }
    size_t bytes() const { return cap * sizeof(T); }
    operator T *() const { return p; }
};
}  // namespace rt
