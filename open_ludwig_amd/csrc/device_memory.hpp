// Owners of device memory, events and streams: move-only, released by the destructor. Plain C++, no HIP: the runtime's calls come in
// through a policy type, so the failure paths can be walked on the host (tests/device_memory_check.cpp).
// The idiom for a group that must exist completely or not at all, and for replacing what a member holds: make locals, and move them
// into the members only after every call has succeeded. Whatever a failure leaves in a local, its destructor releases.
#pragma once

#include <cstddef>

namespace lw {

// Mem: static int alloc(void **p, size_t bytes) - 0 or the runtime's error code; static void release(void *p).
template <class T, class Mem>
class DeviceArray {
    T *p_ = nullptr;
    size_t n_ = 0;

public:
    DeviceArray() = default;
    DeviceArray(DeviceArray &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DeviceArray &operator=(DeviceArray &&o) noexcept     // releases what it held; the copy operations are deleted with this declared
    {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~DeviceArray() { reset(); }
    // `count` elements in place of what was held (released first); 0 elements = null. After a failure: null, and the runtime's code.
    int alloc(size_t count)
    {
        reset();
        void *q = nullptr;
        const int e = count ? Mem::alloc(&q, count * sizeof(T)) : 0;
        if (e || !count) return e;
        p_ = static_cast<T *>(q);
        n_ = count;
        return 0;
    }
    void reset() { if (p_) Mem::release(p_); p_ = nullptr; n_ = 0; }
    size_t size() const { return n_; }
    T *get() const { return p_; }
    operator T *() const { return p_; }     // kernel arguments, parameter structs and `if (L->rho)` read as with a raw pointer
};

// Ops: static int create(H *h, args...) - 0 or the runtime's error code; static int destroy(H h).
template <class H, class Ops>
class DeviceHandle {
    H h_ = H{};

public:
    DeviceHandle() = default;
    DeviceHandle(DeviceHandle &&o) noexcept : h_(o.h_) { o.h_ = H{}; }
    DeviceHandle &operator=(DeviceHandle &&o) noexcept
    {
        if (this != &o) { reset(); h_ = o.h_; o.h_ = H{}; }
        return *this;
    }
    ~DeviceHandle() { reset(); }
    template <class... A>
    int create(A... a)
    {
        reset();
        H h = H{};
        const int e = Ops::create(&h, a...);
        if (e == 0) h_ = h;
        return e;
    }
    void reset() { if (h_) (void)Ops::destroy(h_); h_ = H{}; }
    H get() const { return h_; }
    operator H() const { return h_; }
};

}  // namespace lw
