// devbuf.h — the move-only owners of a handle's device resources (host code): DevBuf<T> of ONE hipMalloc allocation, DevEvent of a hipEvent_t, DevStream
// of a hipStream_t.  Every long-lived device pointer, event and side stream of a handle is one of these: a constructor that fails half-way, a free
// function and a re-upload all release by the same rule - the member's destructor - so no free list has to know every member.  hipFree and the destroy
// calls act on the current device: the handles' free functions keep their DeviceGuard and then delete the handle.  A failed call leaves the owner empty
// and the reason in the last error (tests/cpp/devbuf_check.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>

namespace h2w {

void set_error(const std::string &s);

#define H2W_HIP(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { \
    h2w::set_error(std::string(#expr) + ": " + hipGetErrorString(_e)); return -1; } } while (0)

template <class T> class DevBuf {
    T *p_ = nullptr; size_t n_ = 0;
    static int copy_in(T *d, const T *h, size_t n) { H2W_HIP(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice)); return 0; }
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; } return *this; }
    DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { reset(); }
    T *get() const { return p_; }
    size_t size() const { return n_; }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; n_ = 0; }
    // n elements, uninitialised (n == 0: one element is allocated, so that a filled buffer never hands out null)
    int alloc(size_t n) {
        reset();
        T *q = nullptr;
        H2W_HIP(hipMalloc((void **)&q, (n ? n : 1) * sizeof(T)));
        p_ = q; n_ = n;
        return 0;
    }
    int upload(const T *h, size_t n) {
        if (alloc(n) != 0) return -1;
        if (n && copy_in(p_, h, n) != 0) { reset(); return -1; }
        return 0;
    }
    int upload(const std::vector<T> &h) { return upload(h.data(), h.size()); }
};

// An event / a stream converts to its raw handle and is no larger than it, so an array of owners is indexed and handed to the runtime like an array of handles.
class DevEvent {
    hipEvent_t e_ = nullptr;
public:
    DevEvent() = default;
    DevEvent(DevEvent &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    DevEvent &operator=(DevEvent &&o) noexcept { if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; } return *this; }
    DevEvent(const DevEvent &) = delete; DevEvent &operator=(const DevEvent &) = delete;
    ~DevEvent() { reset(); }
    operator hipEvent_t() const { return e_; }
    void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
    int create() {
        reset();
        hipEvent_t e = nullptr;
        H2W_HIP(hipEventCreate(&e));
        e_ = e;
        return 0;
    }
};
class DevStream {
    hipStream_t s_ = nullptr;
public:
    DevStream() = default;
    DevStream(DevStream &&o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    DevStream &operator=(DevStream &&o) noexcept { if (this != &o) { reset(); s_ = o.s_; o.s_ = nullptr; } return *this; }
    DevStream(const DevStream &) = delete; DevStream &operator=(const DevStream &) = delete;
    ~DevStream() { reset(); }
    operator hipStream_t() const { return s_; }
    void reset() { if (s_) (void)hipStreamDestroy(s_); s_ = nullptr; }
    int create(unsigned flags = hipStreamDefault, int priority = 0) {      // (priority 0: the default one)
        reset();
        hipStream_t s = nullptr;
        H2W_HIP(hipStreamCreateWithPriority(&s, flags, priority));
        s_ = s;
        return 0;
    }
};
static_assert(sizeof(DevEvent) == sizeof(hipEvent_t) && sizeof(DevStream) == sizeof(hipStream_t), "owners are as large as their handles");

}  // namespace h2w
