// devbuf.h — DevBuf<T>: the move-only owner of ONE hipMalloc allocation (host code).  Every long-lived device pointer of a handle is one of
// these: a constructor that fails half-way, a free function and a re-upload all release memory by the same rule - the member's destructor -
// so no free list has to know every pointer.  hipFree acts on the current device: the handles' free functions keep their DeviceGuard and then
// delete the handle.  A failed call leaves the buffer empty and the reason in the last error (tests/cpp/devbuf_check.cpp).
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

}  // namespace h2w
