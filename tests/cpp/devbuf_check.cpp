// DevBuf<T> (csrc/devbuf.h), the owner of every long-lived device table of a handle, as a stand-alone host program.  It passes on a machine without
// a device - there every hipMalloc fails, which is the failure path of alloc / upload - and on one with a device, where it also round-trips data.
// Prints "OK device=<0|1> checks=<n>", or the failed checks.
#include <cstdio>
#include <cstdint>
#include <utility>
#include "devbuf.h"

namespace h2w { static std::string g_err; void set_error(const std::string &s) { g_err = s; } }
using namespace h2w;

static int g_checks = 0, g_failed = 0;
#define CHECK(c) do { g_checks++; if (!(c)) { g_failed++; printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)
template <class T> static bool empty(const DevBuf<T> &b) { return b.get() == nullptr && b.size() == 0; }

int main() {
    DevBuf<uint32_t> first;
    CHECK(empty(first));
    const bool dev = first.alloc(3) == 0;      // the first hipMalloc of the process decides which half runs
    const std::string first_err = g_err;
    { DevBuf<uint64_t> never; CHECK(empty(never)); }      // the destructor of a never-filled buffer
    { DevBuf<uint64_t> e; g_err = "untouched"; e.reset(); e.reset(); CHECK(empty(e) && g_err == "untouched"); }      // reset() of an empty buffer: a no-op
    if (!dev) {
        CHECK(empty(first) && first_err.find("hipMalloc") != std::string::npos);      // -1, empty, and the reason is in the error text
        const std::vector<uint32_t> v{1, 2, 3};
        g_err.clear(); CHECK(first.upload(v) == -1 && empty(first) && !g_err.empty());
        g_err.clear(); CHECK(first.upload(v.data(), 0) == -1 && empty(first) && !g_err.empty());
        g_err.clear(); CHECK(first.alloc(0) == -1 && empty(first) && !g_err.empty());
        DevBuf<uint32_t> b(std::move(first)); CHECK(empty(b) && empty(first));
        DevBuf<uint32_t> c; c = std::move(b); CHECK(empty(c) && empty(b));
        DevBuf<uint32_t> &self = c; c = std::move(self); CHECK(empty(c));      // (self-assignment)
    } else {
        CHECK(first.get() != nullptr && first.size() == 3);
        uint32_t *const p = first.get();
        DevBuf<uint32_t> b(std::move(first)); CHECK(empty(first) && b.get() == p && b.size() == 3);      // the source gives the allocation up: one owner, one hipFree
        DevBuf<uint32_t> c; CHECK(c.alloc(5) == 0);
        c = std::move(b); CHECK(empty(b) && c.get() == p && c.size() == 3);                                 // (what c held is freed by the assignment)
        DevBuf<uint32_t> &self = c; c = std::move(self); CHECK(c.get() == p && c.size() == 3);      // (self-assignment keeps it)
        const std::vector<uint32_t> one{0xC0FFEEu}; uint32_t back = 0;
        CHECK(c.upload(one) == 0 && c.get() != nullptr && c.size() == 1);
        CHECK(hipMemcpy(&back, c.get(), sizeof(back), hipMemcpyDeviceToHost) == hipSuccess && back == 0xC0FFEEu);
        CHECK(c.upload(one.data(), 0) == 0 && c.get() != nullptr && c.size() == 0);                         // nothing to copy, still a pointer a kernel may be handed
        CHECK(c.upload(std::vector<uint32_t>()) == 0 && c.get() != nullptr && c.size() == 0);
        // a request no device can serve (2^60 bytes) is refused by hipMalloc: -1, the reason, and what the buffer held is gone - never half-filled
        DevBuf<uint8_t> big; CHECK(big.alloc(1) == 0);
        g_err.clear(); CHECK(big.alloc((size_t)1 << 60) == -1 && empty(big) && g_err.find("hipMalloc") != std::string::npos);
        (void)hipGetLastError();
        c.reset(); CHECK(empty(c));
    }
    if (g_failed) return 1;
    printf("OK device=%d checks=%d\n", dev ? 1 : 0, g_checks);
    return 0;
}
