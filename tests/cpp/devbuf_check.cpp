// DevBuf<T>, DevEvent and DevStream (csrc/devbuf.h), the owners of every long-lived device table, event and side stream of a handle, as a stand-alone
// host program.  It passes on a machine without a device - there every hipMalloc, hipEventCreate and hipStreamCreateWithPriority fails, which is the
// failure path of alloc / upload / create - and on one with a device, where it also round-trips data, records an event and creates a stream.
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
static bool empty(const DevEvent &e) { return (hipEvent_t)e == nullptr; }
static bool empty(const DevStream &s) { return (hipStream_t)s == nullptr; }

// the event and stream owners, in the same two-sided way as the buffer
static void check_owners(bool dev) {
    { DevEvent never; DevStream never_s; CHECK(empty(never) && empty(never_s)); }      // the destructors of never-created owners
    { DevEvent e; DevStream s; g_err = "untouched"; e.reset(); e.reset(); s.reset(); s.reset(); CHECK(empty(e) && empty(s) && g_err == "untouched"); }
    DevEvent ev; DevStream st;
    if (!dev) {
        g_err.clear(); CHECK(ev.create() == -1 && empty(ev) && g_err.find("hipEventCreate") != std::string::npos);
        g_err.clear(); CHECK(st.create() == -1 && empty(st) && g_err.find("hipStreamCreate") != std::string::npos);
        g_err.clear(); CHECK(st.create(hipStreamNonBlocking, 0) == -1 && empty(st) && !g_err.empty());
        DevEvent e2(std::move(ev)); CHECK(empty(e2) && empty(ev));
        DevEvent e3; e3 = std::move(e2); CHECK(empty(e3) && empty(e2));
        DevEvent &eself = e3; e3 = std::move(eself); CHECK(empty(e3));      // (self-assignment)
        DevStream s2(std::move(st)); CHECK(empty(s2) && empty(st));
        DevStream s3; s3 = std::move(s2); CHECK(empty(s3) && empty(s2));
        DevStream &sself = s3; s3 = std::move(sself); CHECK(empty(s3));
    } else {
        CHECK(ev.create() == 0 && !empty(ev));
        const hipEvent_t raw = ev;
        DevEvent e2(std::move(ev)); CHECK(empty(ev) && (hipEvent_t)e2 == raw);      // the source gives the event up: one owner, one hipEventDestroy
        DevEvent e3; CHECK(e3.create() == 0 && (hipEvent_t)e3 != raw);
        e3 = std::move(e2); CHECK(empty(e2) && (hipEvent_t)e3 == raw);             // (what e3 held is destroyed by the assignment)
        DevEvent &eself = e3; e3 = std::move(eself); CHECK((hipEvent_t)e3 == raw);      // (self-assignment keeps it)
        CHECK(hipEventRecord(e3, nullptr) == hipSuccess && hipEventSynchronize(e3) == hipSuccess);      // the owner is handed to the runtime like the handle
        CHECK(e3.create() == 0 && !empty(e3));                                       // create() of a filled owner replaces what it held
        e3.reset(); CHECK(empty(e3));
        DevEvent ring[2][3]; const DevEvent *row = ring[1];                        // an array of owners is indexed like an array of handles
        CHECK(ring[1][2].create() == 0 && (hipEvent_t)row[2] != nullptr && empty(row[1]) && sizeof(ring) == 6 * sizeof(hipEvent_t));
        int lo_pri = 0, hi_pri = 0; (void)hipDeviceGetStreamPriorityRange(&lo_pri, &hi_pri);
        CHECK(st.create(hipStreamNonBlocking, hi_pri) == 0 && !empty(st));         // flags and priority, as run_batch's side streams
        unsigned flags = 0; int pri = 1 << 20;
        CHECK(hipStreamGetFlags(st, &flags) == hipSuccess && flags == hipStreamNonBlocking && hipStreamGetPriority(st, &pri) == hipSuccess && pri == hi_pri);
        const hipStream_t sraw = st;
        DevStream s2(std::move(st)); CHECK(empty(st) && (hipStream_t)s2 == sraw);
        DevStream s3; s3 = std::move(s2); CHECK(empty(s2) && (hipStream_t)s3 == sraw);
        DevStream &sself = s3; s3 = std::move(sself); CHECK((hipStream_t)s3 == sraw);
        CHECK(hipStreamSynchronize(s3) == hipSuccess);
        s3.reset(); CHECK(empty(s3));                                               // destroyed
        CHECK(s3.create() == 0 && !empty(s3));                                       // the plain form: default flags and priority
    }
}

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
    check_owners(dev);
    if (g_failed) return 1;
    printf("OK device=%d checks=%d\n", dev ? 1 : 0, g_checks);
    return 0;
}
