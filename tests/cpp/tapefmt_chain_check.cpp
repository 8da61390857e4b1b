// The parts of a split select (csrc/tapefmt.h SELIND_*, H2W_TRACE_SPLIT_SELECTS) under tape_check, on the host: a well-formed chain of two and of
// three parts is accepted; every way the chain can be out of shape is refused, by the message that names the first word of the part it is about.
#include <cstdio>
#include <functional>
#include <string>
#include <vector>
#include "tapefmt.h"

using namespace h2w;

static int failures = 0, n_tapes = 0, n_refusals = 0;
#define CHECK(c, ...) do { if (!(c)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

typedef std::vector<uint32_t> V;
static size_t op(V &w, uint32_t code, uint32_t n, uint32_t aux, const V &words) {
    const size_t at = w.size(); w.push_back(code | (n << 8) | (aux << 16) | ((uint32_t)(words.size() + 1) << 24)); w.insert(w.end(), words.begin(), words.end()); return at;
}
// `fetches` four-word DOP_FETCH ops into slots [slot0, ...), then a DOP_FR_SELIND over those entries (indicators: pool entries) -> the part's first word
static size_t part(V &w, uint32_t fetches, uint32_t slot0, uint32_t aux, uint32_t out) {
    for (uint32_t i = 0; i < fetches; i++) op(w, DOP_FETCH, 4, 0, {mkref(RK_IMPORT, WFR, 0), slot0 + 4 * i});
    V words; for (uint32_t i = 0; i < fetches; i++) words.push_back(fastref_ring(WFR, slot0 + 4 * i));
    for (uint32_t i = 0; i < fetches; i++) words.push_back(fastref_pool(W64, LDS_POOL64 + i * 8));
    words.push_back(out);
    return op(w, DOP_FR_SELIND, fetches, aux, words);
}
static TapeLimits limits() { TapeLimits M; M.tmpl = 0; M.nslots = 1000; M.nimps = 1; M.npool64 = 100; M.npoolfr = 4; return M; }
static std::string malformed(size_t word, uint32_t o) { return "internal: malformed device tape (template 0, word " + std::to_string(word) + ", op " + std::to_string(o) + ")"; }
static void accept(const V &w, const char *what) {
    n_tapes++; const std::string e = tape_check(w.data(), w.size(), limits());
    CHECK(e.empty(), "%s: a valid tape is refused: %s", what, e.c_str());
}
static void refuse(const V &tape, const char *what, const std::string &want, const std::function<void(V &)> &corrupt) {
    n_refusals++; V w = tape; corrupt(w);
    const std::string e = tape_check(w.data(), w.size(), limits());
    CHECK(e == want, "%s: got \"%s\", want \"%s\"", what, e.c_str(), want.c_str());
}
static void set_aux(V &w, size_t at, uint32_t aux) { w[at] = (w[at] & ~0xff0000u) | (aux << 16); }
static void set_op(V &w, size_t at, uint32_t code) { w[at] = (w[at] & ~0xffu) | code; }

int main() {
    const uint32_t FIRST = SELIND_CONTINUED, MIDDLE = SELIND_CONTINUES | SELIND_CONTINUED, LAST = SELIND_CONTINUES;
    // ---- two parts: 51 + 13 entries, as a select of 64 imported entries is cut (each part's fetches within the ring: 204 and 52 slots)
    V A; op(A, DOP_CLT, 0, 0, {fastref_pool(W64, LDS_POOL64)});
    const size_t a0 = part(A, 51, 4, FIRST, NO_SLOT), a1 = part(A, 13, 208, LAST, 0);
    const size_t a_clt = op(A, DOP_CLT, 0, 0, {fastref_ring(W64, 0)}); const size_t a_end = op(A, DOP_END, 0, 0, {});
    accept(A, "two parts");
    // ---- three parts, each with a full ring of fetches in front of it (the bound is per part), the last without any fetch; a whole select behind the chain
    V B;
    const size_t b0 = part(B, 64, 4, FIRST, NO_SLOT), b1 = part(B, 64, 260, MIDDLE, NO_SLOT);
    const size_t b2 = op(B, DOP_FR_SELIND, 1, LAST, {fastref_ring(WFR, 516), fastref_pool(W64, LDS_POOL64), 0});
    const size_t b_whole = op(B, DOP_FR_SELIND, 1, 0, {fastref_ring(WFR, 0), fastref_pool(W64, LDS_POOL64), 520});
    const size_t b_narrow = op(B, DOP_SELIND, 1, 0, {fastref_ring(W64, 0), fastref_pool(W64, LDS_POOL64), 524});
    op(B, DOP_END, 0, 0, {});
    accept(B, "three parts");
    { V C; part(C, 2, 0, FIRST, NO_SLOT); part(C, 2, 8, LAST, NO_SLOT); op(C, DOP_END, 0, 0, {}); accept(C, "a chain whose value nothing reads (the last part's result static)"); }

    // ---- aux
    refuse(B, "aux 4 on a whole wide select", malformed(b_whole, DOP_FR_SELIND), [&](V &w) { set_aux(w, b_whole, 4); });
    refuse(B, "aux 6 on a first part", malformed(b0, DOP_FR_SELIND), [&](V &w) { set_aux(w, b0, 6); });
    refuse(B, "aux 255 on a middle part", malformed(b1, DOP_FR_SELIND), [&](V &w) { set_aux(w, b1, 255); });
    refuse(B, "aux 1 on the narrow select", malformed(b_narrow, DOP_SELIND), [&](V &w) { set_aux(w, b_narrow, 1); });
    refuse(B, "aux 2 on the narrow select", malformed(b_narrow, DOP_SELIND), [&](V &w) { set_aux(w, b_narrow, 2); });
    refuse(B, "aux 128 on the narrow select", malformed(b_narrow, DOP_SELIND), [&](V &w) { set_aux(w, b_narrow, 128); });
    // ---- a "continued" part without its successor: the part left open is named
    refuse(A, "continued, then a whole select's op (not continuing)", malformed(a0, DOP_FR_SELIND), [&](V &w) { set_aux(w, a1, 0); });
    refuse(A, "continued, then a first part again", malformed(a0, DOP_FR_SELIND), [&](V &w) { set_aux(w, a1, FIRST); w[a1 + 27] = NO_SLOT; });
    refuse(A, "continued, then the narrow select", malformed(a0, DOP_FR_SELIND), [&](V &w) { set_op(w, a1, DOP_SELIND); });
    refuse(A, "continued, then the end of the tape", malformed(a0, DOP_FR_SELIND), [&](V &w) { w.resize(a1 - 13 * 3); w.push_back(DOP_END | (1u << 24)); });
    refuse(A, "the last part continued too, then another op", malformed(a1, DOP_FR_SELIND), [&](V &w) { set_aux(w, a1, MIDDLE); w[a1 + 27] = NO_SLOT; });
    refuse(B, "the last of three continued, then a whole select", malformed(b2, DOP_FR_SELIND), [&](V &w) { set_aux(w, b2, MIDDLE); w[b2 + 3] = NO_SLOT; });
    refuse(B, "an op that is no fetch between two parts", malformed(b0, DOP_FR_SELIND), [&](V &w) { w[b0 + 130] = DOP_CLT | (2u << 24); w[b0 + 131] = fastref_pool(W64, LDS_POOL64); w[b0 + 132] = DOP_SKIP | (1u << 24); });
    // ---- a "continues" part without its predecessor
    refuse(A, "continues behind an op that is no part", malformed(a0, DOP_FR_SELIND), [&](V &w) { set_aux(w, a0, MIDDLE); });
    refuse(A, "continues behind a whole select", malformed(a1, DOP_FR_SELIND), [&](V &w) { set_aux(w, a0, 0); w[a0 + 103] = 900; });
    refuse(B, "continues behind a part that is not continued", malformed(b2, DOP_FR_SELIND), [&](V &w) { set_aux(w, b1, LAST); w[b1 + 129] = 900; });
    refuse(B, "a whole select made a last part", malformed(b_whole, DOP_FR_SELIND), [&](V &w) { set_aux(w, b_whole, LAST); });
    { V C; part(C, 2, 0, LAST, 20); op(C, DOP_END, 0, 0, {}); refuse(C, "continues as the first op of the tape", malformed(6, DOP_FR_SELIND), [](V &) {}); }
    // ---- a "continued" part stores no result
    refuse(A, "a first part with a result slot", malformed(a0, DOP_FR_SELIND), [&](V &w) { w[a0 + 103] = 0; });
    refuse(B, "a middle part with a result slot", malformed(b1, DOP_FR_SELIND), [&](V &w) { w[b1 + 129] = 996; });
    // ---- the ring bound is per part, and holds for every part
    {   // 1 + 256 slots fetched between two parts: the fetch that passes the ring is named (the count starts anew behind the first part, not behind the chain)
        V D; part(D, 2, 0, FIRST, NO_SLOT);
        const size_t extra = op(D, DOP_FETCH, 1, 0, {mkref(RK_IMPORT, W64, 0), 8}); part(D, 64, 12, LAST, 500); op(D, DOP_END, 0, 0, {});
        refuse(D, "257 slots fetched in front of the second part", malformed(extra + 3 + 3 * 63, DOP_FETCH), [](V &) {});
        V D2 = D; D2.erase(D2.begin() + (long)extra, D2.begin() + (long)extra + 3); accept(D2, "256 slots fetched in front of the second part");
    }
    refuse(A, "the last part's result past the slots", malformed(a1, DOP_FR_SELIND), [&](V &w) { w[a1 + 27] = 997; });
    // ---- the ops around a chain are checked as ever
    refuse(A, "no DOP_END behind a chain", "internal: a device tape does not end", [&](V &w) { w.pop_back(); });
    refuse(A, "the op behind the chain", malformed(a_clt, DOP_CLT), [&](V &w) { w[a_clt + 1] |= 1u << 29; });
    (void)a_end;
    if (failures) { printf("%d FAILED\n", failures); return 1; }
    printf("OK tapes: %d refusals: %d\n", n_tapes, n_refusals);
    return 0;
}
