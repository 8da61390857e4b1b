// The checker a traced plan's verdict table passes before it is uploaded (csrc/verdictfmt.h verdict_table_check), on the host: a table built by hand
// with every ref kind and width is accepted; every single corruption of it is refused, by the message that names the entry.
#include <cstdio>
#include <functional>
#include <string>
#include <vector>
#include "verdictfmt.h"

using namespace h2w;

static int failures = 0, n_tables = 0, n_corruptions = 0;
#define CHECK(c, ...) do { if (!(c)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static const uint32_t INPUTS[3] = {0, 99, 96};      // input 1: a one-word input on the proof's last word; input 2: a four-word one on its last four
static TapeLimits limits() {
    TapeLimits M; M.tmpl = 3; M.nslots = 400; M.nimps = 2; M.inputs = INPUTS; M.ninputs = 3; M.proof_words = 100; M.npool64 = 3000; M.npoolfr = 10;
    return M;
}
static VEntD eq(uint32_t a, uint32_t b, uint32_t site = 0) { VEntD d; d.a = a; d.b = b; d.site = site; d.kind = VK_EQUAL; d.aux = 0; return d; }
static VEntD range(uint32_t a, uint64_t bits, uint32_t site = 0) { VEntD d; d.a = a; d.b = 0; d.site = site; d.kind = VK_RANGE; d.aux = bits; return d; }
static VEntD clt(uint32_t a, uint64_t bound) { VEntD d; d.a = a; d.b = 0; d.site = 7; d.kind = VK_CLT; d.aux = bound; return d; }
static std::string malformed(size_t e) { return "internal: malformed verdict table (template 3, entry " + std::to_string(e) + ")"; }

typedef std::vector<VEntD> Tab;
static void accept(const Tab &t, const TapeLimits &M, const char *what) {
    n_tables++; const std::string e = verdict_table_check(t.data(), t.size(), M);
    CHECK(e.empty(), "%s: a valid table is refused: %s", what, e.c_str());
}
static void refuse(const Tab &t, TapeLimits M, const char *what, size_t entry, const std::function<void(Tab &, TapeLimits &)> &corrupt) {
    n_corruptions++; Tab w = t; corrupt(w, M);
    const std::string e = verdict_table_check(w.data(), w.size(), M);
    CHECK(e == malformed(entry), "%s: got \"%s\", want \"%s\"", what, e.c_str(), malformed(entry).c_str());
}

int main() {
    const TapeLimits M = limits();
    // every ref kind, every width, each at the last place it may stand
    Tab T = {
        /* 0 */ eq(mkref(RK_LOCAL, W64, 399), mkref(RK_LOCAL, W128, 398), 1u << 31),
        /* 1 */ eq(mkref(RK_LOCAL, WFR, 396), mkref(RK_LOCAL, W64, 0)),
        /* 2 */ eq(mkref(RK_IMPORT, W64, 1), mkref(RK_IMPORT, WFR, 0)),
        /* 3 */ eq(mkref(RK_IMPORT, W128, 1), mkref(RK_LIT64, W64, 2999)),
        /* 4 */ eq(mkref(RK_LITFR, WFR, 9), mkref(RK_LITFR, WFR, 0)),
        /* 5 */ eq(mkref(RK_INPUT, W64, 1), mkref(RK_INPUT, WFR, 2)),
        /* 6 */ eq(mkref(RK_INPUT, W64, 0), mkref(RK_LIT64, W64, 0)),
        /* 7 */ range(mkref(RK_LOCAL, W64, 399), 64, 0x20),
        /* 8 */ range(mkref(RK_IMPORT, W64, 0), 0),
        /* 9 */ range(mkref(RK_INPUT, W64, 1), 13),
        /* 10 */ clt(mkref(RK_LOCAL, W64, 5), 0xFFFFFFFF00000001ull),
        /* 11 */ clt(mkref(RK_LIT64, W64, 7), 1),
    };
    accept(T, M, "every kind and width");
    accept(Tab(), M, "no entry");
    { TapeLimits E = M; E.nslots = 0; E.nimps = 0; E.ninputs = 0; E.npool64 = 0; E.npoolfr = 0; accept(Tab(), E, "no entry, no limits"); }
    // ---- a slot + span one past the end, by width
    refuse(T, M, "a one-word local one past the end", 0, [](Tab &w, TapeLimits &) { w[0].a = mkref(RK_LOCAL, W64, 400); });
    refuse(T, M, "a two-word local one past the end", 0, [](Tab &w, TapeLimits &) { w[0].b = mkref(RK_LOCAL, W128, 399); });
    refuse(T, M, "a four-word local one past the end", 1, [](Tab &w, TapeLimits &) { w[1].a = mkref(RK_LOCAL, WFR, 397); });
    refuse(T, M, "one slot fewer", 0, [](Tab &, TapeLimits &m) { m.nslots = 399; });
    refuse(T, M, "a local at the top of the index field", 1, [](Tab &w, TapeLimits &) { w[1].b = mkref(RK_LOCAL, W64, (1u << 27) - 1); });
    // ---- import, input, pool indices
    refuse(T, M, "an import out of range", 2, [](Tab &w, TapeLimits &) { w[2].a = mkref(RK_IMPORT, W64, 2); });
    refuse(T, M, "one import fewer", 2, [](Tab &, TapeLimits &m) { m.nimps = 1; });
    refuse(T, M, "no import table", 2, [](Tab &, TapeLimits &m) { m.nimps = 0; });
    refuse(T, M, "an input out of range", 5, [](Tab &w, TapeLimits &) { w[5].a = mkref(RK_INPUT, W64, 3); });
    refuse(T, M, "a four-word input on the proof's last word", 5, [](Tab &w, TapeLimits &) { w[5].b = mkref(RK_INPUT, WFR, 1); });
    refuse(T, M, "a proof one word shorter", 5, [](Tab &, TapeLimits &m) { m.proof_words = 99; });
    refuse(T, M, "one input fewer", 5, [](Tab &, TapeLimits &m) { m.ninputs = 2; });
    refuse(T, M, "a 64-bit literal out of range", 3, [](Tab &w, TapeLimits &) { w[3].b = mkref(RK_LIT64, W64, 3000); });
    refuse(T, M, "a two-word read of the last 64-bit literal", 3, [](Tab &w, TapeLimits &) { w[3].b = mkref(RK_LIT64, W128, 2999); });
    refuse(T, M, "a wide literal out of range", 4, [](Tab &w, TapeLimits &) { w[4].a = mkref(RK_LITFR, WFR, 10); });
    refuse(T, M, "one wide literal fewer", 4, [](Tab &, TapeLimits &m) { m.npoolfr = 9; });
    // ---- widths and kinds
    for (int k : {(int)RK_LOCAL, (int)RK_IMPORT, (int)RK_LIT64, (int)RK_INPUT, (int)RK_LITFR}) {
        refuse(T, M, "width 3, side a", 6, [k](Tab &w, TapeLimits &) { w[6].a = mkref(k, 3, 0); });
        refuse(T, M, "width 3, side b", 6, [k](Tab &w, TapeLimits &) { w[6].b = mkref(k, 3, 0); });
    }
    for (int k : {(int)RK_RING, 6, 7}) {
        refuse(T, M, "kind 5 and above, side a", 6, [k](Tab &w, TapeLimits &) { w[6].a = mkref(k, W64, 0); });
        refuse(T, M, "kind 5 and above, side b", 6, [k](Tab &w, TapeLimits &) { w[6].b = mkref(k, W64, 0); });
        refuse(T, M, "kind 5 and above, a range site", 7, [k](Tab &w, TapeLimits &) { w[7].a = mkref(k, W64, 0); });
    }
    // ---- range sites
    refuse(T, M, "a range site of 65 bits on a one-word ref", 7, [](Tab &w, TapeLimits &) { w[7].aux = 65; });
    refuse(T, M, "a range site of 2^32 + 1 bits", 9, [](Tab &w, TapeLimits &) { w[9].aux = (1ull << 32) + 1; });
    refuse(T, M, "a range site on a two-word value", 7, [](Tab &w, TapeLimits &) { w[7].a = mkref(RK_LOCAL, W128, 0); });
    refuse(T, M, "a range site on a four-word value", 8, [](Tab &w, TapeLimits &) { w[8].a = mkref(RK_IMPORT, WFR, 0); });
    refuse(T, M, "a range site on a wide literal", 8, [](Tab &w, TapeLimits &) { w[8].a = mkref(RK_LITFR, WFR, 0); });
    refuse(T, M, "a bound check on a four-word input", 10, [](Tab &w, TapeLimits &) { w[10].a = mkref(RK_INPUT, WFR, 2); });
    refuse(T, M, "a range site's operand out of range", 7, [](Tab &w, TapeLimits &) { w[7].a = mkref(RK_LOCAL, W64, 400); });
    refuse(T, M, "a range site with a second operand", 9, [](Tab &w, TapeLimits &) { w[9].b = mkref(RK_LOCAL, W64, 1); });
    refuse(T, M, "an entry kind that does not exist", 11, [](Tab &w, TapeLimits &) { w[11].kind = VK_COUNT; });
    refuse(T, M, "an entry kind of all ones", 0, [](Tab &w, TapeLimits &) { w[0].kind = 0xffffffffu; });
    // the first bad entry is the one named
    refuse(T, M, "two bad entries", 2, [](Tab &w, TapeLimits &) { w[2].a = mkref(RK_IMPORT, W64, 9); w[8].aux = 99; });
    // words of a ref as the kernel reads them
    CHECK(vref_words(mkref(RK_LOCAL, W64, 0)) == 1 && vref_words(mkref(RK_LOCAL, W128, 0)) == 2 && vref_words(mkref(RK_IMPORT, WFR, 0)) == 4 && vref_words(mkref(RK_LITFR, W64, 0)) == 4 &&
          vref_words(mkref(RK_INPUT, W128, 0)) == 1 && vref_words(mkref(RK_INPUT, WFR, 0)) == 4 && vref_words(mkref(RK_LIT64, W64, 0)) == 1, "vref_words");
    if (failures) { printf("%d FAILED\n", failures); return 1; }
    printf("OK tables: %d corruptions: %d\n", n_tables, n_corruptions);
    return 0;
}
