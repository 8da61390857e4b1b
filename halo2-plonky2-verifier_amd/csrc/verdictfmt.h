// verdictfmt.h — the verdict table of a traced plan, stated once: the entries the lowering (tracelower.cpp verdict_tables) makes from the recorded
// assert_equal calls and range checks, verdict_table_check verifies and k_trace_verdict (traceverdict.hip) follows.  Plain C++ like tapefmt.h, whose
// refs and limits it uses: the checker compiles and is tested on the host (tests/cpp/verdict_table_check.cpp).
//
// An entry names its operands by old-style refs, as a DOP_FETCH carries them: mkref(kind, width, idx) with kind RK_LOCAL (a slot of the segment's own
// value store), RK_IMPORT (entry idx of the instance's VERDICT import table: a value of an enclosing segment), RK_LIT64 / RK_LITFR (the plan's constant
// pools), RK_INPUT (entry idx of the instance's input table: a proof word).  The instances of a template share its entries; their import and input
// tables make the refs concrete; so does, for the site words, their site table.
#pragma once
#include "tapefmt.h"

namespace h2w {

enum { VK_EQUAL = 0, VK_RANGE = 1, VK_CLT = 2, VK_COUNT };
// VK_EQUAL: a == b as 256-bit values, zero-extended from their widths.  VK_RANGE: h2w_range_check(a, aux bits).  VK_CLT: h2w_check_less_than_safe(a, aux).
// site: the word of h2w_trace_site in force where the check was recorded - in the template's FIRST instance: isomorphic instances may stand at different
// sites (the Merkle paths of two trees share a template), so the device reads the word of its own instance from the plan's site table, [instance][entry]
struct VEntD { uint32_t a, b, site, kind; uint64_t aux; };

// words the kernel reads of an operand
HD uint32_t vref_words(uint32_t r) { const int k = ref_kind(r), w = ref_width(r); return k == RK_LITFR ? 4u : k == RK_INPUT ? (w == WFR ? 4u : 1u) : (uint32_t)(w == W64 ? 1 : w == W128 ? 2 : 4); }

// ---- the check: every word the device will follow (a wild ref is a GPU fault).  M: the template's limits as tape_check takes them - nslots, inputs /
// ninputs / proof_words, npool64, npoolfr -, with nimps = the entries of the template's verdict import table.
// empty: well formed; else "internal: malformed verdict table (template t, entry e)"
inline std::string verdict_table_check(const VEntD *E, size_t n, const TapeLimits &M) {
    auto okref = [&](uint32_t r) {
        const uint32_t i = ref_idx(r); const int k = ref_kind(r), w = ref_width(r);
        if (w > WFR) return false;
        const uint64_t span = vref_words(r);
        switch (k) {
            case RK_LOCAL: return (uint64_t)i + span <= M.nslots;
            case RK_IMPORT: return i < M.nimps;
            case RK_LIT64: return (uint64_t)i + span <= M.npool64;
            case RK_INPUT: return i < M.ninputs && (uint64_t)M.inputs[i] + span <= M.proof_words;
            case RK_LITFR: return i < M.npoolfr;
            default: return false;      // RK_RING and above: a verdict lane has no ring
        }
    };
    for (size_t e = 0; e < n; e++) {
        const VEntD &v = E[e]; bool ok = v.kind < VK_COUNT && okref(v.a);
        if (ok && v.kind == VK_EQUAL) ok = okref(v.b);
        if (ok && v.kind != VK_EQUAL) ok = vref_words(v.a) == 1 && v.b == 0;      // the range checks the lowering admits are on one-word values
        if (ok && v.kind == VK_RANGE) ok = v.aux <= 64;
        if (!ok) return "internal: malformed verdict table (template " + std::to_string(M.tmpl) + ", entry " + std::to_string(e) + ")";
    }
    return std::string();
}

}  // namespace h2w
