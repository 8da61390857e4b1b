// The checker every device tape of a traced plan passes before it is uploaded (csrc/tapefmt.h tape_check), on the host: hand-built tapes with
// every op are accepted; every single corruption of one is refused, by the message that names the op's first word.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <initializer_list>
#include <string>
#include <vector>
#include "tapefmt.h"

using namespace h2w;

static int failures = 0, n_tapes = 0, n_corruptions = 0;
#define CHECK(c, ...) do { if (!(c)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

struct Tape {
    std::vector<uint32_t> w;
    // an op: its header (the length byte from the words given; DOP_GLOPRUN: 0, its length is not in the header), then the words; -> its first word
    size_t op(uint32_t code, uint32_t n, uint32_t aux, std::initializer_list<uint32_t> words) { return opv(code, n, aux, std::vector<uint32_t>(words)); }
    size_t opv(uint32_t code, uint32_t n, uint32_t aux, const std::vector<uint32_t> &words) {
        const size_t at = w.size(); const uint32_t len = code == DOP_GLOPRUN ? 0u : (uint32_t)words.size() + 1;
        w.push_back(code | (n << 8) | (aux << 16) | (len << 24)); w.insert(w.end(), words.begin(), words.end()); return at;
    }
};
static const uint32_t INPUTS[3] = {0, 98, 96};
static TapeLimits limits() {
    TapeLimits M; M.tmpl = 0; M.nslots = 400; M.nimps = 2; M.inputs = INPUTS; M.ninputs = 3; M.proof_words = 100;
    M.npool64 = 3000; M.npoolfr = 10;      // pool64: beyond its LDS part (POOL64_CAP entries); poolfr: within
    M.nglp = 2; M.nbnp = 2; M.fusing_gl = M.fusing_bn = true; M.glp_block_cells = 123456; M.glp_recs = M.glp_recs_kernel = 2604; M.bn_perm_cells = 4032;
    return M;
}
static uint32_t p64(uint32_t i, int w = W64) { return fastref_pool(w, LDS_POOL64 + i * 8); }
static uint32_t pfr(uint32_t i) { return fastref_pool(WFR, LDS_POOLFR + i * 32); }
static uint32_t ring(uint32_t slot, int w = W64) { return fastref_ring(w, slot); }

static std::string malformed(size_t word, uint32_t op) { return "internal: malformed device tape (template 0, word " + std::to_string(word) + ", op " + std::to_string(op) + ")"; }
static const std::string NO_END = "internal: a device tape does not end";
static void accept(const Tape &t, const TapeLimits &M, const char *what) {
    n_tapes++; const std::string e = tape_check(t.w.data(), t.w.size(), M);
    CHECK(e.empty(), "%s: a valid tape is refused: %s", what, e.c_str());
}
// one corruption of a tape that is accepted as it stands
static void refuse(const Tape &t, TapeLimits M, const char *what, const std::string &want, const std::function<void(std::vector<uint32_t> &, TapeLimits &)> &corrupt) {
    n_corruptions++; std::vector<uint32_t> w = t.w; corrupt(w, M);
    const std::string e = tape_check(w.data(), w.size(), M);
    CHECK(e == want, "%s: got \"%s\", want \"%s\"", what, e.c_str(), want.c_str());
}

// operand words of an op as the lowering always knew them (the switch operand_span was before the table)
static uint32_t operands_by_hand(uint32_t op, uint32_t n) {
    switch (op) {
        case DOP_CONST1: case DOP_FRCELL: case DOP_LOADW: case DOP_REDUCE: case DOP_CLT: case DOP_RANGE: case DOP_IDX2IND: case DOP_NUM2BITS: case DOP_DECOMP565: return 1;
        case DOP_LOADW_DIV: case DOP_LOADW_EXTINV: case DOP_FR_ADD: case DOP_FR_MUL: return 2;
        case DOP_GLOP: case DOP_GATE: case DOP_FR_MULADD: case DOP_SELECT: case DOP_FR_SELECT: return 3;
        case DOP_SELIND: case DOP_FR_SELIND: return 2 * n;
        case DOP_BITS2NUM: case DOP_LIMBS2NUM: return n;
        case DOP_GLPERM: return 12;
        case DOP_BNPERM: return 4;
        default: return 0;
    }
}

int main() {
    const TapeLimits M = limits();
    // ---- tape A: every op but the long lists
    Tape A;
    const size_t a_skip = A.op(DOP_SKIP, 0, 0, {7, 0, 300, 0});
    const size_t a_const = A.op(DOP_CONST1, 0, 0, {p64(2), 1});
    const size_t a_f_local = A.op(DOP_FETCH, 1, 0, {mkref(RK_LOCAL, W64, 5), 300});
    const size_t a_f_imp = A.op(DOP_FETCH, 2, 0, {mkref(RK_IMPORT, W128, 1), 301});
    const size_t a_f_litfr = A.op(DOP_FETCH, 4, 0, {mkref(RK_LITFR, WFR, 9), 303});
    const size_t a_f_lit64 = A.op(DOP_FETCH, 1, 0, {mkref(RK_LIT64, W64, 2999), 307});
    const size_t a_f_in4 = A.op(DOP_FETCH, 4, 0, {mkref(RK_INPUT, WFR, 2), 308});
    const size_t a_f_in1 = A.op(DOP_FETCH, 1, 0, {mkref(RK_INPUT, W64, 1), 312});
    const size_t a_frcell = A.op(DOP_FRCELL, 0, 0, {ring(303, WFR), NO_SLOT});
    A.op(DOP_FRCELL, 0, 0, {pfr(9), 2});
    A.op(DOP_LOADW, 0, 0, {ring(312), 6});
    A.op(DOP_LOADW_DIV, 0, 0, {ring(6), p64(2047), 7});
    A.op(DOP_LOADW_EXTINV, 0, 1, {ring(6), ring(7), 8});
    const size_t a_glop = A.op(DOP_GLOP, 0, T_KA_GLOP, {p64(0), ring(7), ring(8), 9});
    const size_t a_gate = A.op(DOP_GATE, 0, T_GATE, {ring(9), ring(8), p64(1), 10});
    const size_t a_reduce = A.op(DOP_REDUCE, 0, 0, {ring(10, W128), 12});
    const size_t a_clt = A.op(DOP_CLT, 0, 0, {ring(12)});
    A.op(DOP_FR_ADD, 0, 0, {ring(2, WFR), pfr(0), 13});
    A.op(DOP_FR_MUL, 0, 0, {ring(13, WFR), ring(10, W128), 17});
    A.op(DOP_FR_MULADD, 0, 0, {ring(13, WFR), ring(17, WFR), ring(12), 21});
    A.op(DOP_SELECT, 0, 0, {ring(12), ring(9), ring(25), 26});
    A.op(DOP_FR_SELECT, 0, 0, {ring(21, WFR), ring(17, WFR), ring(25), 27});
    const size_t a_idx = A.op(DOP_IDX2IND, 3, 0, {ring(12), 31});
    A.op(DOP_SELIND, 1, 0, {ring(9), ring(31), 34});
    A.op(DOP_FR_SELIND, 2, 0, {ring(21, WFR), ring(12), ring(31), ring(32), 35});
    A.op(DOP_BITS2NUM, 0, 0, {39});
    A.op(DOP_BITS2NUM, 3, 0, {ring(31), ring(32), ring(33), 40});
    A.op(DOP_DECOMP565, 0, 0, {ring(35, WFR), 41});
    A.op(DOP_LIMBS2NUM, 4, 0, {ring(41), ring(42), ring(43), ring(44), 46});
    A.op(DOP_RANGE, 0, 10, {ring(41)});
    const size_t a_run2 = A.op(DOP_GLOPRUN, 2, 0, {130, ring(41), ring(42), p64(0), 50u | ((uint32_t)T_GLOP << 24), ring(50), ring(43), ring(44), 51u | ((uint32_t)T_KB_GLOP << 24)});
    std::vector<uint32_t> st12; for (uint32_t i = 0; i < 12; i++) st12.push_back(i < 5 ? ring(41 + i) : p64(i));
    std::vector<uint32_t> glp = st12; glp.push_back(60); glp.push_back(1); glp.push_back(123456);
    const size_t a_glperm = A.opv(DOP_GLPERM, 0, 0, glp);
    const size_t a_bnperm = A.op(DOP_BNPERM, 0, 0, {ring(46, WFR), pfr(1), ring(60), ring(10, W128), 72, 0, 4032});
    const size_t a_end = A.op(DOP_END, 0, 0, {});
    accept(A, M, "tape A");
    // ---- tape B: the long lists (n = 64, a run of 255)
    Tape B;
    std::vector<uint32_t> sel; for (uint32_t i = 0; i < 128; i++) sel.push_back(ring(i)); sel.push_back(200);
    const size_t b_sel = B.opv(DOP_SELIND, 64, 0, sel);
    sel.back() = 201; B.opv(DOP_FR_SELIND, 64, 0, sel);
    B.op(DOP_NUM2BITS, 64, 0, {ring(200), 205});
    B.op(DOP_IDX2IND, 64, 0, {ring(200), 336});
    std::vector<uint32_t> bits; for (uint32_t i = 0; i < 64; i++) bits.push_back(ring(205 + i)); bits.push_back(399);
    B.opv(DOP_BITS2NUM, 64, 0, bits);
    std::vector<uint32_t> run; run.push_back(255 * 65);
    for (uint32_t i = 0; i < 255; i++) { run.push_back(ring(i)); run.push_back(p64(i)); run.push_back(ring(i + 1)); run.push_back((i + 100) | ((uint32_t)T_GLOP << 24)); }
    const size_t b_run = B.opv(DOP_GLOPRUN, 255, 0, run);
    const size_t b_clt = B.op(DOP_CLT, 0, 0, {ring(399)});
    B.op(DOP_END, 0, 0, {});
    accept(B, M, "tape B");
    // ---- tape C: the fetches in front of one op fill the ring exactly (RING_K slots: 64 four-word fetches); the op between two such stretches starts the count anew
    Tape C;
    for (uint32_t i = 0; i < 64; i++) C.op(DOP_FETCH, 4, 0, {mkref(RK_IMPORT, WFR, 1), 4 * i});
    std::vector<uint32_t> wsel; for (uint32_t i = 0; i < 64; i++) wsel.push_back(ring(4 * i, WFR)); for (uint32_t i = 0; i < 64; i++) wsel.push_back(p64(i)); wsel.push_back(256);
    C.opv(DOP_FR_SELIND, 64, 0, wsel);
    for (uint32_t i = 0; i < 63; i++) C.op(DOP_FETCH, 4, 0, {mkref(RK_IMPORT, WFR, 0), 260 + 2 * i});
    const size_t c_last4 = C.op(DOP_FETCH, 3, 0, {mkref(RK_LOCAL, WFR, 0), 390});
    const size_t c_last = C.op(DOP_FETCH, 1, 0, {mkref(RK_LOCAL, W64, 3), 393});
    C.op(DOP_CLT, 0, 0, {ring(393)});
    C.op(DOP_END, 0, 0, {});
    accept(C, M, "tape C");
    { Tape E; E.op(DOP_END, 0, 0, {}); accept(E, M, "the empty tape"); TapeLimits Z; accept(E, Z, "the empty tape, no limits"); }

    typedef std::vector<uint32_t> V;
    // ---- a length byte off by one
    refuse(A, M, "GLOP one word longer", malformed(a_glop, DOP_GLOP), [&](V &w, TapeLimits &) { w[a_glop] += 1u << 24; });
    refuse(A, M, "GLOP one word shorter", malformed(a_glop, DOP_GLOP), [&](V &w, TapeLimits &) { w[a_glop] -= 1u << 24; });
    refuse(A, M, "SKIP one word longer", malformed(a_skip, DOP_SKIP), [&](V &w, TapeLimits &) { w[a_skip] += 1u << 24; });
    refuse(A, M, "FETCH one word shorter", malformed(a_f_imp, DOP_FETCH), [&](V &w, TapeLimits &) { w[a_f_imp] -= 1u << 24; });
    refuse(A, M, "GLPERM one word longer", malformed(a_glperm, DOP_GLPERM), [&](V &w, TapeLimits &) { w[a_glperm] += 1u << 24; });
    refuse(A, M, "BNPERM one word shorter", malformed(a_bnperm, DOP_BNPERM), [&](V &w, TapeLimits &) { w[a_bnperm] -= 1u << 24; });
    refuse(B, M, "SELIND n = 64 one word longer", malformed(b_sel, DOP_SELIND), [&](V &w, TapeLimits &) { w[b_sel] += 1u << 24; });
    refuse(B, M, "SELIND n = 64 with n = 63", malformed(b_sel, DOP_SELIND), [&](V &w, TapeLimits &) { w[b_sel] -= 1u << 8; });
    refuse(B, M, "a run of 255 as a run of 254", malformed(b_run + 2 + 4 * 254, 254), [&](V &w, TapeLimits &) { w[b_run] -= 1u << 8; });      // (the run's last entry is then read as an op: its first word, the ring ref of slot 254)
    refuse(A, M, "a run of 1", malformed(a_run2, DOP_GLOPRUN), [&](V &w, TapeLimits &) { w[a_run2] -= 1u << 8; });
    refuse(A, M, "IDX2IND n = 0", malformed(a_idx, DOP_IDX2IND), [&](V &w, TapeLimits &) { w[a_idx] &= ~0xff00u; });
    refuse(A, M, "IDX2IND n = 65", malformed(a_idx, DOP_IDX2IND), [&](V &w, TapeLimits &) { w[a_idx] = (w[a_idx] & ~0xff00u) | (65u << 8); });
    refuse(A, M, "the last op runs past the tape", malformed(a_bnperm, DOP_BNPERM), [&](V &w, TapeLimits &) { w.resize(a_bnperm + 5); });
    // ---- operands
    refuse(A, M, "operand bit 29", malformed(a_gate, DOP_GATE), [&](V &w, TapeLimits &) { w[a_gate + 1] |= 1u << 29; });
    refuse(A, M, "operand bit 30", malformed(a_gate, DOP_GATE), [&](V &w, TapeLimits &) { w[a_gate + 3] |= 1u << 30; });
    refuse(A, M, "operand width 3", malformed(a_gate, DOP_GATE), [&](V &w, TapeLimits &) { w[a_gate + 2] |= 3u << 27; });
    refuse(A, M, "ring ref bit 8", malformed(a_gate, DOP_GATE), [&](V &w, TapeLimits &) { w[a_gate + 1] |= 1u << 8; });
    refuse(A, M, "ring ref bit 26", malformed(a_gate, DOP_GATE), [&](V &w, TapeLimits &) { w[a_gate + 2] |= 1u << 26; });
    refuse(B, M, "ring ref bit 17 in a run", malformed(b_run, DOP_GLOPRUN), [&](V &w, TapeLimits &) { w[b_run + 2 + 4 * 200] |= 1u << 17; });
    refuse(A, M, "pool offset misaligned", malformed(a_const, DOP_CONST1), [&](V &w, TapeLimits &) { w[a_const + 1] += 4; });
    refuse(A, M, "pool offset below the pools (in the ring)", malformed(a_const, DOP_CONST1), [&](V &w, TapeLimits &) { w[a_const + 1] = fastref_pool(W64, LDS_POOL64 - 8); });
    refuse(A, M, "pool64 entry past the LDS part", malformed(a_const, DOP_CONST1), [&](V &w, TapeLimits &L) { L.npoolfr = 0; w[a_const + 1] = p64(POOL64_CAP); });
    refuse(A, M, "poolfr entry past the LDS part", malformed(a_const, DOP_CONST1), [&](V &w, TapeLimits &L) { L.npoolfr = POOLFR_CAP + 20; w[a_const + 1] = pfr(POOLFR_CAP); });
    refuse(A, M, "poolfr entry past the pool", malformed(a_const, DOP_CONST1), [&](V &w, TapeLimits &) { w[a_const + 1] = pfr(10); });
    refuse(A, M, "pool64 entry across the pool end", malformed(a_const, DOP_CONST1), [&](V &w, TapeLimits &L) { L.npool64 = 3; L.npoolfr = 0; w[a_const + 1] = p64(2, W128); });
    refuse(A, M, "poolfr entry across the pool end", malformed(a_const, DOP_CONST1), [&](V &w, TapeLimits &) { w[a_const + 1] = fastref_pool(WFR, LDS_POOLFR + 9 * 32 + 8); });
    refuse(A, M, "REDUCE of a one-word operand", malformed(a_reduce, DOP_REDUCE), [&](V &w, TapeLimits &) { w[a_reduce + 1] = ring(10, W64); });
    refuse(A, M, "GLPERM with a two-word operand", malformed(a_glperm, DOP_GLPERM), [&](V &w, TapeLimits &) { w[a_glperm + 12] = ring(10, W128); });
    refuse(A, M, "GLOP with a dynamic template", malformed(a_glop, DOP_GLOP), [&](V &w, TapeLimits &) { w[a_glop] = (w[a_glop] & ~0xff0000u) | ((uint32_t)T_DYNAMIC << 16); });
    // ---- result slots
    refuse(A, M, "GATE result past the slots", malformed(a_gate, DOP_GATE), [&](V &w, TapeLimits &) { w[a_gate + 4] = 399; });
    refuse(A, M, "FRCELL result past the slots", malformed(a_frcell, DOP_FRCELL), [&](V &w, TapeLimits &) { w[a_frcell + 2] = 397; });
    refuse(A, M, "IDX2IND results past the slots", malformed(a_idx, DOP_IDX2IND), [&](V &w, TapeLimits &) { w[a_idx + 2] = 398; });
    refuse(A, M, "a slot of a smaller segment", malformed(a_const, DOP_CONST1), [&](V &, TapeLimits &L) { L.nslots = 1; });
    refuse(A, M, "GLPERM result NO_SLOT", malformed(a_glperm, DOP_GLPERM), [&](V &w, TapeLimits &) { w[a_glperm + 13] = NO_SLOT; });
    refuse(A, M, "BNPERM result NO_SLOT", malformed(a_bnperm, DOP_BNPERM), [&](V &w, TapeLimits &) { w[a_bnperm + 5] = NO_SLOT; });
    refuse(A, M, "GLPERM results past the slots", malformed(a_glperm, DOP_GLPERM), [&](V &w, TapeLimits &) { w[a_glperm + 13] = 389; });
    refuse(A, M, "BNPERM results past the slots", malformed(a_bnperm, DOP_BNPERM), [&](V &w, TapeLimits &) { w[a_bnperm + 5] = 385; });
    refuse(A, M, "a run's result past the slots", malformed(a_run2, DOP_GLOPRUN), [&](V &w, TapeLimits &) { w[a_run2 + 9] = 400u | ((uint32_t)T_GLOP << 24); });
    refuse(A, M, "a run's template dynamic", malformed(a_run2, DOP_GLOPRUN), [&](V &w, TapeLimits &) { w[a_run2 + 5] = 50u | ((uint32_t)T_DYNAMIC << 24); });
    refuse(B, M, "the last template of a run of 255 dynamic", malformed(b_run, DOP_GLOPRUN), [&](V &w, TapeLimits &) { w[b_run + 5 + 4 * 254] |= 0xff000000u; });
    // ---- DOP_FETCH: the old-style ref, kind by kind; its destination
    refuse(A, M, "FETCH of a local slot past the slots", malformed(a_f_local, DOP_FETCH), [&](V &w, TapeLimits &) { w[a_f_local + 1] = mkref(RK_LOCAL, W128, 399); });
    refuse(A, M, "FETCH of an import past the table", malformed(a_f_imp, DOP_FETCH), [&](V &w, TapeLimits &) { w[a_f_imp + 1] = mkref(RK_IMPORT, W128, 2); });
    refuse(A, M, "FETCH of a pool64 entry past the pool", malformed(a_f_lit64, DOP_FETCH), [&](V &w, TapeLimits &) { w[a_f_lit64 + 1] = mkref(RK_LIT64, W64, 3000); });
    refuse(A, M, "FETCH of a proof word past the segment's inputs", malformed(a_f_in1, DOP_FETCH), [&](V &w, TapeLimits &) { w[a_f_in1 + 1] = mkref(RK_INPUT, W64, 3); });
    refuse(A, M, "FETCH of a poolfr entry past the pool", malformed(a_f_litfr, DOP_FETCH), [&](V &w, TapeLimits &) { w[a_f_litfr + 1] = mkref(RK_LITFR, WFR, 10); });
    refuse(A, M, "FETCH with a ring ref", malformed(a_f_local, DOP_FETCH), [&](V &w, TapeLimits &) { w[a_f_local + 1] = mkref(RK_RING, W64, 5); });
    refuse(A, M, "FETCH of four proof words from word 98 of 100", malformed(a_f_in1, DOP_FETCH), [&](V &w, TapeLimits &) { w[a_f_in1 + 1] = mkref(RK_INPUT, WFR, 1); });
    refuse(A, M, "FETCH of a proof word of a shorter proof", malformed(a_f_in4, DOP_FETCH), [&](V &, TapeLimits &L) { L.proof_words = 99; });
    refuse(A, M, "FETCH into slots past the segment's", malformed(a_f_in4, DOP_FETCH), [&](V &w, TapeLimits &) { w[a_f_in4 + 2] = 397; });
    refuse(A, M, "FETCH of five words", malformed(a_f_in4, DOP_FETCH), [&](V &w, TapeLimits &) { w[a_f_in4] += 1u << 8; });
    refuse(A, M, "FETCH of no word", malformed(a_f_local, DOP_FETCH), [&](V &w, TapeLimits &) { w[a_f_local] -= 1u << 8; });
    // ---- more fetched slots in front of one op than the ring holds: the later ones would overwrite the earlier ones (slot mod RING_K)
    refuse(C, M, "257 slots fetched in front of one op", malformed(c_last, DOP_FETCH), [&](V &w, TapeLimits &) { w[c_last4] += 1u << 8; });
    refuse(C, M, "258 slots fetched: the first fetch past the ring is named", malformed(c_last, DOP_FETCH), [&](V &w, TapeLimits &) { w[c_last4] += 1u << 8; w[c_last] += 1u << 8; });
    // ---- the fused permutations' trailing words
    refuse(A, M, "GLPERM list slot", malformed(a_glperm, DOP_GLPERM), [&](V &w, TapeLimits &) { w[a_glperm + 14] = 2; });
    refuse(A, M, "BNPERM list slot", malformed(a_bnperm, DOP_BNPERM), [&](V &w, TapeLimits &) { w[a_bnperm + 6] = 2; });
    refuse(A, M, "GLPERM without the flag", malformed(a_glperm, DOP_GLPERM), [&](V &, TapeLimits &L) { L.fusing_gl = false; });
    refuse(A, M, "BNPERM without the flag", malformed(a_bnperm, DOP_BNPERM), [&](V &, TapeLimits &L) { L.fusing_bn = false; });
    refuse(A, M, "GLPERM cell count", malformed(a_glperm, DOP_GLPERM), [&](V &w, TapeLimits &) { w[a_glperm + 15] += 1; });
    refuse(A, M, "BNPERM cell count", malformed(a_bnperm, DOP_BNPERM), [&](V &w, TapeLimits &) { w[a_bnperm + 7] = 4033; });
    refuse(A, M, "GLPERM on a record block of another size", malformed(a_glperm, DOP_GLPERM), [&](V &, TapeLimits &L) { L.glp_recs = 2603; });
    // ---- op codes, the end
    refuse(A, M, "the first unknown op code", malformed(a_clt, DOP_COUNT), [&](V &w, TapeLimits &) { w[a_clt] = (w[a_clt] & ~0xffu) | DOP_COUNT; });
    refuse(B, M, "op code 255", malformed(b_clt, 255), [&](V &w, TapeLimits &) { w[b_clt] |= 0xffu; });
    refuse(A, M, "no DOP_END", NO_END, [&](V &w, TapeLimits &) { w.pop_back(); });
    refuse(A, M, "a word behind DOP_END", NO_END, [&](V &w, TapeLimits &) { w.push_back(DOP_END | (1u << 24)); });
    refuse(A, M, "DOP_END in the middle", NO_END, [&](V &w, TapeLimits &) { w[a_clt] = DOP_END | (1u << 24); });
    refuse(A, M, "DOP_END of two words", NO_END, [&](V &w, TapeLimits &) { w[a_end] = DOP_END | (2u << 24); });
    { Tape E; const std::string e = tape_check(E.w.data(), 0, M); n_corruptions++; CHECK(e == NO_END, "no word at all: \"%s\"", e.c_str()); }

    // ---- operand_span is the table, and the table is what the lowering always used
    for (uint32_t op = 0; op < DOP_COUNT + 3; op++)
        for (uint32_t n : {0u, 1u, 64u}) {
            uint32_t first = 99, count = 99; operand_span(op, n, first, count);
            const uint32_t tab = op < DOP_COUNT ? OP_DESC[op].nops + OP_DESC[op].nops_per_n * n : 0;
            CHECK(first == 1 && count == tab && count == operands_by_hand(op, n), "operand_span(%u, %u) = [%u, +%u), the table has %u, by hand %u", op, n, first, count, tab, operands_by_hand(op, n));
        }
    if (failures) { printf("%d FAILED\n", failures); return 1; }
    printf("OK tapes: %d corruptions: %d\n", n_tapes, n_corruptions);
    return 0;
}
