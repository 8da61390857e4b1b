// tapefmt.h — the device tape of a traced plan, stated once: the words the lowering (tracelower.cpp) emits, tape_check verifies and the
// interpreter (replay.hip k_replay) follows.  Plain C++: no HIP, so the checker compiles and is tested on the host (tests/cpp/tapefmt_check.cpp).
//
// A tape is a sequence of ops, word 0 of each = op | n << 8 | aux << 16 | (words of the op) << 24, then its operand refs, then (ops with results)
// the first output slot, then (some ops) trailing words; it ends in DOP_END.  OP_DESC below gives that shape per op; the ops it cannot express
// (DOP_FETCH, DOP_GLOPRUN, the trailing words of the fused permutations, the chain of a split select's parts) have their few lines in tape_check next to it.  The interpreter keeps its
// own hand-written decode (its scalar-register window depends on it) and takes only the names from here.
#pragma once
#include <cstdint>
#include <string>
#include "records.h"
#include "field.h"

namespace h2w {

enum { W64 = 0, W128 = 1, WFR = 2 };
enum { RK_LOCAL = 0, RK_IMPORT = 1, RK_LIT64 = 2, RK_INPUT = 3, RK_LITFR = 4, RK_RING = 5 };
constexpr uint32_t RING_K = 256;      // value slots of a lane kept in LDS (64 lanes x 256 x 8 B = 128 KB per block)
// LDS of a block: the ring, then the constant pools (as far as they fit: the rest is fetched like any far operand)
constexpr uint32_t LDS_RING_BYTES = RING_K * 64 * 8, POOL64_CAP = 2048, POOLFR_CAP = 472;
constexpr uint32_t LDS_POOL64 = LDS_RING_BYTES, LDS_POOLFR = LDS_POOL64 + POOL64_CAP * 8, LDS_WORDS = (LDS_POOLFR + POOLFR_CAP * 32) / 8;
// An operand word of a compute op ("fast ref"): bit 31 set: the ring, bits 0..7 = slot mod 256 (word j of the value at slot + j); bit 31 clear: a pool
// entry in LDS, bits 0..17 = its byte offset (word j at + 8 j); bits 27..28: the width as before.  Everything else (a far slot, an enclosing segment's
// value, a proof word, a pool entry beyond the LDS part) is brought into the ring by a DOP_FETCH in front of the op, which carries the old-style ref.
HD uint32_t fastref_ring(int width, uint32_t slot) { return 0x80000000u | ((uint32_t)width << 27) | (slot & (RING_K - 1)); }
HD uint32_t fastref_pool(int width, uint32_t byte_off) { return ((uint32_t)width << 27) | byte_off; }
HD uint32_t mkref(int kind, int width, uint32_t idx) { return ((uint32_t)kind << 29) | ((uint32_t)width << 27) | idx; }
HD int ref_kind(uint32_t r) { return (int)(r >> 29); }
HD int ref_width(uint32_t r) { return (int)((r >> 27) & 3); }
HD uint32_t ref_idx(uint32_t r) { return r & ((1u << 27) - 1); }
constexpr int SLOTS_OF[3] = {1, 2, 4};
constexpr uint32_t NO_SLOT = 0xffffffffu;
// device ops; word 0 = op | n << 8 | aux << 16 | (words of the op) << 24, then operand refs, then (ops with results) the first output slot
enum { DOP_END = 0, DOP_SKIP, DOP_CONST1, DOP_FRCELL, DOP_LOADW, DOP_LOADW_DIV, DOP_LOADW_EXTINV, DOP_GLOP, DOP_GATE, DOP_REDUCE, DOP_CLT,
       DOP_FR_ADD, DOP_FR_MUL, DOP_FR_MULADD, DOP_SELECT, DOP_FR_SELECT, DOP_IDX2IND, DOP_SELIND, DOP_FR_SELIND, DOP_NUM2BITS, DOP_BITS2NUM,
       DOP_DECOMP565, DOP_LIMBS2NUM, DOP_RANGE, DOP_FETCH,
       DOP_GLOPRUN,        // n consecutive DOP_GLOP ops as one: [hdr][cells of the run][A, B, C, out slot | template << 24] x n (2 + 4 n words: its length is NOT in the header)
       DOP_GLPERM,         // a verified Goldilocks-Poseidon permutation as one op (H2W_TRACE_FUSE_GL_PERMUTE): [hdr][12 operands][first output slot][list slot][cells of its record block]
       DOP_BNPERM,         // a verified PoseidonBN254 permutation as one op (H2W_TRACE_FUSE_BN_PERMUTE): [hdr][4 operands][first output slot (4 x 4 slots)][list slot][its cells]
       DOP_COUNT };
// A wide select_by_indicator whose fetched operands do not fit the ring is cut at entry boundaries into PARTS (H2W_TRACE_SPLIT_SELECTS): consecutive
// DOP_FR_SELIND ops, each over a contiguous run of the entries and their indicators, its own DOP_FETCH ops in front of it.  The aux byte of a part
// (0: a whole select) says where it stands in the chain; the running sum passes from a part to the next in the lane's registers, it has no value slot.
constexpr uint32_t SELIND_CONTINUES = 1;      // not the first part: no leading zero cell, the sum starts from the previous part's
constexpr uint32_t SELIND_CONTINUED = 2;      // not the last part: another follows (nothing but its DOP_FETCH ops in between); its result is NO_SLOT
constexpr uint32_t GLPERM_WORDS = 16, BNPERM_WORDS = 8;
constexpr uint32_t GLPERM_IO = 12, BNPERM_IO = 4;      // the states of the two permutations (chips.h SPONGE_WIDTH, BN_WIDTH: asserted where both are seen)
// a list entry of a fused PoseidonBN254 permutation: {first cell of its block in the proof's stream, zero-cell flag (1: the Context's load_zero cell is
// cached, the block is the 4,032 cells), the 4 x 32-byte input state}
constexpr uint32_t BNP_LIST_WORDS = 18;
// ---- the plan's tables as the device reads them (here, not in tracelower.h: the lane tables, lanetable.h, are plain C++ too)
// unit: the depth-1 parallel instance (shard unit) the instance is or lies in, NO_SLOT for the root; ucell0: that unit's first cell (root: 0)
// glp0: the instance's first entry in the proof's list of fused permutations
struct InstD { uint64_t cell0, rec0, ucell0; uint32_t imp0, in0, unit, glp0; };
struct ImpD { uint32_t tmpl, inst, slot; };
struct TmplD { uint32_t tape0, nslots, ninst, inst0, depth; };
// a listed PoseidonBN254 permutation, static per plan: its first cell in the proof's stream, its shard unit (NO_SLOT: the root's block), that unit's first cell
struct BnpD { uint64_t cell0, ucell0; uint32_t unit, pad; };

// ---- the shape of every op
// How many words of an operand the interpreter reads is the ref's own width field (get64(r, 0) for a one-word operand, getfr(r) by width for a
// native one); tape_check bounds a pool ref by that width, a ring ref needs no bound.  The column "reads" below is therefore a comment, not data.
enum { WC_ANY = 0, WC_NOT64, WC_IS64 };               // a constraint on the width field of every operand
enum { RS_NONE = 0, RS_FIXED, RS_N };                 // result slots: none (no slot word), res_slots, n
struct OpDesc {
    bool table;                    // false: DOP_END, DOP_FETCH, DOP_GLOPRUN - their shape is tape_check's special case, they have no fast-ref operands
    uint8_t nops, nops_per_n;      // operand words: nops + nops_per_n * n
    uint8_t wcons;                 // WC_*
    uint8_t res, res_slots;        // RS_*; the slots of an RS_FIXED result
    bool no_slot_ok;               // NO_SLOT may stand for the result (a static value: nothing is stored)
    uint8_t trailing;              // words behind the operands and the result slot
    uint8_t n_min, n_max;          // bounds of n (0, 255: n is not read)
    bool aux_is_tmpl;              // aux is a record template: < T_DYNAMIC
};
constexpr OpDesc OP_SPECIAL = {false, 0, 0, WC_ANY, RS_NONE, 0, false, 0, 0, 255, false};
constexpr OpDesc op_fixed(uint8_t nops, uint8_t res, uint8_t res_slots, uint8_t wcons = WC_ANY, bool aux_is_tmpl = false) { return OpDesc{true, nops, 0, wcons, res, res_slots, true, 0, 0, 255, aux_is_tmpl}; }
constexpr OpDesc op_list(uint8_t per_n, uint8_t res_slots, uint8_t n_min) { return OpDesc{true, 0, per_n, WC_ANY, RS_FIXED, res_slots, true, 0, n_min, 64, false}; }
constexpr OpDesc op_array(uint8_t nops) { return OpDesc{true, nops, 0, WC_ANY, RS_N, 0, true, 0, 1, 64, false}; }      // n results in consecutive slots
constexpr OpDesc OP_DESC[DOP_COUNT] = {
    /* DOP_END          */ OP_SPECIAL,
    /* DOP_SKIP         */ {true, 0, 0, WC_ANY, RS_NONE, 0, false, 4, 0, 255, false},      // [hdr][records, lo hi][cells, lo hi] of a nested segment
    /* DOP_CONST1       */ op_fixed(1, RS_FIXED, 1),                       // reads 1
    /* DOP_FRCELL       */ op_fixed(1, RS_FIXED, 4),                       // reads 4
    /* DOP_LOADW        */ op_fixed(1, RS_FIXED, 1),                       // reads 1
    /* DOP_LOADW_DIV    */ op_fixed(2, RS_FIXED, 1),                       // reads 1, 1
    /* DOP_LOADW_EXTINV */ op_fixed(2, RS_FIXED, 1),                       // reads 1, 1
    /* DOP_GLOP         */ op_fixed(3, RS_FIXED, 1, WC_ANY, true),         // reads 1, 1, 1
    /* DOP_GATE         */ op_fixed(3, RS_FIXED, 2),                       // reads 1, 1, 1
    /* DOP_REDUCE       */ op_fixed(1, RS_FIXED, 1, WC_NOT64),             // reads 2
    /* DOP_CLT          */ op_fixed(1, RS_NONE, 0),                        // reads 1
    /* DOP_FR_ADD       */ op_fixed(2, RS_FIXED, 4),                       // reads 4, 4
    /* DOP_FR_MUL       */ op_fixed(2, RS_FIXED, 4),                       // reads 4, 4
    /* DOP_FR_MULADD    */ op_fixed(3, RS_FIXED, 4),                       // reads 4, 4, 4
    /* DOP_SELECT       */ op_fixed(3, RS_FIXED, 1),                       // reads 1, 1, 1
    /* DOP_FR_SELECT    */ op_fixed(3, RS_FIXED, 4),                       // reads 4, 4, 1
    /* DOP_IDX2IND      */ op_array(1),                                    // reads 1  (NO_SLOT passes for its n results although the interpreter stores them unconditionally: the lowering never emits it)
    /* DOP_SELIND       */ op_list(2, 1, 1),                               // reads 1 x n, 1 x n
    /* DOP_FR_SELIND    */ op_list(2, 4, 1),                               // reads 4 x n, 1 x n; aux: SELIND_* bits (a part of a split select: tape_check holds the chain)
    /* DOP_NUM2BITS     */ op_array(1),                                    // reads 1  (NO_SLOT: as DOP_IDX2IND)
    /* DOP_BITS2NUM     */ op_list(1, 1, 0),                               // reads 1 x n
    /* DOP_DECOMP565    */ op_fixed(1, RS_FIXED, 5),                       // reads 4  (NO_SLOT: as DOP_IDX2IND)
    /* DOP_LIMBS2NUM    */ op_list(1, 4, 0),                               // reads 1 x n
    /* DOP_RANGE        */ op_fixed(1, RS_NONE, 0),                        // reads 1
    /* DOP_FETCH        */ OP_SPECIAL,
    /* DOP_GLOPRUN      */ OP_SPECIAL,
    /* DOP_GLPERM       */ {true, GLPERM_IO, 0, WC_IS64, RS_FIXED, GLPERM_IO, false, 2, 0, 255, false},      // reads 1 x 12; trailing: list slot, cells (tape_check)
    /* DOP_BNPERM       */ {true, BNPERM_IO, 0, WC_ANY, RS_FIXED, 4 * BNPERM_IO, false, 2, 0, 255, false},   // reads 4 x 4; trailing: list slot, cells
};
// words of a table op (DOP_GLOPRUN: 2 + 4 n, not in its header; DOP_FETCH: 3; DOP_END: 1)
constexpr uint32_t op_words(const OpDesc &d, uint32_t n) { return 1u + d.nops + d.nops_per_n * n + (d.res != RS_NONE ? 1u : 0u) + d.trailing; }
static_assert(op_words(OP_DESC[DOP_GLPERM], 0) == GLPERM_WORDS && op_words(OP_DESC[DOP_BNPERM], 0) == BNPERM_WORDS, "the fused ops' word counts");
// operand words of an op (the fast refs the lowering rewrites): [first, first + count)
inline void operand_span(uint32_t op, uint32_t n, uint32_t &first, uint32_t &count) {
    first = 1; count = op < DOP_COUNT ? OP_DESC[op].nops + OP_DESC[op].nops_per_n * n : 0;
}

// ---- the check: every word the device will follow - op lengths, operand kinds and indices, result slots (a wild reference is a GPU fault)
struct TapeLimits {
    size_t tmpl = 0;                                     // the template the tape belongs to (for the message)
    uint32_t nslots = 0; size_t nimps = 0;               // value slots of the segment; its imports
    const uint32_t *inputs = nullptr; size_t ninputs = 0; uint64_t proof_words = 0;      // its proof words (indices into the proof)
    size_t npool64 = 0, npoolfr = 0;                     // entries of the two constant pools
    uint32_t nglp = 0, nbnp = 0;                         // fused permutations of the segment (its list slots)
    bool fusing_gl = false, fusing_bn = false;           // the plan's flags
    uint64_t glp_block_cells = 0;                        // cells of a Goldilocks permutation's record block
    size_t glp_recs = 0, glp_recs_kernel = 0;            // its records as the lowering laid them out; as the emission kernel writes them (glcoop.h GLP_RECS)
    uint64_t bn_perm_cells = 0;                          // cells of a PoseidonBN254 permutation (bntab.h BN_PERM_CELLS)
};
// empty: the tape is well formed; else "internal: malformed device tape (template t, word w, op o)" (w: the first word of the op) or "... does not end"
inline std::string tape_check(const uint32_t *T, size_t nwords, const TapeLimits &M) {
    auto okslow = [&](uint32_t r) {      // the old-style ref a DOP_FETCH carries
        const uint32_t i = ref_idx(r); const int k = ref_kind(r), w = ref_width(r);
        if (w > WFR) return false;
        const uint32_t span = k == RK_LITFR ? 4u : (uint32_t)(k == RK_INPUT ? (w == WFR ? 4 : 1) : SLOTS_OF[w]);
        switch (k) {
            case RK_LOCAL: return (uint64_t)i + span <= M.nslots;
            case RK_IMPORT: return i < M.nimps;
            case RK_LIT64: return (uint64_t)i + span <= M.npool64;
            case RK_INPUT: return i < M.ninputs && (uint64_t)M.inputs[i] + span <= M.proof_words;
            case RK_LITFR: return i < M.npoolfr;
            default: return false;
        }
    };
    const uint32_t lds64 = (uint32_t)(M.npool64 < POOL64_CAP ? M.npool64 : POOL64_CAP) * 8, ldsfr = (uint32_t)(M.npoolfr < POOLFR_CAP ? M.npoolfr : POOLFR_CAP) * 32;
    auto okref = [&](uint32_t r) {       // a fast ref: bounded by its own width field, which is what the interpreter reads by
        if (r & 0x60000000u) return false;
        const uint32_t w = (r >> 27) & 3u; if (w > WFR) return false;
        if (r >> 31) return (r & 0x07ffff00u) == 0;
        const uint32_t off = r & 0x07ffffffu, span = w == WFR ? 32u : w == W128 ? 16u : 8u;
        return (off & 7u) == 0 && ((off >= LDS_POOL64 && off + span <= LDS_POOL64 + lds64) || (off >= LDS_POOLFR && off + span <= LDS_POOLFR + ldsfr));
    };
    auto okout = [&](uint32_t slot, uint32_t nsl, bool no_slot_ok) { return slot == NO_SLOT ? no_slot_ok : (uint64_t)slot + nsl <= M.nslots; };
    size_t pc = 0; bool ended = false;
    uint32_t fetched = 0;      // slots the DOP_FETCH ops in front of one op have written: beyond RING_K the later ones overwrite the earlier ones (slot mod RING_K) before the op reads them
    // the parts of a split select: a "continued" part is open until the next op that is no DOP_FETCH, which must be a "continues" part (the
    // interpreter carries the sum between exactly those two); a broken chain is reported at the part that is left without its neighbour
    const std::string selind = ", op " + std::to_string((int)DOP_FR_SELIND) + ")";
    bool open = false; size_t open_at = 0;
    auto broken = [&](size_t at) { return "internal: malformed device tape (template " + std::to_string(M.tmpl) + ", word " + std::to_string(at) + selind; };
    while (pc < nwords) {
        const uint32_t h = T[pc], op = h & 0xff, n = (h >> 8) & 0xff, len = op == DOP_GLOPRUN ? 2 + 4 * n : h >> 24; bool ok = len >= 1 && pc + len <= nwords;
        if (op != DOP_FETCH) {
            const bool continues = op == DOP_FR_SELIND && (((h >> 16) & 0xff) & SELIND_CONTINUES) != 0;
            if (open && !continues) return broken(open_at);
            if (!open && continues) return broken(pc);
            open = false;
        }
        if (op == DOP_END) { ended = ok && pc + 1 == nwords; break; }
        const uint32_t *R = T + pc;
        fetched = op == DOP_FETCH ? fetched + n : 0;
        if (ok && op == DOP_FETCH) ok = len == 3 && n >= 1 && n <= 4 && okslow(R[1]) && (uint64_t)R[2] + n <= M.nslots && fetched <= RING_K;
        else if (ok && op == DOP_GLOPRUN) {      // [hdr][cells][A, B, C, out slot | template << 24] x n
            ok = n >= 2;
            for (uint32_t k = 0; ok && k < n; k++) ok = okref(R[2 + 4 * k]) && okref(R[3 + 4 * k]) && okref(R[4 + 4 * k]) && (uint64_t)(R[5 + 4 * k] & 0xffffffu) + 1 <= M.nslots && (R[5 + 4 * k] >> 24) < T_DYNAMIC;
        } else if (ok) {
            ok = op < DOP_COUNT && OP_DESC[op].table;
            const OpDesc &D = OP_DESC[ok ? op : DOP_SKIP];
            ok = ok && len == op_words(D, n) && n >= D.n_min && n <= D.n_max && (!D.aux_is_tmpl || ((h >> 16) & 0xff) < T_DYNAMIC);
            const uint32_t nops = D.nops + D.nops_per_n * n;
            for (uint32_t k = 0; ok && k < nops; k++) { const uint32_t w = (R[1 + k] >> 27) & 3u; ok = okref(R[1 + k]) && (D.wcons == WC_ANY || (D.wcons == WC_IS64) == (w == W64)); }
            if (ok && D.res != RS_NONE) ok = okout(R[1 + nops], D.res == RS_N ? n : D.res_slots, D.no_slot_ok);
            // aux of the two selects: the narrow one is never split; a part that is continued stores no result (the last part does)
            if (ok && op == DOP_SELIND) ok = ((h >> 16) & 0xff) == 0;
            if (ok && op == DOP_FR_SELIND) {
                const uint32_t aux = (h >> 16) & 0xff; ok = aux <= (SELIND_CONTINUES | SELIND_CONTINUED);
                if (ok && (aux & SELIND_CONTINUED)) { ok = R[1 + nops] == NO_SLOT; open = true; open_at = pc; }
            }
            // the trailing words of the fused permutations: the plan was built with the flag; the op's slot in the segment's list; its cells
            if (ok && op == DOP_GLPERM) ok = M.fusing_gl && M.glp_recs == M.glp_recs_kernel && R[14] < M.nglp && R[15] == (uint32_t)M.glp_block_cells;
            if (ok && op == DOP_BNPERM) ok = M.fusing_bn && R[6] < M.nbnp && R[7] == (uint32_t)M.bn_perm_cells;
        }
        if (!ok) return "internal: malformed device tape (template " + std::to_string(M.tmpl) + ", word " + std::to_string(pc) + ", op " + std::to_string(op) + ")";
        pc += len;
    }
    return ended ? std::string() : std::string("internal: a device tape does not end");
}

// ---- what a tape holds (h2w_plan_trace_op_counts), counted on a tape that passed tape_check: out[op] for every op; out[DOP_COUNT + k]: the
// DOP_FETCH ops whose ref is of kind k (RK_LOCAL .. RK_LITFR); out[DOP_COUNT + RK_RING]: the longest DOP_GLOPRUN (kept as a maximum, not summed)
constexpr size_t TAPE_COUNTS = DOP_COUNT + RK_RING + 1;
inline void tape_op_counts(const uint32_t *T, size_t nwords, uint64_t *out) {
    for (size_t pc = 0; pc < nwords;) {
        const uint32_t h = T[pc], op = h & 0xff, n = (h >> 8) & 0xff, len = op == DOP_GLOPRUN ? 2 + 4 * n : h >> 24;
        if (op >= DOP_COUNT || len == 0 || pc + len > nwords) return;
        out[op]++;
        if (op == DOP_FETCH && ref_kind(T[pc + 1]) < RK_RING) out[DOP_COUNT + ref_kind(T[pc + 1])]++;
        if (op == DOP_GLOPRUN && n > out[DOP_COUNT + RK_RING]) out[DOP_COUNT + RK_RING] = n;
        if (op == DOP_END) return;
        pc += len;
    }
}

}  // namespace h2w
