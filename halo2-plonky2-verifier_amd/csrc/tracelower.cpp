// tracelower.cpp — from the tape an eager context recorded (trace.h) to the device program of a traced plan (tracelower.h: the stages, in the
// order h2w_plan_from_trace runs them).  Host code: it includes no kernel and launches nothing; the value backend appears once, to lay out the
// record block of a fused Goldilocks-Poseidon permutation as the emission kernel writes it.
// Which op becomes which template is decided on STATIC widths (a value is provably below 2^64 when a Goldilocks-level op, a bit decomposition, a
// one-word input ... produced it), never on the traced values: the layout of the records must not depend on the proof.
// The pieces: Lowering, the pass over the trace (LowerOptions; segments, scope_op, one method per trace op kind, operand_pass and split_select behind an
// op); LoweredOpObserver with its two readers of the lowered ops, MatcherSet (the stretch search) and RootCapture (the canonical tape's source);
// resolve_handle, a handle's cell as a ref, for the lowering's operands and the verdict's sides alike; clear_cells, the range clear of the two cell maps.
// A change here that is meant to change no table is held to it on the host: tools/lowering_digest.py over the dump of traceplan.cpp (H2W_LOWERING_DUMP).
// What brings HIP into a file without a kernel: field.h marks its functions __host__ __device__ once the unit is compiled as HIP (build.sh compiles
// every unit that way, and the annotations need the runtime header in front), and glp_block_layout instantiates ValBackend<LayoutSink> and the
// permutation chip over it (valbackend.h; glcoop.h for GLP_RECS, bntab.h for BN_PERM_CELLS), templates shared with the device sinks.  No function of the runtime is called.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include "tracelower.h"
#include "valbackend.h"
#include "glcoop.h"
#include "bntab.h"

namespace h2w {
static_assert(GLPERM_IO == (uint32_t)SPONGE_WIDTH && BNPERM_IO == (uint32_t)BN_WIDTH, "tapefmt.h states the permutations' widths on its own");

// ---- stretches of a tape that ARE a permutation (H2W_TRACE_FUSE_GL_PERMUTE, H2W_TRACE_FUSE_BN_PERMUTE).  A lowered op, before its operands become fast refs:
struct NormOp {
    uint32_t hdr = 0, nin = 0, ref[3] = {0, 0, 0}, out = NO_SLOT, slots_before = 0; fr_t lit[3] = {fr_zero(), fr_zero(), fr_zero()};      // hdr: op | n << 8 | aux << 16; ref: mkref words; lit: the value of a literal operand
    size_t tr0 = 0, tr1 = 0; uint64_t cell0 = 0, cell1 = 0, out_cell = 0; const TraceIn *tin = nullptr;               // the trace ops / cells it covers; its result handle; its operands on the trace
};
// an operand of the canonical tape: a literal (its value, kind and width), a value computed inside the stretch (the op that produced it, relative to the
// start; its width), one of the inputs
enum { CK_LIT = 0, CK_INTERIOR = 1, CK_INPUT = 2 };
struct CanonOp { uint32_t hdr, nin; uint8_t kind[3], rk[3], width[3]; uint64_t arg[3]; fr_t lit[3]; bool has_out; };
// nio: inputs = outputs (12 one-word values; 4 of width WFR).  in_any_width: an input may be of any width (nothing of the lowering depends on it: the
// PoseidonBN254 tape adds a wide constant to every input first); else an input is one word, as the canonical one.
struct Canon { int id = CANON_GL, nio = SPONGE_WIDTH; bool in_any_width = false; std::vector<CanonOp> ops; uint32_t out_prod[MAX_PERM_IO]; uint64_t ncells = 0; };
// One per segment and canonical tape: the ops arrive in tape order, one behind the lowering (a static CONST1 may still fuse with the GLOP behind it).  A
// partial match that fails restarts AT the failing op, not inside the failed part: a permutation may then stay interpreted (canonical tapes whose first
// ops repeat themselves), it is never fused wrongly.
struct Matcher {
    const Canon *cn; std::vector<Stretch> *found; int seg;
    NormOp pend; bool has_pend = false;
    size_t pos = 0; uint32_t slot0 = 0; std::vector<int32_t> prod;      // matched ops so far; the first slot of the stretch; slot - slot0 -> the op that wrote it
    bool bound[MAX_PERM_IO]; uint32_t bref[MAX_PERM_IO]; Stretch cur;
    void reset() { pos = 0; prod.clear(); }
    bool step(const NormOp &o) {
        const CanonOp &c = cn->ops[pos];
        if (o.hdr != c.hdr || o.nin != c.nin || (o.out != NO_SLOT) != c.has_out) return false;
        if (pos == 0) { slot0 = o.slots_before; for (int i = 0; i < cn->nio; i++) bound[i] = false; cur.tr0 = o.tr0; cur.cell0 = o.cell0; cur.seg = seg; cur.canon = cn->id; cur.nio = cn->nio; cur.const_bad = cur.escaped = false; }
        for (uint32_t k = 0; k < c.nin; k++) {
            const uint32_t r = o.ref[k]; const int rk = ref_kind(r);
            const bool interior = rk == RK_LOCAL && ref_idx(r) >= slot0;
            if (c.kind[k] == CK_LIT) { if (rk != (int)c.rk[k] || ref_width(r) != (int)c.width[k]) return false; if (!fr_eq(o.lit[k], c.lit[k])) cur.const_bad = true; }
            else if (c.kind[k] == CK_INTERIOR) { if (!interior || ref_width(r) != (int)c.width[k] || ref_idx(r) - slot0 >= prod.size() || prod[ref_idx(r) - slot0] != (int32_t)c.arg[k]) return false; }
            else {
                if (interior || (!cn->in_any_width && ref_width(r) != (int)c.width[k])) return false;
                const uint64_t n = c.arg[k];
                if (!bound[n]) { bound[n] = true; bref[n] = r; cur.in[n] = o.tin[k]; } else if (bref[n] != r) return false;
            }
        }
        if (o.out != NO_SLOT) { const uint32_t rel = o.out - slot0; if (prod.size() <= rel) prod.resize(rel + 1, -1); prod[rel] = (int32_t)pos; }
        for (int i = 0; i < cn->nio; i++) if (cn->out_prod[i] == pos) cur.out[i] = o.out_cell;
        if (++pos == cn->ops.size()) {
            cur.tr1 = o.tr1; cur.cell1 = o.cell1; bool all = true; for (int i = 0; i < cn->nio; i++) all = all && bound[i];
            if (all) found->push_back(cur);
            reset();
        }
        return true;
    }
    void commit() { if (!has_pend) return; has_pend = false; if (!step(pend)) { const bool retry = pos != 0; reset(); if (retry) { if (!step(pend)) reset(); } } }
    void feed(const NormOp &o) { commit(); pend = o; has_pend = true; }
    void drop_pending() { has_pend = false; }                   // the pending CONST1 became part of the op that follows
    void boundary() { commit(); reset(); }                      // a stretch never crosses a segment boundary
};
// ---- the two readers of the ops as lowered (NormOp), fed while the lowering runs: nothing keeps the ops of a whole tape
struct LoweredOpObserver {
    virtual ~LoweredOpObserver() {}
    virtual void op(int seg, const NormOp &o, bool replaces_previous) = 0;      // replaces_previous: the op before it in `seg`, a static CONST1, became part of this GLOP
    virtual void boundary(int seg) = 0;                                         // a parallel child starts here in `seg`
    virtual void end() = 0;                                                     // end of tape
};
// the search for permutation-shaped stretches (the first lowering of a fused plan): one Matcher per segment AND canonical tape, made when the segment's first op arrives
struct MatcherSet final : LoweredOpObserver {
    const std::vector<const Canon *> &cns; std::vector<Stretch> &found; std::vector<std::vector<Matcher>> of_seg;
    MatcherSet(const std::vector<const Canon *> &cns_, std::vector<Stretch> &found_) : cns(cns_), found(found_) {}
    std::vector<Matcher> &at(int seg) {
        if (of_seg.size() <= (size_t)seg) of_seg.resize((size_t)seg + 1);
        std::vector<Matcher> &ms = of_seg[(size_t)seg];
        if (ms.empty()) for (const Canon *cn : cns) { ms.emplace_back(); ms.back().cn = cn; ms.back().found = &found; ms.back().seg = seg; }
        return ms;
    }
    void op(int seg, const NormOp &o, bool replaces_previous) override { for (Matcher &m : at(seg)) { if (replaces_previous) m.drop_pending(); m.feed(o); } }
    void boundary(int seg) override { for (Matcher &m : at(seg)) m.boundary(); }
    void end() override { for (std::vector<Matcher> &ms : of_seg) for (Matcher &m : ms) m.commit(); }
};
// the lowered ops of the root segment as they are (the canonical tape is made from them)
struct RootCapture final : LoweredOpObserver {
    std::vector<NormOp> ops;
    void op(int seg, const NormOp &o, bool replaces_previous) override { if (seg != 0) return; if (replaces_previous) ops.pop_back(); ops.push_back(o); }
    void boundary(int) override {}
    void end() override {}
};
static uint64_t rc_cells(int L, uint64_t bits) { if (bits == 0) return 0; const uint64_t n = (bits + L - 1) / L, rem = bits % L; return (n > 1 ? 1 + 3 * (n - 1) : 0) + (rem ? 4 : 0); }

// The record block of one permutation as CoopSinkT::coop_poseidon_permute writes it (what k_glp_emit_traced runs): the sequential gadget on the
// value backend, which is how h2w_plan_compile lays a compiled plan's out.  meta: (template, cell relative to the block).
struct LayoutSink : SinkBase {
    std::vector<uint64_t> *meta; const TemplateTable *tt; uint64_t nrec = 0, cell_off = 0, ndirect = 0;
    void rec(int t, uint64_t, uint64_t, uint64_t, uint64_t) { meta->push_back(meta_pack((uint32_t)t, cell_off)); nrec++; cell_off += (uint64_t)tt->ncells(t); }
    void cell(const fr_t &) { ndirect++; cell_off++; }
    void skip(uint64_t, uint64_t) {}
};
static uint64_t glp_block_layout(const TemplateTable &tt, int L, const h2w_poseidon_consts_t *consts, std::vector<uint64_t> &meta) {
    LayoutSink sink; sink.meta = &meta; sink.tt = &tt;
    ValCfg cfg{}; cfg.L = L; cfg.P = fr_params_init();
    ValBackend<LayoutSink> be(sink, cfg, true);
    PoseidonPermutationChip<ValBackend<LayoutSink>> pg(be, consts);
    uint64_t st[SPONGE_WIDTH] = {0}; pg.permute(st);
    return sink.ndirect == 0 && sink.nrec == (uint64_t)GLP_RECS ? sink.cell_off : 0;
}

// ---- a handle's cell as an operand of something in segment s: the one map from a cell to a ref, for the lowering's operands and the verdict's sides
static bool is_ancestor(const std::vector<SegInfo> &segs, int a, int s) { for (int x = s; x >= 0; x = segs[(size_t)x].parent) if (x == a) return true; return false; }
struct ImportTable { std::vector<ImpD> &imps; std::map<std::pair<uint32_t, uint32_t>, uint32_t> &imp_of; };      // of the reading segment; ImpD::tmpl holds the producer SEGMENT
enum HandleWhy { HANDLE_OK = 0, HANDLE_NOT_TRACED, HANDLE_NOT_ENCLOSING };      // no traced call's result handle; a value of a scope that does not enclose s
// ref: a literal (a static value), a local slot, or an import through `it` (entered there when it is new).  width: the value's (W64 where there is none)
static HandleWhy resolve_handle(const Lowered &LW, int s, uint64_t cell, ImportTable it, uint32_t &ref, int &width) {
    ref = 0; width = W64;
    auto f = LW.val_of.find(cell);
    if (f == LW.val_of.end()) return HANDLE_NOT_TRACED;
    const ValInfo &v = LW.vals[f->second]; width = v.width;
    if (v.is_static) { ref = v.width == WFR ? mkref(RK_LITFR, WFR, v.lit) : mkref(RK_LIT64, W64, v.lit); return HANDLE_OK; }
    if ((int)v.seg == s) { ref = mkref(RK_LOCAL, v.width, v.slot); return HANDLE_OK; }
    if (!is_ancestor(LW.segs, (int)v.seg, s)) return HANDLE_NOT_ENCLOSING;
    const auto key = std::make_pair(v.seg, v.slot);
    auto im = it.imp_of.find(key);
    if (im == it.imp_of.end()) { it.imps.push_back(ImpD{v.seg, 0, v.slot}); im = it.imp_of.emplace(key, (uint32_t)it.imps.size() - 1).first; }
    ref = mkref(RK_IMPORT, v.width, im->second); return HANDLE_OK;
}

// ---- the lowering pass
// fused: the stretches to lower as ONE op (by their first trace op) and the record block of a Goldilocks one
// split_selects: a wide select whose fetched operands do not fit the ring is emitted as parts (tapefmt.h SELIND_*) instead of refused
static const Fusable NOTHING_FUSED;
struct LowerOptions { int L; const TemplateTable &tt; const char *const *parallel_scopes = nullptr; size_t n_scopes = 0; bool split_selects = false; const Fusable &fused = NOTHING_FUSED; };
static bool in_lds(uint32_t r, uint32_t nslots_final) {      // at hand without a fetch: in the lane's ring behind nslots_final slots, or in the LDS part of the pools
    const int k = ref_kind(r); const uint32_t i = ref_idx(r);
    if (k == RK_LOCAL) return (uint64_t)i + RING_K >= (uint64_t)nslots_final;
    if (k == RK_LIT64) return i + 1 <= POOL64_CAP;
    if (k == RK_LITFR) return i + 1 <= POOLFR_CAP;
    return false;
}
static uint32_t words_of(uint32_t r) { const int k = ref_kind(r); return (uint32_t)(k == RK_LITFR ? 4 : k == RK_INPUT ? (ref_width(r) == WFR ? 4 : 1) : SLOTS_OF[ref_width(r)]); }

// One pass over the trace: the segments, then every op in tape order by the method of its kind.  An op method appends the op (header, operands as mkref
// words, result slot) to its segment's tape and returns the cells the device template has; lower_op holds that against the trace and runs the operand
// pass behind it.  The first refusal is LW.err and ends the pass.
struct Lowering {
    const Trace *tr; const LowerOptions &opt; Lowered &LW; LoweredOpObserver *obs;
    std::vector<SegInfo> &segs;
    std::vector<int> open_child; int prev_seg = 0;      // per segment: where its parent's DOP_SKIP words are; the segment of the op before
    // the op being lowered: its index (a fused stretch moves it to the stretch's last op), its segment and that segment's tape, its operands and result handles
    size_t i = 0; const TraceOp *o = nullptr; int s = 0; SegInfo *S = nullptr; std::vector<uint32_t> *T = nullptr; const TraceIn *in = nullptr; const uint64_t *out = nullptr;
    size_t op_at = 0; uint32_t slots_before = 0; bool ka_fused = false;      // where the op starts on the tape; the segment's slots in front of it; it took the CONST1 in front of it in

    Lowering(const Trace *tr_, const LowerOptions &opt_, Lowered &LW_, LoweredOpObserver *obs_) : tr(tr_), opt(opt_), LW(LW_), obs(obs_), segs(LW_.segs) {}
    void bad(const std::string &m) { if (LW.err.empty()) LW.err = m; }

    // ---- pass 1: segments (the instances of the parallel scopes + the root), and one id per parallel scope name (the names compare by string)
    void segments() {
        segs.assign(1, SegInfo()); LW.op_seg.assign(tr->ops.size(), 0);      // (op_seg is kept: the verdict stage places the recorded equalities by it)
        std::vector<int> stack;      // per open scope: the segment it opened, or -1 (an ordinary scope)
        int cur = 0;
        for (size_t k = 0; k < tr->ops.size(); k++) {
            const TraceOp &p = tr->ops[k];
            if (p.code == TR_SCOPE_PUSH) {
                bool par = false; for (size_t n = 0; n < opt.n_scopes; n++) if (tr->names[(size_t)p.imm] == opt.parallel_scopes[n]) par = true;
                if (par) { SegInfo c; c.parent = cur; c.depth = segs[(size_t)cur].depth + 1; c.name = (uint32_t)p.imm; segs.push_back(c); cur = (int)segs.size() - 1; stack.push_back(cur); }
                else stack.push_back(-1);
            } else if (p.code == TR_SCOPE_POP) {
                if (stack.empty()) { bad("unbalanced scopes in the trace"); break; }
                if (stack.back() >= 0) cur = segs[(size_t)stack.back()].parent;
                stack.pop_back();
            }
            LW.op_seg[k] = cur;
        }
        if (!stack.empty()) bad("a scope is still open at the end of the trace");
        std::map<std::string, uint32_t> ids;
        for (SegInfo &c : segs) { if (c.parent < 0) continue; auto it = ids.find(tr->names[c.name]); if (it == ids.end()) it = ids.emplace(tr->names[c.name], (uint32_t)ids.size() + 1).first; c.name = it->second; }
    }

    // ---- values, records, literals
    uint32_t lit64(uint64_t v) { auto it = LW.pool64_of.find(v); if (it != LW.pool64_of.end()) return it->second; LW.pool64.push_back(v); LW.pool64_of[v] = (uint32_t)LW.pool64.size() - 1; return (uint32_t)LW.pool64.size() - 1; }
    uint32_t litfr(const fr_t &v) { for (size_t k = 0; k < LW.poolfr.size(); k++) if (fr_eq(LW.poolfr[k], v)) return (uint32_t)k; LW.poolfr.push_back(v); return (uint32_t)LW.poolfr.size() - 1; }
    // operand of the op: the handle's cell, or a literal
    uint32_t ref_of(const TraceIn &x, int *width_out) {
        if (x.lit) { if (width_out) *width_out = W64; return mkref(RK_LIT64, W64, lit64(x.v)); }
        uint32_t r; int w; const HandleWhy why = resolve_handle(LW, s, x.v, ImportTable{S->imps, S->imp_of}, r, w);
        if (width_out) *width_out = w;
        if (why == HANDLE_NOT_TRACED) bad("an operand is not the result of a traced call (cell " + std::to_string(x.v) + ")");
        if (why == HANDLE_NOT_ENCLOSING) bad("a parallel scope reads a value computed in a scope that does not enclose it: its instances are not independent (cell " + std::to_string(x.v) + ")");
        return why == HANDLE_OK ? r : mkref(RK_LIT64, W64, lit64(0));
    }
    uint32_t new_val(uint64_t cell, int width, bool stat = false, uint32_t lit = 0) {
        ValInfo v; v.seg = (uint32_t)s; v.width = (uint8_t)width; v.is_static = stat ? 1 : 0; v.lit = lit; v.slot = NO_SLOT;
        if (!stat) { v.slot = S->nslots; S->nslots += (uint32_t)SLOTS_OF[width]; }
        LW.vals.push_back(v); LW.val_of[cell] = (uint32_t)LW.vals.size() - 1; return v.slot;
    }
    void add_rec(int tmpl, uint64_t cell) { LW.meta.push_back(meta_pack((uint32_t)tmpl, cell)); LW.nrec++; S->nrecs++; }
    void head(uint32_t op, uint32_t n = 0, uint32_t aux = 0) { if (aux > 255) bad("internal: op parameter too wide"); T->push_back(op | (n << 8) | (aux << 16)); }
    void put(std::initializer_list<uint32_t> words) { T->insert(T->end(), words.begin(), words.end()); }      // (a braced list: its entries are evaluated left to right)

    // ---- scope push / pop
    void scope_op() {
        // entering a parallel child: the parent steps over its records and cells (filled in when the child ends)
        if (o->code == TR_SCOPE_PUSH && s != prev_seg && segs[(size_t)s].parent == prev_seg) {
            SegInfo &Pn = segs[(size_t)prev_seg]; Pn.tape.push_back(DOP_SKIP | (5u << 24)); Pn.last_const_at = -1; if (obs) obs->boundary(prev_seg);
            open_child[(size_t)s] = (int)Pn.tape.size(); for (int k = 0; k < 4; k++) Pn.tape.push_back(0);
            S->cell0 = o->cell0; S->rec0 = LW.nrec; S->started = true;
        }
        if (o->code == TR_SCOPE_POP && s != prev_seg && segs[(size_t)prev_seg].parent == s) {
            SegInfo &C = segs[(size_t)prev_seg]; C.ncells = o->cell0 - C.cell0; C.tape.push_back(DOP_END | (1u << 24));
            // the child's totals include its own children's (they are nested in its cell and record ranges)
            const uint64_t nr = LW.nrec - C.rec0; uint32_t *w = S->tape.data() + open_child[(size_t)prev_seg];
            w[0] = (uint32_t)nr; w[1] = (uint32_t)(nr >> 32); w[2] = (uint32_t)C.ncells; w[3] = (uint32_t)(C.ncells >> 32); C.all_recs = nr;
        }
    }

    // ---- one method per op kind -> the cells the device template has
    // a verified permutation: one op, its results (12 one-word values; PoseidonBN254: 4 of width WFR) in fresh slots
    uint64_t fused_stretch(const Stretch &fz) {
        const bool bn = fz.canon == CANON_BN;
        head(bn ? DOP_BNPERM : DOP_GLPERM);
        for (int k = 0; k < fz.nio; k++) { int w; T->push_back(ref_of(fz.in[k], &w)); if (!bn && w != W64) bad("internal: a wide input of a fused permutation"); }
        const uint32_t base = S->nslots;
        for (int k = 0; k < fz.nio; k++) new_val(fz.out[k], bn ? WFR : W64);
        put({base, bn ? S->nbnp++ : S->nglp++, (uint32_t)(fz.cell1 - fz.cell0)});
        if (bn) S->bnp_cells.push_back(fz.cell0);      // no records: its cells are direct cells, the emission kernel's from where the plan lists them
        else {                                         // its record block laid out as the emission kernel writes it
            for (uint64_t m : opt.fused.glp_meta) LW.meta.push_back(meta_pack(meta_tmpl(m), fz.cell0 + meta_off(m)));
            LW.nrec += opt.fused.glp_meta.size(); S->nrecs += opt.fused.glp_meta.size();
        }
        i = fz.tr1 - 1;      // (the pass goes on behind the stretch)
        return o->ncells;
    }
    uint64_t load_constant() {
        const fr_t c = tr->consts[(size_t)o->imm]; const bool small = (c.l[1] | c.l[2] | c.l[3]) == 0;
        if (o->tag.kind == 1) {
            if (o->tag.n != 1) { bad("a constant that is a proof value must be one Goldilocks word"); return 0; }
            S->inputs.push_back((uint32_t)o->tag.word); head(DOP_CONST1); put({mkref(RK_INPUT, W64, (uint32_t)S->inputs.size() - 1), new_val(out[0], W64)});
            add_rec(T_CONST1, o->cell0); return 1;
        }
        if (o->tag.kind != 0) { bad("a hint tag on a constant"); return 0; }
        if (small) {      // a static CONST1: a GLOP right behind it that takes it as operand A takes it in (glop)
            const uint32_t li = lit64(c.l[0]); head(DOP_CONST1); put({mkref(RK_LIT64, W64, li), NO_SLOT}); new_val(out[0], W64, true, li); add_rec(T_CONST1, o->cell0);
            S->last_const_at = (long)op_at; S->last_const_cell = o->cell0; S->last_const_tr = i; return 1;
        }
        const uint32_t li = litfr(c); head(DOP_FRCELL); put({mkref(RK_LITFR, WFR, li), NO_SLOT}); new_val(out[0], WFR, true, li); return 1;
    }
    uint64_t load_witness() {
        if (o->tag.kind != 1) { bad("h2w_load_witness without h2w_trace_input"); return 0; }
        S->inputs.push_back((uint32_t)o->tag.word);
        if (o->tag.n == 4) { head(DOP_FRCELL); put({mkref(RK_INPUT, WFR, (uint32_t)S->inputs.size() - 1), new_val(out[0], WFR)}); }
        else { head(DOP_CONST1); put({mkref(RK_INPUT, W64, (uint32_t)S->inputs.size() - 1), new_val(out[0], W64)}); add_rec(T_CONST1, o->cell0); }
        return 1;
    }
    uint64_t add_mul() {      // add, mul, mul_add
        int w0 = 0, w1 = 0, w2 = 0;
        const uint32_t a = ref_of(in[0], &w0), b = ref_of(in[1], &w1), c3 = o->code == TR_MUL_ADD ? ref_of(in[2], &w2) : 0;
        const bool narrow = w0 == W64 && w1 == W64 && (o->code != TR_MUL_ADD || w2 == W64);
        if (narrow) {      // [C, A, B, A B + C] on values below 2^64: one gate record (GoldilocksChip::*_no_reduce, base.rs:240-294)
            head(DOP_GATE, 0, T_GATE);
            if (o->code == TR_ADD) put({b, mkref(RK_LIT64, W64, lit64(1)), a});
            else if (o->code == TR_MUL) put({a, b, mkref(RK_LIT64, W64, lit64(0))});
            else put({a, b, c3});
            T->push_back(new_val(out[0], W128)); add_rec(T_GATE, o->cell0);
        } else {
            head(o->code == TR_ADD ? DOP_FR_ADD : o->code == TR_MUL ? DOP_FR_MUL : DOP_FR_MULADD); put({a, b}); if (o->code == TR_MUL_ADD) T->push_back(c3);
            T->push_back(new_val(out[0], WFR));
        }
        return 4;
    }
    uint64_t select() {
        int w0 = 0, w1 = 0, w2 = 0;
        const uint32_t a = ref_of(in[0], &w0), b = ref_of(in[1], &w1), sl = ref_of(in[2], &w2);
        if (w2 != W64) { bad("select: the selector is not a bit"); return 0; }
        const bool narrow = w0 == W64 && w1 == W64;
        head(narrow ? DOP_SELECT : DOP_FR_SELECT); put({a, b, sl, new_val(out[0], narrow ? W64 : WFR)});
        return 8;
    }
    uint64_t idx_to_indicator() {
        int w0 = 0; const uint32_t n = (uint32_t)o->imm; const uint32_t a = ref_of(in[0], &w0);
        if (w0 != W64 || n < 1 || n > 64) { bad("idx_to_indicator: a wide index or more than 64 entries"); return 0; }
        head(DOP_IDX2IND, n); T->push_back(a); const uint32_t base = S->nslots;
        for (uint32_t k = 0; k < n; k++) { const uint32_t sl = new_val(out[k], W64); if (sl != base + k) bad("internal: slots of an array result"); }
        T->push_back(base); return 8 + 12ull * (n - 1);
    }
    uint64_t select_by_indicator() {
        const uint32_t n = (uint32_t)o->imm; if (n < 1 || n > 64) { bad("select_by_indicator: more than 64 entries"); return 0; }
        std::vector<uint32_t> r(2 * n); bool narrow = true;
        for (uint32_t k = 0; k < 2 * n; k++) { int w; r[k] = ref_of(in[k], &w); if (k < n && w != W64) narrow = false; if (k >= n && w != W64) bad("select_by_indicator: an indicator that is not a bit"); }
        head(narrow ? DOP_SELIND : DOP_FR_SELIND, n); T->insert(T->end(), r.begin(), r.end()); T->push_back(new_val(out[0], narrow ? W64 : WFR));
        return 1 + 3ull * n;
    }
    uint64_t num_to_bits() {
        int w0 = 0; const uint32_t n = (uint32_t)o->imm; const uint32_t a = ref_of(in[0], &w0);
        if (w0 != W64 || n < 1 || n > 64) { bad("num_to_bits: a wide value or more than 64 bits"); return 0; }
        head(DOP_NUM2BITS, n); T->push_back(a); const uint32_t base = S->nslots;
        for (uint32_t k = 0; k < n; k++) new_val(out[k], W64);
        T->push_back(base); return (1 + 3ull * (n - 1)) + 4ull * n;
    }
    uint64_t bits_to_num() {
        const uint32_t n = (uint32_t)o->imm; if (n > 64) { bad("bits_to_num: more than 64 bits"); return 0; }
        head(DOP_BITS2NUM, n); for (uint32_t k = 0; k < n; k++) { int w; T->push_back(ref_of(in[k], &w)); if (w != W64) bad("bits_to_num: an operand that is not a bit"); }
        T->push_back(new_val(out[0], W64)); return n ? 1 + 3ull * (n - 1) : 1;
    }
    uint64_t decompose_le() {
        if ((o->imm >> 32) != 56 || (uint32_t)o->imm != 5) { bad("decompose_le: only (56 bits, 5 limbs) is replayable (HashWire::to_goldilocks_vec, hash/poseidon_bn254/hash.rs:31-43)"); return 0; }
        int w0; head(DOP_DECOMP565); T->push_back(ref_of(in[0], &w0)); const uint32_t base = S->nslots; for (int k = 0; k < 5; k++) new_val(out[k], W64); T->push_back(base);
        return 13 + 5 * rc_cells(opt.L, 56);
    }
    uint64_t limbs_to_num() {
        const uint32_t n = o->n_in; if (o->imm != 64 || n < 1 || n > 4) { bad("limbs_to_num: only up to four 64-bit limbs are replayable"); return 0; }
        head(DOP_LIMBS2NUM, n); for (uint32_t k = 0; k < n; k++) { int w; T->push_back(ref_of(in[k], &w)); if (w != W64) bad("limbs_to_num: a wide limb"); }
        T->push_back(new_val(out[0], WFR)); return 1 + 3ull * (n - 1);
    }
    uint64_t range_check() {
        int w0 = 0; const uint32_t a = ref_of(in[0], &w0); if (w0 != W64 || o->imm > 64) { bad("range_check: a wide value"); return 0; }
        head(DOP_RANGE, 0, (uint32_t)o->imm); T->push_back(a); return rc_cells(opt.L, o->imm);
    }
    uint64_t clt_safe() {
        int w0 = 0; const uint32_t a = ref_of(in[0], &w0); if (w0 != W64 || o->imm != GL_P) { bad("check_less_than_safe: only (64-bit value, Goldilocks order) is replayable"); return 0; }
        head(DOP_CLT); T->push_back(a); add_rec(T_CLT_SAFE, o->cell0); return (uint64_t)opt.tt.ncells(T_CLT_SAFE);
    }
    uint64_t gl_witness() {      // a proof word, or a hint: the quotient of a division, a component of an extension inverse
        int w0 = 0, w1 = 0;
        if (o->tag.kind == 1) { if (o->tag.n != 1) { bad("a Goldilocks witness of more than one word"); return 0; } S->inputs.push_back((uint32_t)o->tag.word); head(DOP_LOADW); T->push_back(mkref(RK_INPUT, W64, (uint32_t)S->inputs.size() - 1)); }
        else if (o->tag.kind == 2) { head(DOP_LOADW_DIV); put({ref_of(TraceIn{o->tag.a, 0}, &w0), ref_of(TraceIn{o->tag.b, 0}, &w1)}); if (w0 != W64 || w1 != W64) bad("div: wide operands"); }
        else if (o->tag.kind == 3 || o->tag.kind == 4) { head(DOP_LOADW_EXTINV, 0, (uint32_t)(o->tag.kind - 3)); put({ref_of(TraceIn{o->tag.a, 0}, &w0), ref_of(TraceIn{o->tag.b, 0}, &w1)}); if (w0 != W64 || w1 != W64) bad("ext inverse: wide operands"); }
        else { bad("h2w_gl_load_witness without h2w_trace_input"); return 0; }
        T->push_back(new_val(out[0], W64)); add_rec(T_LOADW, o->cell0); return (uint64_t)opt.tt.ncells(T_LOADW);
    }
    uint64_t gl_reduce() {
        int w0 = 0; const uint32_t a = ref_of(in[0], &w0); if (w0 == W64) { bad("gl_reduce of a value that is not a gate output"); return 0; }
        if (ref_kind(a) != RK_LOCAL && ref_kind(a) != RK_IMPORT && ref_kind(a) != RK_RING) { bad("gl_reduce of a constant"); return 0; }
        head(DOP_REDUCE); put({a, new_val(out[0], W64)}); add_rec(T_REDUCE, o->cell0); return (uint64_t)opt.tt.ncells(T_REDUCE);
    }
    uint64_t glop() {
        int w0 = 0, w1 = 0, w2 = 0;
        const uint32_t a = ref_of(in[0], &w0), b = ref_of(in[1], &w1), c3 = ref_of(in[2], &w2);
        if (w0 != W64 || w1 != W64 || w2 != W64) { bad("a Goldilocks op on a wide value"); return 0; }
        if (o->sub == T_GLOP && !in[0].lit && S->last_const_at >= 0 && (size_t)S->last_const_at + 3 == T->size() && in[0].v == S->last_const_cell && S->last_const_cell + 1 == o->cell0 && ref_kind(a) == RK_LIT64) {
            // load_constant(K) immediately followed by the op that takes it (GoldilocksChip's constant operands, e.g. hash/poseidon/permutation.rs:55-68): ONE record [K][C, A, B, V]...
            op_at = (size_t)S->last_const_at; T->resize(op_at); LW.meta.pop_back(); LW.nrec--; S->nrecs--; ka_fused = true;
            T->push_back(DOP_GLOP | ((uint32_t)T_KA_GLOP << 16)); put({a, b, c3, new_val(out[0], W64)}); add_rec(T_KA_GLOP, o->cell0 - 1);
            S->last_const_at = -1; return (uint64_t)opt.tt.ncells(T_GLOP);
        }
        head(DOP_GLOP, 0, o->sub); put({a, b, c3, new_val(out[0], W64)}); add_rec(o->sub, o->cell0); return (uint64_t)opt.tt.ncells(o->sub);
    }
    uint64_t by_kind() {
        switch (o->code) {
            case TR_LOAD_CONSTANT: return load_constant();
            case TR_LOAD_WITNESS: return load_witness();
            case TR_ADD: case TR_MUL: case TR_MUL_ADD: return add_mul();
            case TR_SELECT: return select();
            case TR_IDX_TO_INDICATOR: return idx_to_indicator();
            case TR_SELECT_BY_INDICATOR: return select_by_indicator();
            case TR_NUM_TO_BITS: return num_to_bits();
            case TR_BITS_TO_NUM: return bits_to_num();
            case TR_DECOMPOSE_LE: return decompose_le();
            case TR_LIMBS_TO_NUM: return limbs_to_num();
            case TR_RANGE_CHECK: return range_check();
            case TR_CLT_SAFE: return clt_safe();
            case TR_GL_WITNESS: return gl_witness();
            case TR_GL_REDUCE: return gl_reduce();
            case TR_GLOP: return glop();
            default: bad("unknown op in the trace"); return 0;
        }
    }

    // ---- behind an op
    // the op as lowered, its operands still as mkref words, to the observer
    void observe(uint32_t first, uint32_t count) {
        const std::vector<uint32_t> &t = *T;
        NormOp no; no.hdr = t[op_at] & 0xffffffu; no.nin = count <= 3 ? count : 0xffu; no.slots_before = slots_before;
        for (uint32_t k = 0; k < count && k < 3; k++) { no.ref[k] = t[op_at + first + k]; if (ref_kind(no.ref[k]) == RK_LIT64) no.lit[k] = fr_from_u64(LW.pool64[ref_idx(no.ref[k])]); else if (ref_kind(no.ref[k]) == RK_LITFR) no.lit[k] = LW.poolfr[ref_idx(no.ref[k])]; }
        no.out = count <= 3 && op_at + first + count < t.size() ? t[op_at + first + count] : NO_SLOT;
        no.tr0 = ka_fused ? S->last_const_tr : i; no.tr1 = i + 1; no.cell0 = ka_fused ? o->cell0 - 1 : o->cell0; no.cell1 = o->cell0 + o->ncells; no.out_cell = o->n_out ? out[0] : 0; no.tin = in;
        obs->op(s, no, ka_fused);
    }
    // the slots to fetch for the operand words R[0, m): a fixed point (the temporaries push the oldest ring slots out, which may be operands too)
    uint32_t fetched_slots(const uint32_t *R, uint32_t m) const { uint32_t t = 0; for (;;) { uint32_t need = 0; for (uint32_t k = 0; k < m; k++) if (!in_lds(R[k], S->nslots + t)) need += words_of(R[k]); if (need == t) return t; t = need; } }
    // R[0, m) become fast refs in place, the DOP_FETCH ops of those not at hand go to `fetches`; the segment's slots move behind the temporaries
    void to_fast_refs(uint32_t *R, uint32_t m, uint32_t temps, std::vector<uint32_t> &fetches) {
        const uint32_t nf = S->nslots + temps; uint32_t tslot = S->nslots;
        for (uint32_t k2 = 0; k2 < m; k2++) {
            const uint32_t r = R[k2]; const int k = ref_kind(r), w = ref_width(r); uint32_t fr2;
            if (in_lds(r, nf)) fr2 = k == RK_LOCAL ? fastref_ring(w, ref_idx(r)) : k == RK_LIT64 ? fastref_pool(W64, LDS_POOL64 + ref_idx(r) * 8) : fastref_pool(WFR, LDS_POOLFR + ref_idx(r) * 32);
            else {
                const uint32_t nw = words_of(r);
                fetches.insert(fetches.end(), {DOP_FETCH | (nw << 8) | (3u << 24), r, tslot});
                fr2 = fastref_ring(nw == 4 ? WFR : nw == 2 ? W128 : W64, tslot); tslot += nw;
            }
            R[k2] = fr2;
        }
        S->nslots = nf;
    }
    // The wide select walks its entries in order and carries one sum: cut at an entry boundary it is two ops that share nothing else.  Parts
    // [e0, e1) in order, each the longest run whose own fetches fit (a shorter run never needs more: the fewest parts), each behind the slots
    // the parts before it took - so a part fetches what their temporaries pushed out of the ring, its indicators included.  The result slot
    // is the unsplit op's (taken by its method) and goes with the last part; the sum in between has no slot.
    void split_select(uint32_t first, uint32_t count) {
        const uint32_t n = count / 2, res = (*T)[op_at + first + count];
        const std::vector<uint32_t> ops(T->begin() + (long)(op_at + first), T->begin() + (long)(op_at + first + count));
        T->resize(op_at);
        for (uint32_t e0 = 0; e0 < n && LW.err.empty();) {
            std::vector<uint32_t> part, fetches; uint32_t e1 = n, pt = 0;
            for (;; e1--) {
                part.assign(ops.begin() + e0, ops.begin() + e1); part.insert(part.end(), ops.begin() + n + e0, ops.begin() + n + e1);
                pt = fetched_slots(part.data(), (uint32_t)part.size());
                if (pt <= RING_K || e1 == e0 + 1) break;
            }
            if (pt > RING_K) { bad("internal: one entry of a split select_by_indicator does not fit the value slots a lane keeps at hand"); break; }
            to_fast_refs(part.data(), (uint32_t)part.size(), pt, fetches);
            const uint32_t m = e1 - e0, aux = (e0 ? SELIND_CONTINUES : 0u) | (e1 < n ? SELIND_CONTINUED : 0u);
            T->insert(T->end(), fetches.begin(), fetches.end());
            T->push_back(DOP_FR_SELIND | (m << 8) | (aux << 16) | ((2 * m + 2) << 24)); T->insert(T->end(), part.begin(), part.end()); T->push_back(e1 < n ? NO_SLOT : res);
            LW.n_select_parts++; e0 = e1;
        }
    }
    // The op's length byte and its operands: those in the lane's ring or in the LDS part of the pools become fast refs; the others are fetched into fresh
    // ring slots by DOP_FETCH ops in front of this one.  The ring holds the last RING_K slots WRITTEN, the temporaries included: decided against the slot
    // count after them.  false: refused - more slots to fetch than the ring has
    bool operand_pass() {
        std::vector<uint32_t> &t = *T;
        uint32_t first, count; operand_span(t[op_at] & 0xff, (t[op_at] >> 8) & 0xff, first, count);
        if (obs && LW.err.empty()) observe(first, count);
        const size_t len = t.size() - op_at; if (len > 255) bad("internal: op too long"); t[op_at] |= (uint32_t)len << 24;
        const uint32_t temps = fetched_slots(t.data() + op_at + first, count);
        // the ring is RING_K slots (slot mod RING_K): with more temporaries than that the later fetches overwrite the earlier ones before the op reads
        // them.  (The op's own result slots may alias them: every op reads all its operands before it stores a result.)
        if (temps > RING_K && opt.split_selects && (t[op_at] & 0xff) == DOP_FR_SELIND) split_select(first, count);
        else if (temps > RING_K) {
            bad((o->code == TR_SELECT_BY_INDICATOR ? std::string("select_by_indicator") : "trace op " + std::to_string((int)o->code) + " (device op " + std::to_string(t[op_at] & 0xff) + ")") + " with " + std::to_string(count) + " operands: " + std::to_string(temps) + " slots of them have to be fetched (values of an enclosing scope, values computed more than " +
                std::to_string(RING_K) + " slots earlier, proof words, far constants), more than the " + std::to_string(RING_K) + " value slots a lane keeps at hand");
            return false;
        } else {
            std::vector<uint32_t> fetches; to_fast_refs(t.data() + op_at + first, count, temps, fetches);
            if (!fetches.empty()) { t.insert(t.begin() + (long)op_at, fetches.begin(), fetches.end()); if (S->last_const_at == (long)op_at) S->last_const_at += (long)fetches.size(); }
        }
        return true;
    }

    // ---- pass 2: the ops in tape order
    bool lower_op() {      // false: the pass ends here
        in = tr->ins.data() + o->first_in; out = tr->outs.data() + o->first_out;
        op_at = T->size(); slots_before = S->nslots; ka_fused = false;
        auto f = opt.fused.fuse.find(i); const bool fz = f != opt.fused.fuse.end();
        const uint64_t want_cells = fz ? fused_stretch(f->second) : by_kind();
        if (fz || !(o->code == TR_LOAD_CONSTANT && S->last_const_at == (long)op_at)) S->last_const_at = -1;
        if (T->size() > op_at && !operand_pass()) return false;
        if (LW.err.empty() && want_cells != o->ncells) bad("internal: op " + std::to_string(o->code) + " appended " + std::to_string(o->ncells) + " cells on the host, the device template has " + std::to_string(want_cells));
        return true;
    }
    void run() {
        segments();
        open_child.assign(segs.size(), -1);
        for (i = 0; i < tr->ops.size() && LW.err.empty(); i++) {
            o = &tr->ops[i]; s = LW.op_seg[i]; S = &segs[(size_t)s]; T = &S->tape;
            if (o->code == TR_SCOPE_PUSH || o->code == TR_SCOPE_POP) scope_op();
            else if (!lower_op()) break;
            prev_seg = s;
        }
        if (obs) obs->end();
        if (!LW.err.empty()) return;
        segs[0].tape.push_back(DOP_END | (1u << 24)); segs[0].cell0 = 0; segs[0].rec0 = 0;
    }
};
static void lower_pass(const Trace *tr, const LowerOptions &opt, Lowered &LW, LoweredOpObserver *obs = nullptr) { Lowering(tr, opt, LW, obs).run(); }

// The canonical tape of ONE permutation on `consts`: the library's own PoseidonChip::permute / PoseidonBN254PermutationChip::permute (what
// h2w_chip_gl_poseidon_permute / h2w_chip_bn_poseidon_permute run) recorded on abstract inputs and lowered by lower_trace like any tape; its operands
// classified (a literal, a value of the stretch, an input).  CANON_BN: recorded behind a load_zero (the cell cached, as every PoseidonBN254 permutation
// of a run but the first to use it finds it); CANON_BN_ZERO: on a fresh context (the load_zero cell inside the first mix).
static bool canonical_tape(int id, int L, TemplateTable &tt, const h2w_poseidon_consts_t *consts, Canon &cn, std::string &err) {
    const bool bn = id != CANON_GL; const int nio = bn ? BN_WIDTH : SPONGE_WIDTH;
    cn.id = id; cn.nio = nio; cn.in_any_width = bn;
    h2w_ctx *c = h2w_ctx_new(L, 1, -1);
    if (!c) { err = "cannot create the recording context"; return false; }
    h2w_assigned_t in[MAX_PERM_IO], out[MAX_PERM_IO], z; int rc = h2w_ctx_trace_begin(c);
    const size_t lead = id == CANON_BN ? 1 : 0;      // ops in front of the input loads
    if (rc == 0 && id == CANON_BN) rc = h2w_load_zero(c, &z);
    for (int i = 0; i < nio && rc == 0; i++) {
        if (bn) { const fr_t v = fr_from_u64((uint64_t)i); rc = h2w_trace_input(c, 4 * (uint64_t)i, 4); if (rc == 0) rc = h2w_load_witness(c, &v, &in[i]); }
        else { rc = h2w_trace_input(c, (uint64_t)i, 1); if (rc == 0) rc = h2w_gl_load_witness(c, (uint64_t)i, &in[i]); }
    }
    if (rc == 0) rc = bn ? h2w_chip_bn_poseidon_permute(c, consts, in, out) : h2w_chip_gl_poseidon_permute(c, consts, in, out);
    const Trace *tr = ctx_trace(c);
    if (rc != 0 || !tr || !tr->err.empty()) { err = "cannot record the canonical permutation"; h2w_ctx_free(c); return false; }
    Lowered LW; RootCapture root; const std::vector<NormOp> &ops = root.ops;
    lower_pass(tr, LowerOptions{L, tt}, LW, &root);
    const size_t first = lead + (size_t)nio;
    bool ok = LW.err.empty() && ops.size() > first;
    if (!ok) err = "the canonical permutation does not lower: " + LW.err;
    // the loads come first
    std::unordered_map<uint32_t, uint32_t> prod, inslot;      // slot -> op of the stretch; slot -> input
    for (int i = 0; ok && i < nio; i++) {
        const NormOp &o = ops[lead + (size_t)i];
        if ((o.hdr & 0xff) != (uint32_t)(bn ? DOP_FRCELL : DOP_LOADW) || o.out == NO_SLOT) { ok = false; err = "internal: inputs of the canonical tape"; } else inslot[o.out] = (uint32_t)i;
    }
    for (size_t j = first; ok && j < ops.size(); j++) {
        const NormOp &o = ops[j]; CanonOp c2; memset(&c2, 0, sizeof(c2)); c2.hdr = o.hdr; c2.nin = o.nin; c2.has_out = o.out != NO_SLOT;
        if (o.nin > 3) { ok = false; err = "internal: an op of the canonical tape with more than three operands"; break; }
        for (uint32_t k = 0; k < o.nin; k++) {
            const int rk = ref_kind(o.ref[k]); const uint32_t ix = ref_idx(o.ref[k]);
            c2.rk[k] = (uint8_t)rk; c2.width[k] = (uint8_t)ref_width(o.ref[k]);
            if (rk == RK_LIT64 || rk == RK_LITFR) { c2.kind[k] = CK_LIT; c2.lit[k] = o.lit[k]; }
            else if (rk == RK_LOCAL && inslot.count(ix)) { c2.kind[k] = CK_INPUT; c2.arg[k] = inslot[ix]; }
            else if (rk == RK_LOCAL && prod.count(ix)) { c2.kind[k] = CK_INTERIOR; c2.arg[k] = prod[ix]; }
            else { ok = false; err = "internal: an operand of the canonical tape"; }
        }
        if (c2.has_out) prod[o.out] = (uint32_t)cn.ops.size();
        cn.ops.push_back(c2);
    }
    for (int i = 0; ok && i < nio; i++) {
        auto it = LW.val_of.find(out[i].offset);
        if (!out[i].has_cell || it == LW.val_of.end() || LW.vals[it->second].is_static || !prod.count(LW.vals[it->second].slot)) { ok = false; err = "internal: outputs of the canonical tape"; break; }
        cn.out_prod[i] = prod[LW.vals[it->second].slot];
    }
    if (ok) cn.ncells = ops.back().cell1 - ops[first].cell0;
    if (ok && id == CANON_BN && LW.nrec != 1) { ok = false; err = "a PoseidonBN254 permutation on these tables has block records (a table entry below 2^64): it cannot be fused"; }
    h2w_ctx_free(c);
    return ok;
}

void lower_trace(const Trace *tr, int L, TemplateTable &tt, const char *const *parallel_scopes, size_t n_scopes, const Fusable &F, bool split_selects, Lowered &LW) {
    lower_pass(tr, LowerOptions{L, tt, parallel_scopes, n_scopes, split_selects, F}, LW);
}

// The stretches that equal a canonical tape word for word, found on a first lowering; those nothing outside reads into are lowered as one op
bool find_fusable(const Trace *tr, int L, TemplateTable &tt, const char *const *parallel_scopes, size_t n_scopes, const h2w_poseidon_consts_t *consts, bool gl, bool bn, bool split_selects, Fusable &F, std::string &err) {
    if (!gl && !bn) return true;
    const std::string ex = "h2w_plan_from_trace_ex: ";
    Canon cn, cnb, cnz; std::string cerr; std::vector<Stretch> found; std::vector<const Canon *> cns;
    if (gl) {
        if (!canonical_tape(CANON_GL, L, tt, consts, cn, cerr)) { err = ex + cerr; return false; }
        F.glp_block_cells = glp_block_layout(tt, L, consts, F.glp_meta);
        if (F.glp_block_cells == 0 || F.glp_block_cells != cn.ncells) { err = ex + "the record block of a permutation (" + std::to_string(F.glp_block_cells) + " cells) is not the traced one (" + std::to_string(cn.ncells) + " cells)"; return false; }
        cns.push_back(&cn);
    }
    if (bn) {
        if (!canonical_tape(CANON_BN, L, tt, consts, cnb, cerr) || !canonical_tape(CANON_BN_ZERO, L, tt, consts, cnz, cerr)) { err = ex + cerr; return false; }
        if (cnb.ncells != (uint64_t)BN_PERM_CELLS || cnz.ncells != (uint64_t)BN_PERM_CELLS + 1) { err = ex + "a PoseidonBN254 permutation has " + std::to_string(cnb.ncells) + " traced cells, the emission kernel writes " + std::to_string(BN_PERM_CELLS); return false; }
        cns.push_back(&cnb); cns.push_back(&cnz);
    }
    { Lowered first; MatcherSet search(cns, found); lower_pass(tr, LowerOptions{L, tt, parallel_scopes, n_scopes, split_selects}, first, &search); if (!first.err.empty()) { err = "h2w_plan_from_trace: " + first.err; return false; } }
    std::sort(found.begin(), found.end(), [](const Stretch &a, const Stretch &b) { return a.cell0 < b.cell0; });
    // an interior value read outside its stretch: every operand handle of the trace (the hints' operands too) against the stretches' cell ranges
    auto reads = [&](size_t op, uint64_t cell) {
        auto it = std::upper_bound(found.begin(), found.end(), cell, [](uint64_t c, const Stretch &x) { return c < x.cell0; });
        if (it == found.begin()) return;
        Stretch &x = *(it - 1);
        if (cell >= x.cell1 || (op >= x.tr0 && op < x.tr1)) return;
        for (int k = 0; k < x.nio; k++) if (x.out[k] == cell) return;
        x.escaped = true;
    };
    for (size_t i = 0; i < tr->ops.size(); i++) {
        const TraceOp &o = tr->ops[i];
        for (uint32_t k = 0; k < o.n_in; k++) if (!tr->ins[o.first_in + k].lit) reads(i, tr->ins[o.first_in + k].v);
        if (o.tag.kind >= 2) { reads(i, o.tag.a); reads(i, o.tag.b); }
    }
    uint64_t n_zero = 0;
    for (const Stretch &x : found) {
        if (x.canon == CANON_BN_ZERO) { F.n_bn_left++; if (!x.const_bad) n_zero++; continue; }      // the permutation that holds the Context's load_zero cell (every later mix of the run reads it): recognised, left interpreted
        const bool xb = x.canon == CANON_BN; const uint64_t have = x.cell1 - x.cell0, want = xb ? (uint64_t)BN_PERM_CELLS : F.glp_block_cells;
        if (have != want) {
            err = ex + (xb ? "a PoseidonBN254 permutation's stretch has " + std::to_string(have) + " traced cells, the emission kernel writes " + std::to_string(want)
                           : "a permutation's stretch has " + std::to_string(have) + " traced cells, its record block " + std::to_string(want));
            return false;
        }
        if (x.const_bad || x.escaped) (xb ? F.n_bn_left : F.n_candidates)++; else F.fuse.emplace(x.tr0, x);
    }
    if (n_zero > 1) { err = ex + "internal: more than one PoseidonBN254 permutation with the load_zero cell"; return false; }
    return true;
}

ShardUnits shard_units(Lowered &LW, uint64_t total_cells) {
    std::vector<SegInfo> &segs = LW.segs; ShardUnits R; std::vector<int> &units = R.units; std::string &why = R.why_unshardable;
    for (size_t si = 1; si < segs.size(); si++) {      // (a segment comes after its parent)
        SegInfo &S = segs[si];
        if (S.depth == 1) { S.unit = (uint32_t)units.size(); units.push_back((int)si); }
        else S.unit = segs[(size_t)S.parent].unit;
    }
    uint64_t c = units.empty() ? 0 : segs[(size_t)units[0]].cell0, r = units.empty() ? 0 : segs[(size_t)units[0]].rec0;
    for (size_t q = 0; q < units.size() && why.empty(); q++) {
        const SegInfo &U = segs[(size_t)units[q]], &U1 = segs[(size_t)units[q > 1 ? 1 : q]];
        if (U.cell0 != c || U.rec0 != r) why = "the root has cells or records between parallel instances " + std::to_string(q ? q - 1 : 0) + " and " + std::to_string(q) + " at depth 1";
        else if (U.ncells != U1.ncells || U.all_recs != U1.all_recs) why = "the parallel instances at depth 1 differ in size (instance " + std::to_string(q) + ")";
        c += U.ncells; r += U.all_recs;
    }
    if (units.empty()) why = "no parallel scope instance at depth 1 (trace the query rounds as parallel: \"verify_query_round\")";
    else if (why.empty() && (c != total_cells || r != LW.nrec)) why = "the root has cells or records after the last parallel instance at depth 1";
    if (!why.empty()) { why = "the traced plan is not shardable: " + why; R.pro_ncell = total_cells; R.pro_nrec = LW.nrec; return R; }
    const SegInfo &U0 = segs[(size_t)units[0]], &U1 = segs[(size_t)units[units.size() > 1 ? 1 : 0]];
    R.num_queries = (uint32_t)units.size();
    R.pro_ncell = U0.cell0; R.pro_nrec = U0.rec0;
    R.q_cell0[0] = U0.cell0; R.q_rec0[0] = U0.rec0; R.q_ncell[0] = U0.ncells; R.q_nrec[0] = U0.all_recs;
    R.q_cell0[1] = U1.cell0; R.q_rec0[1] = U1.rec0; R.q_ncell[1] = U1.ncells; R.q_nrec[1] = U1.all_recs;
    return R;
}

void pack_glop_runs(Lowered &LW, const TemplateTable &tt) {
    for (SegInfo &S : LW.segs) {
        if (S.nslots >= (1u << 24)) continue;
        std::vector<uint32_t> out; out.reserve(S.tape.size()); size_t pc = 0; const std::vector<uint32_t> &T = S.tape;
        while (pc < T.size()) {
            const uint32_t h = T[pc], op = h & 0xff, len = h >> 24;
            if (op != DOP_GLOP) { out.insert(out.end(), T.begin() + (long)pc, T.begin() + (long)(pc + len)); pc += len; continue; }
            size_t e = pc; uint32_t cnt = 0;
            while (e < T.size() && (T[e] & 0xff) == DOP_GLOP && cnt < 255) { e += 5; cnt++; }
            if (cnt < 2) { out.insert(out.end(), T.begin() + (long)pc, T.begin() + (long)(pc + 5)); pc += 5; continue; }
            out.push_back(DOP_GLOPRUN | (cnt << 8));
            { uint32_t cells = 0; for (size_t k2 = pc; k2 < e; k2 += 5) cells += (uint32_t)tt.ncells((int)((T[k2] >> 16) & 0xff)); out.push_back(cells); }
            for (size_t k2 = pc; k2 < e; k2 += 5) { out.push_back(T[k2 + 1]); out.push_back(T[k2 + 2]); out.push_back(T[k2 + 3]); out.push_back((T[k2 + 4] & 0xffffffu) | (((T[k2] >> 16) & 0xff) << 24)); }
            pc = e;
        }
        S.tape.swap(out);
    }
}

bool group_templates(Lowered &LW, const ShardUnits &U, LoweredPlan &P, std::string &err) {
    std::vector<SegInfo> &segs = LW.segs; std::vector<std::vector<int>> members;
    uint32_t maxd = 0; for (const SegInfo &S : segs) if ((uint32_t)S.depth > maxd) maxd = (uint32_t)S.depth;
    for (uint32_t d = 0; d <= maxd; d++)
        for (size_t si = 0; si < segs.size(); si++) {
            SegInfo &S = segs[si]; if ((uint32_t)S.depth != d) continue;
            int found = -1;
            for (size_t t = 0; t < members.size() && found < 0; t++) {
                const SegInfo &M = segs[(size_t)members[t][0]];
                if (M.depth == S.depth && M.name == S.name && M.nslots == S.nslots && M.nglp == S.nglp && M.nbnp == S.nbnp && M.imps.size() == S.imps.size() && M.inputs.size() == S.inputs.size() && M.tape == S.tape) found = (int)t;
            }
            if (found < 0) { members.push_back({}); found = (int)members.size() - 1; }
            S.tmpl = found; S.inst = (uint32_t)members[(size_t)found].size(); members[(size_t)found].push_back((int)si);
        }
    if (members.size() > (size_t)MAX_TMPL) { err = "h2w_plan_from_trace: more than " + std::to_string(MAX_TMPL) + " distinct scope shapes"; return false; }
    for (size_t t = 0; t < members.size(); t++) {
        const SegInfo &M = segs[(size_t)members[t][0]];
        TmplD T; T.tape0 = (uint32_t)P.tape.size(); T.nslots = M.nslots ? M.nslots : 1; T.ninst = (uint32_t)members[t].size(); T.inst0 = (uint32_t)P.insts.size(); T.depth = (uint32_t)M.depth;
        P.tape.insert(P.tape.end(), M.tape.begin(), M.tape.end());
        TapeLimits lim; lim.tmpl = t; lim.nslots = M.nslots; lim.nimps = M.imps.size(); lim.ninputs = M.inputs.size(); lim.nglp = M.nglp; lim.nbnp = M.nbnp;
        P.limits.push_back(lim);
        for (int si : members[t]) {
            const SegInfo &S = segs[(size_t)si];
            InstD I; I.cell0 = S.cell0; I.rec0 = S.rec0; I.imp0 = (uint32_t)P.imps.size(); I.in0 = (uint32_t)P.inputs.size();
            I.unit = S.unit; I.ucell0 = S.unit == NO_SLOT ? 0 : segs[(size_t)U.units[S.unit]].cell0; P.unit.push_back(S.unit);
            I.glp0 = P.nglp; P.nglp += S.nglp; P.glp_unit.insert(P.glp_unit.end(), S.nglp, S.unit);
            P.bnp0.push_back(P.nbnp); P.nbnp += S.nbnp; for (uint64_t c0 : S.bnp_cells) P.bnp.push_back(BnpD{c0, I.ucell0, S.unit, 0});
            for (const ImpD &m : S.imps) { const SegInfo &Pn = segs[(size_t)m.tmpl]; P.imps.push_back(ImpD{(uint32_t)Pn.tmpl, Pn.inst, m.slot}); }
            P.inputs.insert(P.inputs.end(), S.inputs.begin(), S.inputs.end());
            P.insts.push_back(I);
        }
        P.tmpls.push_back(T); P.total_slot_lanes += (uint64_t)T.nslots * T.ninst;
    }
    P.pool64.swap(LW.pool64); P.poolfr.swap(LW.poolfr); P.meta.swap(LW.meta); P.nrec = LW.nrec; P.n_segments = segs.size(); P.n_select_parts = LW.n_select_parts;
    return true;
}

// ---- the verdict stage: a segment's entries with the verdict's own import table; the first reason why there is no verdict stays
struct SegV { std::vector<VEntD> ents; std::vector<ImpD> imps; std::map<std::pair<uint32_t, uint32_t>, uint32_t> imp_of; };
static void no_verdict(VerdictTables &V, const std::string &m) { if (V.why.empty()) V.why = "the traced plan has no verdict: " + m; }
static void share_verdict_entries(const std::vector<SegV> &sv, const std::vector<SegInfo> &segs, const LoweredPlan &P, VerdictTables &V);
VerdictTables verdict_tables(const Trace *tr, const Lowered &LW, const Fusable &F, const LoweredPlan &P) {
    VerdictTables V; V.n_asserts = tr->asserts.size();
    const std::vector<SegInfo> &segs = LW.segs;
    std::vector<SegV> sv(segs.size());
    auto unavailable = [&](const std::string &m) { no_verdict(V, m); };
    // a handle's cell as an operand of a check in segment s (resolve_handle on the finished maps, with the verdict's own imports)
    auto vref = [&](int s, uint64_t cell, bool has_cell, const char *what, uint32_t &r) -> bool {
        r = 0;
        if (!has_cell) { unavailable(std::string(what) + " compares a handle that is no cell of the traced context"); return false; }
        int width; const HandleWhy why = resolve_handle(LW, s, cell, ImportTable{sv[(size_t)s].imps, sv[(size_t)s].imp_of}, r, width);
        if (why == HANDLE_NOT_TRACED) {
            for (const auto &kv : F.fuse) if (cell >= kv.second.cell0 && cell < kv.second.cell1) { unavailable(std::string(what) + " reads a value interior to a fused permutation, which the value store no longer has (cell " + std::to_string(cell) + "): lower the trace without the fuse flag for a verdict"); return false; }
            unavailable(std::string(what) + " reads a cell that is no traced call's result handle (cell " + std::to_string(cell) + ")");
        }
        if (why == HANDLE_NOT_ENCLOSING) unavailable(std::string(what) + " reads a value computed in a scope that does not enclose it (cell " + std::to_string(cell) + ")");
        return why == HANDLE_OK;
    };
    for (const TraceAssert &e : tr->asserts) {
        if (e.at > LW.op_seg.size()) { unavailable("internal: an equality beyond the tape"); break; }
        const int s = e.at == 0 ? 0 : LW.op_seg[(size_t)e.at - 1];
        VEntD d; d.kind = VK_EQUAL; d.site = e.site; d.aux = 0;
        if (!vref(s, e.a, e.a_cell != 0, "an equality", d.a) || !vref(s, e.b, e.b_cell != 0, "an equality", d.b)) break;
        sv[(size_t)s].ents.push_back(d);
    }
    for (const TraceRangeSite &rs : tr->range_sites) {
        if (!V.why.empty()) break;
        if (rs.op >= tr->ops.size()) { unavailable("internal: a range site beyond the tape"); break; }
        const TraceOp &o = tr->ops[(size_t)rs.op]; const int s = LW.op_seg[(size_t)rs.op];
        if (o.n_in != 1 || tr->ins[o.first_in].lit) { unavailable("internal: a range check without its operand"); break; }
        VEntD d; d.kind = o.code == TR_CLT_SAFE ? VK_CLT : VK_RANGE; d.site = rs.site; d.aux = o.imm; d.b = 0;
        if (!vref(s, tr->ins[o.first_in].v, true, "a range check", d.a)) break;
        if (vref_words(d.a) != 1) { unavailable("internal: a range check of a wide value"); break; }
        sv[(size_t)s].ents.push_back(d);
    }
    share_verdict_entries(sv, segs, P, V);
    if (!V.why.empty()) { V.ents.clear(); V.ent0.clear(); V.vimps.clear(); V.vimp0.clear(); V.nvimp.clear(); V.sites.clear(); V.site0.clear(); V.n_eq_lanes = V.n_range = V.n_tmpl = 0; }
    return V;
}
// the instances of a template share one table (their import tables, one per instance, make it concrete): InstD order
static void share_verdict_entries(const std::vector<SegV> &sv, const std::vector<SegInfo> &segs, const LoweredPlan &P, VerdictTables &V) {
    auto unavailable = [&](const std::string &m) { no_verdict(V, m); };
    std::vector<std::vector<int>> members(P.tmpls.size());
    for (size_t si = 0; si < segs.size(); si++) {
        const SegInfo &S = segs[si];
        if (S.tmpl < 0 || (size_t)S.tmpl >= members.size()) { unavailable("internal: a segment without a template"); break; }
        std::vector<int> &m = members[(size_t)S.tmpl]; if (m.size() <= S.inst) m.resize(S.inst + 1, -1); m[S.inst] = (int)si;
    }
    auto same = [](const VEntD &x, const VEntD &y) { return x.a == y.a && x.b == y.b && x.kind == y.kind && x.aux == y.aux; };      // (the site words are per instance)
    for (size_t t = 0; t < P.tmpls.size() && V.why.empty(); t++) {
        V.ent0.push_back((uint32_t)V.ents.size());
        if (members[t].size() != P.tmpls[t].ninst || members[t].empty() || members[t][0] < 0) { unavailable("internal: the instances of a template"); break; }
        const SegV &M = sv[(size_t)members[t][0]];
        for (int si : members[t]) {
            if (si < 0) { unavailable("internal: the instances of a template"); break; }
            const SegV &S = sv[(size_t)si]; bool eq = S.ents.size() == M.ents.size() && S.imps.size() == M.imps.size();
            for (size_t k = 0; eq && k < S.ents.size(); k++) eq = same(S.ents[k], M.ents[k]);
            if (!eq) { unavailable("the instances of one template (isomorphic scope instances) differ in the equalities recorded in them (template " + std::to_string(t) + ")"); break; }
            V.vimp0.push_back((uint32_t)V.vimps.size()); V.site0.push_back((uint32_t)V.sites.size());
            for (const VEntD &d : S.ents) V.sites.push_back(d.site);
            for (const ImpD &m : S.imps) { const SegInfo &Pn = segs[(size_t)m.tmpl]; V.vimps.push_back(ImpD{(uint32_t)Pn.tmpl, Pn.inst, m.slot}); }
            for (const VEntD &d : S.ents) {
                (d.kind == VK_EQUAL ? V.n_eq_lanes : V.n_range)++;
                // an imported value lies within its producer's slots, by the width the entry reads it with
                for (uint32_t r : {d.a, d.kind == VK_EQUAL ? d.b : d.a}) if (ref_kind(r) == RK_IMPORT) {
                    const ImpD &m = S.imps[ref_idx(r)]; const SegInfo &Pn = segs[(size_t)m.tmpl];
                    if ((uint64_t)m.slot + vref_words(r) > P.tmpls[(size_t)Pn.tmpl].nslots) unavailable("internal: an imported value beyond its producer's slots");
                }
            }
        }
        V.ents.insert(V.ents.end(), M.ents.begin(), M.ents.end()); V.nvimp.push_back((uint32_t)M.imps.size());
        if (!M.ents.empty()) V.n_tmpl++;
    }
    V.ent0.push_back((uint32_t)V.ents.size());
}

// clears the bits of the cells [c0, c0 + n) of a one-bit-per-cell map, word by word; false: one of them was clear already (the map is left as far as it got)
static bool clear_cells(std::vector<uint64_t> &bits, uint64_t c0, uint64_t n) {
    for (uint64_t c = c0; c < c0 + n;) {
        const uint64_t k = c & 63, take = std::min<uint64_t>(64 - k, c0 + n - c), mask = (take == 64 ? ~0ull : ((1ull << take) - 1)) << k;
        uint64_t &w = bits[(size_t)(c / 64)];
        if ((w & mask) != mask) return false;
        w &= ~mask; c += take;
    }
    return true;
}
bool direct_cell_map(const LoweredPlan &P, const TemplateTable &tt, uint64_t ncells, std::vector<uint64_t> &direct, uint64_t &n_direct, std::string &err) {
    direct.assign((size_t)(((ncells + 63) / 64 + 63) / 64 * 64), 0);
    for (uint64_t w = 0; w < ncells / 64; w++) direct[(size_t)w] = ~0ull;
    if (ncells & 63) direct[(size_t)(ncells / 64)] = (1ull << (ncells & 63)) - 1;
    uint64_t rec_cells = 0;
    for (size_t i = 0; i < P.meta.size(); i++) {
        const uint64_t c0 = meta_off(P.meta[i]), n = (uint64_t)tt.ncells((int)meta_tmpl(P.meta[i]));
        if (c0 + n > ncells) { err = "h2w_plan_from_trace_ex: internal: record " + std::to_string(i) + " lies beyond the stream"; return false; }
        if (!clear_cells(direct, c0, n)) { err = "h2w_plan_from_trace_ex: internal: record " + std::to_string(i) + " overlaps another record"; return false; }
        rec_cells += n;
    }
    n_direct = 0;
    for (uint64_t w : direct) n_direct += (uint64_t)__builtin_popcountll(w);
    if (n_direct + rec_cells != ncells) { err = "h2w_plan_from_trace_ex: internal: direct cells + record cells != cells of the stream"; return false; }
    return true;
}

bool ranged_cell_map(const LoweredPlan &P, uint64_t perm_cells, const std::vector<uint64_t> &direct, std::vector<uint64_t> &ranged, std::string &err) {
    ranged = direct;
    for (const BnpD &b : P.bnp)
        if (!clear_cells(ranged, b.cell0, perm_cells)) { err = "h2w_plan_from_trace_ex: internal: a fused permutation's cell is a record's cell, or two permutations overlap"; return false; }
    return true;
}

}  // namespace h2w
