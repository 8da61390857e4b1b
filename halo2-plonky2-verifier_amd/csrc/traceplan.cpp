// traceplan.cpp — the host side of a traced plan (traceplan.h): h2w_plan_from_trace in its three stages - lower (tracelower.h's stages in order, every
// tape checked, the verdict stage), fill_handle (the plan handle: strand table, direct and ranged maps, keygen metadata), upload (the device tables) -,
// the lane tables of the calls that do not run every lane in place, the Montgomery form's first-use tables, the information entry points.
// No kernel and no launch: the interpreter and its launchers are replay.hip, whose code a change here cannot move.
#include <hip/hip_runtime.h>
#include <unordered_map>
#include <vector>
#include <string>
#include <cstring>
#include <cstdlib>
#include <cstdio>
#include "traceplan.h"
#include "keygen.h"

namespace h2w {

uint64_t traced_workspace_bytes(const h2w_plan *p, uint64_t n) { return traced_ws(p, n).total; }
uint64_t traced_status_offset(const h2w_plan *p, uint64_t n, bool flags) { const TracedWs w = traced_ws(p, n); return flags ? w.lflag : w.status; }
const char *traced_shard_refusal(const h2w_plan *p) { return p->traced && !p->traced->why_unshardable.empty() ? p->traced->why_unshardable.c_str() : nullptr; }
void traced_free(h2w_plan *p) { delete p->traced; p->traced = nullptr; }      // (its tables and events are owners: devbuf.h)

// ---- the lane tables (lanetable.h fills them)
static int install(LaneTable &T, Lanes &L, const std::vector<uint32_t> *bn_items, uint64_t n, int rank, int world) {
    H2W_HIP(hipDeviceSynchronize());      // a previous call may still read the old table (plans are single-threaded handles, include/h2w.h)
    T.d_lanes.reset(); T.d_bn_items.reset(); T.n_bn_items = bn_items ? bn_items->size() : 0;
    if ((bn_items && T.d_bn_items.upload(*bn_items) != 0) || T.d_lanes.upload(L.words) != 0) return -1;
    T.lane0.swap(L.lane0); T.n = n; T.rank = rank; T.world = world;
    return 0;
}
int traced_sharded_lanes(h2w_plan *p, uint64_t n, const ShardSpec &sh) {
    TracedPlan *t = p->traced;
    if (t->lanes.built_for(n, sh.rank, sh.world)) return 0;
    const uint64_t nq = (uint64_t)p->shape.num_queries;
    Lanes L; std::vector<uint32_t> items;
    const char *why = fill_sharded_lanes(t->tmpls, t->h_unit, n, nq, (uint64_t)sh.rank, (uint64_t)sh.world, L);
    if (!why) why = fill_sharded_bn_items(t->h_bnp, n, nq, (uint64_t)sh.rank, (uint64_t)sh.world, items);
    if (why) { set_error(why); return -1; }
    return install(t->lanes, L, t->nbnp ? &items : nullptr, n, sh.rank, sh.world);
}
int traced_quiet_lanes(h2w_plan *p, uint64_t n) {
    TracedPlan *t = p->traced;
    if (t->qlanes.built_for(n, 0, 1)) return 0;
    Lanes L;
    if (const char *why = fill_quiet_lanes(t->tmpls, n, L)) { set_error(why); return -1; }
    return install(t->qlanes, L, nullptr, n, 0, 1);
}

int traced_mont_tables(const h2w_plan *p, DevBuf<fr_t> &bn_tab_mont, DevBuf<uint64_t> &ranged_bits) {
    if (!p->traced || !p->d_bn_tab.get()) return 0;
    std::vector<fr_t> tab(BK_ALL); bn_table_build(p->h_consts, p->P, tab.data());
    for (int i = 0; i < BK_T; i++) tab[(size_t)i] = fr_mont_mul(tab[(size_t)i], mont_k(), p->P.ninv);
    return bn_tab_mont.upload(tab) != 0 || ranged_bits.upload(p->ranged_bits) != 0 ? -1 : 0;
}

// ---- h2w_plan_from_trace
struct LoweredTrace { Fusable F; ShardUnits U; LoweredPlan LP; VerdictTables VT; std::vector<uint64_t> op_counts; };
#ifdef H2W_LOWERING_DUMP
// What the lowering produced, every item as a count and its raw bytes, to the file H2W_LOWERING_DUMP_FILE names (tools/lowering_digest.py hashes it: a
// change of tracelower.cpp that is meant to change nothing is held to equal files).  A variant build only: the product library has no such switch.
struct LoweringDump {
    FILE *f;
    explicit LoweringDump(const char *mode) { const char *path = getenv("H2W_LOWERING_DUMP_FILE"); f = path ? fopen(path, mode) : nullptr; }
    ~LoweringDump() { if (f) fclose(f); }
    void raw(const void *p, size_t count, size_t size) { if (!f) return; const uint64_t n = count; fwrite(&n, 8, 1, f); if (count) fwrite(p, size, count, f); }
    template <class T> void vec(const std::vector<T> &v) { raw(v.data(), v.size(), sizeof(T)); }
    void num(uint64_t v) { if (f) fwrite(&v, 8, 1, f); }
    void text(const std::string &s) { raw(s.data(), s.size(), 1); }
};
static void dump_lowering(const LoweredTrace &W, uint64_t ncells) {
    LoweringDump D("wb"); const LoweredPlan &LP = W.LP; const ShardUnits &U = W.U; const VerdictTables &VT = W.VT;
    D.vec(LP.tape); D.vec(LP.insts); D.vec(LP.imps); D.vec(LP.inputs); D.vec(LP.pool64); D.vec(LP.poolfr); D.vec(LP.meta); D.vec(LP.tmpls);
    D.vec(LP.unit); D.vec(LP.glp_unit); D.vec(LP.bnp); D.vec(LP.bnp0);
    D.num(LP.nrec); D.num(ncells); D.num(U.num_queries); D.num(U.pro_ncell); D.num(U.pro_nrec);
    for (int k = 0; k < 2; k++) { D.num(U.q_cell0[k]); D.num(U.q_rec0[k]); D.num(U.q_ncell[k]); D.num(U.q_nrec[k]); }
    D.vec(U.units); D.text(U.why_unshardable);
    D.num(W.F.fuse.size()); D.num(W.F.glp_meta.size()); D.num(W.F.glp_block_cells); D.num(W.F.n_candidates); D.num(W.F.n_bn_left); D.num(LP.nglp); D.num(LP.nbnp);
    D.num(LP.total_slot_lanes); D.num(LP.n_segments); D.num(LP.n_select_parts); D.vec(W.op_counts);
    D.vec(VT.ents); D.vec(VT.ent0); D.vec(VT.vimps); D.vec(VT.vimp0); D.vec(VT.nvimp); D.vec(VT.sites); D.vec(VT.site0);
    D.num(VT.n_asserts); D.num(VT.n_eq_lanes); D.num(VT.n_range); D.num(VT.n_tmpl); D.text(VT.why);
}
#endif
// Host only.  false: err is the message
static bool lower(h2w_ctx *ctx, uint64_t proof_words, const char *const *parallel_scopes, size_t n_scopes, const h2w_poseidon_consts_t *consts, uint32_t flags, LoweredTrace &W, std::string &err) {
    const Trace *tr = ctx_trace(ctx);
    if (!tr) { err = "h2w_plan_from_trace: the context is not in trace mode (h2w_ctx_trace_begin)"; return false; }
    if (!tr->err.empty()) { err = "h2w_plan_from_trace: " + tr->err; return false; }
    if (tr->pending.kind) { err = "h2w_plan_from_trace: a h2w_trace_input tag was never consumed"; return false; }
    const bool fusing = (flags & H2W_TRACE_FUSE_GL_PERMUTE) != 0, fusing_bn = (flags & H2W_TRACE_FUSE_BN_PERMUTE) != 0;
    const bool split_selects = (flags & H2W_TRACE_SPLIT_SELECTS) != 0;
    if (flags & ~(uint32_t)(H2W_TRACE_FUSE_GL_PERMUTE | H2W_TRACE_FUSE_BN_PERMUTE | H2W_TRACE_OUTPUT_FORMS | H2W_TRACE_SPLIT_SELECTS)) { err = "h2w_plan_from_trace_ex: unknown flag"; return false; }
    if (fusing && !consts) { err = "h2w_plan_from_trace_ex: H2W_TRACE_FUSE_GL_PERMUTE needs the Poseidon tables the permutations are claimed to use"; return false; }
    if (fusing_bn && !consts) { err = "h2w_plan_from_trace_ex: H2W_TRACE_FUSE_BN_PERMUTE needs the Poseidon tables the permutations are claimed to use"; return false; }
    const int L = ctx_lookup_bits(ctx); const uint64_t ncells = ctx_num_cells(ctx);
    TemplateTable tt(L);
    Fusable &F = W.F; LoweredPlan &LP = W.LP; VerdictTables &VT = W.VT; Lowered LW;
    if (!find_fusable(tr, L, tt, parallel_scopes, n_scopes, consts, fusing, fusing_bn, split_selects, F, err)) return false;
    lower_trace(tr, L, tt, parallel_scopes, n_scopes, F, split_selects, LW);
    if (!LW.err.empty()) { err = "h2w_plan_from_trace: " + LW.err; return false; }
    W.U = shard_units(LW, ncells);
    pack_glop_runs(LW, tt);
    if (!group_templates(LW, W.U, LP, err)) return false;
    // what a template's tape and verdict table are held against: the lowering's counts of its segments + the plan-wide limits
    auto limits = [&](size_t t) {
        TapeLimits M = LP.limits[t]; M.inputs = LP.inputs.data() + LP.insts[LP.tmpls[t].inst0].in0; M.npool64 = LP.pool64.size(); M.npoolfr = LP.poolfr.size();
        M.proof_words = proof_words; M.fusing_gl = fusing; M.fusing_bn = fusing_bn;
        M.glp_block_cells = F.glp_block_cells; M.glp_recs = F.glp_meta.size(); M.glp_recs_kernel = (size_t)GLP_RECS; M.bn_perm_cells = (uint64_t)BN_PERM_CELLS;
        return M;
    };
    for (size_t t = 0; t < LP.tmpls.size(); t++) {
        err = tape_check(LP.tmpl_tape(t), LP.tmpl_tape_words(t), limits(t));
        if (!err.empty()) { err = "h2w_plan_from_trace: " + err; return false; }
    }
    // the verdict stage, behind the final tapes (it reads the lowering's maps and changes nothing); its table checked like a tape before it is uploaded
    VT = verdict_tables(tr, LW, F, LP);
    for (size_t t = 0; VT.why.empty() && t < LP.tmpls.size(); t++) {
        TapeLimits M = limits(t); M.nimps = VT.nvimp[t];
        const std::string verr = verdict_table_check(VT.ents.data() + VT.ent0[t], VT.ent0[t + 1] - VT.ent0[t], M);
        if (!verr.empty()) { VT = VerdictTables(); VT.n_asserts = tr->asserts.size(); VT.why = "the traced plan has no verdict: " + verr; }      // (the witness plan is not the verdict's to refuse)
    }
    W.op_counts.assign(TAPE_COUNTS, 0);      // h2w_plan_trace_op_counts: over every template's final tape
    for (size_t t = 0; t < LP.tmpls.size(); t++) tape_op_counts(LP.tmpl_tape(t), LP.tmpl_tape_words(t), W.op_counts.data());
    for (uint32_t w : LP.inputs) if (w >= proof_words) { err = "h2w_plan_from_trace: an input tag beyond proof_words"; return false; }
    for (const BnpD &b : LP.bnp) if (b.cell0 + (uint64_t)BN_PERM_CELLS > ncells) { err = "h2w_plan_from_trace_ex: internal: a fused permutation's cells lie beyond the stream"; return false; }
#ifdef H2W_LOWERING_DUMP
    dump_lowering(W, ncells);
#endif
    return true;
}
// The plan handle and its TracedPlan, host members only.  null: the last error says why
static h2w_plan *fill_handle(h2w_ctx *ctx, uint64_t proof_words, int device_id, const h2w_poseidon_consts_t *consts, uint32_t flags, LoweredTrace &W) {
    const Trace *tr = ctx_trace(ctx); const int L = ctx_lookup_bits(ctx); const uint64_t ncells = ctx_num_cells(ctx);
    const Fusable &F = W.F; const ShardUnits &U = W.U; const LoweredPlan &LP = W.LP;
    int ndev = 0; const bool on_device = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;      // (none: layout queries only)
    if (on_device && (device_id < 0 || device_id >= ndev)) { set_error("h2w_plan_from_trace: device_id out of range"); return nullptr; }
    TracedPlan *tp = new TracedPlan();
    tp->tmpls = LP.tmpls; tp->total_slot_lanes = LP.total_slot_lanes; tp->h_unit = LP.unit; tp->nglp = LP.nglp; tp->h_glp_unit = LP.glp_unit; tp->nbnp = LP.nbnp; tp->h_bnp = LP.bnp; tp->h_bnp0 = LP.bnp0;
    tp->n_ops = tr->ops.size(); tp->n_segments = LP.n_segments; tp->why_unshardable = U.why_unshardable; tp->n_candidates = F.n_candidates;
    tp->bn_flag = (flags & H2W_TRACE_FUSE_BN_PERMUTE) != 0; tp->n_bn_left = F.n_bn_left; tp->select_parts = LP.n_select_parts != 0;
    tp->npool64 = (uint32_t)LP.pool64.size(); tp->npoolfr = (uint32_t)LP.poolfr.size();
    tp->op_counts.swap(W.op_counts);
    tp->why_no_verdict = W.VT.why; tp->vt = W.VT;
    h2w_plan *pl = new h2w_plan(L);
    memset(&pl->shape, 0, sizeof(pl->shape)); pl->shape.lookup_bits = L; pl->shape.num_queries = U.num_queries; pl->shape.hash_mode = 1;
    pl->device = on_device ? device_id : -1; pl->P = fr_params_init(); memset(&pl->st, 0, sizeof(pl->st)); memset(&pl->pl, 0, sizeof(pl->pl)); memset(&pl->d, 0, sizeof(pl->d));
    pl->pl.total = proof_words; pl->nrec = LP.nrec; pl->ncells = ncells; pl->traced = tp;
    if (flags & H2W_TRACE_OUTPUT_FORMS) {      // the direct-cell map of H2W_OPT_OUTPUT_FORM (the plan does not keep the tape: now)
        std::string err;
        if (!direct_cell_map(LP, pl->tt, ncells, pl->direct_bits, pl->n_direct, err) || !ranged_cell_map(LP, (uint64_t)BN_PERM_CELLS, pl->direct_bits, pl->ranged_bits, err)) { set_error(err); h2w_plan_free(pl); return nullptr; }
        pl->trace_forms = true; pl->trace_bn_ranged = getenv("H2W_TRACE_BN_RANGED") != nullptr;
#ifdef H2W_LOWERING_DUMP
        { LoweringDump D("ab"); D.vec(pl->direct_bits); D.vec(pl->ranged_bits); D.num(pl->n_direct); }
#endif
    }
    if (consts) pl->h_consts = *consts;
    for (uint64_t m : LP.meta) pl->rec_cells += (uint64_t)pl->tt.ncells((int)meta_tmpl(m));
    // the block structure (StrandTable: what h2w_plan_strand_layout / _shard_cells / _shard_block and the sharded expansion read): unshardable, one block
    StrandTable &st = pl->st; st.first_zero_kind = -1; st.first_zero_unit = -1; st.total_rec = LP.nrec; st.total_cell = ncells;
    st.pro_ncell = U.pro_ncell; st.pro_nrec = U.pro_nrec;
    for (int k = 0; k < 2; k++) { st.q_cell0[k] = U.q_cell0[k]; st.q_rec0[k] = U.q_rec0[k]; st.q_ncell[k] = U.q_ncell[k]; st.q_nrec[k] = U.q_nrec[k]; }
    // keygen metadata (witness_gen_only = 0): the tracing context's own lists (keygen.h), as h2w_plan_metadata / h2w_plan_equalities hand them out
    if (const MetaRecorder *mr = ctx_meta(ctx)) {
        pl->sel_bits.assign((size_t)(pl->ncells + 7) / 8, 0); pl->lk_bits.assign(pl->sel_bits.size(), 0);
        for (uint64_t c : mr->sel) if (c < pl->ncells) pl->sel_bits[c / 8] |= (uint8_t)(1u << (c & 7));
        for (uint64_t c : mr->lookups) if (c < pl->ncells) pl->lk_bits[c / 8] |= (uint8_t)(1u << (c & 7));
        for (uint8_t b : pl->sel_bits) pl->n_gates += (uint64_t)__builtin_popcount(b);
        for (uint8_t b : pl->lk_bits) pl->n_lookups += (uint64_t)__builtin_popcount(b);
        pl->meta_ready = true;
        PlanEqualities &E = pl->eqs; E.pairs = mr->eq; E.const_cells = mr->ceq_cell; E.const_values = mr->ceq_val; E.const_word.assign(E.const_cells.size(), -1);
        // proof words loaded as constants (Goldilocks-Poseidon hash wires, hash/poseidon/hash.rs:86-96): their constant equality takes the given proof's word
        std::unordered_map<uint64_t, const TraceOp *> word_const;
        for (const TraceOp &o : tr->ops) if (o.code == TR_LOAD_CONSTANT && o.tag.kind == 1) word_const[o.cell0] = &o;
        for (size_t i = 0; i < E.const_cells.size(); i++) {
            auto it = word_const.find(E.const_cells[i]);
            if (it != word_const.end() && fr_eq(E.const_values[i], tr->consts[(size_t)it->second->imm])) E.const_word[i] = (int64_t)it->second->tag.word;
        }
        E.ready = true;
    }
    if (!on_device && pl->trace_forms) pl->h_meta = LP.meta;      // (h2w_plan_record_ranges: with a device it reads d_meta back)
    return pl;
}
// The device tables.  false: an allocation or a copy failed (the last error)
static bool upload(h2w_plan *pl, LoweredTrace &W, const h2w_poseidon_consts_t *consts) {
    TracedPlan *tp = pl->traced; LoweredPlan &LP = W.LP; const VerdictTables &VT = W.VT;
    DeviceGuard dg(pl->device);
    for (int k2 = 0; k2 < 16; k2++) LP.tape.push_back(DOP_END | (1u << 24));      // the interpreter reads a window ahead
    std::vector<uint64_t> prefix(tp->tmpls.size()); uint64_t acc = 0;
    for (size_t i = 0; i < tp->tmpls.size(); i++) { prefix[i] = acc; acc += (uint64_t)tp->tmpls[i].nslots * tp->tmpls[i].ninst; }
    bool ok = pl->dt.upload(pl->tt) == 0 && pl->d_meta.upload(LP.meta) == 0 && tp->d_tape.upload(LP.tape) == 0 && tp->d_tm.upload(tp->tmpls) == 0 &&
              tp->d_prefix.upload(prefix) == 0 && tp->d_insts.upload(LP.insts) == 0 && tp->d_imps.upload(LP.imps) == 0 && tp->d_inputs.upload(LP.inputs) == 0 &&
              tp->d_pool64.upload(LP.pool64) == 0 && tp->d_poolfr.upload(LP.poolfr) == 0 && upload_tmpl_cells(pl->d_ncells, pl->tt) == 0 &&
              pl->d_inv.upload(inverse_table(pl->P)) == 0;
    // the tables the fused permutations were verified on (handletabs.h); which shard unit a listed permutation belongs to / where it lies
    if (ok && tp->nglp) ok = upload_glp_consts(pl->d_consts, *consts) == 0 && tp->d_glp_unit.upload(tp->h_glp_unit) == 0;
    if (ok && tp->nbnp) ok = upload_bn_tab(pl->d_bn_tab, *consts, pl->P) == 0 && tp->d_bnp.upload(tp->h_bnp) == 0 && tp->d_bnp0.upload(tp->h_bnp0) == 0;
    if (ok && VT.why.empty()) {      // the verdict's tables: the entries, per instance {first verdict import, first input, unit}, the imports, per template {prefix, instances}
        std::vector<VInstD> vi(LP.insts.size()); std::vector<VImpD> vm(VT.vimps.size()); std::vector<uint64_t> ti(2 * tp->tmpls.size());
        for (size_t i = 0; i < vi.size(); i++) vi[i] = VInstD{VT.vimp0[i], LP.insts[i].in0, LP.insts[i].unit, VT.site0[i]};
        for (size_t i = 0; i < vm.size(); i++) vm[i] = VImpD{VT.vimps[i].tmpl, VT.vimps[i].inst, VT.vimps[i].slot, 0};
        for (size_t i = 0; i < tp->tmpls.size(); i++) { ti[2 * i] = prefix[i]; ti[2 * i + 1] = tp->tmpls[i].ninst; }
        ok = tp->d_vinst.upload(vi) == 0 && tp->d_tinfo.upload(ti) == 0 && (VT.ents.empty() || (tp->d_vents.upload(VT.ents) == 0 && tp->d_vsites.upload(VT.sites) == 0)) && (vm.empty() || tp->d_vimps.upload(vm) == 0);
    }
    return ok;
}
static h2w_plan *plan_from_trace(h2w_ctx *ctx, uint64_t proof_words, const char *const *parallel_scopes, size_t n_scopes, int device_id, const h2w_poseidon_consts_t *consts, uint32_t flags) {
    LoweredTrace W; std::string err;
    if (!lower(ctx, proof_words, parallel_scopes, n_scopes, consts, flags, W, err)) { set_error(err); return nullptr; }
    h2w_plan *pl = fill_handle(ctx, proof_words, device_id, consts, flags, W);
    if (pl && pl->device >= 0 && !upload(pl, W, consts)) { h2w_plan_free(pl); return nullptr; }
    return pl;
}

}  // namespace h2w

extern "C" h2w_plan *h2w_plan_from_trace(h2w_ctx *ctx, uint64_t proof_words, const char *const *parallel_scopes, size_t n_scopes, int device_id) {
    return plan_from_trace(ctx, proof_words, parallel_scopes, n_scopes, device_id, nullptr, 0);
}
extern "C" h2w_plan *h2w_plan_from_trace_ex(h2w_ctx *ctx, uint64_t proof_words, const char *const *parallel_scopes, size_t n_scopes, int device_id, const h2w_poseidon_consts_t *consts, uint32_t flags) {
    return plan_from_trace(ctx, proof_words, parallel_scopes, n_scopes, device_id, consts, flags);
}
// the plan of an information entry point; null: the last error says what is wrong with it
static const TracedPlan *info_plan(const char *entry, const h2w_plan *p, bool args_ok, const char *else_hint = "") {
    if (!p || !args_ok) { set_error(std::string(entry) + ": null argument"); return nullptr; }
    if (!p->traced) { set_error(std::string(entry) + ": not a traced plan (h2w_plan_from_trace)" + else_hint); return nullptr; }
    return p->traced;
}
extern "C" int h2w_plan_trace_info(const h2w_plan *p, uint64_t out[6]) {
    const TracedPlan *t = info_plan("h2w_plan_trace_info", p, out != nullptr);
    if (!t) return -1;
    out[0] = t->n_ops; out[1] = t->n_segments; out[2] = t->tmpls.size(); out[3] = t->nglp; out[4] = t->n_candidates; out[5] = t->nglp;
    return 0;
}
extern "C" int h2w_plan_trace_info_bn(const h2w_plan *p, uint64_t out[3]) {
    const TracedPlan *t = info_plan("h2w_plan_trace_info_bn", p, out != nullptr);
    if (!t) return -1;
    out[0] = t->nbnp; out[1] = t->n_bn_left; out[2] = t->nbnp;
    return 0;
}
extern "C" int h2w_plan_trace_verdict_info(const h2w_plan *p, uint64_t out[6]) {
    const TracedPlan *t = info_plan("h2w_plan_trace_verdict_info", p, out != nullptr, "; a plan of h2w_plan_compile has h2w_fri_verdict_batch");
    if (!t) return -1;
    const VerdictTables &V = t->vt;
    out[0] = V.n_asserts; out[1] = V.n_eq_lanes; out[2] = V.n_range; out[3] = t->why_no_verdict.empty() ? 1 : 0; out[4] = V.n_tmpl; out[5] = 0;
    if (!t->why_no_verdict.empty()) set_error("h2w_plan_trace_verdict_info: " + t->why_no_verdict);
    return 0;
}
extern "C" int h2w_plan_trace_op_counts(const h2w_plan *p, uint64_t *out, size_t n_out) {
    const TracedPlan *t = info_plan("h2w_plan_trace_op_counts", p, out || !n_out);
    if (!t) return -1;
    const std::vector<uint64_t> &c = t->op_counts;
    for (size_t i = 0; i < n_out; i++) out[i] = i < c.size() ? c[i] : 0;
    return (int)c.size();
}
// ms of the kernels of the last call: the k_replay launch of every depth, k_glp_emit_traced, (plans built with H2W_TRACE_FUSE_BN_PERMUTE) k_bn_emit_traced,
// (plans built with H2W_TRACE_OUTPUT_FORMS) the direct cells' conversion - nothing in canonical form -, the expansion.  The first call switches the events on
// (0 entries); later ones wait for the last call and report it.
extern "C" int h2w_plan_trace_timing(h2w_plan *p, float *ms, uint32_t cap) {
    if (!p || !ms) { set_error("h2w_plan_trace_timing: null argument"); return -1; }
    if (!p->traced || p->device < 0) { set_error("h2w_plan_trace_timing: not a traced plan on a device"); return -1; }
    TracedPlan *t = p->traced; DeviceGuard dg(p->device);
    if (!t->timing) { for (DevEvent &e : t->tev) if (e.create() != 0) return -1; t->timing = true; return 0; }
    if (t->tev_used < 2) return 0;
    H2W_HIP(hipEventSynchronize(t->tev[t->tev_used - 1]));
    int n = 0;
    for (int i = 0; i + 1 < t->tev_used && (uint32_t)n < cap; i++, n++) H2W_HIP(hipEventElapsedTime(&ms[n], t->tev[i], t->tev[i + 1]));
    return n;
}
