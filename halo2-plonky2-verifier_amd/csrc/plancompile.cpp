// plancompile.cpp — the compiled plan of API level 3 (include/h2w.h), host side: what is fixed per shape before any proof is seen.
//
//   h2w_plan_compile  : shape compiler.  Replays the gadget once on the host with a counting sink (ValBackend<PlanSink>) on an all-zero proof to fix
//                       the offset of every cell block and strand for this shape, then uploads the shape's tables (handletabs.h) into the handle.
//   h2w_plan_metadata : keygen-side metadata of the cell stream (selectors, looked-up cells): a second host replay, on demand.
//   h2w_plan_free, the plan's layout queries (h2w_plan_num_*, _direct_cells, _record_ranges, _strand_layout, _num_chain_cells, _selectors,
//   _lookup_cells), h2w_break_points, and the plan_* accessors the other units reach the handle through.
// The launch sequence of a witness call is batch.hip; what works on a finished advice stream is advicetools.hip.
#include <hip/hip_runtime.h>
#include <vector>
#include <string>
#include <cstring>
#include "plan.h"
#include "traceplan.h"

namespace h2w {

struct PlanSink : SinkBase {
    std::vector<uint64_t> *meta; const TemplateTable *tt; StrandTable *st;
    uint64_t nrec = 0, cell_off = 0, cur_q_rec = 0, cur_q_cell = 0, mk_rec0 = 0, mk_cell0 = 0; bool mk_zc = false;
    std::vector<uint64_t> *unit_cell = nullptr; uint64_t nunit = 0, cur_q_unit = 0, mk_unit0 = 0; bool pu_zc = false;
    uint64_t nglp = 0, cur_q_glp = 0, mk_glp0 = 0; int cur_q = -1;
    std::vector<LoadItem> *items = nullptr, *cap_items = nullptr;
    void note_load(uint64_t w, int kind) { LoadItem it; it.word = (uint32_t)w; it.kind = (uint32_t)kind; it.rec = nrec; it.cell = cell_off; items->push_back(it); }
    void note_cap_hash(uint64_t w) { if (cap_items) { LoadItem it; it.word = (uint32_t)w; it.kind = 4; it.rec = nrec; it.cell = cell_off; cap_items->push_back(it); } }
    void bn_perm_begin(bool zc) { unit_cell->push_back(cell_off); pu_zc = zc; }
    void bn_perm_end(bool zc) { if (!pu_zc && zc) st->first_zero_unit = (int64_t)nunit; nunit++; }
    void glp_note() { nglp++; }
    // keygen metadata pass (h2w_plan_metadata): one bit per cell, set from the template slot flags / the backend's G()/LK() markers
    std::vector<uint8_t> *sel_bits = nullptr, *lk_bits = nullptr; uint8_t pend = 0;
    std::vector<uint64_t> *direct = nullptr;      // one bit per cell: written by a value kernel itself, not by the expansion kernel (H2W_OPT_OUTPUT_FORM)
    void mark(uint64_t cell, uint8_t f) {
        if (f & CF_GATE) { if (sel_bits->size() <= cell / 8) sel_bits->resize(cell / 8 + 4096, 0); (*sel_bits)[cell / 8] |= (uint8_t)(1u << (cell & 7)); }
        if (f & CF_LOOKUP) { if (lk_bits->size() <= cell / 8) lk_bits->resize(cell / 8 + 4096, 0); (*lk_bits)[cell / 8] |= (uint8_t)(1u << (cell & 7)); }
    }
    void gate() { pend |= CF_GATE; }
    void lookup() { pend |= CF_LOOKUP; }
    void rec(int t, uint64_t, uint64_t, uint64_t, uint64_t) {
        if (meta) meta->push_back(meta_pack((uint32_t)t, cell_off));
        if (sel_bits) { const tmpl_info_t &ti = tt->info[t]; for (int i = 0; i < ti.ncells; i++) { const uint8_t f = tt->slot_flags[ti.slot_base + i]; if (f) mark(cell_off + i, f); } }
        nrec++; cell_off += (uint64_t)tt->ncells(t);
    }
    void cell(const fr_t &) {
        if (sel_bits && pend) mark(cell_off, pend);
        if (direct) { if (direct->size() <= cell_off / 64) direct->resize(cell_off / 64 + 65536, 0); (*direct)[cell_off / 64] |= 1ull << (cell_off & 63); }
        pend = 0; cell_off++;
    }
    void skip(uint64_t, uint64_t) {}
    void merkle_begin(int, int, bool zc, uint64_t) { mk_rec0 = nrec; mk_cell0 = cell_off; mk_zc = zc; mk_unit0 = nunit; mk_glp0 = nglp; }
    void merkle_end(int q, int kind, bool zc) {
        if (q > 1) return;
        st->mk_rec_rel[q][kind] = mk_rec0 - cur_q_rec; st->mk_cell_rel[q][kind] = mk_cell0 - cur_q_cell;
        st->mk_nrec[q][kind] = nrec - mk_rec0; st->mk_ncell[q][kind] = cell_off - mk_cell0; st->mk_unit_rel[q][kind] = mk_unit0 - cur_q_unit;
        st->mk_nunit[kind] = (uint32_t)(nunit - mk_unit0); st->mk_glp_rel[kind] = (uint32_t)(mk_glp0 - cur_q_glp); st->mk_nglp[kind] = (uint32_t)(nglp - mk_glp0);
        if (!mk_zc && zc) st->first_zero_kind = (q == 0) ? kind : -2;
    }
    void query_begin(int q, uint64_t) {
        cur_q_rec = nrec; cur_q_cell = cell_off; cur_q_unit = nunit; cur_q_glp = nglp;
        if (q == 0) st->pro_nglp = (uint32_t)nglp;
        if (q <= 1) { st->q_rec0[q] = nrec; st->q_cell0[q] = cell_off; st->q_unit0[q] = nunit; }
    }
    void query_end(int q, uint64_t) { if (q <= 1) { st->q_nrec[q] = nrec - cur_q_rec; st->q_ncell[q] = cell_off - cur_q_cell; st->q_nunit[q] = nunit - cur_q_unit; st->q_nglp = (uint32_t)(nglp - cur_q_glp); } }
};

// the configuration of both host replays: the sequential run, no strand table, nothing split off - every field not named here is null / 0 / false
static ValCfg host_replay_cfg(const h2w_shape_t &s, const FrParams &P, const std::vector<fr_t> &inv, const uint64_t *proof) {
    ValCfg cfg{}; cfg.proof = proof; cfg.mode = s.hash_mode; cfg.L = s.lookup_bits; cfg.P = P; cfg.inv_pos = inv.data(); cfg.inv_neg = inv.data() + INV_TAB;
    return cfg;
}
PlanEqualities &plan_equalities(h2w_plan *p) { return p->eqs; }
bool plan_traced(const h2w_plan *p) { return p->traced != nullptr; }
const h2w_shape_t &plan_shape(const h2w_plan *p) { return p->shape; }
const h2w_poseidon_consts_t &plan_consts(const h2w_plan *p) { return p->h_consts; }
uint64_t plan_cells(const h2w_plan *p) { return p->ncells; }
}

extern "C" {

h2w_plan *h2w_plan_compile(const h2w_shape_t *shape, const h2w_poseidon_consts_t *consts, int device_id) {
    if (!shape || !consts) { set_error("h2w_plan_compile: null argument"); return nullptr; }
    const h2w_shape_t &s = *shape;
    if (const char *why = shape_check(s)) { set_error(std::string("h2w_plan_compile: unsupported shape: ") + why); return nullptr; }
    h2w_plan *pl = new h2w_plan(s.lookup_bits);
    pl->shape = s; pl->device = device_id; pl->P = fr_params_init(); pl->h_consts = *consts;
    pl->d = derive_shape(s); pl->pl = proof_layout(s, pl->d);
    memset(&pl->st, 0, sizeof(pl->st)); pl->st.first_zero_kind = -1; pl->st.first_zero_unit = -1;
    std::vector<uint64_t> unit_cell; std::vector<LoadItem> items, cap_items;
    const std::vector<fr_t> inv = inverse_table(pl->P);
    // shape compile: sequential replay with the counting sink on an all-zero proof
    std::vector<uint64_t> meta; std::vector<uint64_t> zero_proof(pl->pl.total, 0);
    {
        PlanSink sink; sink.meta = &meta; sink.tt = &pl->tt; sink.st = &pl->st; sink.unit_cell = &unit_cell; sink.items = &items; sink.cap_items = &cap_items;
        sink.direct = &pl->direct_bits;
        ValBackend<PlanSink> be(sink, host_replay_cfg(s, pl->P, inv, zero_proof.data()), false);
        Verifier<ValBackend<PlanSink>> V(be, pl->shape, consts);
        ChallengeBlock<ValBackend<PlanSink>> *cb = new ChallengeBlock<ValBackend<PlanSink>>();
        V.run_all(*cb);
        delete cb;
        pl->n_items = (uint32_t)items.size(); pl->n_cap_items = s.hash_mode == 1 ? (uint32_t)cap_items.size() : 0;
        if (!items.empty()) {   // records / cells of the load phase: from the first item to the end of the last one
            // the load phase starts right after the 12 zero-state constants and is contiguous in records and cells
            const LoadItem &last = items.back();
            uint64_t last_nrec = last.kind == 3 ? 0 : 1, last_ncell = last.kind == 0 ? (uint64_t)pl->tt.ncells(T_LOADW) : last.kind == 1 ? 1 : last.kind == 2 ? 4 : 1;
            pl->load_nrec = last.rec + last_nrec - items.front().rec; pl->load_ncell = last.cell + last_ncell - items.front().cell;
        }
        pl->nrec = sink.nrec; pl->ncells = sink.cell_off; pl->nunit = sink.nunit; pl->st.total_unit = sink.nunit;
        pl->direct_bits.resize((size_t)(((pl->ncells + 63) / 64 + 63) / 64 * 64), 0);
        for (uint64_t w : pl->direct_bits) pl->n_direct += (uint64_t)__builtin_popcountll(w);
        for (uint64_t m : meta) pl->rec_cells += (uint64_t)pl->tt.ncells((int)meta_tmpl(m));
        pl->st.pro_nrec = pl->st.q_rec0[0]; pl->st.pro_ncell = pl->st.q_cell0[0]; pl->st.total_rec = sink.nrec; pl->st.total_cell = sink.cell_off;
        if (s.num_queries == 1) {
            pl->st.q_unit0[1] = pl->st.q_unit0[0]; pl->st.q_nunit[1] = pl->st.q_nunit[0];
            for (int k2 = 0; k2 < MK_KINDS; k2++) pl->st.mk_unit_rel[1][k2] = pl->st.mk_unit_rel[0][k2];
            pl->st.q_rec0[1] = pl->st.q_rec0[0]; pl->st.q_cell0[1] = pl->st.q_cell0[0]; pl->st.q_nrec[1] = pl->st.q_nrec[0]; pl->st.q_ncell[1] = pl->st.q_ncell[0];
            for (int k2 = 0; k2 < MK_KINDS; k2++) { pl->st.mk_rec_rel[1][k2] = pl->st.mk_rec_rel[0][k2]; pl->st.mk_cell_rel[1][k2] = pl->st.mk_cell_rel[0][k2]; pl->st.mk_nrec[1][k2] = pl->st.mk_nrec[0][k2]; pl->st.mk_ncell[1][k2] = pl->st.mk_ncell[0][k2]; }
        }
        if (pl->st.first_zero_kind == -2) { set_error("h2w_plan_compile: internal: first load_zero outside query 0"); delete pl; return nullptr; }
        // the two-phase strands' static tables: permutation list slots, emission work items of a query
        pl->st.total_glp = (uint32_t)sink.nglp;
        if (s.hash_mode == 1) pl->st.q_nglp = 0;
        if ((uint64_t)pl->st.pro_nglp + (uint64_t)s.num_queries * pl->st.q_nglp != sink.nglp) { set_error("h2w_plan_compile: internal: permutation list layout"); delete pl; return nullptr; }
        uint32_t it = 0;
        for (int k2 = 0, slot = 0; k2 < MK_KINDS; k2++) {      // (kinds a shape does not have own no items)
            pl->st.mk_item0[k2] = it;
            if (slot < pl->d.n_oracles + pl->d.n_steps && merkle_kind(s.n_perm_z, slot) == k2) { it += pl->st.mk_nunit[k2] ? pl->st.mk_nunit[k2] : 1; slot++; }
        }
        pl->st.mk_item0[MK_KINDS] = it;
        pl->small_mds = glp_small_mds(*consts);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        // no GPU: the plan is still usable for layout queries (cells, records, proof words); batch calls fail.
        pl->device = -1; pl->h_meta.swap(meta); return pl;      // (h2w_plan_record_ranges: with a device it reads d_meta back)
    }
    if (device_id < 0 || device_id >= ndev) { set_error("h2w_plan_compile: device_id out of range"); delete pl; return nullptr; }
    DeviceGuard dg(device_id);
    auto up = [&]() -> int {
        if (pl->n_cap_items) items.insert(items.end(), cap_items.begin(), cap_items.end());
        rf::RowConst rk; rf::rowconst_init(rk, pl->P);                              // the row-cooperative values pass' constants (rowfr.h)
        FriTab ft; fri_tab_build(ft, pl->shape.degree_bits + pl->shape.rate_bits);      // the FRI gadgets' shape constants (valbackend.h FriTab): per-call host work in the reference, a table here
        if (pl->dt.upload(pl->tt) != 0 || pl->d_meta.upload(meta) != 0 || (!items.empty() && pl->d_items.upload(items) != 0) ||
            upload_bn_tab(pl->d_bn_tab, *consts, pl->P, &pl->d_bn_tab9) != 0 || pl->d_rowk.upload(&rk, 1) != 0 || pl->d_fri.upload(&ft, 1) != 0 ||
            pl->d_st.upload(&pl->st, 1) != 0 || upload_glp_consts(pl->d_consts, *consts) != 0 || upload_tmpl_cells(pl->d_ncells, pl->tt) != 0 ||
            pl->d_inv.upload(inv) != 0) return -1;
        for (auto &ring : pl->evr) for (DevEvent &e : ring) if (e.create() != 0) return -1;
        return 0;
    };
    if (up() != 0) { h2w_plan_free(pl); return nullptr; }
    return pl;
}
// The device tables are DevBufs of the handle (and of its TracedPlan): the events and side streams are owners too; deleting the handle with its device current releases them all.
void h2w_plan_free(h2w_plan *p) {
    if (!p) return;
    DeviceGuard dg(p->device);
    traced_free(p);
    delete p;
}
uint64_t h2w_plan_num_cells(const h2w_plan *p) { return p ? p->ncells : 0; }
uint64_t h2w_plan_proof_words(const h2w_plan *p) { return p ? p->pl.total : 0; }
uint64_t h2w_plan_num_records(const h2w_plan *p) { return p ? p->nrec : 0; }
uint64_t h2w_plan_num_record_cells(const h2w_plan *p) { return p ? p->rec_cells : 0; }
int h2w_plan_direct_cells(const h2w_plan *p, uint8_t *bitmap) {
    if (!p || !bitmap) { set_error("h2w_plan_direct_cells: null argument"); return -1; }
    if (p->traced && !p->trace_forms) { set_error("h2w_plan_direct_cells: not for traced plans lowered without H2W_TRACE_OUTPUT_FORMS"); return -1; }
    for (uint64_t i = 0; i < (p->ncells + 7) / 8; i++) bitmap[i] = (uint8_t)(p->direct_bits[i / 8] >> (8 * (i & 7)));
    return 0;
}
int h2w_plan_record_ranges(const h2w_plan *p, uint64_t *ranges) {
    if (!p || !ranges) { set_error("h2w_plan_record_ranges: null argument"); return -1; }
    if (p->traced && !p->trace_forms) { set_error("h2w_plan_record_ranges: not for traced plans lowered without H2W_TRACE_OUTPUT_FORMS"); return -1; }
    std::vector<uint64_t> back; const uint64_t *m = p->h_meta.data();
    if (p->device >= 0) {
        DeviceGuard dg(p->device); back.resize((size_t)p->nrec);
        H2W_HIP(hipMemcpy(back.data(), p->d_meta.get(), back.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        m = back.data();
    }
    for (uint64_t i = 0; i < p->nrec; i++) { ranges[2 * i] = meta_off(m[i]); ranges[2 * i + 1] = (uint64_t)p->tt.ncells((int)meta_tmpl(m[i])); }
    return 0;
}
int h2w_plan_strand_layout(const h2w_plan *p, uint64_t out[4]) {
    if (!p || !out) { set_error("h2w_plan_strand_layout: null argument"); return -1; }
    out[0] = p->st.pro_ncell; out[1] = p->st.q_ncell[0]; out[2] = p->shape.num_queries > 1 ? p->st.q_ncell[1] : p->st.q_ncell[0]; out[3] = p->ncells;
    return 0;
}
uint64_t h2w_plan_num_chain_cells(const h2w_plan *p) {      // cells of the Merkle strands: what k_merkle_bn_fused writes per proof (hash_mode 1)
    if (!p) return 0;
    uint64_t n = 0;
    for (int k = 0; k < MK_KINDS; k++) n += p->st.mk_ncell[0][k] + (uint64_t)(p->shape.num_queries - 1) * p->st.mk_ncell[1][k];
    return n;
}
// ---- keygen-side metadata of the cell stream: static per shape, computed by a second host replay
int h2w_plan_metadata(h2w_plan *pl) {
    if (!pl) { set_error("h2w_plan_metadata: null plan"); return -1; }
    if (pl->meta_ready) return 0;      // (a traced plan: the tracing context's lists, h2w_plan_from_trace)
    if (pl->traced) { set_error("h2w_plan_metadata: the plan was traced on a context with witness_gen_only != 0, which records no keygen lists (trace with witness_gen_only = 0)"); return -1; }
    if (pl->shape.lookup_bits >= 48) { set_error("h2w_plan_metadata: lookup_bits >= 48 makes a single-limb range check look up its SOURCE cell; not tracked"); return -1; }
    const std::vector<fr_t> inv = inverse_table(pl->P);
    std::vector<uint64_t> zero_proof(pl->pl.total, 0), unit_cell; std::vector<LoadItem> items; StrandTable st; memset(&st, 0, sizeof(st));
    pl->sel_bits.assign((size_t)(pl->ncells + 7) / 8, 0); pl->lk_bits.assign((size_t)(pl->ncells + 7) / 8, 0);
    PlanSink sink; sink.meta = nullptr; sink.tt = &pl->tt; sink.st = &st; sink.unit_cell = &unit_cell; sink.items = &items;
    sink.sel_bits = &pl->sel_bits; sink.lk_bits = &pl->lk_bits;
    ValBackend<PlanSink> be(sink, host_replay_cfg(pl->shape, pl->P, inv, zero_proof.data()), false);
    Verifier<ValBackend<PlanSink>> V(be, pl->shape, &pl->h_consts);
    ChallengeBlock<ValBackend<PlanSink>> *cb = new ChallengeBlock<ValBackend<PlanSink>>();
    V.run_all(*cb);
    delete cb;
    if (sink.cell_off != pl->ncells) { set_error("h2w_plan_metadata: internal: replay length mismatch"); return -1; }
    pl->sel_bits.resize((size_t)(pl->ncells + 7) / 8); pl->lk_bits.resize((size_t)(pl->ncells + 7) / 8);
    pl->n_gates = pl->n_lookups = 0;
    for (uint8_t b : pl->sel_bits) pl->n_gates += (uint64_t)__builtin_popcount(b);
    for (uint8_t b : pl->lk_bits) pl->n_lookups += (uint64_t)__builtin_popcount(b);
    pl->meta_ready = true;
    return 0;
}
uint64_t h2w_plan_num_gates(h2w_plan *p) { return p && h2w_plan_metadata(p) == 0 ? p->n_gates : 0; }
uint64_t h2w_plan_num_lookups(h2w_plan *p) { return p && h2w_plan_metadata(p) == 0 ? p->n_lookups : 0; }
int h2w_plan_selectors(h2w_plan *p, uint8_t *bitmap) {
    if (!p || !bitmap) { set_error("h2w_plan_selectors: null argument"); return -1; }
    if (h2w_plan_metadata(p) != 0) return -1;
    memcpy(bitmap, p->sel_bits.data(), p->sel_bits.size()); return 0;
}
int h2w_plan_lookup_cells(h2w_plan *p, uint64_t *cells) {
    if (!p || !cells) { set_error("h2w_plan_lookup_cells: null argument"); return -1; }
    if (h2w_plan_metadata(p) != 0) return -1;
    uint64_t k2 = 0;
    for (uint64_t i = 0; i < p->ncells; i++) if (p->lk_bits[i / 8] >> (i & 7) & 1) cells[k2++] = i;     // registration order = stream order (RangeChip::range_check)
    return 0;
}
// FlexGate break points (halo2-base assign_with_constraints, ROTATIONS = 4 [R]): walk the stream down a column of
// max_rows = 2^k - unusable_rows; break when a gate would not fit or the column is full; the breaking cell is assigned twice
// (last row of the old column, row 0 of the new one).
int h2w_break_points(const uint8_t *selectors, uint64_t n_cells, int k, int unusable_rows, uint64_t *out, uint64_t cap, uint64_t *n_out) {
    if (!selectors || !n_out || k < 3 || k > 40 || unusable_rows < 0 || ((uint64_t)1 << k) <= (uint64_t)unusable_rows + 4) { set_error("h2w_break_points: bad argument"); return -1; }
    const uint64_t max_rows = ((uint64_t)1 << k) - (uint64_t)unusable_rows; uint64_t row = 0, n = 0;
    for (uint64_t i = 0; i < n_cells; i++) {
        const bool q = selectors[i / 8] >> (i & 7) & 1;
        if ((q && row + 4 > max_rows) || row >= max_rows - 1) { if (out && n < cap) out[n] = row; n++; row = 0; }
        row++;
    }
    *n_out = n;
    if (out && n > cap) { set_error("h2w_break_points: output too small"); return -1; }
    return 0;
}

}  // extern "C"
