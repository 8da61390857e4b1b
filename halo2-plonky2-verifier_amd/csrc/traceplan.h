// traceplan.h — a traced plan (include/h2w.h 2d) between its units: what h2w_plan_from_trace leaves behind (TracedPlan), the layout of a call's
// workspace, and every function one unit calls in another.  traceplan.cpp is the host side - the lowering stage by stage, the handle, the uploads, the
// lane tables, the information entry points; it launches nothing.  replay.hip is the kernels and what launches them.  batch.hip and plancompile.cpp
// dispatch to both.
#pragma once
#include "plan.h"
#include "tracelower.h"
#include "lanetable.h"
#include "traceverdict.h"

namespace h2w {

// A lane table on the device (lanetable.h: its words) and the call it was built for.  A failed install leaves no table: the next call builds it again.
struct LaneTable {
    std::vector<uint32_t> lane0; DevBuf<uint32_t> d_lanes;
    DevBuf<uint32_t> d_bn_items; uint64_t n_bn_items = 0;      // a sharded call's, on plans with fused PoseidonBN254 permutations (fill_sharded_bn_items)
    uint64_t n = 0; int rank = -1, world = 0;
    bool built_for(uint64_t n_, int rank_, int world_) const { return d_lanes.get() && n == n_ && rank == rank_ && world == world_; }
};

struct TracedPlan {
    std::vector<TmplD> tmpls; uint64_t total_slot_lanes = 0;      // sum over templates of nslots * ninst: u64 elements of the value store per proof
    DevBuf<TmplD> d_tm; DevBuf<uint64_t> d_prefix; uint32_t npool64 = 0, npoolfr = 0;
    DevBuf<uint32_t> d_tape; DevBuf<InstD> d_insts; DevBuf<ImpD> d_imps; DevBuf<uint32_t> d_inputs; DevBuf<uint64_t> d_pool64; DevBuf<fr_t> d_poolfr;
    uint64_t n_ops = 0, n_segments = 0;
    std::vector<uint64_t> op_counts;      // tape_op_counts over the templates' tapes (h2w_plan_trace_op_counts)
    // fused Goldilocks-Poseidon permutations: per proof nglp list entries (entry e belongs to shard unit h_glp_unit[e], NO_SLOT: the root's block)
    uint32_t nglp = 0; uint64_t n_candidates = 0; std::vector<uint32_t> h_glp_unit; DevBuf<uint32_t> d_glp_unit;
    // fused PoseidonBN254 permutations: per proof nbnp list entries
    bool bn_flag = false; uint32_t nbnp = 0; uint64_t n_bn_left = 0; std::vector<BnpD> h_bnp; DevBuf<BnpD> d_bnp; std::vector<uint32_t> h_bnp0; DevBuf<uint32_t> d_bnp0;
    bool select_parts = false;      // the tapes hold parts of split selects (H2W_TRACE_SPLIT_SELECTS): the plan launches the interpreter's instantiation that carries their sum
    DevEvent tev[17]; int tev_used = 0; bool timing = false;      // h2w_plan_trace_timing: around every kernel of the last call (12 depths at most, three kernels, the expansion)
    // sharding: the depth-1 instances are the units (query q = the q-th in tape order); why_unshardable empty: they tile the stream behind the root's block
    std::string why_unshardable; std::vector<uint32_t> h_unit;      // h_unit: the unit of every instance (InstD order)
    // the verdict (h2w_trace_verdict_batch): the lowered tables (tracelower.h verdict_tables; why_no_verdict non-empty: unavailable) and their device copies
    VerdictTables vt; std::string why_no_verdict; DevBuf<VEntD> d_vents; DevBuf<VInstD> d_vinst; DevBuf<VImpD> d_vimps; DevBuf<uint64_t> d_tinfo; DevBuf<uint32_t> d_vsites;
    // the table of the last sharded call (n, rank, world) and the quiet one of the last verdict call (n): two, so that neither passes for the other nor evicts it
    LaneTable lanes, qlanes;
};

// a call's workspace: per proof the records, the status and range-flag words, the expansion's counter, the value store, the two lists of fused permutations
struct TracedWs { size_t recs, status, lflag, ctr, vals, glist, blist, total; };
inline TracedWs traced_ws(const h2w_plan *p, uint64_t n) {
    TracedWs w; size_t o = 0;
    w.recs = o; o += align_up((size_t)n * p->nrec * sizeof(rec_t), 256);
    w.status = o; o += align_up((size_t)n * 4, 256); w.lflag = o; o += align_up((size_t)n * 4, 256); w.ctr = o; o += align_up((size_t)n * 4, 256);
    w.vals = o; o += align_up((size_t)n * p->traced->total_slot_lanes * 8, 256);
    w.glist = o; o += align_up((size_t)n * p->traced->nglp * GLP_LIST_WORDS * 8, 256);      // the fused permutations' list (none: the layout of an unfused plan)
    w.blist = o; o += align_up((size_t)n * p->traced->nbnp * BNP_LIST_WORDS * 8, 256);      // the fused PoseidonBN254 permutations' list (none: nothing)
    w.total = o; return w;
}

// ---- traceplan.cpp
uint64_t traced_workspace_bytes(const h2w_plan *p, uint64_t n);
uint64_t traced_status_offset(const h2w_plan *p, uint64_t n, bool flags);      // of the status words; flags: of the range-flag words
const char *traced_shard_refusal(const h2w_plan *p);      // null: the traced plan shards by its depth-1 parallel instances
void traced_free(h2w_plan *p);
// p->traced->lanes for this call / ->qlanes for n proofs, built and installed unless it is the last call's.  -1: the refusal or the failed upload is the last error
int traced_sharded_lanes(h2w_plan *p, uint64_t n, const ShardSpec &sh);
int traced_quiet_lanes(h2w_plan *p, uint64_t n);
// H2W_FORM_MONTGOMERY, first use (h2w_plan_configure), on a traced plan with fused PoseidonBN254 permutations: the emitter's cell table in Montgomery
// form and the ranged kernel's map.  Any other plan: nothing, 0.
int traced_mont_tables(const h2w_plan *p, DevBuf<fr_t> &bn_tab_mont, DevBuf<uint64_t> &ranged_bits);
// ---- replay.hip
int traced_run(h2w_plan *p, const uint64_t *proofs_dev, uint64_t n_proofs, void *advice_dev, void *workspace_dev, void *stream_, ColMap cm, uint64_t cell_stride, const ShardSpec &sh);

}  // namespace h2w
