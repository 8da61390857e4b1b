// plan.h — the plan handle of API level 3 (include/h2w.h): a compiled shape (plancompile.cpp h2w_plan_compile) or a traced run (traceplan.cpp h2w_plan_from_trace).
// Every device table, event and side stream of the handle is an owner of devbuf.h: h2w_plan_free sets the device and deletes the handle.
#pragma once
#include "common.h"
#include "batchargs.h"
#include "montform.h"
#include "handletabs.h"

namespace h2w {
struct TracedPlan;
struct ShardSpec { int rank = 0, world = 1, compact = 0; };
}
using namespace h2w;      // (included by the plan's units only - plancompile.cpp, batch.hip, advicetools.hip, traceplan.cpp, replay.hip -, which live in that namespace's vocabulary)
struct h2w_plan {
    h2w_shape_t shape; int device;
    TemplateTable tt; DeviceTables dt; StrandTable st; FrParams P;
    Derived d; ProofLayout pl;
    uint64_t nrec = 0, ncells = 0, rec_cells = 0;
    DevBuf<LoadItem> d_items; uint32_t n_items = 0, n_cap_items = 0; uint64_t load_nrec = 0, load_ncell = 0;      // d_items: the load phase's items, then the cap hashes'
    h2w_poseidon_consts_t h_consts;                       // host copy (keygen-metadata replay)
    bool meta_ready = false; std::vector<uint8_t> sel_bits, lk_bits; uint64_t n_gates = 0, n_lookups = 0; DevBuf<uint32_t> d_lookup_cells; DevBuf<uint8_t> d_sel_bits;
    DevBuf<uint64_t> d_col_tab; std::vector<uint64_t> h_col_tab; int col_k = -1;     // column-major emission: [starts | lens] of the last break-point set
    PlanEqualities eqs;
    DevBuf<fr_t> d_bn_tab; DevBuf<uint32_t> d_bn_tab9; DevBuf<FriTab> d_fri; uint64_t nunit = 0; DevBuf<rf::RowConst> d_rowk;     // PoseidonBN254 tables of this plan (handletabs.h upload_bn_tab)
    DevBuf<StrandTable> d_st;                         // device copy of st
    bool small_mds = false;                           // Goldilocks-Poseidon MDS entries are tiny (glcoop.h glp_small_mds)
    DevBuf<uint64_t> d_meta; DevBuf<GlpConsts> d_consts; DevBuf<uint16_t> d_ncells; DevBuf<fr_t> d_inv;
    static constexpr int EV_RING = 64, N_SIDE = 16;
    // event slots of a call: slot i < H2W_EV_COUNT is the public H2W_EV_* i (include/h2w.h: call start / end, prologue block complete, glue (+ Goldilocks
    // Merkle strands) start / end, chain kernels start / end, expansion start / end), then the internal ones
    enum { EV_PROLOGUE_VALUES_END = H2W_EV_COUNT, EV_CHAIN_VALUES_END, EV_GLP_START, EV_GLP_END, EV_DIRECT_END, N_EV };
    DevEvent evr[EV_RING][N_EV]; int passes_of[EV_RING] = {0};      // (created by h2w_plan_compile; a traced plan has none)
    DevStream side[N_SIDE]; hipStream_t side_of[N_SIDE]; int n_side = 0;   // PoseidonBN254 chain kernels run beside the glue + expansion kernels
    DevEvent vev[N_SIDE][2];         // h2w_fri_verdict_batch_ex, H2W_VERDICT_FORK: fork / join of the call on side stream k (created with the first such call)
    int chain_passes = 0;            // H2W_OPT_CHAIN_PASSES (0: by the size of the launch)
    int values_form = 0;             // H2W_OPT_VALUES_FORM (0: by the size of the launch)
    int serial_expand = 1;           // H2W_OPT_SERIAL_EXPAND: the expansion kernel of a call waits for the previous call's
    // H2W_OPT_OUTPUT_FORM.  The shape compiler marks the cells of a proof's stream that value kernels write themselves (one bit per cell, padded to whole
    // 64-word rows for k_direct_to_montgomery); the Montgomery form's constants and the bitmap go to the device when the form is first selected.
    // A traced plan has the bitmap (made at lowering, tracelower.h direct_cell_map) and the option only when lowered with H2W_TRACE_OUTPUT_FORMS.
    int output_form = 0; std::vector<uint64_t> direct_bits, h_meta; uint64_t n_direct = 0; DevBuf<uint64_t> d_direct_bits; DevBuf<MontForm> d_mont;
    bool trace_forms = false;        // traced with H2W_TRACE_OUTPUT_FORMS
    // ... with fused PoseidonBN254 permutations: their cells leave k_bn_emit_traced in Montgomery form (d_bn_tab_mont: the plan's table with its canonical
    // half converted, uploaded with the form's constants), and the ranged kernel works from ranged_bits, the direct map without those cells.
    // trace_bn_ranged (H2W_TRACE_BN_RANGED set in the environment when the plan was lowered; measurement, tools/replay_timing.py): canonical emission and
    // the ranged kernel over the full map instead.
    std::vector<uint64_t> ranged_bits; DevBuf<uint64_t> d_ranged_bits; DevBuf<fr_t> d_bn_tab_mont; bool trace_bn_ranged = false;
    bool fork_chains = true;         // of their own batch (they share only the prologue): one side stream per caller stream seen (created on demand)
    uint64_t n_batches = 0; bool ev_recorded = false;
    h2w::TracedPlan *traced = nullptr;      // set: the plan replays a recorded tape (traceplan.h); the strand tables above are unused
    explicit h2w_plan(int L) : tt(L) {}
};
extern "C" int h2w_plan_metadata(h2w_plan *pl);      // plancompile.cpp: the keygen-metadata replay, once per plan (the selector / lookup queries and advicetools.hip call it)
namespace h2w {
// The plan's side stream for the caller's stream `s` (batch.hip WitnessCall: the chain kernels; verdict.hip: the glue kernel of a H2W_VERDICT_FORK call - a
// witness call and such a verdict call on one caller stream share it, in order): slot k of side[] / side_of[], created when `s` is first seen.  -1: every side
// stream is another caller stream's (the call does not fork); -2: the stream could not be created (the reason is in the last error).
inline int plan_side_slot(h2w_plan *p, hipStream_t s) {
    int k = 0; while (k < p->n_side && p->side_of[k] != s) k++;
    if (k < p->n_side) return k;
    if (p->n_side == h2w_plan::N_SIDE) return -1;
    int lo_pri = 0, hi_pri = 0; (void)hipDeviceGetStreamPriorityRange(&lo_pri, &hi_pri);      // the chain is the longest dependent piece of a launch: let its blocks be placed first
    if (p->side[k].create(hipStreamNonBlocking, hi_pri) != 0) return -2;
    p->side_of[k] = s; p->n_side++;
    return k;
}
// plan_side_slot's codes resolved for a call on `s` that asks for a fork or not: *side is the plan's side stream for `s`, or `s` itself where the call does not
// fork (then *slot, where asked for, is -1).  -1: error.
inline int plan_side_stream(h2w_plan *p, hipStream_t s, bool fork, hipStream_t *side, int *slot = nullptr) {
    const int k = fork ? plan_side_slot(p, s) : -1;
    if (k == -2) return -1;
    *side = k >= 0 ? (hipStream_t)p->side[k] : s;
    if (slot) *slot = k;
    return 0;
}
// The owner of a call's fork onto that stream: `caller` the caller's stream, `side` the side stream (the same: the call does not fork), `open` while work
// enqueued on `side` is not yet ordered in front of `caller`.  The events are the call's own and it records them itself, where its timing marks belong
// (h2w_plan_timing*, h2w_plan_event_gap); the owner only waits.
// A call that leaves with the fork open - an enqueue failed behind fork_at - has kernels on the side stream that may still read and write its buffers, and
// nothing orders the caller's stream behind them any more: the destructor waits for them.  So the owner lives inside whatever releases the call's workspace,
// and the caller sees the error, and may release its buffers, only after the wait.
struct SideFork {
    const hipStream_t caller, side; bool open = false;
    SideFork(hipStream_t caller_, hipStream_t side_) : caller(caller_), side(side_) {}
    SideFork(const SideFork &) = delete; SideFork &operator=(const SideFork &) = delete;
    ~SideFork() { if (open) (void)hipStreamSynchronize(side); }
    // `side` waits for `e`, which the call has recorded on `caller`; nothing to do for a call that does not fork
    int fork_at(hipEvent_t e) { if (side == caller) return 0; H2W_HIP(hipStreamWaitEvent(side, e, 0)); open = true; return 0; }
    // `caller` waits for `e`, which the call has recorded on `side`; nothing to do where no fork is open
    int join_at(hipEvent_t e) { if (!open) return 0; H2W_HIP(hipStreamWaitEvent(caller, e, 0)); open = false; return 0; }
};
// The plan's part of a call's kernel arguments (batch.hip run_batch, verdict.hip verdict_call): the shape, its device tables, the proofs.  What belongs to
// the call - workspace pointers, the output buffer and its stride, cm, sh - is value-initialised here and the caller's to set.
inline BatchArgs plan_batch_args(const h2w_plan *p, const uint64_t *proofs_dev, uint64_t n_proofs) {
    BatchArgs A{};
    A.shape = p->shape; A.consts = p->d_consts.get(); A.proofs = proofs_dev; A.proof_words = p->pl.total;
    A.rowk = p->d_rowk.get(); A.glp_small_mds = p->small_mds ? 1 : 0;
    A.bn_tab = p->d_bn_tab.get(); A.bn_tab9 = p->d_bn_tab9.get(); A.fri = p->d_fri.get();
    A.load_items = p->d_items.get(); A.n_load_items = p->n_items; A.n_cap_items = p->n_cap_items; A.load_nrec = p->load_nrec; A.load_ncell = p->load_ncell;
    A.ncells = p->d_ncells.get(); A.inv_pos = p->d_inv.get(); A.inv_neg = p->d_inv.get() + INV_TAB; A.st = p->d_st.get(); A.P = p->P; A.nproofs = (int)n_proofs;
    return A;
}
// The expansion launch of a plan's call (batch.hip: run_batch, h2w_fri_expand_records; replay.hip traced_run): records[n_proofs][p->nrec] -> cells
// out[n_proofs][cell_stride] through cm.  sh: the (proof, query) sharding of the record ranges; null: every proof is one block (a traced plan has
// no strand table).  tile_ctr: n_proofs words of workspace, zeroed here.  roam_per_cu: ExpandArgs.
int launch_plan_expand(const h2w_plan *p, uint64_t n_proofs, const rec_t *recs, uint32_t *tile_ctr, fr_t *out, uint64_t cell_stride, ColMap cm,
                       const ShardSpec *sh, uint32_t roam_per_cu, hipStream_t stream);
// H2W_FORM_MONTGOMERY, the direct cells of a plan's call (batch.hip k_direct_to_montgomery; run_batch, replay.hip traced_run): the cells of the bitmap
// `bits` (device; the plan's d_direct_bits or d_ranged_bits) in out[n_proofs][cell_stride] get the full product in place, through cm and, sharded, in this rank's blocks only (packed: at their local
// addresses).  Behind every kernel that writes a direct cell; in front of the column fix-up, which copies converted boundary cells.
int launch_plan_direct(const h2w_plan *p, const uint64_t *bits, uint64_t n_proofs, fr_t *out, uint64_t cell_stride, ColMap cm, const ShardSpec &sh, hipStream_t stream);
}

