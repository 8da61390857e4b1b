// replay.hip — record and replay (include/h2w.h 2d): h2w_plan_from_trace lowers the tape an eager context recorded in trace mode (trace.h: one
// entry per level-1 / level-2 call of ONE run of the reference's gadget through the operator API, field/native.rs:28-193 and
// field/goldilocks/base.rs:61-399) to a device program; h2w_fri_witness_batch on such a plan replays it on a batch of other proofs.
//
//   segments   the instances of the scopes the caller names as parallel (fri/mod.rs:488-501 "verify_query_round", merkle/mod.rs:57-78
//              "verify_proof_to_cap_with_cap_index") + the root; the claim is VERIFIED on the tape: an op may read values of its own segment and of
//              the segments enclosing it (produced before it started), nothing else - which also says that nothing outside reads what a parallel
//              segment computes.  Isomorphic instances (word-for-word equal lowered tapes) share one TEMPLATE.
//   device     one lane per (proof, instance), one kernel launch per template, depth by depth (a segment needs its ancestors' values).  The lanes of a
//              wavefront run the same template in lockstep: the tape is read with scalar loads, branches are uniform.  An op computes its value
//              with the arithmetic of the value backend (valbackend.h: the same templates the batched kernels use) and appends its cells - block
//              records for the Goldilocks-level templates (expanded by expand_fast afterwards), direct cells for the rest.  Values live in a
//              per-template store [slot][lane] (coalesced across the lanes), static constants in the tape.
//   the ring   A load waits for every store issued before it (one in-order counter on this family), and every op stores a record: with the values in
//              global memory alone an op cost 2-7 us.  The last RING_K value slots of a lane live in LDS as well (a different counter): the lowering
//              knows the distance from every operand to its producer (99.8 % of the prologue's operands, 93 % of the glue's, all of a PoseidonBN254
//              path's are within 256 slots) and addresses those through the ring; the global store stays (write-through: far operands, imports).
// This file is the device side and what launches it, and nothing else: the interpreter k_replay, the two emission kernels of the fused permutations,
// the witness call (traced_run) and the verdict call (h2w_trace_verdict_batch).  Every function here is a kernel or enqueues one: the unit's LDS
// variables are laid out together and the interpreter's code is held to the instruction, so what need not be compiled with it is not.  The plan
// itself - h2w_plan_from_trace, TracedPlan, the workspace layout, the lane tables, the information entry points - is traceplan.h / traceplan.cpp; the
// tape format (ops, operand words, the checker every tape passes before it is uploaded) is tapefmt.h; the lowering (segments, templates, fused
// stretches, shard units: host code) is tracelower.h / tracelower.cpp.
#define H2W_FLATTEN_CHIPS 1      // the interpreter's ops are the value backend's, inlined: out of line every op is a function call, and a call waits for the stores in flight (glue.hip)
#include <hip/hip_runtime.h>
#include <vector>
#include <string>
#include <cstring>
#include <algorithm>
#include "traceplan.h"
#include "glpval.h"
#include "bnpval.h"
#include "bnemit.h"

namespace h2w {
static_assert(GLPERM_IO == (uint32_t)SPONGE_WIDTH && BNPERM_IO == (uint32_t)BN_WIDTH, "tapefmt.h states the permutations' widths on its own");

struct ReplayArgs {
    const uint32_t *tape; const InstD *insts; const ImpD *imps; const uint32_t *inputs; const uint64_t *pool64; const fr_t *poolfr;
    const uint64_t *proofs; uint64_t proof_words; rec_t *recs; uint64_t rec_stride; fr_t *out; uint64_t cell_stride; ColMap cm; uint64_t *vals; uint32_t *status;
    const uint16_t *ncells; const fr_t *inv_pos, *inv_neg; FrParams P; int L; uint32_t nproofs;
    uint32_t depth, ntmpl, npool64, npoolfr;
    const TmplD *tm; const uint64_t *prefix;      // per template (device tables of the plan): its description; the u64 elements per proof of the value stores before it
    uint32_t blk0[MAX_TMPL + 1];                  // first block of each template among the blocks of this launch (templates of `depth` only)
    uint32_t *lflag;                              // per proof: 4 when a proof word is outside its field (h2w_plan_status)
    // (proof, query) sharding (ShardSpec): lanes != null lists the lanes of this rank, template t's at [lane0[t], lane0[t + 1]) (lanetable.h)
    const uint32_t *lanes; uint32_t lane0[MAX_TMPL + 1];
    uint32_t sh_world, sh_rank, sh_compact, nq; uint64_t pro_ncell, q_slot;      // the packed layout (shardmap.h)
    // fused permutations (DOP_GLPERM): the Goldilocks block of the tables the lowering verified them on; the list [nproofs][nglp][GLP_LIST_WORDS]
    const uint64_t *glk; uint64_t *glist; uint32_t nglp;
};
// the arguments of k_replay<BN>: plans without fused PoseidonBN254 permutations pass exactly ReplayArgs
template <bool BN> struct ReplayArgsSel { typedef ReplayArgs type; };
// fused PoseidonBN254 permutations (DOP_BNPERM): the times-R half of the plan's table (bntab.h); the list [nproofs][nbnp][BNP_LIST_WORDS]; bnp0: per
// instance (InstD order) its first entry in the proof's list
struct ReplayArgsBN : ReplayArgs { const fr_t *bnk; uint64_t *blist; const uint32_t *bnp0; uint32_t nbnp; };
template <> struct ReplayArgsSel<true> { typedef ReplayArgsBN type; };
template <bool BN> using ReplayArgsT = typename ReplayArgsSel<BN>::type;

// ------------------------------------------------------------------------------------------------------------------- device
// (its own sink type: the flattened value backend of this unit is instantiated nowhere else - field.h HNI)
struct ReplaySink : SinkBase {
    rec_t *recs; uint64_t nrec; fr_t *out; uint64_t cell_off; const uint32_t *ncells;      // ncells: an LDS table (a global load per record would wait for the record stores in flight)
    ColCursor cc;      // the FlexGate column layout of a direct cell (flat stream: the identity, never located)
    uint32_t emit;     // 0: a root lane of a proof another rank emits (sharded) - values only; uniform over the wavefront (the lane table groups them)
    HF void rec(int t, uint64_t a, uint64_t b, uint64_t c, uint64_t d) { if (emit) g_store_rec(recs + nrec, a, b, c, d); nrec++; cell_off += ncells[t]; }
    HF void cell(const fr_t &v) { if (emit) g_store_fr(out + cc.map(cell_off), v); cell_off++; }
    HF void skip(uint64_t nr, uint64_t nc) { nrec += nr; cell_off += nc; }
};
typedef ValBackend<ReplaySink> RB;
__shared__ uint64_t s_lds[LDS_WORDS];      // [ring | pool64 | poolfr]
__shared__ uint32_t s_nc[T_MAX];
// what the rare operand kinds need (uniform over the block), in LDS: the out-of-line path below must not take the address of the kernel arguments
struct SlowCtx { uint64_t *gvals; const TmplD *tm; const uint64_t *prefix; const ImpD *imps; const uint32_t *inputs; const uint64_t *pool64; const fr_t *poolfr; uint32_t nproofs; };
__shared__ SlowCtx s_cx;
__device__ __forceinline__ uint32_t tw(const uint32_t *tape, uint32_t i) { return *(const __attribute__((address_space(4))) uint32_t *)(tape + i); }
// an operand word that is not in LDS: a far slot of the own store, a value of an enclosing segment, a proof word, a far pool entry (DOP_FETCH only)
__device__ __noinline__ uint64_t slow_get64(uint32_t r, uint32_t j, const uint64_t *vals_g, uint64_t Lt, uint32_t p, uint32_t imp0, uint32_t in0, const uint64_t *proof) {
    const uint32_t i = ref_idx(r); const int k = ref_kind(r);
    if (k == RK_LOCAL || k == RK_RING) return H2W_GLOAD64(vals_g + (uint64_t)(i + j) * Lt);
    if (k == RK_INPUT) return g_load_u64(proof + s_cx.inputs[in0 + i] + j);
    if (k == RK_LIT64) return g_load_u64(s_cx.pool64 + i + j);
    if (k == RK_LITFR) return g_load_u64(reinterpret_cast<const uint64_t *>(s_cx.poolfr + i) + j);
    const ImpD d = s_cx.imps[imp0 + i]; const uint32_t ni = s_cx.tm[d.tmpl].ninst;
    return H2W_GLOAD64(s_cx.gvals + (uint64_t)s_cx.nproofs * s_cx.prefix[d.tmpl] + (uint64_t)(d.slot + j) * ((uint64_t)s_cx.nproofs * ni) + (uint64_t)p * ni + d.inst);
}

// BN: the instantiation with the DOP_BNPERM case (plans built with H2W_TRACE_FUSE_BN_PERMUTE); every other plan launches k_replay<false>, whose code is
// what it was without that op.  The body is replay_lane.h, the text of both kernels: k_replay_parts is the interpreter with the parts of split selects
// (H2W_TRACE_SPLIT_SELECTS), launched by the plans whose lowering made one (TracedPlan::select_parts); every other plan launches k_replay, whose code
// is what it was without them.  (One function template inlined into both kernels was tried first: the same source came out of the compiler as other
// code - a register and some twenty instructions - for the kernels existing plans launch.)
template <bool BN> __global__ __launch_bounds__(64) __attribute__((flatten)) void k_replay(ReplayArgsT<BN> R) {
#define H2W_REPLAY_PARTS 0
#include "replay_lane.h"
#undef H2W_REPLAY_PARTS
}
template <bool BN> __global__ __launch_bounds__(64) __attribute__((flatten)) void k_replay_parts(ReplayArgsT<BN> R) {
#define H2W_REPLAY_PARTS 1
#include "replay_lane.h"
#undef H2W_REPLAY_PARTS
}

// One wavefront per listed permutation of the launch: its GLP_RECS records from the entry {first record, input state}, as k_glp_emit (batch.hip)
// writes a compiled plan's - the traced plan's list is flat, [proof][entry].  Sharded: the entries of this rank's blocks only.
struct GlpEmitArgs { const h2w_poseidon_consts_t *consts; const uint64_t *list; rec_t *recs; uint64_t rec_stride; const uint16_t *ncells; const uint32_t *unit; uint32_t nglp, world, rank, nq; };
__global__ __launch_bounds__(64) void k_glp_emit_traced(GlpEmitArgs A) {
    typedef CoopSinkT<false, false> Sink;
    const uint32_t p = blockIdx.x / A.nglp, e = blockIdx.x % A.nglp;
    if (A.world > 1) {
        const uint32_t u = A.unit[e];
        if ((u == NO_SLOT ? (uint64_t)p : (uint64_t)p * A.nq + u) % A.world != A.rank) return;
    }
    stage_glp_consts(A.consts, threadIdx.x, 64);
    Sink sink; sink.recs = A.recs + (uint64_t)p * A.rec_stride; sink.out = nullptr; sink.ncells = A.ncells; sink.lane = threadIdx.x; sink.bind_lds(); sink.cell_off = 0; sink.emit = true;
    const uint64_t *ent = A.list + ((uint64_t)p * A.nglp + e) * GLP_LIST_WORDS;
    const uint64_t w = threadIdx.x < GLP_LIST_WORDS ? g_load_u64(ent + threadIdx.x) : 0;
    uint64_t st[SPONGE_WIDTH];
#pragma unroll
    for (int i = 0; i < SPONGE_WIDTH; i++) st[i] = readlane64(w, i + 1);
    sink.nrec = readlane64(w, 0);
    sink.coop_poseidon_permute(st, A.consts);
}

// k_bn_emit_traced: one QUAD per listed PoseidonBN254 permutation of the launch (bnemit.h: how it works, its arguments).  Its Montgomery twin lives in
// bnemit_mont.hip - a unit of its own, so that this unit's LDS layout and with it the code of k_replay and of this kernel stay what they are.
template <bool COLS> __global__ __launch_bounds__(QUAD_BLOCK) H2W_QUAD_ATTR void k_bn_emit_traced(BnEmitArgs A) {
    typedef QuadSinkT<COLS, QUAD_FUSED> Sink;
    stage_bn_consts(A.bn_tab, threadIdx.x, QUAD_BLOCK);      // (block-wide barrier inside: before any wavefront leaves)
    if ((((uint64_t)blockIdx.x * QUAD_BLOCK + (threadIdx.x & ~63u)) >> 2) >= A.nitems) return;      // a whole wavefront past the last item
    uint64_t g = ((uint64_t)blockIdx.x * QUAD_BLOCK + threadIdx.x) >> 2;
    if (g >= A.nitems) g = A.nitems - 1;
    const uint64_t it = A.items ? (uint64_t)A.items[g] : g;      // proof * nbnp + entry
    const uint64_t p = it / A.nbnp; const uint32_t e = (uint32_t)(it % A.nbnp);
    const BnpD D = A.bnp[e];
    const uint64_t *ent = A.list + it * BNP_LIST_WORDS;
    fr_t *outb = A.out + p * A.cell_stride;
    if (A.sh_compact)           // the packed buffer: the permutation's block at its local start
        outb = A.out + packed_block_start(A.sh_world, A.sh_rank, A.nq, A.pro_ncell, A.q_slot, p, D.unit == NO_SLOT ? -1 : (int64_t)D.unit) - D.ucell0;
    if (g_load_u64(ent) != D.cell0 && (threadIdx.x & 3) == 0) atomicCAS(&A.status[p], 0u, 97u);
    fr_t st[BN_WIDTH];
#pragma unroll
    for (int i = 0; i < BN_WIDTH; i++) st[i] = g_load_fr(reinterpret_cast<const fr_t *>(ent + 2) + i);
    Sink sink; sink.recs = nullptr; sink.nrec = 0; sink.out = outb; sink.cell_off = D.cell0; sink.ncells = nullptr; sink.l4 = threadIdx.x & 3; sink.cc.init(A.cm);
    sink.ustate = nullptr; sink.sbx = nullptr;
    ValCfg cfg; cfg.proof = nullptr; cfg.mode = 1; cfg.L = 0; cfg.P = A.P; cfg.inv_pos = cfg.inv_neg = nullptr; cfg.st = nullptr; cfg.split = false; cfg.split_bn = true;
    cfg.load_items = nullptr; cfg.n_load_items = 0; cfg.load_nrec = cfg.load_ncell = 0; cfg.n_cap_items = 0; cfg.fri = nullptr;
    bool zc = true;             // (a stretch with the Context's load_zero cell in it is never fused)
    sink.template bn_emit_cells<false>(st, cfg, zc);
}

// ------------------------------------------------------------------------------------------------------------------- launches
// the plan's part of k_replay's arguments; what belongs to the call - recs, out, the lane table, the sharding - is zero and the caller's to set
static ReplayArgs replay_args(const h2w_plan *p, const uint64_t *proofs_dev, uint64_t n_proofs, char *ws, const TracedWs &wl) {
    const TracedPlan *t = p->traced;
    ReplayArgs R; memset(&R, 0, sizeof(R));
    R.tape = t->d_tape.get(); R.insts = t->d_insts.get(); R.imps = t->d_imps.get(); R.inputs = t->d_inputs.get(); R.pool64 = t->d_pool64.get(); R.poolfr = t->d_poolfr.get();
    R.proofs = proofs_dev; R.proof_words = p->pl.total; R.recs = (rec_t *)(ws + wl.recs); R.rec_stride = p->nrec;
    R.vals = (uint64_t *)(ws + wl.vals); R.status = (uint32_t *)(ws + wl.status); R.ncells = p->d_ncells.get(); R.inv_pos = p->d_inv.get(); R.inv_neg = p->d_inv.get() + INV_TAB; R.P = p->P; R.L = p->shape.lookup_bits;
    R.nproofs = (uint32_t)n_proofs; R.lflag = (uint32_t *)(ws + wl.lflag);
    R.glk = reinterpret_cast<const uint64_t *>(p->d_consts.get()); R.glist = (uint64_t *)(ws + wl.glist); R.nglp = t->nglp;
    R.ntmpl = (uint32_t)t->tmpls.size(); R.tm = t->d_tm.get(); R.prefix = t->d_prefix.get(); R.npool64 = t->npool64; R.npoolfr = t->npoolfr;
    return R;
}
static void use_lanes(ReplayArgs &R, const LaneTable &T) { R.lanes = T.d_lanes.get(); for (size_t i = 0; i < T.lane0.size(); i++) R.lane0[i] = T.lane0[i]; }
// The k_replay launches of a call, depth by depth (a segment reads its ancestors' values; the templates of one depth share a launch).  lanes: the
// table R.lanes is of (a sharded call's, the verdict call's quiet one), else null: every (proof, instance) in place.
static void replay_launches(h2w_plan *p, ReplayArgs &R, const LaneTable *lanes, uint64_t n_proofs, uint64_t *blist, hipStream_t stream) {
    TracedPlan *t = p->traced;
    uint32_t maxd = 0; for (const TmplD &T : t->tmpls) if (T.depth > maxd) maxd = T.depth;
    for (uint32_t d = 0; d <= maxd; d++) {
        uint32_t nb = 0;
        for (size_t i = 0; i < t->tmpls.size(); i++) {
            R.blk0[i] = nb;
            if (t->tmpls[i].depth == d) nb += (uint32_t)(((lanes ? lanes->lane0[i + 1] - lanes->lane0[i] : n_proofs * t->tmpls[i].ninst) + 63) / 64);
        }
        R.blk0[t->tmpls.size()] = nb; R.depth = d;
        if (t->timing && t->tev_used < 12) (void)hipEventRecord(t->tev[t->tev_used++], stream);
        if (nb && t->nbnp) {
            ReplayArgsT<true> RB; static_cast<ReplayArgs &>(RB) = R; RB.bnk = p->d_bn_tab.get() + BK_T; RB.blist = blist; RB.bnp0 = t->d_bnp0.get(); RB.nbnp = t->nbnp;
            if (t->select_parts) hipLaunchKernelGGL(k_replay_parts<true>, dim3(nb), dim3(64), 0, stream, RB);
            else hipLaunchKernelGGL(k_replay<true>, dim3(nb), dim3(64), 0, stream, RB);
        } else if (nb && t->select_parts) hipLaunchKernelGGL(k_replay_parts<false>, dim3(nb), dim3(64), 0, stream, R);
        else if (nb) hipLaunchKernelGGL(k_replay<false>, dim3(nb), dim3(64), 0, stream, R);
    }
}
int traced_run(h2w_plan *p, const uint64_t *proofs_dev, uint64_t n_proofs, void *advice_dev, void *workspace_dev, void *stream_, ColMap cm, uint64_t cell_stride, const ShardSpec &sh) {
    TracedPlan *t = p->traced;
    if (n_proofs > 65535) { set_error("h2w_fri_witness_batch: more than 65535 proofs per call"); return -1; }
    const bool sharded = sh.world > 1;
    if ((sharded || sh.compact) && !t->why_unshardable.empty()) { set_error("h2w_fri_witness_batch_shard: " + t->why_unshardable); return -1; }
    if (sh.compact && !sharded) { set_error("h2w_fri_witness_batch_shard_compact: world 1 on a traced plan: use h2w_fri_witness_batch (the packed form of one rank is the flat stream)"); return -1; }
    DeviceGuard dg(p->device);
    if (sharded && traced_sharded_lanes(p, n_proofs, sh) != 0) return -1;
    // the grids of the two emission kernels: a wavefront per listed Goldilocks-Poseidon permutation, a quad per PoseidonBN254 one of this rank's blocks
    const uint64_t bn_items = !t->nbnp ? 0 : sharded ? t->lanes.n_bn_items : n_proofs * t->nbnp, bn_blocks = (bn_items * 4 + QUAD_BLOCK - 1) / QUAD_BLOCK;
    if (n_proofs * t->nglp >= 0x7fffffffull || bn_blocks >= 0x7fffffffull) { set_error("h2w_fri_witness_batch: too many fused permutations in one call"); return -1; }
    hipStream_t stream = (hipStream_t)stream_;
    const TracedWs wl = traced_ws(p, n_proofs); char *ws = (char *)workspace_dev;
    ReplayArgs R = replay_args(p, proofs_dev, n_proofs, ws, wl);
    R.out = (fr_t *)advice_dev; R.cell_stride = cell_stride; R.cm = cm;      // (cm.starts: the FlexGate columns of every proof, cell_stride = ncols << k; else the flat stream)
    if (sharded) {
        use_lanes(R, t->lanes);
        R.sh_world = (uint32_t)sh.world; R.sh_rank = (uint32_t)sh.rank; R.sh_compact = (uint32_t)sh.compact; R.nq = (uint32_t)p->shape.num_queries;
        R.pro_ncell = p->st.pro_ncell; R.q_slot = std::max(p->st.q_ncell[0], p->st.q_ncell[1]);
    }
    H2W_HIP(hipMemsetAsync(ws + wl.status, 0, n_proofs * 4, stream));
    H2W_HIP(hipMemsetAsync(ws + wl.lflag, 0, n_proofs * 4, stream));
    uint64_t *const blist = (uint64_t *)(ws + wl.blist);
    // Montgomery form: the fused PoseidonBN254 permutations' cells leave their emission kernel converted; the ranged kernel takes the other direct cells
    const bool mont = p->output_form == H2W_FORM_MONTGOMERY, emit_mont = mont && t->nbnp && !p->trace_bn_ranged;
    t->tev_used = 0;
    replay_launches(p, R, sharded ? &t->lanes : nullptr, n_proofs, blist, stream);
    if (t->timing) H2W_HIP(hipEventRecord(t->tev[t->tev_used++], stream));
    if (t->nglp) {      // the records of the listed permutations, side by side
        GlpEmitArgs E; E.consts = p->d_consts.get(); E.list = R.glist; E.recs = R.recs; E.rec_stride = R.rec_stride; E.ncells = p->d_ncells.get(); E.unit = t->d_glp_unit.get();
        E.nglp = t->nglp; E.world = sharded ? (uint32_t)sh.world : 1u; E.rank = (uint32_t)sh.rank; E.nq = (uint32_t)p->shape.num_queries;
        hipLaunchKernelGGL(k_glp_emit_traced, dim3((uint32_t)(n_proofs * t->nglp)), dim3(64), 0, stream, E);
    }
    if (t->timing && t->bn_flag) H2W_HIP(hipEventRecord(t->tev[t->tev_used++], stream));
    if (t->nbnp) {      // the cells of the listed PoseidonBN254 permutations, a quad each (direct cells: nothing of the expansion depends on them, nor they on it)
        BnEmitMontArgs EM; memset(&EM, 0, sizeof(EM)); BnEmitArgs &E = EM;
        EM.bn_tab_mont = p->d_bn_tab_mont.get(); EM.mont_k = mont_k();
        E.bn_tab = p->d_bn_tab.get(); E.list = blist; E.bnp = t->d_bnp.get(); E.nbnp = t->nbnp; E.out = R.out; E.cell_stride = cell_stride; E.cm = cm; E.P = p->P; E.status = R.status;
        E.items = sharded ? t->lanes.d_bn_items.get() : nullptr; E.nitems = bn_items;
        if (sharded) { E.sh_world = R.sh_world; E.sh_rank = R.sh_rank; E.sh_compact = R.sh_compact; E.nq = R.nq; E.pro_ncell = R.pro_ncell; E.q_slot = R.q_slot; }
        if (bn_blocks && emit_mont) launch_bn_emit_traced_mont(EM, cm.starts != nullptr, (uint32_t)bn_blocks, stream);
        else if (bn_blocks) launch_cols(cm.starts != nullptr, k_bn_emit_traced<true>, k_bn_emit_traced<false>, dim3((uint32_t)bn_blocks), dim3(QUAD_BLOCK), 0, stream, E);
    }
    if (t->timing) H2W_HIP(hipEventRecord(t->tev[t->tev_used++], stream));
    // Montgomery form (plans lowered with H2W_TRACE_OUTPUT_FORMS): the direct cells - the interpreter's; the emission kernel's above too where it wrote
    // canonical cells - in place, behind their writers on the call's stream; the expansion kernel converts its own cells as it writes them.  The column fix-up (h2w_fri_witness_batch_columns)
    // follows the call, as on a compiled plan: it repeats converted boundary cells.
    if (mont && launch_plan_direct(p, emit_mont ? p->d_ranged_bits.get() : p->d_direct_bits.get(), n_proofs, R.out, cell_stride, cm, sh, stream) != 0) return -1;
    if (t->timing && p->trace_forms) H2W_HIP(hipEventRecord(t->tev[t->tev_used++], stream));
    // expansion of the block records
    if (launch_plan_expand(p, n_proofs, R.recs, (uint32_t *)(ws + wl.ctr), R.out, cell_stride, cm, sharded ? &sh : nullptr, 2, stream) != 0) return -1;
    if (t->timing) H2W_HIP(hipEventRecord(t->tev[t->tev_used++], stream));
    H2W_HIP(hipGetLastError());
    return 0;
}
static int trace_verdict_run(h2w_plan *p, const uint64_t *proofs_dev, uint64_t n_proofs, h2w_verdict_t *verdict_dev, void *workspace_dev, void *stream_) {
    TracedPlan *t = p->traced; const VerdictTables &V = t->vt;
    for (size_t i = 0; i < t->tmpls.size(); i++)
        if ((uint64_t)n_proofs * t->tmpls[i].ninst * (V.ent0[i + 1] - V.ent0[i]) >= 0x80000000ull) { set_error("h2w_trace_verdict_batch: 2^31 or more (proof, instance, check) lanes in one call; split the batch"); return -1; }
    DeviceGuard dg(p->device);
    if (traced_quiet_lanes(p, n_proofs) != 0) return -1;
    hipStream_t stream = (hipStream_t)stream_;
    const TracedWs wl = traced_ws(p, n_proofs); char *ws = (char *)workspace_dev;
    // 1. the values: k_replay as traced_run launches it, every lane quiet (no advice buffer: R.out stays null, nothing is stored through it)
    ReplayArgs R = replay_args(p, proofs_dev, n_proofs, ws, wl);
    R.cm = flat_cols(); R.cell_stride = p->ncells;
    use_lanes(R, t->qlanes);
    R.sh_world = 1; R.sh_rank = 0; R.sh_compact = 0; R.nq = (uint32_t)p->shape.num_queries;
    H2W_HIP(hipMemsetAsync(ws + wl.status, 0, n_proofs * 4, stream));
    H2W_HIP(hipMemsetAsync(ws + wl.lflag, 0, n_proofs * 4, stream));
    TraceVerdictArgs A; memset(&A, 0, sizeof(A));
    A.ents = t->d_vents.get(); A.vinst = t->d_vinst.get(); A.vimps = t->d_vimps.get(); A.sites = t->d_vsites.get(); A.tinfo = t->d_tinfo.get(); A.inputs = t->d_inputs.get(); A.pool64 = t->d_pool64.get(); A.poolfr = t->d_poolfr.get();
    A.vals = R.vals; A.proofs = proofs_dev; A.proof_words = p->pl.total; A.verdict = verdict_dev; A.status = R.status; A.lflag = R.lflag; A.nproofs = (uint32_t)n_proofs; A.L = p->shape.lookup_bits;
    launch_trace_verdict_init(A, stream);
    const bool timing = t->timing; t->timing = false;      // (h2w_plan_trace_timing reports witness calls: this call records no events and leaves the last call's alone)
    replay_launches(p, R, &t->qlanes, n_proofs, (uint64_t *)(ws + wl.blist), stream);
    t->timing = timing;
    // 2. the checks, template by template, behind the deepest depth
    for (size_t i = 0; i < t->tmpls.size(); i++) {
        A.tmpl = (uint32_t)i; A.inst0 = t->tmpls[i].inst0; A.ninst = t->tmpls[i].ninst; A.ent0 = V.ent0[i]; A.nent = V.ent0[i + 1] - V.ent0[i];
        launch_trace_verdict(A, stream);
    }
    launch_trace_verdict_finish(A, stream);
    H2W_HIP(hipGetLastError());
    return 0;
}
}  // namespace h2w

extern "C" int h2w_trace_verdict_batch(h2w_plan *p, const uint64_t *proofs_dev, uint64_t n_proofs, h2w_verdict_t *verdict_dev, void *workspace_dev, void *stream) {
    if (!p) { set_error("h2w_trace_verdict_batch: null plan"); return -1; }
    if (!p->traced) { set_error("h2w_trace_verdict_batch: a plan of h2w_plan_compile: use h2w_fri_verdict_batch"); return -1; }
    if (!p->traced->why_no_verdict.empty()) { set_error("h2w_trace_verdict_batch: " + p->traced->why_no_verdict); return -1; }
    if (p->device < 0) { set_error("h2w_trace_verdict_batch: no HIP device — the replay only runs on the GPU (no CPU fallback)"); return -1; }
    if (n_proofs == 0) return 0;
    if (!proofs_dev || !verdict_dev || !workspace_dev) { set_error("h2w_trace_verdict_batch: null buffer"); return -1; }
    if (n_proofs > 65535) { set_error("h2w_trace_verdict_batch: more than 65535 proofs per call"); return -1; }
    return trace_verdict_run(p, proofs_dev, n_proofs, verdict_dev, workspace_dev, stream);
}
