// verdict.hip - per-proof verdicts without a witness (include/h2w.h 3b): h2w_fri_verdict_batch, h2w_fri_verdict_batch_ex, h2w_plan_verdict_form, h2w_plan_proof_layout.
//
// The verifier gadget's protocol checks are assert_equal copy constraints (chips.h MerkleTreeChip, verifier.h query_round): they emit no cells, so a
// stream made from a rejected proof looks like one made from an accepted proof.  Every value those checks compare is computed by the value kernels
// of a witness call anyway; this unit runs the same single-source chips on sinks that keep NOTHING but the comparisons (valbackend.h SinkBase
// compare / site): the only global stores of its kernels are the challenge blocks and the verdict words.
//   launch_prologue_values  k_prologue_values as it is (glue.hip), with a shard map under which no proof's block is owned: what a non-owner rank of a
//                           sharded run does - values only -> challenge blocks, the prologue's status word
//   k_verdict_init          one lane per proof: the verdict's start value, the PoW bit (fri/mod.rs:130-145) from the challenge block
//   k_verdict_check         one lane per (proof, load item): status 4, by k_prologue_load's (batch.hip) predicate: batchargs.h load_item_out_of_field
//   k_verdict_glue          one lane per (proof, query): Verifier::query_round on a sink without cells - the fold steps' consistency checks and the
//                           final polynomial's evaluation
//   k_verdict_merkle_gl     Goldilocks caps: one wavefront per (proof, query, tree), permutations on glp_permute_lanes (k_merkle_gl_values without list or records)
//   k_verdict_merkle_bn     PoseidonBN254 caps: four lanes per (proof, query, tree) on the lazy nine-limb values walk (bnquad.h QuadSinkT bn_values, QUAD_VERDICT:
//                           no unit states, no S-box values; the cap lookup's value is taken)
//   k_verdict_merkle_row    PoseidonBN254 caps, few paths (h2w_fri_verdict_batch_ex, H2W_VERDICT_FORM_ROW): one wavefront per (proof, query, tree), the four rows
//                           of the wavefront = the four state elements (rowfr.h; rowperm.h bn_permute_rows<false>: the permutation of k_merkle_bn_values_row
//                           without its S-box stores).  A path's 18 dependent permutations take half the time of the four-lane form's
//   k_verdict_finish        one lane per proof: status 4 where no strand reported a condition of its own (h2w_plan_status's order)
// h2w_fri_verdict_batch_ex picks the PoseidonBN254 form by the number of paths (VERDICT_ROW_MAX_PATHS) and may run k_verdict_glue on the plan's side
// stream beside the Merkle kernel (H2W_VERDICT_FORK): the two read the challenge blocks and meet in the verdict words' atomics alone.
// Flattened like glue.hip: the sinks below exist in this unit alone (field.h HNI).
#define H2W_FLATTEN_CHIPS 1
#include <hip/hip_runtime.h>
#include <string>
#include "plan.h"
#define RF_TAB9 s_bn_tab9
#include "rowperm.h"

namespace h2w {

static_assert(sizeof(h2w_verdict_t) == 16, "four words per proof");

// what a sink of this unit does with a comparison: count it, flag its site, note its query - on the one lane of the strand that speaks for it
struct VerdictAcc {
    h2w_verdict_t *v; uint32_t q; int n_perm_z, cur; bool on;
    __device__ __forceinline__ void init(h2w_verdict_t *verdict, int p, int query, int npz, bool speaks) { v = verdict + p; q = (uint32_t)query; n_perm_z = npz; cur = SITE_NONE; on = speaks; }
    __device__ __forceinline__ uint32_t flag() const {
        if (cur >= SITE_FINAL) return H2W_VERDICT_FINAL;
        if (cur >= SITE_FOLD) return H2W_VERDICT_FOLD;
        if (cur < SITE_MERKLE) return 0;
        const int kind = cur - SITE_MERKLE;      // verifier.h merkle_kind: without permutation Zs oracle 1 is the quotient tree
        return kind >= 3 ? H2W_VERDICT_MERKLE_STEP : kind == 0 ? H2W_VERDICT_MERKLE_TRACE : (kind == 1 && n_perm_z > 0) ? H2W_VERDICT_MERKLE_PERM_Z : H2W_VERDICT_MERKLE_QUOTIENT;
    }
    __device__ __forceinline__ void compare(bool differ) {
        if (!differ || !on) return;
        atomicAdd(&v->n_failed, 1u); atomicOr(&v->flags, flag()); atomicMin(&v->first_query, q);
    }
    __device__ __forceinline__ void status(uint32_t s) { if (s && on) atomicCAS(&v->status, 0u, s); }
};

// a sink of this unit: Base's walk on values with no record, no cell and no cursor - the comparisons alone, to the accumulator
template <class Base> struct VerdictSinkT : Base {
    VerdictAcc acc;
    __device__ __forceinline__ void rec(int, uint64_t, uint64_t, uint64_t, uint64_t) {}
    __device__ __forceinline__ void cell(const fr_t &) {}
    __device__ __forceinline__ void skip(uint64_t, uint64_t) {}
    __device__ __forceinline__ void compare(bool differ) { acc.compare(differ); }
    __device__ __forceinline__ void site(int s) { acc.cur = s; }
};
struct VerdictGlueBase : SinkBase { static constexpr bool kSplitOnly = true; };
// one wavefront per path, every lane on the same values (glue.hip RowSink without anything it leaves for an emission pass): no unit states, no S-box
// values - the permutation stores nothing -, and the cap lookup's value is taken; lane 0 speaks
struct VerdictRowBase : SinkBase {
    static constexpr bool kBnUnits = true; static constexpr int kHashMode = 1;
    const rf::RowConst *rowk;
    __device__ __forceinline__ bool level_skip(fr_t &, bool &) { return false; }
    __device__ __forceinline__ bool tail_skip() const { return false; }
    __device__ __forceinline__ void permute_unit(fr_t *st) {
        const rf::RowConst K = load_row_consts(rowk);
        const rf::LaneK L = rf::lane_consts();
        rf::bn_permute_rows<false>(st, K, L, nullptr);
    }
    __device__ __forceinline__ bool bn_emit_inline(fr_t *st, const ValCfg &, bool &) { permute_unit(st); return true; }
};
typedef VerdictSinkT<VerdictGlueBase> VerdictGlueSink;
typedef VerdictSinkT<CoopSinkT<false, true, 0>> VerdictCoopSink;      // (emit = false: no list entry; rec / cell hidden: no cursor either)
typedef VerdictSinkT<QuadSinkT<false, QUAD_VERDICT>> VerdictQuadSink;
typedef VerdictSinkT<VerdictRowBase> VerdictRowSink;

struct VerdictArgs { BatchArgs A; h2w_verdict_t *verdict; uint32_t *lflag; };

__global__ __launch_bounds__(256) void k_verdict_init(VerdictArgs V) {
    const unsigned p = blockIdx.x * 256 + threadIdx.x;
    if (p >= (unsigned)V.A.nproofs) return;
    const int pb = V.A.shape.pow_bits;
    const uint64_t resp = V.A.cbs[p].fri_pow_response;
    h2w_verdict_t v;
    v.flags = (pb > 0 && (resp >> (64 - pb)) != 0) ? (uint32_t)H2W_VERDICT_POW : 0u;      // (pow_bits 0: a 64-bit range check of a 64-bit word)
    // RangeChip::range_check decomposes the response into ceil((64 - pow_bits) / lookup_bits) limbs and constrains their sum to equal it: a response
    // that does not fit the limbs breaks that copy constraint too - the one failing equality of a proof that no query owns
    const int L = V.A.shape.lookup_bits, nl = (64 - pb + L - 1) / L;
    v.n_failed = (nl > 1 && nl * L < 64 && (resp >> (nl * L)) != 0) ? 1u : 0u;
    v.first_query = 0xFFFFFFFFu; v.status = V.A.status[p];
    V.verdict[p] = v;
}

__global__ __launch_bounds__(256) void k_verdict_check(VerdictArgs V) {
    const uint32_t items = V.A.n_load_items;      // (kinds 0-3; the cap hashes' limb decompositions behind them check nothing)
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x, p = g / items; const uint32_t i = (uint32_t)(g % items);
    if (p >= (uint64_t)V.A.nproofs) return;
    const uint64_t wk = g_load_u64(reinterpret_cast<const uint64_t *>(V.A.load_items + i));
    const uint32_t word = (uint32_t)wk, kind = (uint32_t)(wk >> 32);
    const uint64_t *w = V.A.proofs + p * V.A.proof_words + word; const uint64_t w0 = g_load_u64(w);
    fr_t v; v.l[0] = w0;
    if (kind >= 2) { v.l[1] = g_load_u64(w + 1); v.l[2] = g_load_u64(w + 2); v.l[3] = g_load_u64(w + 3); }
    const bool bad = load_item_out_of_field(kind, v);
    if (bad) atomicOr(&V.lflag[p], 4u);
}

__global__ __launch_bounds__(256) void k_verdict_finish(VerdictArgs V) {
    const unsigned p = blockIdx.x * 256 + threadIdx.x;
    if (p >= (unsigned)V.A.nproofs) return;
    if (V.verdict[p].status == 0) V.verdict[p].status = V.lflag[p];      // (the strands' conditions come first: h2w_plan_status)
}

__global__ __launch_bounds__(64) __attribute__((flatten)) void k_verdict_glue(VerdictArgs V) {
    typedef ValBackend<VerdictGlueSink> GlueB;
    int p, q;
    if (!own_unit_at(V.A, blockIdx.x * blockDim.x + threadIdx.x, p, q)) return;
    VerdictGlueSink sink; sink.acc.init(V.verdict, p, q, V.A.shape.n_perm_z, true);
    const ChallengeBlock<GlueB> &cb = *reinterpret_cast<const ChallengeBlock<GlueB> *>(&V.A.cbs[p]);
    ValCfg cfg = make_cfg(V.A, p); cfg.split = false;      // (kSplitOnly: the Merkle calls are the kernels' below; nothing to step over)
    GlueB be(sink, cfg, true);
    const h2w_shape_t shp = V.A.shape;      // (a reference into the kernel arguments would put all of them on every lane's stack)
    Verifier<GlueB> Vf(be, shp, V.A.consts);
    Vf.query_round(q, cb);
    sink.acc.status(be.status);
}

__global__ __launch_bounds__(64) __attribute__((flatten)) void k_verdict_merkle_gl(VerdictArgs V) {
    typedef ValBackend<VerdictCoopSink> CoopB;
    __builtin_amdgcn_s_setprio(3);
    stage_glp_consts<true>(V.A.consts, threadIdx.x, 64);
    int p, q;
    if (!own_unit_at(V.A, blockIdx.x, p, q)) return;
    const int kind = merkle_kind(V.A.shape.n_perm_z, blockIdx.y);
    VerdictCoopSink sink; coop_sink_init(sink, V.A, p, q); sink.emit = false; sink.nrec = 0; sink.cell_off = 0; sink.glp_slot = 0;
    sink.acc.init(V.verdict, p, q, V.A.shape.n_perm_z, threadIdx.x == 0);      // wave-uniform values: lane 0 speaks
    CoopB be(sink, make_cfg(V.A, p), true);
    const h2w_shape_t shp = V.A.shape;
    Verifier<CoopB> Vf(be, shp, V.A.consts);
    Vf.merkle_strand_at(q, kind, V.A.cbs[p].fri_query_indices[q]);
    sink.acc.status(be.status);
}

// LDS: the nine-limb tables alone.  The quads of a wavefront run in lockstep: no wavefront leaves early, tail quads redo the last strand and keep silent
__global__ __launch_bounds__(QUAD_BLOCK) __attribute__((flatten)) void k_verdict_merkle_bn(VerdictArgs V) {
    typedef ValBackend<VerdictQuadSink> QuadB;
    stage_bn_consts9(V.A.bn_tab9, threadIdx.x, QUAD_BLOCK);    // (block-wide barrier inside: before any wavefront leaves)
    const unsigned total = V.A.sh.n_own_units;
    if (((blockIdx.x * QUAD_BLOCK + (threadIdx.x & ~63u)) >> 2) >= total) return;      // a wavefront past the last strand
    unsigned idx = (blockIdx.x * QUAD_BLOCK + threadIdx.x) >> 2;
    const bool tail = idx >= total;
    if (tail) idx = total - 1;
    int p, q; own_unit_at(V.A, idx, p, q);
    const int kind = merkle_kind(V.A.shape.n_perm_z, blockIdx.y);
    VerdictQuadSink sink; sink.recs = nullptr; sink.nrec = 0; sink.out = nullptr; sink.cell_off = 0; sink.ncells = nullptr; sink.l4 = threadIdx.x & 3; sink.ustate = nullptr; sink.sbx = nullptr;
    sink.acc.init(V.verdict, p, q, V.A.shape.n_perm_z, !tail && (threadIdx.x & 3) == 0);      // quad-uniform values: lane 0 of the quad speaks
    ValCfg mc = make_cfg(V.A, p); mc.split_bn = true;
    QuadB be(sink, mc, true);
    const h2w_shape_t shp = V.A.shape;
    Verifier<QuadB> Vf(be, shp, V.A.consts);
    Vf.merkle_strand_at(q, kind, V.A.cbs[p].fri_query_indices[q]);
    sink.acc.status(be.status);
}

// LDS: the nine-limb tables alone.  Global memory is written through the VerdictAcc atomics only
__global__ __launch_bounds__(QUAD_BLOCK) __attribute__((flatten)) void k_verdict_merkle_row(VerdictArgs V) {
    typedef ValBackend<VerdictRowSink> RowB;
    stage_bn_consts9(V.A.bn_tab9, threadIdx.x, QUAD_BLOCK);    // (block-wide barrier inside: before any wavefront leaves)
    const unsigned idx = blockIdx.x * QUAD_WAVES + (threadIdx.x >> 6);      // this wavefront's (proof, query) unit
    int p, q;
    if (!own_unit_at(V.A, idx, p, q)) return;      // a wavefront past the last unit
    const int kind = merkle_kind(V.A.shape.n_perm_z, blockIdx.y);
    VerdictRowSink sink; sink.rowk = V.A.rowk;
    sink.acc.init(V.verdict, p, q, V.A.shape.n_perm_z, (threadIdx.x & 63) == 0);      // wave-uniform values: lane 0 speaks
    ValCfg mc = make_cfg(V.A, p); mc.split_bn = true;
    RowB be(sink, mc, true);
    const h2w_shape_t shp = V.A.shape;
    Verifier<RowB> Vf(be, shp, V.A.consts);
    Vf.merkle_strand_at(q, kind, V.A.cbs[p].fri_query_indices[q]);
    sink.acc.status(be.status);
}

// H2W_VERDICT_FORM_AUTO: the wavefront-per-path form up to this many Merkle paths = n_proofs x num_queries x (n_oracles + n_steps) of a call with
// PoseidonBN254 caps.  A path is 18 dependent permutations in either form; the row form walks it in half the time with sixteen times the lanes, so it
// wins while the four-lane form leaves the chip idle.  The largest path count of the sweep at which it was not the slower one, a call alone on the
// chip (cfg 3, 196 paths per proof: 12 proofs 2.96 against 3.43 ms, 16 proofs 3.55 against 3.42; DESIGN 5g, profiles/verdict_forms_cfg3.json).  A caller
// that keeps other launches in flight pays for the row form's instructions earlier (batch.hip on H2W_OPT_VALUES_FORM): it names its form itself.
constexpr uint64_t VERDICT_ROW_MAX_PATHS = 2352;

static unsigned verdict_form_of(const h2w_plan *p, uint64_t n_proofs) {
    if (p->shape.hash_mode == 0) return H2W_VERDICT_FORM_QUAD;      // Goldilocks caps: the one kernel there is already one wavefront per path
    const uint64_t per_proof = (uint64_t)p->shape.num_queries * (uint64_t)(p->d.n_oracles + p->d.n_steps);
    return per_proof == 0 || n_proofs <= VERDICT_ROW_MAX_PATHS / per_proof ? H2W_VERDICT_FORM_ROW : H2W_VERDICT_FORM_QUAD;
}

// The launches of a verdict call on its arguments V (workspace pointers set).  gstream: the glue kernel's stream - the caller's, or the plan's side stream
// with `vev`, that side stream's two events (null: the call does not fork).  The SideFork lives in here, inside verdict_call's release of the workspace.
static int verdict_enqueue(const h2w_plan *p, VerdictArgs &V, uint64_t n_proofs, hipStream_t stream, hipStream_t gstream, const DevEvent *vev, unsigned form) {
    BatchArgs &A = V.A;
    SideFork fork(stream, gstream);
    H2W_HIP(hipMemsetAsync(V.lflag, 0, n_proofs * sizeof(uint32_t), stream));
    // the prologue on values: a world in which this rank owns no proof's block (own_prologue: p % world == rank never holds below 2^30 proofs)
    A.sh.world = 0x40000000; A.sh.rank = 0x3fffffff;
    launch_prologue_values(A, stream);
    // every (proof, query) unit is this call's
    A.sh.world = 1; A.sh.rank = 0; A.sh.n_own_units = (uint32_t)(n_proofs * (uint64_t)p->shape.num_queries); A.sh.n_own_proofs = (uint32_t)n_proofs;
    const unsigned pgrid = (unsigned)((n_proofs + 255) / 256), nunits = A.sh.n_own_units, nkinds = (unsigned)(p->d.n_oracles + p->d.n_steps);
    hipLaunchKernelGGL(k_verdict_init, dim3(pgrid), dim3(256), 0, stream, V);
    if (p->n_items) hipLaunchKernelGGL(k_verdict_check, dim3((unsigned)((n_proofs * p->n_items + 255) / 256)), dim3(256), 0, stream, V);
    // the glue kernel and the Merkle kernel read the challenge blocks and meet in the verdict words' atomics alone: with H2W_VERDICT_FORK the glue kernel runs on
    // the plan's side stream beside the Merkle kernel and the caller's stream waits for it before k_verdict_finish and before the workspace is released
    if (vev) {
        H2W_HIP(hipEventRecord(vev[0], stream));
        if (fork.fork_at(vev[0]) != 0) return -1;
    }
    hipLaunchKernelGGL(k_verdict_glue, dim3((nunits + 63) / 64), dim3(64), 0, gstream, V);
    if (vev) H2W_HIP(hipEventRecord(vev[1], gstream));
    if (p->shape.hash_mode == 0) hipLaunchKernelGGL(k_verdict_merkle_gl, dim3(nunits, nkinds), dim3(64), 0, stream, V);
    else if (form == H2W_VERDICT_FORM_ROW) hipLaunchKernelGGL(k_verdict_merkle_row, dim3((nunits + QUAD_WAVES - 1) / QUAD_WAVES, nkinds), dim3(QUAD_BLOCK), 0, stream, V);
    else hipLaunchKernelGGL(k_verdict_merkle_bn, dim3((nunits * 4 + QUAD_BLOCK - 1) / QUAD_BLOCK, nkinds), dim3(QUAD_BLOCK), 0, stream, V);
    if (vev && fork.join_at(vev[1]) != 0) return -1;
    hipLaunchKernelGGL(k_verdict_finish, dim3(pgrid), dim3(256), 0, stream, V);
    H2W_HIP(hipGetLastError());
    return 0;
}

// the checks both entry points share, in h2w_fri_verdict_batch's order, and the call itself.  form: H2W_VERDICT_FORM_QUAD or _ROW
static int verdict_call(const char *who, h2w_plan *p, const uint64_t *proofs_dev, uint64_t n_proofs, h2w_verdict_t *verdict_dev, void *stream_, unsigned form, bool fork) {
    const std::string w(who);
    if (p->device < 0) { set_error(w + ": no HIP device — the verdict kernels only run on the GPU (no CPU fallback)"); return -1; }
    if (n_proofs == 0) return 0;
    if (!proofs_dev || !verdict_dev) { set_error(w + ": null buffer"); return -1; }
    const uint64_t nq = (uint64_t)p->shape.num_queries;
    if (n_proofs > 0x3fffffffull / (4 * nq)) { set_error(w + ": batch too large; split the batch"); return -1; }
    DeviceGuard dg(p->device);
    hipStream_t stream = (hipStream_t)stream_, gstream;      // gstream: the glue kernel's
    int slot;      // (-1: no fork asked for, or every side stream is another caller stream's - this call does not fork)
    if (plan_side_stream(p, stream, fork, &gstream, &slot) != 0) return -1;
    if (slot >= 0) for (DevEvent &e : p->vev[slot]) if (!(hipEvent_t)e && e.create() != 0) return -1;
    // the call's workspace: challenge blocks, the prologue's status words, the range flags
    const size_t o_status = align_up((size_t)n_proofs * sizeof(DevCB), 256), o_lflag = o_status + align_up((size_t)n_proofs * sizeof(uint32_t), 256), total = o_lflag + align_up((size_t)n_proofs * sizeof(uint32_t), 256);
    char *ws = nullptr;
    H2W_HIP(hipMallocAsync((void **)&ws, total, stream));
    VerdictArgs V; BatchArgs &A = V.A;
    A = plan_batch_args(p, proofs_dev, n_proofs);      // (no records, no advice, no unit buffers, no permutation list: those stay null)
    A.cm = flat_cols(); A.cbs = (DevCB *)ws; A.status = (uint32_t *)(ws + o_status); A.load_flag = (uint32_t *)(ws + o_lflag);
    V.verdict = verdict_dev; V.lflag = A.load_flag;
    const int rc = verdict_enqueue(p, V, n_proofs, stream, gstream, slot >= 0 ? p->vev[slot] : nullptr, form);      // (failed behind its fork: it has waited for the side stream)
    (void)hipFreeAsync(ws, stream);
    return rc;
}

}  // namespace h2w

extern "C" {

int h2w_fri_verdict_batch(h2w_plan *p, const uint64_t *proofs_dev, uint64_t n_proofs, h2w_verdict_t *verdict_dev, void *stream_) {
    if (!p) { set_error("h2w_fri_verdict_batch: null plan"); return -1; }
    if (p->traced) { set_error("h2w_fri_verdict_batch: a traced plan (h2w_plan_from_trace) replays a tape and has no verifier strands to judge: use a plan of h2w_plan_compile"); return -1; }
    return verdict_call("h2w_fri_verdict_batch", p, proofs_dev, n_proofs, verdict_dev, stream_, H2W_VERDICT_FORM_QUAD, false);
}

int h2w_fri_verdict_batch_ex(h2w_plan *p, const uint64_t *proofs_dev, uint64_t n_proofs, h2w_verdict_t *verdict_dev, void *stream_, uint32_t flags) {
    if (!p) { set_error("h2w_fri_verdict_batch_ex: null plan"); return -1; }
    if (flags & ~(H2W_VERDICT_FORM_MASK | H2W_VERDICT_FORK)) { set_error("h2w_fri_verdict_batch_ex: unknown flag bits " + std::to_string(flags & ~(H2W_VERDICT_FORM_MASK | H2W_VERDICT_FORK)) + " (H2W_VERDICT_FORM_* | H2W_VERDICT_FORK)"); return -1; }
    unsigned form = flags & H2W_VERDICT_FORM_MASK;
    if (form > H2W_VERDICT_FORM_ROW) { set_error("h2w_fri_verdict_batch_ex: unknown form " + std::to_string(form) + " (H2W_VERDICT_FORM_AUTO, _QUAD, _ROW)"); return -1; }
    if (p->traced) { set_error("h2w_fri_verdict_batch_ex: a traced plan (h2w_plan_from_trace) replays a tape and has no verifier strands to judge: use a plan of h2w_plan_compile"); return -1; }
    if (form == H2W_VERDICT_FORM_ROW && p->shape.hash_mode == 0) { set_error("h2w_fri_verdict_batch_ex: H2W_VERDICT_FORM_ROW is a PoseidonBN254 form and the plan's hash_mode is 0 (Goldilocks caps have one kernel: H2W_VERDICT_FORM_QUAD or _AUTO)"); return -1; }
    if (form == H2W_VERDICT_FORM_AUTO) form = verdict_form_of(p, n_proofs);
    return verdict_call("h2w_fri_verdict_batch_ex", p, proofs_dev, n_proofs, verdict_dev, stream_, form, (flags & H2W_VERDICT_FORK) != 0);
}

int h2w_plan_verdict_form(const h2w_plan *p, uint64_t n_proofs) {
    if (!p) { set_error("h2w_plan_verdict_form: null plan"); return -1; }
    if (p->traced) { set_error("h2w_plan_verdict_form: a traced plan (h2w_plan_from_trace) has no verdict call"); return -1; }
    return (int)verdict_form_of(p, n_proofs);
}

int h2w_plan_proof_layout(const h2w_plan *p, uint64_t *out, size_t n_out) {
    if (!p) { set_error("h2w_plan_proof_layout: null plan"); return -1; }
    if (p->traced) { set_error("h2w_plan_proof_layout: not for traced plans (a tape names proof words, not a shape's layout)"); return -1; }
    const ProofLayout &L = p->pl; const Derived &d = p->d;
    const size_t need = 12 + 1 + 3 * (size_t)d.n_oracles + 1 + 3 * (size_t)d.n_steps;
    if (!out) return (int)need;
    if (n_out < need) { set_error("h2w_plan_proof_layout: " + std::to_string(need) + " words needed"); return -1; }
    size_t k = 0;
    const uint64_t head[12] = {L.trace_cap, L.quotient_cap, L.openings, L.perm_cap, L.pow_witness, L.final_poly, L.commit_caps, L.queries, L.query_words, L.pis, L.total, (uint64_t)d.cap_size};
    for (uint64_t w : head) out[k++] = w;
    out[k++] = (uint64_t)d.n_oracles;
    for (int o = 0; o < d.n_oracles; o++) { out[k++] = L.init_off[o]; out[k++] = (uint64_t)d.oracle_polys[o]; out[k++] = (uint64_t)L.init_sibs; }
    out[k++] = (uint64_t)d.n_steps;
    for (int i = 0; i < d.n_steps; i++) { out[k++] = L.step_off[i]; out[k++] = 2ull << d.arity[i]; out[k++] = (uint64_t)L.step_sibs[i]; }
    return (int)need;
}

}  // extern "C"
