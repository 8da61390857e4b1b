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
// Which op becomes which template is decided on STATIC widths (a value is provably below 2^64 when a Goldilocks-level op, a bit decomposition, a
// one-word input ... produced it), never on the traced values: the layout of the records must not depend on the proof.
#define H2W_FLATTEN_CHIPS 1      // the interpreter's ops are the value backend's, inlined: out of line every op is a function call, and a call waits for the stores in flight (glue.hip)
#include <hip/hip_runtime.h>
#include <unordered_map>
#include <map>
#include <vector>
#include <string>
#include <cstring>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include "plan.h"
#include "trace.h"
#include "keygen.h"
#include "glpval.h"
#include "bnpval.h"

struct h2w_ctx;
namespace h2w {
Trace *ctx_trace(h2w_ctx *); int ctx_lookup_bits(const h2w_ctx *); uint64_t ctx_num_cells(const h2w_ctx *); const MetaRecorder *ctx_meta(const h2w_ctx *);      // eager.cpp

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
// device ops; word 0 = op | n << 8 | aux << 16 | (words of the op) << 24, then operand refs, then (ops with results) the first output slot
enum { DOP_END = 0, DOP_SKIP, DOP_CONST1, DOP_FRCELL, DOP_LOADW, DOP_LOADW_DIV, DOP_LOADW_EXTINV, DOP_GLOP, DOP_GATE, DOP_REDUCE, DOP_CLT,
       DOP_FR_ADD, DOP_FR_MUL, DOP_FR_MULADD, DOP_SELECT, DOP_FR_SELECT, DOP_IDX2IND, DOP_SELIND, DOP_FR_SELIND, DOP_NUM2BITS, DOP_BITS2NUM,
       DOP_DECOMP565, DOP_LIMBS2NUM, DOP_RANGE, DOP_FETCH,
       DOP_GLOPRUN,        // n consecutive DOP_GLOP ops as one: [hdr][cells of the run][A, B, C, out slot | template << 24] x n (2 + 4 n words: its length is NOT in the header)
       DOP_GLPERM,         // a verified Goldilocks-Poseidon permutation as one op (H2W_TRACE_FUSE_GL_PERMUTE): [hdr][12 operands][first output slot][list slot][cells of its record block]
       DOP_BNPERM };       // a verified PoseidonBN254 permutation as one op (H2W_TRACE_FUSE_BN_PERMUTE): [hdr][4 operands][first output slot (4 x 4 slots)][list slot][its cells]
constexpr uint32_t GLPERM_WORDS = 16, BNPERM_WORDS = 8;
// a list entry of a fused PoseidonBN254 permutation: {first cell of its block in the proof's stream, zero-cell flag (1: the Context's load_zero cell is
// cached, the block is the 4,032 cells), the 4 x 32-byte input state}
constexpr uint32_t BNP_LIST_WORDS = 18;
// operand words of an op: [first, first + count)
HD void operand_span(uint32_t op, uint32_t n, uint32_t &first, uint32_t &count) {
    first = 1; count = 0;
    switch (op) {
        case DOP_CONST1: case DOP_FRCELL: case DOP_LOADW: case DOP_REDUCE: case DOP_CLT: case DOP_RANGE: case DOP_IDX2IND: case DOP_NUM2BITS: case DOP_DECOMP565: count = 1; break;
        case DOP_LOADW_DIV: case DOP_LOADW_EXTINV: case DOP_FR_ADD: case DOP_FR_MUL: count = 2; break;
        case DOP_GLOP: case DOP_GATE: case DOP_FR_MULADD: case DOP_SELECT: case DOP_FR_SELECT: count = 3; break;
        case DOP_SELIND: case DOP_FR_SELIND: count = 2 * n; break;
        case DOP_BITS2NUM: case DOP_LIMBS2NUM: count = n; break;
        case DOP_GLPERM: count = SPONGE_WIDTH; break;
        case DOP_BNPERM: count = BN_WIDTH; break;
        default: break;
    }
}
constexpr int MAX_TMPL = 48;
constexpr uint32_t NO_SLOT = 0xffffffffu;

// unit: the depth-1 parallel instance (shard unit) the instance is or lies in, NO_SLOT for the root; ucell0: that unit's first cell (root: 0)
// glp0: the instance's first entry in the proof's list of fused permutations
struct InstD { uint64_t cell0, rec0, ucell0; uint32_t imp0, in0, unit, glp0; };
struct ImpD { uint32_t tmpl, inst, slot; };
struct TmplD { uint32_t tape0, nslots, ninst, inst0, depth; };

struct ReplayArgs {
    const uint32_t *tape; const InstD *insts; const ImpD *imps; const uint32_t *inputs; const uint64_t *pool64; const fr_t *poolfr;
    const uint64_t *proofs; uint64_t proof_words; rec_t *recs; uint64_t rec_stride; fr_t *out; uint64_t cell_stride; ColMap cm; uint64_t *vals; uint32_t *status;
    const uint16_t *ncells; const fr_t *inv_pos, *inv_neg; FrParams P; int L; uint32_t nproofs;
    uint32_t depth, ntmpl, npool64, npoolfr;
    const TmplD *tm; const uint64_t *prefix;      // per template (device tables of the plan): its description; the u64 elements per proof of the value stores before it
    uint32_t blk0[MAX_TMPL + 1];                  // first block of each template among the blocks of this launch (templates of `depth` only)
    uint32_t *lflag;                              // per proof: 4 when a proof word is outside its field (h2w_plan_status)
    // (proof, query) sharding (ShardSpec): lanes != null lists the lanes of this rank, template t's at [lane0[t], lane0[t + 1]) (lane_table)
    const uint32_t *lanes; uint32_t lane0[MAX_TMPL + 1];
    uint32_t sh_world, sh_rank, sh_compact, nq; uint64_t pro_ncell, q_slot;      // the packed layout (batchargs.h block_out)
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
// a listed PoseidonBN254 permutation, static per plan: its first cell in the proof's stream, its shard unit (NO_SLOT: the root's block), that unit's first cell
struct BnpD { uint64_t cell0, ucell0; uint32_t unit, pad; };

struct TracedPlan {
    std::vector<TmplD> tmpls; uint64_t total_slot_lanes = 0;      // sum over templates of nslots * ninst: u64 elements of the value store per proof
    TmplD *d_tm = nullptr; uint64_t *d_prefix = nullptr; uint32_t npool64 = 0, npoolfr = 0;
    uint32_t *d_tape = nullptr; InstD *d_insts = nullptr; ImpD *d_imps = nullptr; uint32_t *d_inputs = nullptr; uint64_t *d_pool64 = nullptr; fr_t *d_poolfr = nullptr;
    uint64_t n_ops = 0, n_segments = 0;
    // fused Goldilocks-Poseidon permutations: per proof nglp list entries (entry e belongs to shard unit h_glp_unit[e], NO_SLOT: the root's block)
    uint32_t nglp = 0; uint64_t n_candidates = 0; std::vector<uint32_t> h_glp_unit; uint32_t *d_glp_unit = nullptr;
    // fused PoseidonBN254 permutations: per proof nbnp list entries; items: the (proof, entry) pairs of this rank's blocks (sharded calls, beside the lane table)
    bool bn_flag = false; uint32_t nbnp = 0; uint64_t n_bn_left = 0; std::vector<BnpD> h_bnp; BnpD *d_bnp = nullptr; std::vector<uint32_t> h_bnp0; uint32_t *d_bnp0 = nullptr, *d_bn_items = nullptr; uint64_t n_bn_items = 0;
    hipEvent_t tev[16]; int n_tev = 0, tev_used = 0; bool timing = false;      // h2w_plan_trace_timing: around every kernel of the last call
    // sharding: the depth-1 instances are the units (query q = the q-th in tape order); why_unshardable empty: they tile the stream behind the root's block
    std::string why_unshardable; std::vector<uint32_t> h_unit;      // h_unit: the unit of every instance (InstD order)
    std::vector<uint32_t> h_lanes, lane0; uint32_t *d_lanes = nullptr; uint64_t lanes_n = 0; int lanes_rank = -1, lanes_world = 0;      // the lane table of the last (n, rank, world)
};

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
// what it was without that op
template <bool BN> __global__ __launch_bounds__(64) __attribute__((flatten)) void k_replay(ReplayArgsT<BN> R) {
    const uint32_t lane = threadIdx.x;
    if (lane < T_MAX) s_nc[lane] = R.ncells[lane];
    if (lane == 0) { s_cx.gvals = R.vals; s_cx.tm = R.tm; s_cx.prefix = R.prefix; s_cx.imps = R.imps; s_cx.inputs = R.inputs; s_cx.pool64 = R.pool64; s_cx.poolfr = R.poolfr; s_cx.nproofs = R.nproofs; }
    for (uint32_t i = lane; i < R.npool64 && i < POOL64_CAP; i += 64) s_lds[LDS_POOL64 / 8 + i] = g_load_u64(R.pool64 + i);
    for (uint32_t i = lane; i < 4 * R.npoolfr && i < 4 * POOLFR_CAP; i += 64) s_lds[LDS_POOLFR / 8 + i] = g_load_u64(reinterpret_cast<const uint64_t *>(R.poolfr) + i);
    __syncthreads();
    // which template this block runs (the templates of one depth share a launch: they do not depend on one another)
    uint32_t t = 0;
#pragma unroll 1
    for (uint32_t i = 0; i < R.ntmpl; i++) if (R.tm[i].depth == R.depth && blockIdx.x >= R.blk0[i]) t = i;
    // (a value loaded from global memory is "divergent" to the compiler even at a uniform address: without the readfirstlane the tape pointer is a
    //  vector register, every tape word a VECTOR load - behind the record stores in flight, 2.5 us per op - and every branch of the interpreter a lane mask)
    t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
    const TmplD T = R.tm[t];
    const uint32_t ninst = (uint32_t)__builtin_amdgcn_readfirstlane((int)T.ninst), tape0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)T.tape0), inst0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)T.inst0);
    const uint32_t gl = (blockIdx.x - R.blk0[t]) * 64 + lane;
    uint32_t g, emit = 1u;      // g = p * ninst + inst: the lane's place in the value store
    if (R.lanes) {              // sharded: the lanes this rank owns; bit 31: a root lane of a proof it does not own; NO_SLOT: padding
        const uint32_t base = R.lane0[t];
        if (gl >= R.lane0[t + 1] - base) return;
        const uint32_t e = R.lanes[base + gl];
        if (e == NO_SLOT) return;
        g = e & 0x7fffffffu; emit = (uint32_t)__builtin_amdgcn_readfirstlane((int)((e >> 31) ^ 1u));
    } else { g = gl; if (g >= R.nproofs * ninst) return; }
    const uint32_t p = g / ninst, inst = g % ninst;
    const InstD *const I = R.insts + inst0 + inst;
    const uint32_t imp0 = I->imp0, in0 = I->in0, glp0 = I->glp0;
    [[maybe_unused]] uint32_t bnp0 = 0; if constexpr (BN) bnp0 = R.bnp0[inst0 + inst];
    fr_t *outb = R.out + (uint64_t)p * R.cell_stride;
    if (R.sh_compact) {         // the packed buffer: the lane's block (the root's: the prologue block) at its local start, its cells at their global offsets
        const uint64_t W = R.sh_world, r = R.sh_rank, u0 = (uint64_t)p * R.nq, unit = I->unit;
        const uint64_t units_before = (u0 + W - 1 - r) / W;
        uint64_t local = (((uint64_t)p + W - 1 - r) / W) * R.pro_ncell + units_before * R.q_slot;
        if (unit != NO_SLOT) local += ((uint64_t)p % W == r ? R.pro_ncell : 0) + ((u0 + unit + W - 1 - r) / W - units_before) * R.q_slot;
        outb = R.out + local - I->ucell0;
    }
    ReplaySink sink; sink.recs = R.recs + (uint64_t)p * R.rec_stride; sink.out = outb; sink.ncells = s_nc; sink.cc.init(R.cm); sink.emit = emit;
    sink.nrec = I->rec0; sink.cell_off = I->cell0;
    ValCfg cfg; cfg.proof = R.proofs + (uint64_t)p * R.proof_words; cfg.mode = 1; cfg.L = R.L; cfg.P = R.P; cfg.inv_pos = R.inv_pos; cfg.inv_neg = R.inv_neg; cfg.st = nullptr;
    cfg.split = false; cfg.split_bn = false; cfg.load_items = nullptr; cfg.n_load_items = 0; cfg.load_nrec = cfg.load_ncell = 0; cfg.n_cap_items = 0; cfg.fri = nullptr;
    RB be(sink, cfg, true);
    const uint64_t Lt = (uint64_t)R.nproofs * ninst;
    const uint64_t pre = R.prefix[t];
    uint64_t *const vals_g = R.vals + (uint64_t)R.nproofs * (((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(pre >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)pre)) + g;
    const uint64_t *const proof = cfg.proof; const uint32_t *const tape = R.tape;
    const uint32_t lane8 = lane * 8;
    const char *const lds = reinterpret_cast<const char *>(s_lds);
    // word j of an operand: the ring or a pool entry, both in LDS, no branch (the ref says which: fastref_*)
    auto get64 = [&](uint32_t r, uint32_t j) -> uint64_t {
        const bool ring = (r >> 31) != 0;
        const uint32_t off = ring ? (((r + j) & (RING_K - 1)) << 9) : ((r & 0x3ffffu) + (j << 3));
        return *reinterpret_cast<const uint64_t *>(lds + off + (ring ? lane8 : 0u));
    };
    auto getfr = [&](uint32_t r) -> fr_t {
        const uint32_t w = (r >> 27) & 3u;      // W64, W128, WFR
        const uint64_t a = get64(r, 0), b = w != W64 ? get64(r, 1) : 0, c = w == WFR ? get64(r, 2) : 0, d = w == WFR ? get64(r, 3) : 0;
        fr_t v; v.l[0] = a; v.l[1] = b; v.l[2] = c; v.l[3] = d; return v;
    };
    auto ring_put = [&](uint32_t slot, uint64_t v) { s_lds[(slot & (RING_K - 1)) * 64 + lane] = v; };
    auto st1 = [&](uint32_t slot, uint64_t v) { ring_put(slot, v); H2W_GSTORE64(vals_g + (uint64_t)slot * Lt, v); };
    auto put64 = [&](uint32_t slot, uint64_t v) { if (slot != NO_SLOT) st1(slot, v); };
    auto putfr = [&](uint32_t slot, const fr_t &v) { if (slot != NO_SLOT) { st1(slot, v.l[0]); st1(slot + 1, v.l[1]); st1(slot + 2, v.l[2]); st1(slot + 3, v.l[3]); } };
    uint64_t ta[64], tb[64];
    bool bad_word = false;
    // The op at pc sits in eight scalar registers (a window of the tape); the window of the NEXT op is requested before this one runs: a scalar load
    // waited for where it is used was ~200 cycles, five times per op.  (Ops with operand lists read the words beyond the window themselves.)
    uint32_t pc = tape0;
    uint32_t w0 = tw(tape, pc), w1 = tw(tape, pc + 1u), w2 = tw(tape, pc + 2u), w3 = tw(tape, pc + 3u), w4 = tw(tape, pc + 4u);
#pragma unroll 1
    for (;;) {
        const uint32_t h = w0; const uint32_t op = h & 0xff, n = (h >> 8) & 0xff, aux = (h >> 16) & 0xff;
        if (op == DOP_END) break;
        const uint32_t pcn = pc + (op == DOP_GLOPRUN ? 2u + 4u * n : (h >> 24));
        const uint32_t n0 = tw(tape, pcn), n1 = tw(tape, pcn + 1), n2 = tw(tape, pcn + 2), n3 = tw(tape, pcn + 3), n4 = tw(tape, pcn + 4);
        if constexpr (BN) {
            if (op == DOP_BNPERM) {     // (in front of the switch: the instantiation without it keeps its code)  The lane keeps the VALUES of the permutation (bnpval.h); its cells are k_bn_emit_traced's, from the listed input state
                fr_t st[BN_WIDTH];
                st[0] = getfr(w1); st[1] = getfr(w2); st[2] = getfr(w3); st[3] = getfr(w4);
                const uint32_t o = tw(tape, pc + 5), ls = tw(tape, pc + 6), nc = tw(tape, pc + 7);
                if (sink.emit) {
                    uint64_t *e = R.blist + ((uint64_t)p * R.nbnp + bnp0 + ls) * BNP_LIST_WORDS;
                    H2W_GSTORE64(e, sink.cell_off); H2W_GSTORE64(e + 1, 1ull);
#pragma unroll
                    for (int i = 0; i < BN_WIDTH; i++) { H2W_GSTORE64(e + 2 + 4 * i, st[i].l[0]); H2W_GSTORE64(e + 3 + 4 * i, st[i].l[1]); H2W_GSTORE64(e + 4 + 4 * i, st[i].l[2]); H2W_GSTORE64(e + 5 + 4 * i, st[i].l[3]); }
                }
                const unsigned long long *const bk = reinterpret_cast<const unsigned long long *>(R.bnk);
                bn_permute_values(st, R.P, [&](int i) -> fr_t { fr_t v; v.l[0] = H2W_CLOAD64(bk + 4 * i); v.l[1] = H2W_CLOAD64(bk + 4 * i + 1); v.l[2] = H2W_CLOAD64(bk + 4 * i + 2); v.l[3] = H2W_CLOAD64(bk + 4 * i + 3); return v; });
                putfr(o, st[0]); putfr(o + 4, st[1]); putfr(o + 8, st[2]); putfr(o + 12, st[3]);
                sink.skip(0, nc);
                pc = pcn; w0 = n0; w1 = n1; w2 = n2; w3 = n3; w4 = n4;
                continue;
            }
        }
        switch (op) {
            case DOP_SKIP: { const uint64_t nr = ((uint64_t)w2 << 32) | w1, nc = ((uint64_t)w4 << 32) | w3; sink.skip(nr, nc); break; }
            case DOP_CONST1: { const uint64_t v = get64(w1, 0); sink.rec(T_CONST1, v, 0, 0, 0); put64(w2, v); break; }
            case DOP_FRCELL: { const fr_t v = getfr(w1); be.cell(v); putfr(w2, v); break; }
            case DOP_LOADW: { const uint64_t v = get64(w1, 0); sink.rec(T_LOADW, v, 0, 0, 0); put64(w2, v); break; }
            case DOP_LOADW_DIV: {      // the hint of GoldilocksChip::div (base.rs:371-393): a / b; b == 0: status 1, the cells of the op on 1
                const uint64_t a = get64(w1, 0); uint64_t b = get64(w2, 0);
                if (b == 0) { be.fail(1); b = 1; }
                const uint64_t v = gl_mul(a, gl_inv(b)); sink.rec(T_LOADW, v, 0, 0, 0); put64(w3, v); break;
            }
            case DOP_LOADW_EXTINV: {   // extension.rs:320-340
                gle_t a; a.c[0] = get64(w1, 0); a.c[1] = get64(w2, 0);
                if (a.c[0] == 0 && a.c[1] == 0) { be.fail(2); a.c[0] = 1; }
                const gle_t iv = gle_inv(a); const uint64_t v = (aux & 1) ? iv.c[1] : iv.c[0]; sink.rec(T_LOADW, v, 0, 0, 0); put64(w3, v); break;
            }
            case DOP_GLOP: { const uint64_t A = get64(w1, 0), B = get64(w2, 0), C = get64(w3, 0); sink.rec((int)aux, A, B, C, 0); put64(w4, gl_reduce128((u128)A * B + C)); break; }
            case DOP_GATE: { const uint64_t A = get64(w1, 0), B = get64(w2, 0), C = get64(w3, 0); sink.rec((int)aux, A, B, C, 0);
                             const u128 v = (u128)A * B + C; const uint32_t o = w4; if (o != NO_SLOT) { st1(o, (uint64_t)v); st1(o + 1, (uint64_t)(v >> 64)); } break; }
            case DOP_REDUCE: { const uint32_t r = w1; const uint64_t lo = get64(r, 0), hi = get64(r, 1); sink.rec(T_REDUCE, lo, hi, 0, 0); put64(w2, gl_reduce128(((u128)hi << 64) | lo)); break; }
            case DOP_CLT: { sink.rec(T_CLT_SAFE, get64(w1, 0), 0, 0, 0); break; }
            case DOP_FR_ADD: { const fr_t v = be.fr_add(getfr(w1), getfr(w2)); putfr(w3, v); break; }
            case DOP_FR_MUL: { const fr_t v = be.fr_mul(getfr(w1), getfr(w2)); putfr(w3, v); break; }
            case DOP_FR_MULADD: { const fr_t v = be.fr_mul_add(getfr(w1), getfr(w2), getfr(w3)); putfr(w4, v); break; }
            case DOP_SELECT: { const uint64_t v = be.select(get64(w1, 0), get64(w2, 0), get64(w3, 0)); put64(w4, v); break; }
            case DOP_FR_SELECT: { const fr_t v = be.fr_select(getfr(w1), getfr(w2), get64(w3, 0)); putfr(w4, v); break; }
            case DOP_IDX2IND: { be.idx_to_indicator(get64(w1, 0), (int)n, ta); const uint32_t o = w2; for (uint32_t i = 0; i < n; i++) st1(o + i, ta[i]); break; }
            case DOP_SELIND: { for (uint32_t i = 0; i < n; i++) { ta[i] = get64(tw(tape, pc + 1 + i), 0); tb[i] = get64(tw(tape, pc + 1 + n + i), 0); }
                               put64(tw(tape, pc + 1 + 2 * n), be.select_by_indicator(ta, 1, tb, (int)n)); break; }
            case DOP_FR_SELIND: {      // GateChip::select_by_indicator on native values: [0, a0, ind0, s0, a1, ind1, s1, ...] (gates at 3 i)
                fr_t sum = fr_zero(); if (n > 0) be.G(); be.cell64(0);
                for (uint32_t i = 0; i < n; i++) { const fr_t a = getfr(tw(tape, pc + 1 + i)); const uint64_t ind = get64(tw(tape, pc + 1 + n + i), 0); if (ind) sum = h2w::fr_add(sum, a); be.cell(a); be.cell64(ind); if (i + 1 < n) be.G(); be.cell(sum); }
                putfr(tw(tape, pc + 1 + 2 * n), sum); break;
            }
            case DOP_NUM2BITS: { be.num_to_bits(get64(w1, 0), (int)n, ta); const uint32_t o = w2; for (uint32_t i = 0; i < n; i++) st1(o + i, ta[i]); break; }
            case DOP_BITS2NUM: { for (uint32_t i = 0; i < n; i++) ta[i] = get64(tw(tape, pc + 1 + i), 0); put64(tw(tape, pc + 1 + n), be.bits_to_num(ta, (int)n)); break; }
            case DOP_DECOMP565: { be.decompose_le_56_5(getfr(w1), ta); const uint32_t o = w2; for (int i = 0; i < 5; i++) st1(o + i, ta[i]); break; }
            case DOP_LIMBS2NUM: { for (uint32_t i = 0; i < n; i++) ta[i] = get64(tw(tape, pc + 1 + i), 0); putfr(tw(tape, pc + 1 + n), be.limbs_to_num(ta, (int)n)); break; }
            case DOP_RANGE: { be.range_check(get64(w1, 0), (int)aux); break; }
            case DOP_GLOPRUN: {      // the Goldilocks-level ops of a gadget come in runs (a Poseidon round: hash/poseidon/permutation.rs:43-239): no dispatch between them, the next op's words requested before this one is computed
                uint32_t q = pc + 2; uint32_t a = w2, b = w3, c = w4, o = tw(tape, pc + 5);
                rec_t *rp = sink.recs + sink.nrec;      // (the cell cursor is only needed by direct cells: it moves by the run's total, from the tape, once)
#pragma unroll 1
                for (uint32_t i = 0; i < n; i++) {
                    q += 4;
                    const uint32_t na = tw(tape, q), nb = tw(tape, q + 1), nc = tw(tape, q + 2), no = tw(tape, q + 3);      // (past the last op: the next op's first words, unused)
                    const uint64_t A = get64(a, 0), B = get64(b, 0), C = get64(c, 0);
                    if (sink.emit) g_store_rec(rp, A, B, C, 0);
                    rp++; st1(o & 0xffffffu, gl_reduce128((u128)A * B + C));
                    a = na; b = nb; c = nc; o = no;
                }
                sink.nrec += n; sink.cell_off += w1;
                break;
            }
            case DOP_GLPERM: {     // the lane keeps the VALUES of the permutation; its records are k_glp_emit_traced's, from the listed input state
                uint64_t st[SPONGE_WIDTH];
#pragma unroll
                for (uint32_t i = 0; i < (uint32_t)SPONGE_WIDTH; i++) st[i] = get64(tw(tape, pc + 1 + i), 0);
                const uint32_t o = tw(tape, pc + 13), ls = tw(tape, pc + 14), nc = tw(tape, pc + 15);
                if (sink.emit) {
                    uint64_t *e = R.glist + ((uint64_t)p * R.nglp + glp0 + ls) * GLP_LIST_WORDS;
                    H2W_GSTORE64(e, sink.nrec);
#pragma unroll
                    for (int i = 0; i < SPONGE_WIDTH; i++) H2W_GSTORE64(e + 1 + i, st[i]);
                }
                const uint64_t *const glk = R.glk;
                glp_permute_values(st, [&](int i) -> uint64_t { return H2W_CLOAD64(glk + i); });
#pragma unroll
                for (uint32_t i = 0; i < (uint32_t)SPONGE_WIDTH; i++) st1(o + i, st[i]);
                sink.skip(GLP_RECS, nc);
                break;
            }
            case DOP_FETCH: {      // a far operand into the ring (no write-through: a copy)
                bool ge = true;        // a proof word (every one enters here): at least the modulus of its field (one word: Goldilocks, four: BN254)?
                for (uint32_t j = 0; j < n; j++) {
                    const uint64_t x = slow_get64(w1, j, vals_g, Lt, p, imp0, in0, proof), m = n == 1 ? GL_P : fr_mod_limb((int)j);
                    ring_put(w2 + j, x); ge = x > m || (x == m && ge);
                }
                if (ref_kind(w1) == RK_INPUT && ge) bad_word = true;      // status 4 (as k_prologue_load); the cells still come from the raw value
                break;
            }
            default: be.fail(99); break;      // (unreachable: the lowering emits nothing else)
        }
        pc = pcn; w0 = n0; w1 = n1; w2 = n2; w3 = n3; w4 = n4;
    }
    if (be.status) atomicCAS(&R.status[p], 0u, be.status);
    if (bad_word) atomicOr(&R.lflag[p], 4u);
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

// One QUAD per listed PoseidonBN254 permutation of the launch: its 4,032 cells from the entry's input state, by the one-pass emitter the compiled plan's
// k_merkle_bn_fused runs (coop.h QuadSinkT::bn_emit_cells<false>: it walks the S-box chain itself; 64 contiguous bytes per quad and store).  The launch
// works from a dense list of items: every (proof, entry) pair, or - sharded - `items`, the pairs of this rank's blocks (the others' entries were never
// written).  The quads of a wavefront cooperate (cross-lane moves over the whole wavefront): none leaves early, tail quads redo the last item and write
// identical bytes.  WHERE a permutation's cells go is static (BnpD, checked against the entry: status 97 if the interpreter listed another cell); only
// the state comes from the list.  LDS: the tables (34.7 KB) + 10 KB of value slots per wavefront, as k_merkle_bn_fused: two blocks per CU.
struct BnEmitArgs {
    const fr_t *bn_tab; const uint64_t *list; const BnpD *bnp; const uint32_t *items; uint64_t nitems; uint32_t nbnp;
    fr_t *out; uint64_t cell_stride; ColMap cm; FrParams P; uint32_t *status;
    uint32_t sh_world, sh_rank, sh_compact, nq; uint64_t pro_ncell, q_slot;
};
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
    if (A.sh_compact) {         // the packed buffer: as k_replay places the lane's block
        const uint64_t W = A.sh_world, r = A.sh_rank, u0 = p * A.nq, unit = D.unit;
        const uint64_t units_before = (u0 + W - 1 - r) / W;
        uint64_t local = ((p + W - 1 - r) / W) * A.pro_ncell + units_before * A.q_slot;
        if (D.unit != NO_SLOT) local += (p % W == r ? A.pro_ncell : 0) + ((u0 + unit + W - 1 - r) / W - units_before) * A.q_slot;
        outb = A.out + local - D.ucell0;
    }
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

// ------------------------------------------------------------------------------------------------------------------- host: lowering
struct ValInfo { uint32_t seg, slot; uint8_t width, is_static; uint32_t lit; };
struct SegInfo {
    int parent = -1, depth = 0; uint32_t name = 0;
    std::vector<uint32_t> tape; uint32_t nslots = 0; std::vector<ImpD> imps /* tmpl field holds the producer SEGMENT until templates exist */; std::vector<uint32_t> inputs;
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> imp_of;
    uint64_t cell0 = 0, rec0 = 0, ncells = 0, nrecs = 0, all_recs = 0; bool started = false;      // all_recs: with the nested segments' (ncells includes them)
    uint32_t unit = NO_SLOT;      // the depth-1 instance (shard unit) this segment is or lies in
    int tmpl = -1; uint32_t inst = 0;
    long last_const_at = -1; uint64_t last_const_cell = 0; size_t last_const_tr = 0;      // the op emitted last is a static CONST1 (its tape position, its cell): a GLOP right behind it that takes it as operand A fuses with it
    uint32_t nglp = 0, glp0 = 0;      // fused permutations (DOP_GLPERM) of this segment; its first entry in the proof's list
    std::vector<struct Matcher *> mt; // the searches for permutation-shaped stretches (first lowering of a fused plan): one per canonical tape
    uint32_t nbnp = 0, bnp0 = 0; std::vector<uint64_t> bnp_cells;      // fused PoseidonBN254 permutations (DOP_BNPERM) of this segment: their first cells; its first entry in the proof's list
};
// ---- stretches of a tape that ARE a permutation (H2W_TRACE_FUSE_GL_PERMUTE, H2W_TRACE_FUSE_BN_PERMUTE).  A lowered op, before its operands become fast refs:
struct NormOp {
    uint32_t hdr = 0, nin = 0, ref[3] = {0, 0, 0}, out = NO_SLOT, slots_before = 0; fr_t lit[3] = {fr_zero(), fr_zero(), fr_zero()};      // hdr: op | n << 8 | aux << 16; ref: mkref words; lit: the value of a literal operand
    size_t tr0 = 0, tr1 = 0; uint64_t cell0 = 0, cell1 = 0, out_cell = 0; const TraceIn *tin = nullptr;               // the trace ops / cells it covers; its result handle; its operands on the trace
};
// an operand of the canonical tape: a literal (its value, kind and width), a value computed inside the stretch (the op that produced it, relative to the
// start; its width), one of the inputs
enum { CK_LIT = 0, CK_INTERIOR = 1, CK_INPUT = 2 };
enum { CANON_GL = 0, CANON_BN = 1, CANON_BN_ZERO = 2 };      // CANON_BN_ZERO: the PoseidonBN254 tape recorded on a fresh context (the load_zero cell inside its first mix)
constexpr int MAX_PERM_IO = SPONGE_WIDTH;
struct CanonOp { uint32_t hdr, nin; uint8_t kind[3], rk[3], width[3]; uint64_t arg[3]; fr_t lit[3]; bool has_out; };
// nio: inputs = outputs (12 one-word values; 4 of width WFR).  in_any_width: an input may be of any width (nothing of the lowering depends on it: the
// PoseidonBN254 tape adds a wide constant to every input first); else an input is one word, as the canonical one.
struct Canon { int id = CANON_GL, nio = SPONGE_WIDTH; bool in_any_width = false; std::vector<CanonOp> ops; uint32_t out_prod[MAX_PERM_IO]; uint64_t ncells = 0; };
// a stretch that matched a canonical tape in op codes, record templates, widths and dataflow; const_bad: on other constants; escaped: an interior value is read outside
struct Stretch { size_t tr0, tr1; int seg, canon, nio; TraceIn in[MAX_PERM_IO]; uint64_t out[MAX_PERM_IO]; uint64_t cell0, cell1; bool const_bad, escaped; };
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
static uint64_t rc_cells(int L, uint64_t bits) { if (bits == 0) return 0; const uint64_t n = (bits + L - 1) / L, rem = bits % L; return (n > 1 ? 1 + 3 * (n - 1) : 0) + (rem ? 4 : 0); }

}  // namespace h2w

using namespace h2w;

namespace h2w {
uint64_t traced_workspace_bytes(const h2w_plan *p, uint64_t n);
int traced_run(h2w_plan *p, const uint64_t *proofs_dev, uint64_t n_proofs, void *advice_dev, void *workspace_dev, void *stream_, ColMap cm, uint64_t cell_stride, const ShardSpec &sh);
void traced_free(h2w_plan *p);
const char *traced_shard_refusal(const h2w_plan *p) { return p->traced && !p->traced->why_unshardable.empty() ? p->traced->why_unshardable.c_str() : nullptr; }
struct TracedWs { size_t recs, status, lflag, ctr, vals, glist, blist, total; };
static size_t al(size_t x) { return (x + 255) / 256 * 256; }
static TracedWs traced_ws(const h2w_plan *p, uint64_t n) {
    TracedWs w; size_t o = 0;
    w.recs = o; o += al((size_t)n * p->nrec * sizeof(rec_t));
    w.status = o; o += al((size_t)n * 4); w.lflag = o; o += al((size_t)n * 4); w.ctr = o; o += al((size_t)n * 4);
    w.vals = o; o += al((size_t)n * p->traced->total_slot_lanes * 8);
    w.glist = o; o += al((size_t)n * p->traced->nglp * GLP_LIST_WORDS * 8);      // the fused permutations' list (none: the layout of an unfused plan)
    w.blist = o; o += al((size_t)n * p->traced->nbnp * BNP_LIST_WORDS * 8);      // the fused PoseidonBN254 permutations' list (none: nothing)
    w.total = o; return w;
}
uint64_t traced_workspace_bytes(const h2w_plan *p, uint64_t n) { return traced_ws(p, n).total; }
uint64_t traced_status_offset(const h2w_plan *p, uint64_t n, bool flags) { const TracedWs w = traced_ws(p, n); return flags ? w.lflag : w.status; }
void traced_free(h2w_plan *p) {
    TracedPlan *t = p->traced; if (!t) return;
    if (t->d_tm) (void)hipFree(t->d_tm); if (t->d_prefix) (void)hipFree(t->d_prefix);
    if (t->d_tape) (void)hipFree(t->d_tape); if (t->d_insts) (void)hipFree(t->d_insts); if (t->d_imps) (void)hipFree(t->d_imps);
    if (t->d_inputs) (void)hipFree(t->d_inputs); if (t->d_pool64) (void)hipFree(t->d_pool64); if (t->d_poolfr) (void)hipFree(t->d_poolfr);
    if (t->d_lanes) (void)hipFree(t->d_lanes); if (t->d_glp_unit) (void)hipFree(t->d_glp_unit);
    if (t->d_bnp) (void)hipFree(t->d_bnp); if (t->d_bnp0) (void)hipFree(t->d_bnp0); if (t->d_bn_items) (void)hipFree(t->d_bn_items);
    for (int i = 0; i < t->n_tev; i++) (void)hipEventDestroy(t->tev[i]);
    delete t; p->traced = nullptr;
}
// The lanes a rank launches (sharded calls), template by template: the root lane of every proof - those of the proofs the rank owns first, then, from
// the next wavefront on, the others marked with bit 31 (they compute the values the units import, and store nothing else) -, and of every deeper
// template only the (proof, instance) pairs whose unit (proof * nq + q) % world == rank (h2w_plan_shard_block, distributed.py unit_owner).
static int lane_table(h2w_plan *p, uint64_t n, const ShardSpec &sh) {
    TracedPlan *t = p->traced;
    if (t->d_lanes && t->lanes_n == n && t->lanes_rank == sh.rank && t->lanes_world == sh.world) return 0;
    const uint64_t W = (uint64_t)sh.world, r = (uint64_t)sh.rank, nq = (uint64_t)p->shape.num_queries;
    std::vector<uint32_t> &L = t->h_lanes; L.clear(); t->lane0.assign(t->tmpls.size() + 1, 0);
    for (size_t i = 0; i < t->tmpls.size(); i++) {
        const TmplD &T = t->tmpls[i]; t->lane0[i] = (uint32_t)L.size();
        if (n * T.ninst >= 0x80000000ull) { set_error("h2w_fri_witness_batch_shard: too many (proof, instance) lanes in one call"); return -1; }
        if (T.depth == 0) {
            for (uint64_t pr = r; pr < n; pr += W) L.push_back((uint32_t)pr);
            while ((L.size() - t->lane0[i]) % 64) L.push_back(NO_SLOT);
            for (uint64_t pr = 0; pr < n; pr++) if (pr % W != r) L.push_back((uint32_t)pr | 0x80000000u);
        } else
            for (uint64_t pr = 0; pr < n; pr++)
                for (uint32_t k = 0; k < T.ninst; k++) if ((pr * nq + t->h_unit[T.inst0 + k]) % W == r) L.push_back((uint32_t)(pr * T.ninst + k));
    }
    t->lane0[t->tmpls.size()] = (uint32_t)L.size();
    // the listed PoseidonBN254 permutations of this rank's blocks, dense: (proof, entry) as proof * nbnp + entry - the root's of the proofs it owns, a
    // unit's where it owns the unit (the lanes above that run with emit set: the entries that get written)
    std::vector<uint32_t> items;
    if (t->nbnp) {
        if (n * t->nbnp >= 0xffffffffull) { set_error("h2w_fri_witness_batch_shard: too many fused permutations in one call"); return -1; }
        for (uint64_t pr = 0; pr < n; pr++)
            for (uint32_t e = 0; e < t->nbnp; e++) {
                const uint32_t u = t->h_bnp[e].unit;
                if ((u == NO_SLOT ? pr : pr * nq + u) % W == r) items.push_back((uint32_t)(pr * t->nbnp + e));
            }
    }
    H2W_HIP(hipDeviceSynchronize());      // a previous call may still read the old table (plans are single-threaded handles, include/h2w.h)
    if (t->d_bn_items) { (void)hipFree(t->d_bn_items); t->d_bn_items = nullptr; }
    t->n_bn_items = items.size();
    if (t->nbnp) { H2W_HIP(hipMalloc((void **)&t->d_bn_items, (items.empty() ? 1 : items.size()) * 4)); if (!items.empty()) H2W_HIP(hipMemcpy(t->d_bn_items, items.data(), items.size() * 4, hipMemcpyHostToDevice)); }
    if (t->d_lanes) { (void)hipFree(t->d_lanes); t->d_lanes = nullptr; }
    H2W_HIP(hipMalloc((void **)&t->d_lanes, (L.empty() ? 1 : L.size()) * 4));
    if (!L.empty()) H2W_HIP(hipMemcpy(t->d_lanes, L.data(), L.size() * 4, hipMemcpyHostToDevice));
    t->lanes_n = n; t->lanes_rank = sh.rank; t->lanes_world = sh.world;
    return 0;
}
int traced_run(h2w_plan *p, const uint64_t *proofs_dev, uint64_t n_proofs, void *advice_dev, void *workspace_dev, void *stream_, ColMap cm, uint64_t cell_stride, const ShardSpec &sh) {
    TracedPlan *t = p->traced;
    if (n_proofs > 65535) { set_error("h2w_fri_witness_batch: more than 65535 proofs per call"); return -1; }
    const bool sharded = sh.world > 1;
    if ((sharded || sh.compact) && !t->why_unshardable.empty()) { set_error("h2w_fri_witness_batch_shard: " + t->why_unshardable); return -1; }
    if (sh.compact && !sharded) { set_error("h2w_fri_witness_batch_shard_compact: world 1 on a traced plan: use h2w_fri_witness_batch (the packed form of one rank is the flat stream)"); return -1; }
    DeviceGuard dg(p->device);
    if (sharded && lane_table(p, n_proofs, sh) != 0) return -1;
    hipStream_t stream = (hipStream_t)stream_;
    const TracedWs wl = traced_ws(p, n_proofs); char *ws = (char *)workspace_dev;
    ReplayArgs R; memset(&R, 0, sizeof(R));
    R.tape = t->d_tape; R.insts = t->d_insts; R.imps = t->d_imps; R.inputs = t->d_inputs; R.pool64 = t->d_pool64; R.poolfr = t->d_poolfr;
    R.proofs = proofs_dev; R.proof_words = p->pl.total; R.recs = (rec_t *)(ws + wl.recs); R.rec_stride = p->nrec; R.out = (fr_t *)advice_dev; R.cell_stride = cell_stride; R.cm = cm;      // (cm.starts: the FlexGate columns of every proof, cell_stride = ncols << k; else the flat stream)
    R.vals = (uint64_t *)(ws + wl.vals); R.status = (uint32_t *)(ws + wl.status); R.ncells = p->d_ncells; R.inv_pos = p->d_inv; R.inv_neg = p->d_inv + INV_TAB; R.P = p->P; R.L = p->shape.lookup_bits;
    R.nproofs = (uint32_t)n_proofs; R.lflag = (uint32_t *)(ws + wl.lflag);
    R.glk = reinterpret_cast<const uint64_t *>(p->d_consts); R.glist = (uint64_t *)(ws + wl.glist); R.nglp = t->nglp;
    R.ntmpl = (uint32_t)t->tmpls.size(); R.tm = t->d_tm; R.prefix = t->d_prefix; R.npool64 = t->npool64; R.npoolfr = t->npoolfr;
    if (sharded) {
        R.lanes = t->d_lanes; for (size_t i = 0; i < t->lane0.size(); i++) R.lane0[i] = t->lane0[i];
        R.sh_world = (uint32_t)sh.world; R.sh_rank = (uint32_t)sh.rank; R.sh_compact = (uint32_t)sh.compact; R.nq = (uint32_t)p->shape.num_queries;
        R.pro_ncell = p->st.pro_ncell; R.q_slot = std::max(p->st.q_ncell[0], p->st.q_ncell[1]);
    }
    H2W_HIP(hipMemsetAsync(ws + wl.status, 0, n_proofs * 4, stream));
    H2W_HIP(hipMemsetAsync(ws + wl.lflag, 0, n_proofs * 4, stream));
    uint32_t maxd = 0; for (const TmplD &T : t->tmpls) if (T.depth > maxd) maxd = T.depth;
    uint64_t *const blist = (uint64_t *)(ws + wl.blist);
    t->tev_used = 0;
    for (uint32_t d = 0; d <= maxd; d++) {      // a segment reads its ancestors' values: depth by depth; the templates of one depth in one launch
        uint32_t nb = 0;
        for (size_t i = 0; i < t->tmpls.size(); i++) {
            R.blk0[i] = nb;
            if (t->tmpls[i].depth == d) nb += (uint32_t)(((sharded ? t->lane0[i + 1] - t->lane0[i] : n_proofs * t->tmpls[i].ninst) + 63) / 64);
        }
        R.blk0[t->tmpls.size()] = nb; R.depth = d;
        if (t->timing && t->tev_used < 12) H2W_HIP(hipEventRecord(t->tev[t->tev_used++], stream));
        if (nb && t->nbnp) {
            ReplayArgsT<true> RB; static_cast<ReplayArgs &>(RB) = R; RB.bnk = p->d_bn_tab + BK_T; RB.blist = blist; RB.bnp0 = t->d_bnp0; RB.nbnp = t->nbnp;
            hipLaunchKernelGGL(k_replay<true>, dim3(nb), dim3(64), 0, stream, RB);
        } else if (nb) hipLaunchKernelGGL(k_replay<false>, dim3(nb), dim3(64), 0, stream, R);
    }
    if (t->timing) H2W_HIP(hipEventRecord(t->tev[t->tev_used++], stream));
    if (t->nglp) {      // the records of the listed permutations, side by side
        GlpEmitArgs E; E.consts = p->d_consts; E.list = R.glist; E.recs = R.recs; E.rec_stride = R.rec_stride; E.ncells = p->d_ncells; E.unit = t->d_glp_unit;
        E.nglp = t->nglp; E.world = sharded ? (uint32_t)sh.world : 1u; E.rank = (uint32_t)sh.rank; E.nq = (uint32_t)p->shape.num_queries;
        if ((uint64_t)n_proofs * t->nglp >= 0x7fffffffull) { set_error("h2w_fri_witness_batch: too many fused permutations in one call"); return -1; }
        hipLaunchKernelGGL(k_glp_emit_traced, dim3((uint32_t)(n_proofs * t->nglp)), dim3(64), 0, stream, E);
    }
    if (t->timing && t->bn_flag) H2W_HIP(hipEventRecord(t->tev[t->tev_used++], stream));
    if (t->nbnp) {      // the cells of the listed PoseidonBN254 permutations, a quad each (direct cells: nothing of the expansion depends on them, nor they on it)
        BnEmitArgs E; memset(&E, 0, sizeof(E));
        E.bn_tab = p->d_bn_tab; E.list = blist; E.bnp = t->d_bnp; E.nbnp = t->nbnp; E.out = R.out; E.cell_stride = cell_stride; E.cm = cm; E.P = p->P; E.status = R.status;
        if (sharded) {
            E.items = t->d_bn_items; E.nitems = t->n_bn_items;
            E.sh_world = R.sh_world; E.sh_rank = R.sh_rank; E.sh_compact = R.sh_compact; E.nq = R.nq; E.pro_ncell = R.pro_ncell; E.q_slot = R.q_slot;
        } else { E.items = nullptr; E.nitems = (uint64_t)n_proofs * t->nbnp; }
        const uint64_t nblk = (E.nitems * 4 + QUAD_BLOCK - 1) / QUAD_BLOCK;
        if (nblk >= 0x7fffffffull) { set_error("h2w_fri_witness_batch: too many fused permutations in one call"); return -1; }
        if (nblk) { if (cm.starts) hipLaunchKernelGGL(k_bn_emit_traced<true>, dim3((uint32_t)nblk), dim3(QUAD_BLOCK), 0, stream, E); else hipLaunchKernelGGL(k_bn_emit_traced<false>, dim3((uint32_t)nblk), dim3(QUAD_BLOCK), 0, stream, E); }
    }
    if (t->timing) H2W_HIP(hipEventRecord(t->tev[t->tev_used++], stream));
    // expansion of the block records
    if (launch_plan_expand(p, n_proofs, R.recs, (uint32_t *)(ws + wl.ctr), R.out, cell_stride, cm, sharded ? &sh : nullptr, 2, stream) != 0) return -1;
    if (t->timing) H2W_HIP(hipEventRecord(t->tev[t->tev_used++], stream));
    H2W_HIP(hipGetLastError());
    return 0;
}
}  // namespace h2w

// The tape lowered segment by segment (passes 1 and 2 of h2w_plan_from_trace): what a plan is assembled from.
struct Lowered {
    std::vector<SegInfo> segs; std::vector<ValInfo> vals; std::unordered_map<uint64_t, uint32_t> val_of;      // val_of: cell offset of a handle -> value
    std::vector<uint64_t> pool64; std::map<uint64_t, uint32_t> pool64_of; std::vector<fr_t> poolfr;
    std::vector<uint64_t> meta; uint64_t nrec = 0; std::string err;
};
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
    ValCfg cfg; memset(&cfg, 0, sizeof(cfg)); cfg.L = L; cfg.P = fr_params_init();
    ValBackend<LayoutSink> be(sink, cfg, true);
    PoseidonPermutationChip<ValBackend<LayoutSink>> pg(be, consts);
    uint64_t st[SPONGE_WIDTH] = {0}; pg.permute(st);
    return sink.ndirect == 0 && sink.nrec == (uint64_t)GLP_RECS ? sink.cell_off : 0;
}
// fuse: the stretches to lower as ONE op (by their first trace op), glp_meta their record block; cn: look for stretches instead (-> found);
// capture: the lowered ops of the root segment as they are (the canonical tape is made from them)
static void lower_trace(const Trace *tr, int L, TemplateTable &tt, const char *const *parallel_scopes, size_t n_scopes, Lowered &LW,
                        const std::map<size_t, Stretch> *fuse, const std::vector<uint64_t> *glp_meta, const std::vector<const Canon *> *cns, std::vector<Stretch> *found, std::vector<NormOp> *capture) {
    std::string &err = LW.err;
    auto bad = [&](const std::string &m) { if (err.empty()) err = m; };
    // ---- pass 1: segments
    std::vector<SegInfo> &segs = LW.segs; segs.assign(1, SegInfo());
    std::vector<int> op_seg(tr->ops.size(), 0);
    {
        std::vector<int> stack;      // per open scope: the segment it opened, or -1 (an ordinary scope)
        int cur = 0;
        for (size_t i = 0; i < tr->ops.size(); i++) {
            const TraceOp &o = tr->ops[i];
            if (o.code == TR_SCOPE_PUSH) {
                bool par = false; for (size_t k = 0; k < n_scopes; k++) if (tr->names[(size_t)o.imm] == parallel_scopes[k]) par = true;
                if (par) { SegInfo s; s.parent = cur; s.depth = segs[(size_t)cur].depth + 1; s.name = (uint32_t)o.imm; segs.push_back(s); cur = (int)segs.size() - 1; stack.push_back(cur); }
                else stack.push_back(-1);
            } else if (o.code == TR_SCOPE_POP) {
                if (stack.empty()) { bad("unbalanced scopes in the trace"); break; }
                if (stack.back() >= 0) cur = segs[(size_t)stack.back()].parent;
                stack.pop_back();
            }
            op_seg[i] = cur;
        }
        if (!stack.empty()) bad("a scope is still open at the end of the trace");
    }
    // scope names compare by string: give every parallel name one id
    { std::map<std::string, uint32_t> ids; for (SegInfo &s : segs) { if (s.parent < 0) continue; auto it = ids.find(tr->names[s.name]); if (it == ids.end()) it = ids.emplace(tr->names[s.name], (uint32_t)ids.size() + 1).first; s.name = it->second; } }
    // ---- pass 2: lowering, in tape order
    std::unordered_map<uint64_t, uint32_t> &val_of = LW.val_of; std::vector<ValInfo> &vals = LW.vals;
    std::vector<uint64_t> &pool64 = LW.pool64; std::map<uint64_t, uint32_t> &pool64_of = LW.pool64_of; std::vector<fr_t> &poolfr = LW.poolfr;
    std::vector<Matcher> matchers;
    if (cns) {
        matchers.resize(segs.size() * cns->size());
        for (size_t si = 0; si < segs.size(); si++) for (size_t ci = 0; ci < cns->size(); ci++) { Matcher &m = matchers[si * cns->size() + ci]; m.cn = (*cns)[ci]; m.found = found; m.seg = (int)si; segs[si].mt.push_back(&m); }
    }
    auto lit64 = [&](uint64_t v) { auto it = pool64_of.find(v); if (it != pool64_of.end()) return it->second; pool64.push_back(v); pool64_of[v] = (uint32_t)pool64.size() - 1; return (uint32_t)pool64.size() - 1; };
    auto litfr = [&](const fr_t &v) { for (size_t i = 0; i < poolfr.size(); i++) if (fr_eq(poolfr[i], v)) return (uint32_t)i; poolfr.push_back(v); return (uint32_t)poolfr.size() - 1; };
    std::vector<uint64_t> &meta = LW.meta; uint64_t &nrec = LW.nrec;
    auto is_ancestor = [&](int a, int s) { for (int x = s; x >= 0; x = segs[(size_t)x].parent) if (x == a) return true; return false; };
    // operand of op in segment s: the handle's cell, or a literal
    auto ref_of = [&](int s, const TraceIn &in, int *width_out) -> uint32_t {
        if (in.lit) { if (width_out) *width_out = W64; return mkref(RK_LIT64, W64, lit64(in.v)); }
        auto it = val_of.find(in.v);
        if (it == val_of.end()) { bad("an operand is not the result of a traced call (cell " + std::to_string(in.v) + ")"); if (width_out) *width_out = W64; return mkref(RK_LIT64, W64, lit64(0)); }
        const ValInfo &v = vals[it->second]; if (width_out) *width_out = v.width;
        if (v.is_static) return v.width == WFR ? mkref(RK_LITFR, WFR, v.lit) : mkref(RK_LIT64, W64, v.lit);
        if ((int)v.seg == s) return mkref(RK_LOCAL, v.width, v.slot);
        if (!is_ancestor((int)v.seg, s)) { bad("a parallel scope reads a value computed in a scope that does not enclose it: its instances are not independent (cell " + std::to_string(in.v) + ")"); return mkref(RK_LIT64, W64, lit64(0)); }
        SegInfo &S = segs[(size_t)s]; const auto key = std::make_pair(v.seg, v.slot);
        auto im = S.imp_of.find(key);
        if (im == S.imp_of.end()) { S.imps.push_back(ImpD{v.seg, 0, v.slot}); im = S.imp_of.emplace(key, (uint32_t)S.imps.size() - 1).first; }
        return mkref(RK_IMPORT, v.width, im->second);
    };
    auto new_val = [&](int s, uint64_t cell, int width, bool stat, uint32_t lit) -> uint32_t {
        SegInfo &S = segs[(size_t)s]; ValInfo v; v.seg = (uint32_t)s; v.width = (uint8_t)width; v.is_static = stat ? 1 : 0; v.lit = lit; v.slot = NO_SLOT;
        if (!stat) { v.slot = S.nslots; S.nslots += (uint32_t)SLOTS_OF[width]; }
        vals.push_back(v); val_of[cell] = (uint32_t)vals.size() - 1; return v.slot;
    };
    auto add_rec = [&](int s, int tmpl, uint64_t cell) { meta.push_back(meta_pack((uint32_t)tmpl, cell)); nrec++; segs[(size_t)s].nrecs++; };
    std::vector<int> open_child(segs.size(), -1);
    int prev_seg = 0;
    for (size_t i = 0; i < tr->ops.size() && err.empty(); i++) {
        const TraceOp &o = tr->ops[i]; const int s = op_seg[i]; SegInfo &S = segs[(size_t)s];
        if (o.code == TR_SCOPE_PUSH || o.code == TR_SCOPE_POP) {
            // entering a parallel child: the parent steps over its records and cells (filled in when the child ends)
            if (o.code == TR_SCOPE_PUSH && s != prev_seg && segs[(size_t)s].parent == prev_seg) {
                SegInfo &Pn = segs[(size_t)prev_seg]; Pn.tape.push_back(DOP_SKIP | (5u << 24)); Pn.last_const_at = -1; for (Matcher *m : Pn.mt) m->boundary(); open_child[(size_t)s] = (int)Pn.tape.size(); for (int k = 0; k < 4; k++) Pn.tape.push_back(0);
                S.cell0 = o.cell0; S.rec0 = nrec; S.started = true;
            }
            if (o.code == TR_SCOPE_POP && s != prev_seg && segs[(size_t)prev_seg].parent == s) {
                SegInfo &C = segs[(size_t)prev_seg]; C.ncells = o.cell0 - C.cell0; C.tape.push_back(DOP_END | (1u << 24));
                // the child's totals include its own children's (they are nested in its cell and record ranges)
                const uint64_t nr = nrec - C.rec0; uint32_t *w = S.tape.data() + open_child[(size_t)prev_seg];
                w[0] = (uint32_t)nr; w[1] = (uint32_t)(nr >> 32); w[2] = (uint32_t)C.ncells; w[3] = (uint32_t)(C.ncells >> 32); C.all_recs = nr;
            }
            prev_seg = s; continue;
        }
        prev_seg = s;
        const TraceIn *in = tr->ins.data() + o.first_in; const uint64_t *out = tr->outs.data() + o.first_out;
        std::vector<uint32_t> &T = S.tape; uint64_t want_cells = 0; int w0 = 0, w1 = 0, w2 = 0;
        size_t op_at = T.size();
        auto head = [&](uint32_t op, uint32_t n = 0, uint32_t aux = 0) { if (aux > 255) bad("internal: op parameter too wide"); T.push_back(op | (n << 8) | (aux << 16)); };
        const uint32_t slots_before = S.nslots; bool ka_fused = false;
        const Stretch *fz = nullptr;
        if (fuse) { auto f = fuse->find(i); if (f != fuse->end()) fz = &f->second; }
        if (fz && fz->canon == CANON_BN) {      // a verified PoseidonBN254 permutation: one op, its 4 results in fresh slots; no records - its cells are direct cells
            head(DOP_BNPERM);
            for (int k = 0; k < BN_WIDTH; k++) { int w; T.push_back(ref_of(s, fz->in[k], &w)); }
            const uint32_t base = S.nslots;
            for (int k = 0; k < BN_WIDTH; k++) new_val(s, fz->out[k], WFR, false, 0);
            T.push_back(base); T.push_back(S.nbnp++); T.push_back((uint32_t)(fz->cell1 - fz->cell0)); S.bnp_cells.push_back(fz->cell0);
            S.last_const_at = -1;
            want_cells = o.ncells; i = fz->tr1 - 1;
        } else if (fz) {      // a verified permutation: one op, its 12 results in fresh slots, its record block laid out as the emission kernel writes it
            head(DOP_GLPERM);
            for (int k = 0; k < SPONGE_WIDTH; k++) { int w; T.push_back(ref_of(s, fz->in[k], &w)); if (w != W64) bad("internal: a wide input of a fused permutation"); }
            const uint32_t base = S.nslots;
            for (int k = 0; k < SPONGE_WIDTH; k++) new_val(s, fz->out[k], W64, false, 0);
            T.push_back(base); T.push_back(S.nglp++); T.push_back((uint32_t)(fz->cell1 - fz->cell0));
            for (uint64_t m : *glp_meta) meta.push_back(meta_pack(meta_tmpl(m), fz->cell0 + meta_off(m)));
            nrec += glp_meta->size(); S.nrecs += glp_meta->size(); S.last_const_at = -1;
            want_cells = o.ncells; i = fz->tr1 - 1;      // (the loop goes on behind the stretch)
        } else
        switch (o.code) {
            case TR_LOAD_CONSTANT: {
                const fr_t c = tr->consts[(size_t)o.imm]; const bool small = (c.l[1] | c.l[2] | c.l[3]) == 0;
                if (o.tag.kind == 1) {
                    if (o.tag.n != 1) { bad("a constant that is a proof value must be one Goldilocks word"); break; }
                    S.inputs.push_back((uint32_t)o.tag.word); head(DOP_CONST1); T.push_back(mkref(RK_INPUT, W64, (uint32_t)S.inputs.size() - 1)); T.push_back(new_val(s, out[0], W64, false, 0));
                    add_rec(s, T_CONST1, o.cell0); want_cells = 1;
                } else if (o.tag.kind != 0) bad("a hint tag on a constant");
                else if (small) { const uint32_t li = lit64(c.l[0]); head(DOP_CONST1); T.push_back(mkref(RK_LIT64, W64, li)); T.push_back(NO_SLOT); new_val(s, out[0], W64, true, li); add_rec(s, T_CONST1, o.cell0); want_cells = 1;
                                  S.last_const_at = (long)op_at; S.last_const_cell = o.cell0; S.last_const_tr = i; }
                else { const uint32_t li = litfr(c); head(DOP_FRCELL); T.push_back(mkref(RK_LITFR, WFR, li)); T.push_back(NO_SLOT); new_val(s, out[0], WFR, true, li); want_cells = 1; }
                break;
            }
            case TR_LOAD_WITNESS: {
                if (o.tag.kind != 1) { bad("h2w_load_witness without h2w_trace_input"); break; }
                S.inputs.push_back((uint32_t)o.tag.word);
                if (o.tag.n == 4) { head(DOP_FRCELL); T.push_back(mkref(RK_INPUT, WFR, (uint32_t)S.inputs.size() - 1)); T.push_back(new_val(s, out[0], WFR, false, 0)); }
                else { head(DOP_CONST1); T.push_back(mkref(RK_INPUT, W64, (uint32_t)S.inputs.size() - 1)); T.push_back(new_val(s, out[0], W64, false, 0)); add_rec(s, T_CONST1, o.cell0); }
                want_cells = 1; break;
            }
            case TR_ADD: case TR_MUL: case TR_MUL_ADD: {
                const uint32_t a = ref_of(s, in[0], &w0), b = ref_of(s, in[1], &w1), c3 = o.code == TR_MUL_ADD ? ref_of(s, in[2], &w2) : 0;
                const bool narrow = w0 == W64 && w1 == W64 && (o.code != TR_MUL_ADD || w2 == W64);
                if (narrow) {      // [C, A, B, A B + C] on values below 2^64: one gate record (GoldilocksChip::*_no_reduce, base.rs:240-294)
                    head(DOP_GATE, 0, T_GATE);
                    if (o.code == TR_ADD) { T.push_back(b); T.push_back(mkref(RK_LIT64, W64, lit64(1))); T.push_back(a); }
                    else if (o.code == TR_MUL) { T.push_back(a); T.push_back(b); T.push_back(mkref(RK_LIT64, W64, lit64(0))); }
                    else { T.push_back(a); T.push_back(b); T.push_back(c3); }
                    T.push_back(new_val(s, out[0], W128, false, 0)); add_rec(s, T_GATE, o.cell0);
                } else {
                    head(o.code == TR_ADD ? DOP_FR_ADD : o.code == TR_MUL ? DOP_FR_MUL : DOP_FR_MULADD); T.push_back(a); T.push_back(b); if (o.code == TR_MUL_ADD) T.push_back(c3);
                    T.push_back(new_val(s, out[0], WFR, false, 0));
                }
                want_cells = 4; break;
            }
            case TR_SELECT: {
                const uint32_t a = ref_of(s, in[0], &w0), b = ref_of(s, in[1], &w1), sl = ref_of(s, in[2], &w2);
                if (w2 != W64) { bad("select: the selector is not a bit"); break; }
                const bool narrow = w0 == W64 && w1 == W64;
                head(narrow ? DOP_SELECT : DOP_FR_SELECT); T.push_back(a); T.push_back(b); T.push_back(sl); T.push_back(new_val(s, out[0], narrow ? W64 : WFR, false, 0));
                want_cells = 8; break;
            }
            case TR_IDX_TO_INDICATOR: {
                const uint32_t n = (uint32_t)o.imm; const uint32_t a = ref_of(s, in[0], &w0);
                if (w0 != W64 || n < 1 || n > 64) { bad("idx_to_indicator: a wide index or more than 64 entries"); break; }
                head(DOP_IDX2IND, n); T.push_back(a); const uint32_t base = S.nslots;
                for (uint32_t k = 0; k < n; k++) { const uint32_t sl = new_val(s, out[k], W64, false, 0); if (sl != base + k) bad("internal: slots of an array result"); }
                T.push_back(base); want_cells = 8 + 12ull * (n - 1); break;
            }
            case TR_SELECT_BY_INDICATOR: {
                const uint32_t n = (uint32_t)o.imm; if (n < 1 || n > 64) { bad("select_by_indicator: more than 64 entries"); break; }
                std::vector<uint32_t> r(2 * n); bool narrow = true;
                for (uint32_t k = 0; k < 2 * n; k++) { int w; r[k] = ref_of(s, in[k], &w); if (k < n && w != W64) narrow = false; if (k >= n && w != W64) bad("select_by_indicator: an indicator that is not a bit"); }
                head(narrow ? DOP_SELIND : DOP_FR_SELIND, n); for (uint32_t x : r) T.push_back(x); T.push_back(new_val(s, out[0], narrow ? W64 : WFR, false, 0));
                want_cells = 1 + 3ull * n; break;
            }
            case TR_NUM_TO_BITS: {
                const uint32_t n = (uint32_t)o.imm; const uint32_t a = ref_of(s, in[0], &w0);
                if (w0 != W64 || n < 1 || n > 64) { bad("num_to_bits: a wide value or more than 64 bits"); break; }
                head(DOP_NUM2BITS, n); T.push_back(a); const uint32_t base = S.nslots;
                for (uint32_t k = 0; k < n; k++) new_val(s, out[k], W64, false, 0);
                T.push_back(base); want_cells = (1 + 3ull * (n - 1)) + 4ull * n; break;
            }
            case TR_BITS_TO_NUM: {
                const uint32_t n = (uint32_t)o.imm; if (n > 64) { bad("bits_to_num: more than 64 bits"); break; }
                head(DOP_BITS2NUM, n); for (uint32_t k = 0; k < n; k++) { int w; T.push_back(ref_of(s, in[k], &w)); if (w != W64) bad("bits_to_num: an operand that is not a bit"); }
                T.push_back(new_val(s, out[0], W64, false, 0)); want_cells = n ? 1 + 3ull * (n - 1) : 1; break;
            }
            case TR_DECOMPOSE_LE: {
                if ((o.imm >> 32) != 56 || (uint32_t)o.imm != 5) { bad("decompose_le: only (56 bits, 5 limbs) is replayable (HashWire::to_goldilocks_vec, hash/poseidon_bn254/hash.rs:31-43)"); break; }
                head(DOP_DECOMP565); T.push_back(ref_of(s, in[0], &w0)); const uint32_t base = S.nslots; for (int k = 0; k < 5; k++) new_val(s, out[k], W64, false, 0); T.push_back(base);
                want_cells = 13 + 5 * rc_cells(L, 56); break;
            }
            case TR_LIMBS_TO_NUM: {
                const uint32_t n = o.n_in; if (o.imm != 64 || n < 1 || n > 4) { bad("limbs_to_num: only up to four 64-bit limbs are replayable"); break; }
                head(DOP_LIMBS2NUM, n); for (uint32_t k = 0; k < n; k++) { int w; T.push_back(ref_of(s, in[k], &w)); if (w != W64) bad("limbs_to_num: a wide limb"); }
                T.push_back(new_val(s, out[0], WFR, false, 0)); want_cells = 1 + 3ull * (n - 1); break;
            }
            case TR_RANGE_CHECK: {
                const uint32_t a = ref_of(s, in[0], &w0); if (w0 != W64 || o.imm > 64) { bad("range_check: a wide value"); break; }
                head(DOP_RANGE, 0, (uint32_t)o.imm); T.push_back(a); want_cells = rc_cells(L, o.imm); break;
            }
            case TR_CLT_SAFE: {
                const uint32_t a = ref_of(s, in[0], &w0); if (w0 != W64 || o.imm != GL_P) { bad("check_less_than_safe: only (64-bit value, Goldilocks order) is replayable"); break; }
                head(DOP_CLT); T.push_back(a); add_rec(s, T_CLT_SAFE, o.cell0); want_cells = (uint64_t)tt.ncells(T_CLT_SAFE); break;
            }
            case TR_GL_WITNESS: {
                if (o.tag.kind == 1) { if (o.tag.n != 1) { bad("a Goldilocks witness of more than one word"); break; } S.inputs.push_back((uint32_t)o.tag.word); head(DOP_LOADW); T.push_back(mkref(RK_INPUT, W64, (uint32_t)S.inputs.size() - 1)); }
                else if (o.tag.kind == 2) { head(DOP_LOADW_DIV); T.push_back(ref_of(s, TraceIn{o.tag.a, 0}, &w0)); T.push_back(ref_of(s, TraceIn{o.tag.b, 0}, &w1)); if (w0 != W64 || w1 != W64) bad("div: wide operands"); }
                else if (o.tag.kind == 3 || o.tag.kind == 4) { head(DOP_LOADW_EXTINV, 0, (uint32_t)(o.tag.kind - 3)); T.push_back(ref_of(s, TraceIn{o.tag.a, 0}, &w0)); T.push_back(ref_of(s, TraceIn{o.tag.b, 0}, &w1)); if (w0 != W64 || w1 != W64) bad("ext inverse: wide operands"); }
                else { bad("h2w_gl_load_witness without h2w_trace_input"); break; }
                T.push_back(new_val(s, out[0], W64, false, 0)); add_rec(s, T_LOADW, o.cell0); want_cells = (uint64_t)tt.ncells(T_LOADW); break;
            }
            case TR_GL_REDUCE: {
                const uint32_t a = ref_of(s, in[0], &w0); if (w0 == W64) { bad("gl_reduce of a value that is not a gate output"); break; }
                if (ref_kind(a) != RK_LOCAL && ref_kind(a) != RK_IMPORT && ref_kind(a) != RK_RING) { bad("gl_reduce of a constant"); break; }
                head(DOP_REDUCE); T.push_back(a); T.push_back(new_val(s, out[0], W64, false, 0)); add_rec(s, T_REDUCE, o.cell0); want_cells = (uint64_t)tt.ncells(T_REDUCE); break;
            }
            case TR_GLOP: {
                const uint32_t a = ref_of(s, in[0], &w0), b = ref_of(s, in[1], &w1), c3 = ref_of(s, in[2], &w2);
                if (w0 != W64 || w1 != W64 || w2 != W64) { bad("a Goldilocks op on a wide value"); break; }
                if (o.sub == T_GLOP && !in[0].lit && S.last_const_at >= 0 && (size_t)S.last_const_at + 3 == T.size() && in[0].v == S.last_const_cell && S.last_const_cell + 1 == o.cell0 && ref_kind(a) == RK_LIT64) {
                    // load_constant(K) immediately followed by the op that takes it (GoldilocksChip's constant operands, e.g. hash/poseidon/permutation.rs:55-68): ONE record [K][C, A, B, V]...
                    op_at = (size_t)S.last_const_at; T.resize(op_at); meta.pop_back(); nrec--; S.nrecs--; ka_fused = true;
                    T.push_back(DOP_GLOP | ((uint32_t)T_KA_GLOP << 16)); T.push_back(a); T.push_back(b); T.push_back(c3); T.push_back(new_val(s, out[0], W64, false, 0)); add_rec(s, T_KA_GLOP, o.cell0 - 1);
                    S.last_const_at = -1; want_cells = (uint64_t)tt.ncells(T_GLOP); break;
                }
                head(DOP_GLOP, 0, o.sub); T.push_back(a); T.push_back(b); T.push_back(c3); T.push_back(new_val(s, out[0], W64, false, 0)); add_rec(s, o.sub, o.cell0); want_cells = (uint64_t)tt.ncells(o.sub); break;
            }
            default: bad("unknown op in the trace");
        }
        if (fz || !(o.code == TR_LOAD_CONSTANT && S.last_const_at == (long)op_at)) S.last_const_at = -1;
        if (T.size() > op_at) {
            if ((!S.mt.empty() || (capture && s == 0)) && err.empty()) {      // the op as lowered, its operands still as mkref words
                uint32_t first, count; operand_span(T[op_at] & 0xff, (T[op_at] >> 8) & 0xff, first, count);
                NormOp no; no.hdr = T[op_at] & 0xffffffu; no.nin = count <= 3 ? count : 0xffu; no.slots_before = slots_before;
                for (uint32_t k2 = 0; k2 < count && k2 < 3; k2++) { no.ref[k2] = T[op_at + first + k2]; if (ref_kind(no.ref[k2]) == RK_LIT64) no.lit[k2] = fr_from_u64(pool64[ref_idx(no.ref[k2])]); else if (ref_kind(no.ref[k2]) == RK_LITFR) no.lit[k2] = poolfr[ref_idx(no.ref[k2])]; }
                no.out = count <= 3 && op_at + first + count < T.size() ? T[op_at + first + count] : NO_SLOT;
                no.tr0 = ka_fused ? S.last_const_tr : i; no.tr1 = i + 1; no.cell0 = ka_fused ? o.cell0 - 1 : o.cell0; no.cell1 = o.cell0 + o.ncells; no.out_cell = o.n_out ? out[0] : 0; no.tin = in;
                if (!S.mt.empty()) { for (Matcher *m : S.mt) { if (ka_fused) m->drop_pending(); m->feed(no); } } else { if (ka_fused) capture->pop_back(); capture->push_back(no); }
            }
            const size_t len = T.size() - op_at; if (len > 255) bad("internal: op too long"); T[op_at] |= (uint32_t)len << 24;
            // operands: those in the lane's ring or in the LDS part of the pools become fast refs; the others are fetched into fresh ring slots by DOP_FETCH
            // ops in front of this one.  The ring holds the last RING_K slots WRITTEN, the temporaries included: decided against the slot count after them.
            uint32_t first, count; operand_span(T[op_at] & 0xff, (T[op_at] >> 8) & 0xff, first, count);
            auto in_lds = [&](uint32_t r, uint32_t nslots_final) {
                const int k = ref_kind(r); const uint32_t i = ref_idx(r);
                if (k == RK_LOCAL) return (uint64_t)i + RING_K >= (uint64_t)nslots_final;
                if (k == RK_LIT64) return i + 1 <= POOL64_CAP;
                if (k == RK_LITFR) return i + 1 <= POOLFR_CAP;
                return false;
            };
            auto words_of = [&](uint32_t r) { const int k = ref_kind(r); return (uint32_t)(k == RK_LITFR ? 4 : k == RK_INPUT ? (ref_width(r) == WFR ? 4 : 1) : SLOTS_OF[ref_width(r)]); };
            uint32_t temps = 0;
            for (;;) { uint32_t need = 0; for (uint32_t k2 = 0; k2 < count; k2++) { const uint32_t r = T[op_at + first + k2]; if (!in_lds(r, S.nslots + temps)) need += words_of(r); } if (need == temps) break; temps = need; }
            std::vector<uint32_t> fetches; const uint32_t nf = S.nslots + temps; uint32_t tslot = S.nslots;
            for (uint32_t k2 = 0; k2 < count; k2++) {
                const uint32_t r = T[op_at + first + k2]; const int k = ref_kind(r), w = ref_width(r); uint32_t fr2;
                if (in_lds(r, nf)) fr2 = k == RK_LOCAL ? fastref_ring(w, ref_idx(r)) : k == RK_LIT64 ? fastref_pool(W64, LDS_POOL64 + ref_idx(r) * 8) : fastref_pool(WFR, LDS_POOLFR + ref_idx(r) * 32);
                else {
                    const uint32_t nw = words_of(r);
                    fetches.push_back(DOP_FETCH | (nw << 8) | (3u << 24)); fetches.push_back(r); fetches.push_back(tslot);
                    fr2 = fastref_ring(nw == 4 ? WFR : nw == 2 ? W128 : W64, tslot); tslot += nw;
                }
                T[op_at + first + k2] = fr2;
            }
            S.nslots = nf;
            if (!fetches.empty()) { T.insert(T.begin() + (long)op_at, fetches.begin(), fetches.end()); if (S.last_const_at == (long)op_at) S.last_const_at += (long)fetches.size(); }
        }
        if (err.empty() && want_cells != o.ncells) bad("internal: op " + std::to_string(o.code) + " appended " + std::to_string(o.ncells) + " cells on the host, the device template has " + std::to_string(want_cells));
    }
    for (Matcher &m : matchers) m.commit();
    for (SegInfo &S : segs) S.mt.clear();
    if (!err.empty()) return;
    segs[0].tape.push_back(DOP_END | (1u << 24)); segs[0].cell0 = 0; segs[0].rec0 = 0;
}

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
    Lowered LW; std::vector<NormOp> ops;
    lower_trace(tr, L, tt, nullptr, 0, LW, nullptr, nullptr, nullptr, nullptr, &ops);
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

static h2w_plan *plan_from_trace(h2w_ctx *ctx, uint64_t proof_words, const char *const *parallel_scopes, size_t n_scopes, int device_id, const h2w_poseidon_consts_t *consts, uint32_t flags) {
    Trace *tr = ctx_trace(ctx);
    if (!tr) { set_error("h2w_plan_from_trace: the context is not in trace mode (h2w_ctx_trace_begin)"); return nullptr; }
    if (!tr->err.empty()) { set_error("h2w_plan_from_trace: " + tr->err); return nullptr; }
    if (tr->pending.kind) { set_error("h2w_plan_from_trace: a h2w_trace_input tag was never consumed"); return nullptr; }
    const bool fusing = (flags & H2W_TRACE_FUSE_GL_PERMUTE) != 0, fusing_bn = (flags & H2W_TRACE_FUSE_BN_PERMUTE) != 0;
    if (flags & ~(uint32_t)(H2W_TRACE_FUSE_GL_PERMUTE | H2W_TRACE_FUSE_BN_PERMUTE)) { set_error("h2w_plan_from_trace_ex: unknown flag"); return nullptr; }
    if (fusing && !consts) { set_error("h2w_plan_from_trace_ex: H2W_TRACE_FUSE_GL_PERMUTE needs the Poseidon tables the permutations are claimed to use"); return nullptr; }
    if (fusing_bn && !consts) { set_error("h2w_plan_from_trace_ex: H2W_TRACE_FUSE_BN_PERMUTE needs the Poseidon tables the permutations are claimed to use"); return nullptr; }
    const int L = ctx_lookup_bits(ctx);
    TemplateTable tt(L);
    Lowered LW; std::map<size_t, Stretch> fuse; std::vector<uint64_t> glp_meta; uint64_t n_candidates = 0, glp_block_cells = 0, n_bn_left = 0;
    if (fusing || fusing_bn) {
        // the stretches that equal a canonical tape word for word, found on a first lowering; those nothing outside reads into are lowered as one op
        Canon cn, cnb, cnz; std::string cerr; std::vector<Stretch> found; std::vector<const Canon *> cns;
        uint64_t block_cells = 0;
        if (fusing) {
            if (!canonical_tape(CANON_GL, L, tt, consts, cn, cerr)) { set_error("h2w_plan_from_trace_ex: " + cerr); return nullptr; }
            block_cells = glp_block_cells = glp_block_layout(tt, L, consts, glp_meta);
            if (block_cells == 0 || block_cells != cn.ncells) { set_error("h2w_plan_from_trace_ex: the record block of a permutation (" + std::to_string(block_cells) + " cells) is not the traced one (" + std::to_string(cn.ncells) + " cells)"); return nullptr; }
            cns.push_back(&cn);
        }
        if (fusing_bn) {
            if (!canonical_tape(CANON_BN, L, tt, consts, cnb, cerr) || !canonical_tape(CANON_BN_ZERO, L, tt, consts, cnz, cerr)) { set_error("h2w_plan_from_trace_ex: " + cerr); return nullptr; }
            if (cnb.ncells != (uint64_t)BN_PERM_CELLS || cnz.ncells != (uint64_t)BN_PERM_CELLS + 1) { set_error("h2w_plan_from_trace_ex: a PoseidonBN254 permutation has " + std::to_string(cnb.ncells) + " traced cells, the emission kernel writes " + std::to_string(BN_PERM_CELLS)); return nullptr; }
            cns.push_back(&cnb); cns.push_back(&cnz);
        }
        { Lowered first; lower_trace(tr, L, tt, parallel_scopes, n_scopes, first, nullptr, nullptr, &cns, &found, nullptr); if (!first.err.empty()) { set_error("h2w_plan_from_trace: " + first.err); return nullptr; } }
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
            if (x.canon == CANON_GL) {
                if (x.cell1 - x.cell0 != block_cells) { set_error("h2w_plan_from_trace_ex: a permutation's stretch has " + std::to_string(x.cell1 - x.cell0) + " traced cells, its record block " + std::to_string(block_cells)); return nullptr; }
                if (x.const_bad || x.escaped) n_candidates++; else fuse.emplace(x.tr0, x);
            } else if (x.canon == CANON_BN) {
                if (x.cell1 - x.cell0 != (uint64_t)BN_PERM_CELLS) { set_error("h2w_plan_from_trace_ex: a PoseidonBN254 permutation's stretch has " + std::to_string(x.cell1 - x.cell0) + " traced cells, the emission kernel writes " + std::to_string(BN_PERM_CELLS)); return nullptr; }
                if (x.const_bad || x.escaped) n_bn_left++; else fuse.emplace(x.tr0, x);
            } else {      // the permutation that holds the Context's load_zero cell (every later mix of the run reads it): recognised, left interpreted
                n_bn_left++; if (!x.const_bad) n_zero++;
            }
        }
        if (n_zero > 1) { set_error("h2w_plan_from_trace_ex: internal: more than one PoseidonBN254 permutation with the load_zero cell"); return nullptr; }
    }
    lower_trace(tr, L, tt, parallel_scopes, n_scopes, LW, fuse.empty() ? nullptr : &fuse, &glp_meta, nullptr, nullptr, nullptr);
    std::string &err = LW.err;
    auto bad = [&](const std::string &m) { if (err.empty()) err = m; };
    if (!err.empty()) { set_error("h2w_plan_from_trace: " + err); return nullptr; }
    std::vector<SegInfo> &segs = LW.segs; std::vector<uint64_t> &meta = LW.meta; const uint64_t nrec = LW.nrec;
    std::vector<uint64_t> &pool64 = LW.pool64; std::vector<fr_t> &poolfr = LW.poolfr;
    // ---- shard units: the depth-1 instances in tape order (unit q: the q-th; "verify_query_round" instance q of the standard trace, where the
    // compiled plan's query block q starts: AbiBackend::query_begin).  Shardable: the root's block [0, unit 0) and the units back to back to the end
    // of the stream and of the records, units 1.. all of one size (the compiled plan's StrandTable: query 0, a later query).
    std::vector<int> units;
    for (size_t si = 1; si < segs.size(); si++) {      // (a segment comes after its parent)
        SegInfo &S = segs[si];
        if (S.depth == 1) { S.unit = (uint32_t)units.size(); units.push_back((int)si); }
        else S.unit = segs[(size_t)S.parent].unit;
    }
    std::string why_unshardable;
    {
        uint64_t c = units.empty() ? 0 : segs[(size_t)units[0]].cell0, r = units.empty() ? 0 : segs[(size_t)units[0]].rec0;
        for (size_t q = 0; q < units.size() && why_unshardable.empty(); q++) {
            const SegInfo &U = segs[(size_t)units[q]], &U1 = segs[(size_t)units[q > 1 ? 1 : q]];
            if (U.cell0 != c || U.rec0 != r) why_unshardable = "the root has cells or records between parallel instances " + std::to_string(q ? q - 1 : 0) + " and " + std::to_string(q) + " at depth 1";
            else if (U.ncells != U1.ncells || U.all_recs != U1.all_recs) why_unshardable = "the parallel instances at depth 1 differ in size (instance " + std::to_string(q) + ")";
            c += U.ncells; r += U.all_recs;
        }
        if (units.empty()) why_unshardable = "no parallel scope instance at depth 1 (trace the query rounds as parallel: \"verify_query_round\")";
        else if (why_unshardable.empty() && (c != ctx_num_cells(ctx) || r != nrec)) why_unshardable = "the root has cells or records after the last parallel instance at depth 1";
        if (!why_unshardable.empty()) why_unshardable = "the traced plan is not shardable: " + why_unshardable;
    }
    // ---- consecutive Goldilocks-level ops -> runs (DOP_GLOPRUN)
    for (SegInfo &S : segs) {
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
    // ---- templates: isomorphic instances (equal tapes, slot counts, table sizes) share one
    TracedPlan *tp = new TracedPlan();
    std::vector<uint32_t> tape_all; std::vector<InstD> insts; std::vector<ImpD> imps; std::vector<uint32_t> inputs;
    std::vector<std::vector<int>> members;
    {
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
        if (members.size() > (size_t)MAX_TMPL) { set_error("h2w_plan_from_trace: more than " + std::to_string(MAX_TMPL) + " distinct scope shapes"); delete tp; return nullptr; }
        for (size_t t = 0; t < members.size(); t++) {
            const SegInfo &M = segs[(size_t)members[t][0]];
            TmplD T; T.tape0 = (uint32_t)tape_all.size(); T.nslots = M.nslots ? M.nslots : 1; T.ninst = (uint32_t)members[t].size(); T.inst0 = (uint32_t)insts.size(); T.depth = (uint32_t)M.depth;
            tape_all.insert(tape_all.end(), M.tape.begin(), M.tape.end());
            for (int si : members[t]) {
                const SegInfo &S = segs[(size_t)si];
                InstD I; I.cell0 = S.cell0; I.rec0 = S.rec0; I.imp0 = (uint32_t)imps.size(); I.in0 = (uint32_t)inputs.size();
                I.unit = S.unit; I.ucell0 = S.unit == NO_SLOT ? 0 : segs[(size_t)units[S.unit]].cell0; tp->h_unit.push_back(S.unit);
                I.glp0 = tp->nglp; tp->nglp += S.nglp; tp->h_glp_unit.insert(tp->h_glp_unit.end(), S.nglp, S.unit);
                tp->h_bnp0.push_back(tp->nbnp); tp->nbnp += S.nbnp; for (uint64_t c0 : S.bnp_cells) tp->h_bnp.push_back(BnpD{c0, I.ucell0, S.unit, 0});
                for (const ImpD &m : S.imps) { const SegInfo &Pn = segs[(size_t)m.tmpl]; imps.push_back(ImpD{(uint32_t)Pn.tmpl, Pn.inst, m.slot}); }
                inputs.insert(inputs.end(), S.inputs.begin(), S.inputs.end());
                insts.push_back(I);
            }
            tp->tmpls.push_back(T); tp->total_slot_lanes += (uint64_t)T.nslots * T.ninst;
        }
    }
    // ---- every word the device will follow, checked here: op lengths, operand kinds and indices, result slots (a wild reference is a GPU fault)
    for (size_t t = 0; t < members.size() && err.empty(); t++) {
        const SegInfo &M = segs[(size_t)members[t][0]]; const std::vector<uint32_t> &T = M.tape; size_t pc = 0; bool ended = false;
        auto okslow = [&](uint32_t r) {      // the old-style ref a DOP_FETCH carries
            const uint32_t i = ref_idx(r); const int k = ref_kind(r), w = ref_width(r);
            if (w > WFR) return false;
            const uint32_t span = k == RK_LITFR ? 4u : (uint32_t)(k == RK_INPUT ? (w == WFR ? 4 : 1) : SLOTS_OF[w]);
            switch (k) {
                case RK_LOCAL: return (uint64_t)i + span <= M.nslots;
                case RK_IMPORT: return i < M.imps.size();
                case RK_LIT64: return (uint64_t)i + span <= pool64.size();
                case RK_INPUT: return i < M.inputs.size() && (uint64_t)M.inputs[i] + span <= proof_words;
                case RK_LITFR: return i < poolfr.size();
                default: return false;
            }
        };
        auto okref = [&](uint32_t r, int) {      // a fast ref
            if (r & 0x60000000u) return false;
            const uint32_t w = (r >> 27) & 3u; if (w > WFR) return false;
            if (r >> 31) return (r & 0x07ffff00u) == 0;
            const uint32_t off = r & 0x07ffffffu, span = w == WFR ? 32u : w == W128 ? 16u : 8u;
            return (off & 7u) == 0 && ((off >= LDS_POOL64 && off + span <= LDS_POOL64 + (uint32_t)std::min<size_t>(pool64.size(), POOL64_CAP) * 8) || (off >= LDS_POOLFR && off + span <= LDS_POOLFR + (uint32_t)std::min<size_t>(poolfr.size(), POOLFR_CAP) * 32));
        };
        auto okout = [&](uint32_t slot, uint32_t nsl) { return slot == NO_SLOT || (uint64_t)slot + nsl <= M.nslots; };
        while (pc < T.size()) {
            const uint32_t h = T[pc], op = h & 0xff, n = (h >> 8) & 0xff, len = op == DOP_GLOPRUN ? 2 + 4 * n : h >> 24; bool ok = len >= 1 && pc + len <= T.size();
            if (op == DOP_END) { ended = ok && pc + 1 == T.size(); break; }
            auto R_ = [&](size_t k2) { return T[pc + k2]; };
            if (ok) switch (op) {
                case DOP_SKIP: ok = len == 5; break;
                case DOP_GLOPRUN: ok = n >= 2; for (uint32_t k2 = 0; ok && k2 < n; k2++) ok = okref(R_(2 + 4 * k2), 1) && okref(R_(3 + 4 * k2), 1) && okref(R_(4 + 4 * k2), 1) && (uint64_t)(R_(5 + 4 * k2) & 0xffffffu) + 1 <= M.nslots && (R_(5 + 4 * k2) >> 24) < T_DYNAMIC; break;
                case DOP_GLPERM: ok = len == GLPERM_WORDS && fusing && glp_meta.size() == (size_t)GLP_RECS && okout(R_(13), SPONGE_WIDTH) && R_(13) != NO_SLOT && R_(14) < M.nglp && R_(15) == (uint32_t)glp_block_cells;
                                 for (uint32_t k2 = 0; ok && k2 < (uint32_t)SPONGE_WIDTH; k2++) ok = okref(R_(1 + k2), 1) && ((R_(1 + k2) >> 27) & 3u) == W64; break;
                case DOP_BNPERM: ok = len == BNPERM_WORDS && fusing_bn && okout(R_(5), 4 * BN_WIDTH) && R_(5) != NO_SLOT && R_(6) < M.nbnp && R_(7) == (uint32_t)BN_PERM_CELLS;
                                 for (uint32_t k2 = 0; ok && k2 < (uint32_t)BN_WIDTH; k2++) ok = okref(R_(1 + k2), 4); break;
                case DOP_FETCH: ok = len == 3 && n >= 1 && n <= 4 && okslow(R_(1)) && (uint64_t)R_(2) + n <= M.nslots; break;
                case DOP_CONST1: case DOP_LOADW: ok = len == 3 && okref(R_(1), 1) && okout(R_(2), 1); break;
                case DOP_FRCELL: ok = len == 3 && okref(R_(1), 4) && okout(R_(2), 4); break;
                case DOP_LOADW_DIV: case DOP_LOADW_EXTINV: ok = len == 4 && okref(R_(1), 1) && okref(R_(2), 1) && okout(R_(3), 1); break;
                case DOP_GLOP: ok = len == 5 && okref(R_(1), 1) && okref(R_(2), 1) && okref(R_(3), 1) && okout(R_(4), 1) && ((h >> 16) & 0xff) < T_DYNAMIC; break;
                case DOP_GATE: ok = len == 5 && okref(R_(1), 1) && okref(R_(2), 1) && okref(R_(3), 1) && okout(R_(4), 2); break;
                case DOP_REDUCE: ok = len == 3 && okref(R_(1), 2) && ((R_(1) >> 27) & 3u) != W64 && okout(R_(2), 1); break;
                case DOP_CLT: case DOP_RANGE: ok = len == 2 && okref(R_(1), 1); break;
                case DOP_FR_ADD: case DOP_FR_MUL: ok = len == 4 && okref(R_(1), 4) && okref(R_(2), 4) && okout(R_(3), 4); break;
                case DOP_FR_MULADD: ok = len == 5 && okref(R_(1), 4) && okref(R_(2), 4) && okref(R_(3), 4) && okout(R_(4), 4); break;
                case DOP_SELECT: ok = len == 5 && okref(R_(1), 1) && okref(R_(2), 1) && okref(R_(3), 1) && okout(R_(4), 1); break;
                case DOP_FR_SELECT: ok = len == 5 && okref(R_(1), 4) && okref(R_(2), 4) && okref(R_(3), 1) && okout(R_(4), 4); break;
                case DOP_IDX2IND: case DOP_NUM2BITS: ok = len == 3 && n >= 1 && n <= 64 && okref(R_(1), 1) && okout(R_(2), n); break;
                case DOP_DECOMP565: ok = len == 3 && okref(R_(1), 4) && okout(R_(2), 5); break;
                case DOP_SELIND: case DOP_FR_SELIND: ok = len == 2 + 2 * n && n >= 1 && n <= 64; for (uint32_t k2 = 0; ok && k2 < 2 * n; k2++) ok = okref(R_(1 + k2), 4); ok = ok && okout(R_(1 + 2 * n), op == DOP_SELIND ? 1 : 4); break;
                case DOP_BITS2NUM: case DOP_LIMBS2NUM: ok = len == 2 + n && n <= 64; for (uint32_t k2 = 0; ok && k2 < n; k2++) ok = okref(R_(1 + k2), 1); ok = ok && okout(R_(1 + n), op == DOP_BITS2NUM ? 1 : 4); break;
                default: ok = false;
            }
            if (!ok) { bad("internal: malformed device tape (template " + std::to_string(t) + ", word " + std::to_string(pc) + ", op " + std::to_string(op) + ")"); break; }
            pc += len;
        }
        if (err.empty() && !ended) bad("internal: a device tape does not end");
    }
    if (!err.empty()) { set_error("h2w_plan_from_trace: " + err); delete tp; return nullptr; }
    for (uint32_t w : inputs) if (w >= proof_words) { set_error("h2w_plan_from_trace: an input tag beyond proof_words"); delete tp; return nullptr; }
    tp->n_ops = tr->ops.size(); tp->n_segments = segs.size(); tp->why_unshardable = why_unshardable; tp->n_candidates = n_candidates;
    tp->bn_flag = fusing_bn; tp->n_bn_left = n_bn_left;
    for (const BnpD &b : tp->h_bnp) if (b.cell0 + (uint64_t)BN_PERM_CELLS > ctx_num_cells(ctx)) { set_error("h2w_plan_from_trace_ex: internal: a fused permutation's cells lie beyond the stream"); delete tp; return nullptr; }

    // ---- the plan handle
    h2w_plan *pl = new h2w_plan(L);
    memset(&pl->shape, 0, sizeof(pl->shape)); pl->shape.lookup_bits = L; pl->shape.num_queries = 1; pl->shape.hash_mode = 1;
    pl->device = device_id; pl->P = fr_params_init(); memset(&pl->st, 0, sizeof(pl->st)); memset(&pl->pl, 0, sizeof(pl->pl)); memset(&pl->d, 0, sizeof(pl->d));
    pl->pl.total = proof_words; pl->nrec = nrec; pl->ncells = ctx_num_cells(ctx); pl->traced = tp;
    if (consts) pl->h_consts = *consts;
    for (uint64_t m : meta) pl->rec_cells += (uint64_t)pl->tt.ncells((int)meta_tmpl(m));
    // the block structure (StrandTable: what h2w_plan_strand_layout / _shard_cells / _shard_block and the sharded expansion read): unshardable, one block
    StrandTable &st = pl->st; st.first_zero_kind = -1; st.first_zero_unit = -1; st.total_rec = nrec; st.total_cell = pl->ncells;
    if (why_unshardable.empty()) {
        const SegInfo &U0 = segs[(size_t)units[0]], &U1 = segs[(size_t)units[units.size() > 1 ? 1 : 0]];
        pl->shape.num_queries = (uint32_t)units.size();
        st.pro_ncell = U0.cell0; st.pro_nrec = U0.rec0;
        st.q_cell0[0] = U0.cell0; st.q_rec0[0] = U0.rec0; st.q_ncell[0] = U0.ncells; st.q_nrec[0] = U0.all_recs;
        st.q_cell0[1] = U1.cell0; st.q_rec0[1] = U1.rec0; st.q_ncell[1] = U1.ncells; st.q_nrec[1] = U1.all_recs;
    } else { st.pro_ncell = pl->ncells; st.pro_nrec = nrec; }
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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { pl->device = -1; return pl; }      // layout queries only
    if (device_id < 0 || device_id >= ndev) { set_error("h2w_plan_from_trace: device_id out of range"); h2w_plan_free(pl); return nullptr; }
    DeviceGuard dg(device_id);
    auto up = [&]() -> int {
        if (pl->dt.upload(pl->tt) != 0) return -1;
        auto put = [&](void **d, const void *h, size_t bytes) -> int { H2W_HIP(hipMalloc(d, bytes ? bytes : 8)); if (bytes) H2W_HIP(hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice)); return 0; };
        if (put((void **)&pl->d_meta, meta.data(), meta.size() * 8) != 0) return -1;
        for (int k2 = 0; k2 < 16; k2++) tape_all.push_back(DOP_END | (1u << 24));      // the interpreter reads a window ahead
        if (put((void **)&tp->d_tape, tape_all.data(), tape_all.size() * 4) != 0) return -1;
        std::vector<uint64_t> prefix(tp->tmpls.size()); uint64_t acc = 0;
        for (size_t i = 0; i < tp->tmpls.size(); i++) { prefix[i] = acc; acc += (uint64_t)tp->tmpls[i].nslots * tp->tmpls[i].ninst; }
        if (put((void **)&tp->d_tm, tp->tmpls.data(), tp->tmpls.size() * sizeof(TmplD)) != 0) return -1;
        if (put((void **)&tp->d_prefix, prefix.data(), prefix.size() * 8) != 0) return -1;
        if (put((void **)&tp->d_insts, insts.data(), insts.size() * sizeof(InstD)) != 0) return -1;
        if (put((void **)&tp->d_imps, imps.data(), imps.size() * sizeof(ImpD)) != 0) return -1;
        if (put((void **)&tp->d_inputs, inputs.data(), inputs.size() * 4) != 0) return -1;
        tp->npool64 = (uint32_t)pool64.size(); tp->npoolfr = (uint32_t)poolfr.size();
        if (put((void **)&tp->d_pool64, pool64.data(), pool64.size() * 8) != 0) return -1;
        if (put((void **)&tp->d_poolfr, poolfr.data(), poolfr.size() * sizeof(fr_t)) != 0) return -1;
        std::vector<uint16_t> nc(T_MAX, 0); for (size_t i = 0; i < pl->tt.info.size(); i++) nc[i] = pl->tt.info[i].ncells;
        if (put((void **)&pl->d_ncells, nc.data(), nc.size() * 2) != 0) return -1;
        std::vector<fr_t> inv(2 * INV_TAB, fr_zero());
        for (int k2 = 1; k2 < INV_TAB; k2++) { inv[k2] = fr_inv(fr_from_u64((uint64_t)k2), pl->P); inv[INV_TAB + k2] = fr_neg(inv[k2]); }
        if (put((void **)&pl->d_inv, inv.data(), inv.size() * sizeof(fr_t)) != 0) return -1;
        if (tp->nglp) {      // the tables the fused permutations were verified on, the derived tables behind them (as h2w_plan_compile builds a compiled plan's)
            std::vector<uint64_t> aux(GLP_AUX_WORDS); glp_aux_tables(*consts, aux.data());
            H2W_HIP(hipMalloc((void **)&pl->d_consts, sizeof(h2w_poseidon_consts_t) + aux.size() * sizeof(uint64_t)));
            H2W_HIP(hipMemcpy(pl->d_consts, consts, sizeof(h2w_poseidon_consts_t), hipMemcpyHostToDevice));
            H2W_HIP(hipMemcpy(pl->d_consts + 1, aux.data(), aux.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
            if (put((void **)&tp->d_glp_unit, tp->h_glp_unit.data(), tp->h_glp_unit.size() * 4) != 0) return -1;
        }
        if (tp->nbnp) {      // the PoseidonBN254 tables, canonical and times R (as h2w_plan_compile builds a compiled plan's); where every listed permutation lies
            std::vector<fr_t> tab(BK_ALL); bn_table_build(*consts, pl->P, tab.data());
            if (put((void **)&pl->d_bn_tab, tab.data(), tab.size() * sizeof(fr_t)) != 0) return -1;
            if (put((void **)&tp->d_bnp, tp->h_bnp.data(), tp->h_bnp.size() * sizeof(BnpD)) != 0) return -1;
            if (put((void **)&tp->d_bnp0, tp->h_bnp0.data(), tp->h_bnp0.size() * 4) != 0) return -1;
        }
        return 0;
    };
    if (up() != 0) { h2w_plan_free(pl); return nullptr; }
    return pl;
}

extern "C" h2w_plan *h2w_plan_from_trace(h2w_ctx *ctx, uint64_t proof_words, const char *const *parallel_scopes, size_t n_scopes, int device_id) {
    return plan_from_trace(ctx, proof_words, parallel_scopes, n_scopes, device_id, nullptr, 0);
}
extern "C" h2w_plan *h2w_plan_from_trace_ex(h2w_ctx *ctx, uint64_t proof_words, const char *const *parallel_scopes, size_t n_scopes, int device_id, const h2w_poseidon_consts_t *consts, uint32_t flags) {
    return plan_from_trace(ctx, proof_words, parallel_scopes, n_scopes, device_id, consts, flags);
}
extern "C" int h2w_plan_trace_info(const h2w_plan *p, uint64_t out[6]) {
    if (!p || !out) { set_error("h2w_plan_trace_info: null argument"); return -1; }
    if (!p->traced) { set_error("h2w_plan_trace_info: not a traced plan (h2w_plan_from_trace)"); return -1; }
    const TracedPlan *t = p->traced;
    out[0] = t->n_ops; out[1] = t->n_segments; out[2] = t->tmpls.size(); out[3] = t->nglp; out[4] = t->n_candidates; out[5] = t->nglp;
    return 0;
}
extern "C" int h2w_plan_trace_info_bn(const h2w_plan *p, uint64_t out[3]) {
    if (!p || !out) { set_error("h2w_plan_trace_info_bn: null argument"); return -1; }
    if (!p->traced) { set_error("h2w_plan_trace_info_bn: not a traced plan (h2w_plan_from_trace)"); return -1; }
    const TracedPlan *t = p->traced;
    out[0] = t->nbnp; out[1] = t->n_bn_left; out[2] = t->nbnp;
    return 0;
}
// ms of the kernels of the last call: the k_replay launch of every depth, k_glp_emit_traced, (plans built with H2W_TRACE_FUSE_BN_PERMUTE) k_bn_emit_traced, the expansion.  The first call switches the events on
// (0 entries); later ones wait for the last call and report it.
extern "C" int h2w_plan_trace_timing(h2w_plan *p, float *ms, uint32_t cap) {
    if (!p || !ms) { set_error("h2w_plan_trace_timing: null argument"); return -1; }
    if (!p->traced || p->device < 0) { set_error("h2w_plan_trace_timing: not a traced plan on a device"); return -1; }
    TracedPlan *t = p->traced; DeviceGuard dg(p->device);
    if (!t->timing) { for (; t->n_tev < 16; t->n_tev++) H2W_HIP(hipEventCreate(&t->tev[t->n_tev])); t->timing = true; return 0; }
    if (t->tev_used < 2) return 0;
    H2W_HIP(hipEventSynchronize(t->tev[t->tev_used - 1]));
    int n = 0;
    for (int i = 0; i + 1 < t->tev_used && (uint32_t)n < cap; i++, n++) H2W_HIP(hipEventElapsedTime(&ms[n], t->tev[i], t->tev[i + 1]));
    return n;
}
