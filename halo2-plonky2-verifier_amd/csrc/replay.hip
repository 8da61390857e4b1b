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
        // (shardmap.h packed_block_start, written out: the call moves the interpreter loop below by three instructions, and the root lane of an unfused plan measured 1.5 % slower: profiles/replay_split_bench.json.  The packed tests hold this copy to h2w_plan_shard_block, which calls the function)
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
        // Every case reads ALL its operands (into registers, ta / tb) before its first st1 / putfr: the lowering lets an op's result slots alias the ring
        // slots of its fetched operands (tracelower.cpp bounds the fetched slots alone by RING_K; tape_check the same).  A case that stores before its last read breaks that.
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
            case DOP_LIMBS2NUM: { for (uint32_t i = 0; i < n; i++) ta[i] = get64(tw(tape, pc + 1 + i), 0); putfr(tw(tape, pc + 1 + n), n == 4 ? be.limbs_to_num4(ta) : be.limbs_to_num(ta, (int)n)); break; }
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
            hipLaunchKernelGGL(k_replay<true>, dim3(nb), dim3(64), 0, stream, RB);
        } else if (nb) hipLaunchKernelGGL(k_replay<false>, dim3(nb), dim3(64), 0, stream, R);
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
