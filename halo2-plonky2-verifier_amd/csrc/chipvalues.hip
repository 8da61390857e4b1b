// chipvalues.hip - the batched hash and Merkle chip ops on VALUES (include/h2w.h 2c): h2w_chipbatch_values, h2w_chipbatch_num_results.
//
// h2w_chipbatch_run (chiphash.hip) can only produce an instance's whole advice stream.  Two things a caller wants first are not in it: what the op
// computed - the permutation's output state, the digest - and whether a Merkle opening holds: the root check is an assert_equal, which writes no
// cells.  This unit runs the same program (chiphash.h hash_program) on sinks that keep nothing but the comparisons (valbackend.h SinkBase compare),
// what verdict.hip does for whole proofs; the program hands its output wires to the kernel, and the lane that speaks for the instance stores them.
//   k_chipvalues_gl    Goldilocks-Poseidon (hash_mode 0, GL_PERMUTE): one wavefront per instance walks the op wave-uniformly on glcoop.h
//                      CoopSinkT<false, true, 0> with emit = false - no list entry, no record -, permutations on glp_permute_lanes; lane 0 speaks
//   k_chipvalues_bn    PoseidonBN254 (hash_mode 1, BN_PERMUTE): four lanes per instance on the lazy nine-limb walk (bnquad.h QuadSinkT bn_values,
//                      QUAD_VERDICT); tail quads redo the last instance and keep silent; lane 0 of the quad speaks
//   k_chipvalues_row   PoseidonBN254, H2W_CHIPBATCH_FORM_ROW: one wavefront per instance, the four rows of the wavefront = the four state elements
//                      (rowfr.h; rowperm.h bn_permute_rows<false>); lane 0 speaks
// The only global stores of these kernels are the result words and the verdict's n_failed word, one strand per instance: plain stores, no atomics.
// The status word is k_chiphash_check's (chiphash.hip), the one place that decides status 4.  The walks are lazy; a permutation's output state leaves
// them canonical (bn_values: S / R < r + 1 and one conditional subtraction; rowperm.h gather_canonical), and a result word is such a value or an
// operand-derived Goldilocks value of the canonical arithmetic - nothing is stored that was not reduced below its modulus.
// Flattened like chiphash.hip: the sinks below exist in this unit alone (field.h HNI).
#define H2W_FLATTEN_CHIPS 1
#include <hip/hip_runtime.h>
#include <string>
#include "chiphash.h"
#define RF_TAB9 s_bn_tab9
#include "rowperm.h"

namespace h2w {

static_assert(sizeof(h2w_chipbatch_verdict_t) == 8, "two words per instance");

// a sink of this unit: Base's walk on values with no record, no cell and no cursor - the failing comparisons alone, counted in a register
template <class Base> struct ValuesSinkT : Base {
    uint32_t n_failed = 0;
    __device__ __forceinline__ void rec(int, uint64_t, uint64_t, uint64_t, uint64_t) {}
    __device__ __forceinline__ void cell(const fr_t &) {}
    __device__ __forceinline__ void skip(uint64_t, uint64_t) {}
    __device__ __forceinline__ void compare(bool differ) { n_failed += differ ? 1u : 0u; }
};
// one wavefront per instance, every lane on the same values (verdict.hip VerdictRowBase): the permutation stores nothing, the cap lookup's value is taken
struct ValuesRowBase : SinkBase {
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
typedef ValuesSinkT<CoopSinkT<false, true, 0>> ValuesCoopSink;      // (emit = false: no list entry; rec / cell hidden: no cursor either)
typedef ValuesSinkT<QuadSinkT<false, QUAD_VERDICT>> ValuesQuadSink;
typedef ValuesSinkT<ValuesRowBase> ValuesRowSink;

struct ValuesArgs {
    HashParams hp; int L; FrParams P; const uint64_t *operands; uint32_t nw, nres; uint64_t n; uint64_t *results; h2w_chipbatch_verdict_t *verdict;
    const uint16_t *tmpl_cells; const fr_t *inv;
    const h2w_poseidon_consts_t *consts; int small_mds;      // Goldilocks-Poseidon: the constants (+ derived tables)
    const uint32_t *bn_tab9; const rf::RowConst *rowk;       // PoseidonBN254: the limb-form tables (bntab.h), the row form's constants (rowfr.h)
};

// hash_program's output wires -> the instance's result words, by the lane that speaks (the values are the same on every lane of the strand)
struct ResultOut {
    uint64_t *res; bool on;
    __device__ __forceinline__ void gl(const uint64_t *v, int n) const {
        if (!on) return;
        unsigned long long *q = reinterpret_cast<unsigned long long *>(res);
        for (int i = 0; i < n; i++) H2W_GSTORE64(q + i, v[i]);
    }
    __device__ __forceinline__ void fr(const fr_t *v, int n) const {
        if (!on) return;
        for (int i = 0; i < n; i++) g_store_fr(reinterpret_cast<fr_t *>(res) + i, v[i]);
    }
};
__device__ __forceinline__ void store_n_failed(const ValuesArgs &A, uint64_t i, uint32_t n_failed) { A.verdict[i].n_failed = n_failed; }

// LDS: the Goldilocks-Poseidon constants and derived tables.  The grid is the instances of the call
__global__ __launch_bounds__(64) __attribute__((flatten)) void k_chipvalues_gl(ValuesArgs A) {
    typedef ValBackend<ValuesCoopSink> CoopB;
    stage_glp_consts<true>(A.consts, threadIdx.x, 64);
    const uint64_t i = blockIdx.x;
    ValuesCoopSink sink; sink.recs = nullptr; sink.out = nullptr; sink.ncells = A.tmpl_cells; sink.lane = threadIdx.x; sink.cc.init(flat_cols());
    sink.glp = nullptr; sink.small_mds = A.small_mds != 0; sink.bind_lds();
    sink.nrec = 0; sink.cell_off = 0; sink.glp_slot = 0; sink.emit = false;
    CoopB be(sink, chiphash_cfg(0, A.L, A.P, A.inv, false), false);
    const HashParams hp = A.hp;
    const bool speaks = threadIdx.x == 0;      // wave-uniform values: lane 0 speaks
    hash_program<0>(be, hp, A.consts, A.operands + i * (uint64_t)A.nw, ResultOut{A.results + i * (uint64_t)A.nres, speaks});
    if (speaks) store_n_failed(A, i, sink.n_failed);
}

// LDS: the nine-limb tables alone.  The quads of a wavefront run in lockstep: no wavefront leaves early, tail quads redo the last instance and keep silent
__global__ __launch_bounds__(QUAD_BLOCK) __attribute__((flatten)) void k_chipvalues_bn(ValuesArgs A) {
    typedef ValBackend<ValuesQuadSink> QuadB;
    stage_bn_consts9(A.bn_tab9, threadIdx.x, QUAD_BLOCK);      // (block-wide barrier inside: before any wavefront leaves)
    if ((((uint64_t)blockIdx.x * QUAD_BLOCK + (threadIdx.x & ~63u)) >> 2) >= A.n) return;      // a whole wavefront past the last instance
    uint64_t i = ((uint64_t)blockIdx.x * QUAD_BLOCK + threadIdx.x) >> 2;
    const bool tail = i >= A.n;
    if (tail) i = A.n - 1;
    ValuesQuadSink sink; sink.recs = nullptr; sink.nrec = 0; sink.out = nullptr; sink.cell_off = 0; sink.ncells = nullptr; sink.l4 = threadIdx.x & 3; sink.ustate = nullptr; sink.sbx = nullptr;
    QuadB be(sink, chiphash_cfg(1, A.L, A.P, A.inv, true), false);
    const HashParams hp = A.hp;
    const bool speaks = !tail && (threadIdx.x & 3) == 0;      // quad-uniform values: lane 0 of the quad speaks
    hash_program<1>(be, hp, nullptr, A.operands + i * (uint64_t)A.nw, ResultOut{A.results + i * (uint64_t)A.nres, speaks});
    if (speaks) store_n_failed(A, i, sink.n_failed);
}

// LDS: the nine-limb tables alone.  A wavefront past the last instance leaves after the tables' barrier
__global__ __launch_bounds__(QUAD_BLOCK) __attribute__((flatten)) void k_chipvalues_row(ValuesArgs A) {
    typedef ValBackend<ValuesRowSink> RowB;
    stage_bn_consts9(A.bn_tab9, threadIdx.x, QUAD_BLOCK);      // (block-wide barrier inside: before any wavefront leaves)
    const uint64_t i = (uint64_t)blockIdx.x * QUAD_WAVES + (threadIdx.x >> 6);      // this wavefront's instance
    if (i >= A.n) return;
    ValuesRowSink sink; sink.rowk = A.rowk;
    RowB be(sink, chiphash_cfg(1, A.L, A.P, A.inv, true), false);
    const HashParams hp = A.hp;
    const bool speaks = (threadIdx.x & 63) == 0;      // wave-uniform values: lane 0 speaks
    hash_program<1>(be, hp, nullptr, A.operands + i * (uint64_t)A.nw, ResultOut{A.results + i * (uint64_t)A.nres, speaks});
    if (speaks) store_n_failed(A, i, sink.n_failed);
}

// H2W_CHIPBATCH_FORM_AUTO with PoseidonBN254: the wavefront-per-instance form up to this many instances of a call.  A permutation takes the row form
// half the time on sixteen times the lanes, so it wins while the four-lane form leaves the chip idle.  The largest n of the sweep at which it was not
// the slower one, a call alone on the chip (tools/bench_chipbatch.py --values --sweep: MERKLE_VERIFY, hash_mode 1, depth 20, cap 4, leaf 20, n = 1 .. 16,384
// by powers of two; 2,048 instances 1.98 against 2.52 ms, 4,096 instances 3.66 against 2.53; DESIGN 5h, profiles/chipbatch_values.json), as verdict.hip
// VERDICT_ROW_MAX_PATHS was taken.  A caller that keeps other launches in flight pays for the row form's instructions earlier: it names its form itself.
constexpr uint64_t CHIPVALUES_ROW_MAX_INSTANCES = 2048;
// instances of one call at most: every grid of the call (the check kernel's is one lane per operand item: at most 4,096 + 1 + 64 + 32 of them) stays below 2^31 blocks
constexpr uint64_t CHIPVALUES_MAX_N = 1ull << 26;

static uint64_t num_results_of(const HashParams &hp) {
    switch (hp.op) {
        case H2W_OP_GL_PERMUTE: return SPONGE_WIDTH;
        case H2W_OP_BN_PERMUTE: return 4 * BN_WIDTH;
        case H2W_OP_HASH_NO_PAD: case H2W_OP_TWO_TO_ONE: return 4;      // four Goldilocks words / one Fr
        default: return 0;      // MERKLE_VERIFY: the verdict alone
    }
}

static int chipvalues_run(h2w_chipbatch *h, const uint64_t *operands_dev, uint64_t n, uint64_t *results_dev, h2w_chipbatch_verdict_t *verdict_dev, unsigned form, void *stream_) {
    ChipHash *c = h->hash;
    DeviceGuard dg(h->device);
    hipStream_t stream = (hipStream_t)stream_;
    ValuesArgs A; A.hp = c->hp; A.L = h->L; A.P = h->P; A.operands = operands_dev; A.nw = (uint32_t)h->nw; A.nres = (uint32_t)num_results_of(c->hp); A.n = n;
    A.results = results_dev; A.verdict = verdict_dev; A.tmpl_cells = h->d_tmpl_cells.get(); A.inv = c->d_inv.get();
    A.consts = c->d_consts.get(); A.small_mds = c->small_mds; A.bn_tab9 = c->d_bn_tab9.get(); A.rowk = c->d_rowk.get();
    H2W_HIP(hipMemsetAsync(verdict_dev, 0, n * sizeof(h2w_chipbatch_verdict_t), stream));
    CheckArgs K; K.operands = operands_dev; K.o = c->o; K.depth = c->hp.depth; K.n = n; K.status = &verdict_dev->status; K.stride = sizeof(h2w_chipbatch_verdict_t) / sizeof(uint32_t);
    chiphash_launch_check(K, stream);
    if (!c->bn) hipLaunchKernelGGL(k_chipvalues_gl, dim3((unsigned)n), dim3(64), 0, stream, A);
    else if (form == H2W_CHIPBATCH_FORM_ROW) hipLaunchKernelGGL(k_chipvalues_row, dim3((unsigned)((n + QUAD_WAVES - 1) / QUAD_WAVES)), dim3(QUAD_BLOCK), 0, stream, A);
    else hipLaunchKernelGGL(k_chipvalues_bn, dim3((unsigned)((n * 4 + QUAD_BLOCK - 1) / QUAD_BLOCK)), dim3(QUAD_BLOCK), 0, stream, A);
    H2W_HIP(hipGetLastError());
    return 0;
}

}  // namespace h2w

using namespace h2w;

extern "C" {

uint64_t h2w_chipbatch_num_results(const h2w_chipbatch *h) {
    if (!h) { set_error("h2w_chipbatch_num_results: null argument"); return 0; }
    if (!h->hash) { set_error("h2w_chipbatch_num_results: a handle of h2w_chipbatch_new (the field ops, 0-8) has no values call: use a handle of h2w_chipbatch_new_hash"); return 0; }
    return num_results_of(h->hash->hp);
}

int h2w_chipbatch_values(h2w_chipbatch *h, const uint64_t *operands_dev, uint64_t n, uint64_t *results_dev, h2w_chipbatch_verdict_t *verdict_dev, unsigned form, void *stream) {
    if (!h) { set_error("h2w_chipbatch_values: null handle"); return -1; }
    if (!h->hash) { set_error("h2w_chipbatch_values: a handle of h2w_chipbatch_new (the field ops, 0-8) has no values call: use a handle of h2w_chipbatch_new_hash"); return -1; }
    if (form > H2W_CHIPBATCH_FORM_ROW) { set_error("h2w_chipbatch_values: unknown form " + std::to_string(form) + " (H2W_CHIPBATCH_FORM_AUTO, _QUAD, _ROW)"); return -1; }
    const ChipHash *c = h->hash;
    if (form == H2W_CHIPBATCH_FORM_ROW && !c->bn) {
        set_error("h2w_chipbatch_values: H2W_CHIPBATCH_FORM_ROW is a PoseidonBN254 form and the handle's hash_mode is 0 (Goldilocks-Poseidon ops, GL_PERMUTE among them, have one kernel: H2W_CHIPBATCH_FORM_QUAD or _AUTO)");
        return -1;
    }
    if (!operands_dev || !verdict_dev || (!results_dev && num_results_of(c->hp) != 0)) { set_error("h2w_chipbatch_values: null buffer (results_dev may be null for MERKLE_VERIFY alone)"); return -1; }
    if (h->device < 0) { set_error("h2w_chipbatch_values: no HIP device - the value kernels only run on the GPU (no CPU fallback)"); return -1; }
    if (n == 0) return 0;
    if (n > CHIPVALUES_MAX_N) { set_error("h2w_chipbatch_values: batch too large (more than 2^26 instances); split the batch"); return -1; }
    if (form == H2W_CHIPBATCH_FORM_AUTO) form = c->bn && n <= CHIPVALUES_ROW_MAX_INSTANCES ? H2W_CHIPBATCH_FORM_ROW : H2W_CHIPBATCH_FORM_QUAD;
    return chipvalues_run(h, operands_dev, n, results_dev, verdict_dev, form, stream);
}

}  // extern "C"
