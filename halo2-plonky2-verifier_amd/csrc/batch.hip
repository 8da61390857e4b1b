// batch.hip — API level 3 of include/h2w.h: the batched hot path, the launch sequence of a witness call and its kernels.  (The shape compiler
// that fixes the offset of every cell block and strand, and the handle's tables: plancompile.cpp; tools on a finished stream: advicetools.hip.)
//
//   h2w_fri_witness_batch : per batch, on the caller's stream (+ one side stream of the plan)
//        k_prologue_values  one wavefront per proof : witness load, Fiat-Shamir challenger ON VALUES (serial sponge), PoW, reduced
//                           openings -> challenge block, the prologue's direct cells / non-permutation records, the permutation list
//        k_glp_emit         one wavefront per listed Goldilocks-Poseidon permutation -> its 2,604 block records
//        k_strands          one lane per (proof, query) : FRI query glue (glue.hip) -> records
//        PoseidonBN254 caps : k_merkle_bn_values  one quad per (proof, query, tree): the Merkle path ON VALUES -> unit states
//                             k_merkle_bn_emit    one quad per permutation unit of every path: its cells, straight to the advice
//        Goldilocks caps    : k_merkle_gl_values  one wavefront per (proof, query, tree) -> select records, the permutation list
//        expand_fast        block records -> cells: the HBM-write-bound materialisation (expand.hip)
// Data layout in HBM (per batch): proofs [n][proof_words] u64 ; records [n][n_records] 32 B ; challenge blocks [n] ; unit states
// [n][units][4] 32 B ; permutation list [n][perms][13] u64 ; advice [n][n_cells] 32 B canonical-LE Fr.  Record metas / templates /
// Poseidon constants are per-shape and shared.
// Here: the kernels of a call (k_prologue_load, k_glp_emit, k_sbox_canon*, k_merkle_bn_fused, k_direct_to_montgomery, k_columns_fixup), ws_layout, WitnessCall
// (a call's phases) and run_batch, the h2w_fri_witness_batch* entry points and the shard queries, h2w_fri_expand_records, h2w_plan_status, the timing calls, h2w_plan_configure.
#include <hip/hip_runtime.h>
#include <vector>
#include <string>
#include <cstring>
#include "plan.h"
#include "traceplan.h"

namespace h2w {

// WitnessChip::load_proof_with_pis (witness/mod.rs:267-294) and the limb decompositions of the caps' BN254 hashes (challenger/mod.rs:65-74,
// hash/poseidon_bn254/hash.rs:31-43): every item is a function of a few proof words - one lane per (proof, item).  Every rank checks every
// proof's words (status 4); the proof's owner writes the records and cells.
template <bool COLS> __global__ __launch_bounds__(256) void k_prologue_load(BatchArgs A) {
    const int p = blockIdx.y; const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n_load_items + A.n_cap_items) return;
    const bool emit = own_prologue(A, p);
    rec_t *recs = A.recs + (uint64_t)p * A.rec_stride; fr_t *out = block_out(A, p, -1);
    const uint64_t *ip = reinterpret_cast<const uint64_t *>(A.load_items + i);
    const uint64_t wk = g_load_u64(ip), irec = g_load_u64(ip + 1), icell = g_load_u64(ip + 2);
    const uint32_t word = (uint32_t)wk, kind = (uint32_t)(wk >> 32);
    const uint64_t *w = A.proofs + (uint64_t)p * A.proof_words + word;
    fr_t v; v.l[0] = g_load_u64(w); v.l[1] = v.l[2] = v.l[3] = 0;
    if (kind >= 2) { v.l[1] = g_load_u64(w + 1); v.l[2] = g_load_u64(w + 2); v.l[3] = g_load_u64(w + 3); }
    if (emit) {
        if (kind <= 2) g_store_rec(recs + irec, v.l[0], v.l[1], v.l[2], v.l[3]);      // (kinds 0-1: the one word, three zeros)
        else if (kind == 3) { ColPolicy<COLS> cc; cc.init(A.cm); g_store_fr(out + cc.map(icell), v); }
        else {      // kind 4: RangeChip::decompose_le(x, 56, 5) - 13 cells of limb sums + 5 range checks
            DevSinkT<COLS> sink; sink.recs = recs; sink.nrec = irec; sink.out = out; sink.cell_off = icell; sink.ncells = A.ncells; sink.cc.init(A.cm);
            ValBackend<DevSinkT<COLS>> be(sink, make_cfg(A, p), true);
            uint64_t limbs[5]; be.decompose_le_56_5(v, limbs);
        }
    }
    const bool bad = load_item_out_of_field(kind, v);
    if (bad) atomicOr(&A.load_flag[p], 4u);
}

// one wavefront per LISTED Goldilocks-Poseidon permutation of this rank's blocks: the prologues' (every owned proof), then - Goldilocks
// caps - the Merkle strands' (every owned (proof, query) unit)
template <bool COLS> __global__ __launch_bounds__(64) void k_glp_emit(BatchArgs A) {
    typedef CoopSinkT<COLS, false> Sink;
    stage_glp_consts(A.consts, threadIdx.x, 64);
    unsigned b = blockIdx.x; int p, slot;
    const unsigned n_pro = A.sh.n_own_proofs * A.st->pro_nglp;
    if (b < n_pro) { p = (int)(b / A.st->pro_nglp) * A.sh.world + A.sh.rank; slot = (int)(b % A.st->pro_nglp); }
    else {
        b -= n_pro; int q;
        if (A.st->q_nglp == 0 || !own_unit_at(A, b / A.st->q_nglp, p, q)) return;
        slot = (int)(A.st->pro_nglp + (unsigned)q * A.st->q_nglp + b % A.st->q_nglp);
    }
    Sink sink; coop_sink_init(sink, A, p, -1); sink.cell_off = 0; sink.emit = true;
    const uint64_t *e = A.glp_list + ((uint64_t)p * A.st->total_glp + (uint64_t)slot) * GLP_LIST_WORDS;
    const uint64_t w = threadIdx.x < GLP_LIST_WORDS ? g_load_u64(e + threadIdx.x) : 0;
    uint64_t st[SPONGE_WIDTH];
#pragma unroll
    for (int i = 0; i < SPONGE_WIDTH; i++) st[i] = readlane64(w, i + 1);
    sink.nrec = readlane64(w, 0);
    sink.coop_poseidon_permute(st, A.consts);
}

// between the two passes: the S-box values of the owned units' partial rounds, as the values pass left them (times R), to the canonical
// values the emission shows - one lane per value, 168 per permutation unit
__global__ __launch_bounds__(256) void k_sbox_canon(BatchArgs A, uint32_t units_per_query) {
    const uint64_t per_q = (uint64_t)units_per_query * (BN_PARTIAL_ROUNDS * 3);
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned i = (unsigned)(idx / per_q); const uint64_t v = idx % per_q;
    int p, q; if (!own_unit_at(A, i, p, q)) return;
    if (v >= A.st->q_nunit[q == 0 ? 0 : 1] * (uint64_t)(BN_PARTIAL_ROUNDS * 3)) return;
    fr_t *const x = A.unit_sbox + (uint64_t)i * A.sh.unit_slot * (BN_PARTIAL_ROUNDS * 3) + v;
    g_store_fr(x, fr_mont_mul(g_load_fr(x), fr_from_u64(1), A.P.ninv));
}
// the same for the row-cooperative values pass (rowperm.h): it leaves every S-box value as twelve dwords of 29-bit limbs (times R, lazy, limbs a few
// units above 2^29): carry pass, one Montgomery product by 1, one conditional subtraction -> the canonical value, into unit_sbox
__global__ __launch_bounds__(256) void k_sbox_canon9(BatchArgs A, uint32_t units_per_query) {
    const uint64_t per_q = (uint64_t)units_per_query * (BN_PARTIAL_ROUNDS * 3);
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned i = (unsigned)(idx / per_q); const uint64_t v = idx % per_q;
    int p, q; if (!own_unit_at(A, i, p, q)) return;
    if (v >= A.st->q_nunit[q == 0 ? 0 : 1] * (uint64_t)(BN_PARTIAL_ROUNDS * 3)) return;
    const uint64_t at = (uint64_t)i * A.sh.unit_slot * (BN_PARTIAL_ROUNDS * 3) + v;
    const uint4 *src = reinterpret_cast<const uint4 *>(A.unit_sbox9 + at * rf::SBX9_W);
    const uint4 a = src[0], b = src[1], c4 = src[2];
    const uint32_t t[9] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c4.x};
    fr9_t n; uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) { const uint32_t x = t[j] + c; n.t[j] = x & rf::M29; c = x >> 29; }
    n.t[8] = t[8] + c;
    fr9_t one9;
#pragma unroll
    for (int j = 0; j < 9; j++) one9.t[j] = j == 0 ? 1u : 0u;
    fr_t s = fr9_pack(fr9_mont(n, one9, (uint32_t)A.P.ninv & rf::M29));
    if (fr_geq_mod(s)) s = fr_sub_mod_raw(s);
    g_store_fr(A.unit_sbox + at, s);
}
// one pass (H2W_OPT_CHAIN_PASSES 1): four lanes per (owned unit, kind) walk the path and emit every unit of it - the least arithmetic per
// cell (352 wavefront-level products per permutation, none twice), serial in the path's depth; blockIdx.y = kind slot
template <bool COLS> __global__ __launch_bounds__(QUAD_BLOCK) H2W_QUAD_ATTR void k_merkle_bn_fused(BatchArgs A) {
    typedef QuadSinkT<COLS, QUAD_FUSED> Sink; typedef ValBackend<Sink> QuadB;
    stage_bn_consts(A.bn_tab, threadIdx.x, QUAD_BLOCK);
    const unsigned total = A.sh.n_own_units;
    if (((blockIdx.x * QUAD_BLOCK + (threadIdx.x & ~63u)) >> 2) >= total) return;
    unsigned idx = (blockIdx.x * QUAD_BLOCK + threadIdx.x) >> 2;
    if (idx >= total) idx = total - 1;
    int p, q; own_unit_at(A, idx, p, q);
    const int kind = merkle_kind(A.shape.n_perm_z, blockIdx.y);
    Sink sink;
    quad_strand<QuadB>(A, sink, idx, p, q, kind);
}
// H2W_OPT_OUTPUT_FORM = Montgomery, the direct cells: the cells of a proof's stream that the value kernels wrote themselves (canonical; the plan's bitmap)
// get the full product, in place, at the address their writer used - column shift, and with (proof, query) sharding only the blocks of this rank, at their
// packed addresses in the compact form.  A wavefront takes 64 words of the bitmap (4,096 cells) and walks the words that have a bit set, lane = cell.
struct DirectArgs {
    const uint64_t *bits; uint64_t ncells; fr_t *out; uint64_t cell_stride; ColMap cm;
    int rank, world, compact; uint32_t nq; uint64_t pro_ncell, q_cell0_first, q_cell0_rest, q_ncell_rest, q_slot;
    fr_t kconst; uint64_t ninv;
};
template <bool COLS> __global__ __launch_bounds__(256) void k_direct_to_montgomery(DirectArgs D) {
    const uint64_t p = blockIdx.y; const int lane = threadIdx.x & 63;
    const uint64_t nwords = (D.ncells + 63) / 64, w0 = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (w0 >= nwords) return;
    const unsigned long long mine = w0 + (uint64_t)lane < nwords ? g_load_u64(D.bits + w0 + lane) : 0ull;
    ColPolicy<COLS> cc; cc.init(D.cm);
    unsigned long long nz = __ballot(mine != 0);
    while (nz) {
        const int k = __ffsll((long long)nz) - 1; nz &= nz - 1;
        const unsigned long long word = __shfl(mine, k, 64);      // (before any lane leaves the iteration: nz and k are wavefront-uniform, every lane reaches this)
        if (!((word >> lane) & 1)) continue;
        const uint64_t cell = (w0 + (uint64_t)k) * 64 + (uint64_t)lane;
        fr_t *base = D.out + p * D.cell_stride;
        if (D.world > 1) {      // the block of the cell: prologue (q < 0) or query q; batchargs.h block_out
            const uint64_t W = (uint64_t)D.world, r = (uint64_t)D.rank, u0 = p * D.nq;
            long long q = -1;
            if (cell >= D.pro_ncell) {
                q = (D.nq == 1 || cell < D.q_cell0_rest) ? 0 : 1 + (long long)((cell - D.q_cell0_rest) / (D.q_ncell_rest ? D.q_ncell_rest : 1));
                if (q >= (long long)D.nq) q = (long long)D.nq - 1;
            }
            if ((q < 0 ? p : u0 + (uint64_t)q) % W != r) continue;
            if (D.compact) {      // (shardmap.h packed_block_start, written out: the call costs the kernel a scalar register and three instructions)
                const uint64_t pro_before = (p + W - 1 - r) / W, units_before = (u0 + W - 1 - r) / W;
                uint64_t local = pro_before * D.pro_ncell + units_before * D.q_slot, global = 0;
                if (q >= 0) {
                    if (p % W == r) local += D.pro_ncell;
                    local += ((u0 + (uint64_t)q + W - 1 - r) / W - units_before) * D.q_slot;
                    global = q == 0 ? D.q_cell0_first : D.q_cell0_rest + (uint64_t)(q - 1) * D.q_ncell_rest;
                }
                base = D.out + local - global;
            }
        }
        fr_t *at = base + cc.map(cell);
        g_store_fr(at, fr_mont_mul(g_load_fr(at), D.kconst, D.ninv));
    }
}

}  // namespace h2w

// column-major emission: boundary cells repeated in the previous column, unused rows zeroed
extern "C" __global__ void k_columns_fixup(ulonglong2 *cols, const uint64_t *lens, uint32_t ncols, uint32_t k) {
    const uint64_t rows2 = (uint64_t)2 << k; const uint32_t p = blockIdx.z, c = blockIdx.y;
    ulonglong2 *col = cols + ((uint64_t)p * ncols + c) * rows2; const uint64_t len2 = lens[c] * 2;
    if (c + 1 < ncols && blockIdx.x == 0 && threadIdx.x < 2) col[len2 - 2 + threadIdx.x] = col[rows2 + threadIdx.x];       // (c, len-1) <- (c+1, 0)
    for (uint64_t h = len2 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < rows2; h += (uint64_t)gridDim.x * blockDim.x) col[h] = make_ulonglong2(0, 0);
}

namespace h2w {
static bool bad_shard(int rank, int world) { return world < 1 || rank < 0 || rank >= world; }
static ShardSpec shard_spec(int rank, int world, int compact = 0) { ShardSpec sh; sh.rank = rank; sh.world = world; sh.compact = compact; return sh; }
static uint64_t own_count(uint64_t total, int rank, int world) { return total > (uint64_t)rank ? (total - (uint64_t)rank + (uint64_t)world - 1) / (uint64_t)world : 0; }
static uint32_t unit_slot_of(const h2w_plan *p) { return (uint32_t)(p->st.q_nunit[0] > p->st.q_nunit[1] ? p->st.q_nunit[0] : p->st.q_nunit[1]); }
static uint64_t shard_q_slot(const h2w_plan *p) { return p->st.q_ncell[0] > p->st.q_ncell[1] ? p->st.q_ncell[0] : p->st.q_ncell[1]; }      // a query block's slot in the packed layout (ShardMap)
// Per-proof pieces first (their offsets do not depend on the sharding: h2w_plan_status finds the status words whatever call filled them), then the
// PoseidonBN254 unit buffers, which hold the units of THIS RANK's (proof, query) units only.
struct WsLayout { size_t recs, cbs, status, lflag, units, sbox, sbox9, glp, ctr, total; };
static WsLayout ws_layout(const h2w_plan *p, uint64_t n, const ShardSpec &sh = ShardSpec()) {
    WsLayout w; size_t o = 0;
    w.recs = o; o += align_up((size_t)n * p->nrec * sizeof(rec_t), 256);
    w.cbs = o; o += align_up((size_t)n * sizeof(DevCB), 256);
    w.status = o; o += align_up((size_t)n * sizeof(uint32_t), 256);
    w.lflag = o; o += align_up((size_t)n * sizeof(uint32_t), 256);      // per proof: a word outside its field's range (k_prologue_load)
    w.glp = o; o += align_up((size_t)n * p->st.total_glp * GLP_LIST_WORDS * sizeof(uint64_t), 256);     // listed Goldilocks-Poseidon permutations
    w.ctr = o; o += align_up((size_t)n * sizeof(uint32_t), 256);                                       // expansion kernel's per-proof tile counters
    const size_t own_units = (size_t)own_count(n * (uint64_t)p->shape.num_queries, sh.rank, sh.world) * unit_slot_of(p);
    w.units = o; o += align_up(own_units * 4 * sizeof(fr_t), 256);                                     // PoseidonBN254 unit states (values phase -> emission)
    w.sbox = o; o += align_up(own_units * BN_PARTIAL_ROUNDS * 3 * sizeof(fr_t), 256);                  // ... and the S-box values of their partial rounds
    w.sbox9 = o; o += align_up(own_units * BN_PARTIAL_ROUNDS * 3 * rf::SBX9_W * sizeof(uint32_t), 256);  // ... in the limb form the row-cooperative values pass leaves them in
    w.total = o;
    return w;
}
static void fill_expand_shard(const h2w_plan *p, ExpandArgs &E, const ShardSpec &sh) {
    E.shard_rank = (uint32_t)sh.rank; E.shard_world = (uint32_t)sh.world; E.shard_compact = (uint32_t)sh.compact; E.nq = (uint32_t)p->shape.num_queries;
    E.pro_nrec = p->st.pro_nrec; E.q_rec0_first = p->st.q_rec0[0]; E.q_rec0_rest = p->st.q_rec0[1]; E.q_nrec_first = p->st.q_nrec[0]; E.q_nrec_rest = p->st.q_nrec[1] ? p->st.q_nrec[1] : 1;
    if (p->shape.num_queries == 1) E.q_rec0_rest = ~0ull;
    E.pro_ncell = p->st.pro_ncell; E.q_cell0_first = p->st.q_cell0[0]; E.q_cell0_rest = p->st.q_cell0[1]; E.q_ncell_rest = p->st.q_ncell[1]; E.q_slot = shard_q_slot(p);
}
int launch_plan_expand(const h2w_plan *p, uint64_t n_proofs, const rec_t *recs, uint32_t *tile_ctr, fr_t *out, uint64_t cell_stride, ColMap cm,
                       const ShardSpec *sh, uint32_t roam_per_cu, hipStream_t stream) {
    ExpandArgs E;
    E.meta = p->d_meta.get(); E.recs = recs; E.nrec = p->nrec; E.rec_stride = p->nrec; E.out = out; E.cell_stride = cell_stride; E.pool = nullptr; E.cm = cm;
    if (sh) fill_expand_shard(p, E, *sh); else expand_unsharded(E);
    p->dt.fill(E);
    E.tile_ctr = tile_ctr; E.roam_per_cu = roam_per_cu; E.mont = p->output_form == H2W_FORM_MONTGOMERY ? p->d_mont.get() : nullptr;
    H2W_HIP(hipMemsetAsync(tile_ctr, 0, n_proofs * sizeof(uint32_t), stream));
    int gx = (int)(2048 / (n_proofs < 2048 ? n_proofs : 2048)); if (gx < 8) gx = 8;
    return launch_expand(E, n_proofs, gx, stream);
}
// roam_per_cu of the plan's expansion launches (profiles/r02_expand_grid.txt); the Montgomery form's kernel is bound by instruction issue, not by stores:
// it needs every wavefront a CU holds (profiles/montgomery_form_cfg3.json)
static uint32_t plan_roam_per_cu(const h2w_plan *p) { return (p->shape.hash_mode == 0 || p->output_form == H2W_FORM_MONTGOMERY) ? 2 : 1; }
// k_direct_to_montgomery for a call (plan.h): the plan's bitmap and block sizes, the call's output buffer, column map and sharding
int launch_plan_direct(const h2w_plan *p, const uint64_t *bits, uint64_t n_proofs, fr_t *out, uint64_t cell_stride, ColMap cm, const ShardSpec &sh, hipStream_t stream) {
    DirectArgs D;
    D.bits = bits; D.ncells = p->ncells; D.out = out; D.cell_stride = cell_stride; D.cm = cm;
    D.rank = sh.rank; D.world = sh.world; D.compact = sh.compact; D.nq = (uint32_t)p->shape.num_queries;
    D.pro_ncell = p->st.pro_ncell; D.q_cell0_first = p->st.q_cell0[0]; D.q_cell0_rest = p->st.q_cell0[1]; D.q_ncell_rest = p->st.q_ncell[1]; D.q_slot = shard_q_slot(p);
    D.kconst = mont_k(); D.ninv = p->P.ninv;
    const uint64_t nwaves = ((p->ncells + 63) / 64 + 63) / 64;
    launch_cols(cm.starts != nullptr, k_direct_to_montgomery<true>, k_direct_to_montgomery<false>, dim3((unsigned)((nwaves + 3) / 4), (unsigned)n_proofs), dim3(256), 0, stream, D);
    return 0;
}
// A workspace as typed pointers, by ws_layout's offsets
struct WsPtrs {
    rec_t *recs; DevCB *cbs; uint32_t *status, *load_flag, *ctr; fr_t *unit_state, *unit_sbox; uint32_t *unit_sbox9; uint64_t *glp_list;
    void fill(BatchArgs &A) const { A.recs = recs; A.cbs = cbs; A.status = status; A.load_flag = load_flag; A.unit_state = unit_state; A.unit_sbox = unit_sbox; A.unit_sbox9 = unit_sbox9; A.glp_list = glp_list; }
};
static WsPtrs ws_ptrs(void *workspace_dev, const WsLayout &wl) {
    char *ws = (char *)workspace_dev;
    return {(rec_t *)(ws + wl.recs), (DevCB *)(ws + wl.cbs), (uint32_t *)(ws + wl.status), (uint32_t *)(ws + wl.lflag), (uint32_t *)(ws + wl.ctr),
            (fr_t *)(ws + wl.units), (fr_t *)(ws + wl.sbox), (uint32_t *)(ws + wl.sbox9), (uint64_t *)(ws + wl.glp)};
}
// One witness call of a compiled plan (run_batch): what outlives a phase, and one method per phase, cut at the public event marks (include/h2w.h H2W_EV_*)
// and called in this order.  Every method enqueues and returns 0, or -1 with the reason in the last error; a call that leaves early waits for its side
// stream (plan.h SideFork).
struct WitnessCall {
    h2w_plan *const p; const uint64_t n_proofs; BatchArgs A; const WsLayout wl; const WsPtrs wp;
    const hipStream_t stream, estream, cstream;      // the caller's, the expansion kernel's, the chain kernels' (either may be the caller's)
    const DevEvent *const prev_ev, *const ev;        // the event rows of the previous call (null: none) and of this one
    const ColMap cm; const uint64_t cell_stride; const ShardSpec sh;
    unsigned nunits, nkinds, n_pro_perms, n_mk_perms;
    SideFork fork; int side_end = H2W_EV_CHAINS_END;      // side_end: the event that closes the work on the side stream, named by the method that opened the fork

    WitnessCall(h2w_plan *p_, const uint64_t *proofs_dev, uint64_t n, void *advice_dev, void *workspace_dev, hipStream_t s, hipStream_t es, hipStream_t cs, ColMap cm_, uint64_t cell_stride_, const ShardSpec &sh_)
        : p(p_), n_proofs(n), A(plan_batch_args(p_, proofs_dev, n)), wl(ws_layout(p_, n, sh_)), wp(ws_ptrs(workspace_dev, wl)), stream(s), estream(es), cstream(cs),
          prev_ev((p_->n_batches && p_->ev_recorded) ? p_->evr[(p_->n_batches - 1) % h2w_plan::EV_RING] : nullptr), ev(p_->evr[p_->n_batches % h2w_plan::EV_RING]),
          cm(cm_), cell_stride(cell_stride_), sh(sh_), fork(s, cs) {
        wp.fill(A); A.rec_stride = p->nrec; A.out = (fr_t *)advice_dev; A.cell_stride = cell_stride; A.cm = cm;
        A.sh.rank = sh.rank; A.sh.world = sh.world; A.sh.compact = sh.compact; A.sh.q_slot = shard_q_slot(p); A.sh.unit_slot = unit_slot_of(p);
        A.sh.n_own_units = (uint32_t)own_count(n_proofs * (uint64_t)p->shape.num_queries, sh.rank, sh.world);
        A.sh.n_own_proofs = (uint32_t)own_count(n_proofs, sh.rank, sh.world);
        nunits = A.sh.n_own_units; nkinds = (unsigned)(p->d.n_oracles + p->d.n_steps);
        n_pro_perms = A.sh.n_own_proofs * p->st.pro_nglp; n_mk_perms = nunits * p->st.q_nglp;
    }
    // ---- H2W_EV_CALL_START .. H2W_EV_PROLOGUE_END
    int prologue() {
        H2W_HIP(hipEventRecord(ev[H2W_EV_CALL_START], stream));
        // prologue strands, values: one wavefront per proof (witness load, Fiat-Shamir sponge, PoW, reduced openings) -> challenge blocks.  FIRST: everything
        // else of the launch waits for the challenges, nothing for the load cells
        launch_prologue_values(A, stream);
        H2W_HIP(hipEventRecord(ev[h2w_plan::EV_PROLOGUE_VALUES_END], stream));
        // witness load + cap-hash limb decompositions: one lane per (proof, item).  Cells and a flag word only (nobody's input): behind the prologue, beside the
        // Merkle chains that fork off at this point
        H2W_HIP(hipMemsetAsync(A.load_flag, 0, n_proofs * sizeof(uint32_t), stream));
        if (p->n_items + p->n_cap_items) {
            const dim3 lgrid((p->n_items + p->n_cap_items + 255) / 256, (unsigned)n_proofs);
            launch_cols(cm.starts != nullptr, k_prologue_load<true>, k_prologue_load<false>, lgrid, dim3(256), 0, stream, A);
        }
        if (p->shape.hash_mode == 1) { if (glp_emit(n_pro_perms) != 0) return -1; }
        H2W_HIP(hipEventRecord(ev[H2W_EV_PROLOGUE_END], stream));
        return 0;
    }
    // the records of n listed Goldilocks-Poseidon permutations, once per call: with PoseidonBN254 caps the prologues' (prologue); with Goldilocks caps
    // together with the Merkle strands' (glue).  (Defined behind prologue: the kernel templates appear in the device code in the order of their first use.)
    int glp_emit(unsigned n) {
        H2W_HIP(hipEventRecord(ev[h2w_plan::EV_GLP_START], stream));
        if (n) launch_cols(cm.starts != nullptr, k_glp_emit<true>, k_glp_emit<false>, dim3(n), dim3(64), 0, stream, A);
        H2W_HIP(hipEventRecord(ev[h2w_plan::EV_GLP_END], stream));
        return 0;
    }
    // ---- PoseidonBN254 Merkle chains (hash_mode 1), the fork .. H2W_EV_CHAINS_END: values, then one quad per permutation unit.  They write their cells
    // themselves and no block records, so nothing but the challenge blocks orders them against the other kernels of the batch: they run on a side
    // stream of the plan and rejoin at the end of the call.
    int bn_chains() {
        if (p->shape.hash_mode != 1) return 0;
        if (fork.fork_at(ev[h2w_plan::EV_PROLOGUE_VALUES_END]) != 0) return -1;
        side_end = H2W_EV_CHAINS_END;
        H2W_HIP(hipEventRecord(ev[H2W_EV_CHAINS_START], cstream));
        const dim3 sgrid((nunits * 4 + QUAD_BLOCK - 1) / QUAD_BLOCK, nkinds);
        // one pass or two (include/h2w.h H2W_OPT_CHAIN_PASSES): a launch whose paths do not fill the chip is bound by the depth of a path - split it
        const int passes = p->chain_passes ? p->chain_passes : (nunits <= 512 ? 2 : 1);
        p->passes_of[p->n_batches % h2w_plan::EV_RING] = passes;
        if (nunits && passes == 1) launch_cols(cm.starts != nullptr, k_merkle_bn_fused<true>, k_merkle_bn_fused<false>, sgrid, dim3(QUAD_BLOCK), 0, cstream, A);
        if (nunits && passes != 1) {
            // the values of the paths: one wavefront per path (rowperm.h: a path's 18 permutations in 1.3 ms instead of 2.6) for a launch of a few proofs - the form for
            // one proof's latency; four lanes per path (bnquad.h bn_values: a sixth of the instructions per path) beyond that: alone on the chip the wavefront form
            // wins up to ~2,500 paths (profiles/r04_values_forms.jsonl), but a caller with several launches in flight pays for its instructions (cfg 1 pipelined,
            // 1,024 paths per launch: 160 G cells/s against 175-190), so the default switches early and H2W_OPT_VALUES_FORM = 2 is the caller's to set
            const bool rows = p->values_form ? p->values_form == 2 : (uint64_t)nunits * nkinds <= 784;
            const uint32_t upq = unit_slot_of(p);
            const uint64_t nval = (uint64_t)nunits * upq * (BN_PARTIAL_ROUNDS * 3);
            if (rows) {
                launch_merkle_bn_values_row(A, nkinds, cstream);
                if (nval) hipLaunchKernelGGL(k_sbox_canon9, dim3((unsigned)((nval + 255) / 256)), dim3(256), 0, cstream, A, upq);
            } else {
                launch_merkle_bn_values(A, sgrid, cstream);
                if (nval) hipLaunchKernelGGL(k_sbox_canon, dim3((unsigned)((nval + 255) / 256)), dim3(256), 0, cstream, A, upq);
            }
        }
        H2W_HIP(hipEventRecord(ev[h2w_plan::EV_CHAIN_VALUES_END], cstream));
        const unsigned long long items = passes == 1 ? 0ull : (unsigned long long)((nunits + 15u) & ~15u) * p->st.mk_item0[MK_KINDS];
        if (items) launch_merkle_bn_emit(A, dim3((unsigned)((items * 4 + QUAD_BLOCK - 1) / QUAD_BLOCK)), cstream);
        H2W_HIP(hipEventRecord(ev[H2W_EV_CHAINS_END], cstream));
        return 0;
    }
    // ---- H2W_EV_GLUE_START .. H2W_EV_GLUE_END: query glue strands (FriChip::verify_query_round minus its Merkle proofs), one lane per owned (proof, query);
    // Goldilocks-Poseidon Merkle strands (hash_mode 0), values: one cooperating wavefront per (proof, query, tree).  The two read the challenge blocks and
    // write disjoint records (and list entries): with Goldilocks caps the Merkle strands run on the plan's side stream beside the glue strands and rejoin
    // before the permutations' records are emitted.
    int glue() {
        H2W_HIP(hipEventRecord(ev[H2W_EV_GLUE_START], stream));
        if (p->shape.hash_mode == 0) {
            if (fork.fork_at(ev[h2w_plan::EV_PROLOGUE_VALUES_END]) != 0) return -1;
            side_end = H2W_EV_CHAINS_END;
            H2W_HIP(hipEventRecord(ev[H2W_EV_CHAINS_START], cstream));
            if (nunits) launch_merkle_gl_values(A, nunits, nkinds, cstream);
            H2W_HIP(hipEventRecord(ev[h2w_plan::EV_CHAIN_VALUES_END], cstream)); H2W_HIP(hipEventRecord(ev[H2W_EV_CHAINS_END], cstream));
        }
        if (nunits) launch_glue_strands(A, stream);
        if (p->shape.hash_mode == 0) {
            if (fork.join_at(ev[H2W_EV_CHAINS_END]) != 0) return -1;
            if (glp_emit(n_pro_perms + n_mk_perms) != 0) return -1;
        }
        H2W_HIP(hipEventRecord(ev[H2W_EV_GLUE_END], stream));
        return 0;
    }
    // ---- H2W_EV_EXPAND_START .. H2W_EV_EXPAND_END: expansion of the block records (HBM-write-bound)
    int expand() {
        if (estream != stream) H2W_HIP(hipStreamWaitEvent(estream, ev[H2W_EV_GLUE_END], 0));    // value strands done -> expansion on the emit stream
        // One expansion kernel at a time over all the streams a plan is driven on: its blocks are persistent and hold their CUs until the
        // launch is written, so two of them side by side keep the latency-bound strands of the other launches in flight off the chip
        // (measured: +8..12 % for the whole job with PoseidonBN254 caps, profiles/r02_sweep5.txt; +5 % with Goldilocks caps since that kernel
        // runs on a grid of resident blocks there and reaches its rate alone, profiles/r02_expand_grid.txt).
        if (p->serial_expand != 0 && prev_ev) H2W_HIP(hipStreamWaitEvent(estream, prev_ev[H2W_EV_EXPAND_END], 0));
        H2W_HIP(hipEventRecord(ev[H2W_EV_EXPAND_START], estream));
        if (launch_plan_expand(p, n_proofs, A.recs, wp.ctr, A.out, cell_stride, cm, &sh, plan_roam_per_cu(p), estream) != 0) return -1;
        H2W_HIP(hipEventRecord(ev[H2W_EV_EXPAND_END], estream));
        return 0;
    }
    // ---- Montgomery form: the direct cells, behind the chain kernels on the stream they ran on, beside the expansion kernel (which converts its own cells
    // as it writes them).  The glue strands' and the prologue's direct cells were written on the caller's stream: the side stream waits for them.
    int direct_cells() {
        if (p->output_form != H2W_FORM_MONTGOMERY) return 0;
        if (fork.fork_at(ev[H2W_EV_GLUE_END]) != 0) return -1;
        side_end = h2w_plan::EV_DIRECT_END;
        if (launch_plan_direct(p, p->d_direct_bits.get(), n_proofs, A.out, A.cell_stride, A.cm, sh, cstream) != 0) return -1;
        if (cstream != stream) H2W_HIP(hipEventRecord(ev[h2w_plan::EV_DIRECT_END], cstream));
        return 0;
    }
    // ---- .. H2W_EV_CALL_END: the caller's stream completes when the advice is complete
    int finish() {
        if (estream != stream) H2W_HIP(hipStreamWaitEvent(stream, ev[H2W_EV_EXPAND_END], 0));
        if (fork.join_at(ev[side_end]) != 0) return -1;
        H2W_HIP(hipEventRecord(ev[H2W_EV_CALL_END], stream));
        H2W_HIP(hipGetLastError());
        return 0;
    }
};
static int run_batch(h2w_plan *p, const uint64_t *proofs_dev, uint64_t n_proofs, void *advice_dev, void *workspace_dev, void *stream_, void *emit_stream_, ColMap cm, uint64_t cell_stride, const ShardSpec &sh) {
    if (!p) { set_error("h2w_fri_witness_batch: null plan"); return -1; }
    if (p->device < 0) { set_error("h2w_fri_witness_batch: no HIP device — the hot path only runs on the GPU (no CPU fallback)"); return -1; }
    if (!proofs_dev || !advice_dev || !workspace_dev) { set_error("h2w_fri_witness_batch: null buffer"); return -1; }
    if (n_proofs == 0) return 0;
    if (p->traced) {      // a recorded run (traceplan.h; replay.hip traced_run): the flat stream, the FlexGate columns, or this rank's (proof, query) units
        if (emit_stream_ != stream_) { set_error("h2w_fri_witness_batch: a traced plan runs on one stream"); return -1; }
        return traced_run(p, proofs_dev, n_proofs, advice_dev, workspace_dev, stream_, cm, cell_stride, sh);
    }
    if (n_proofs * (uint64_t)p->shape.num_queries * (p->st.mk_item0[MK_KINDS] ? p->st.mk_item0[MK_KINDS] : 1) > 0x3fffffffull) { set_error("h2w_fri_witness_batch: batch too large"); return -1; }
    if (n_proofs > 65535) { set_error("h2w_fri_witness_batch: more than 65535 proofs per call (the proof index is a grid dimension of the load and expansion kernels); split the batch"); return -1; }
    DeviceGuard dg(p->device);
    hipStream_t stream = (hipStream_t)stream_, cstream;      // cstream: the chain kernels' (more caller streams than side streams: the extra ones do not fork)
    if (plan_side_stream(p, stream, p->fork_chains, &cstream) != 0) return -1;
    WitnessCall c(p, proofs_dev, n_proofs, advice_dev, workspace_dev, stream, (hipStream_t)emit_stream_, cstream, cm, cell_stride, sh);
    if (c.prologue()) return -1;
    if (c.bn_chains()) return -1;
    if (c.glue()) return -1;
    if (c.expand()) return -1;
    if (c.direct_cells()) return -1;
    if (c.finish()) return -1;
    p->n_batches++; p->ev_recorded = true;
    return 0;
}
// the event row of the call `back` calls before the last one (a ring of EV_RING); null, and `error` set, where there is none
static const DevEvent *call_events(h2w_plan *p, uint64_t back, const char *error) {
    if (!p || !p->ev_recorded || back >= p->n_batches || back >= (uint64_t)h2w_plan::EV_RING) { set_error(error); return nullptr; }
    return p->evr[(p->n_batches - 1 - back) % h2w_plan::EV_RING];
}

}  // namespace h2w

extern "C" {

uint64_t h2w_plan_workspace_bytes(const h2w_plan *p, uint64_t n_proofs) { return !p ? 0 : p->traced ? traced_workspace_bytes(p, n_proofs) : ws_layout(p, n_proofs).total; }
uint64_t h2w_plan_shard_workspace_bytes(const h2w_plan *p, uint64_t n_proofs, int rank, int world) {
    if (!p || bad_shard(rank, world)) return 0;
    if (const char *why = traced_shard_refusal(p)) { set_error(std::string("h2w_plan_shard_workspace_bytes: ") + why); return 0; }
    if (p->traced) return traced_workspace_bytes(p, n_proofs);      // (value store and records per proof: the unsharded size)
    return ws_layout(p, n_proofs, shard_spec(rank, world)).total;
}
int h2w_fri_witness_batch(h2w_plan *p, const uint64_t *proofs_dev, uint64_t n_proofs, void *advice_dev, void *workspace_dev, void *stream_) {
    return run_batch(p, proofs_dev, n_proofs, advice_dev, workspace_dev, stream_, stream_, flat_cols(), p ? p->ncells : 0, ShardSpec());
}
int h2w_fri_witness_batch2(h2w_plan *p, const uint64_t *proofs_dev, uint64_t n_proofs, void *advice_dev, void *workspace_dev, void *stream_, void *emit_stream_) {
    return run_batch(p, proofs_dev, n_proofs, advice_dev, workspace_dev, stream_, emit_stream_, flat_cols(), p ? p->ncells : 0, ShardSpec());
}
int h2w_fri_witness_batch_columns(h2w_plan *p, const uint64_t *proofs_dev, uint64_t n_proofs, const uint64_t *break_points, uint64_t n_bp, int k,
                                  void *columns_dev, void *workspace_dev, void *stream_) {
    if (!p || (!break_points && n_bp) || !columns_dev) { set_error("h2w_fri_witness_batch_columns: null argument"); return -1; }
    if (k < 12 || k > 34 || n_bp + 1 > 4096) { set_error("h2w_fri_witness_batch_columns: k must be in [12, 34] and at most 4096 columns"); return -1; }
    if (p->device < 0) { set_error("h2w_fri_witness_batch_columns: no HIP device — the hot path only runs on the GPU (no CPU fallback)"); return -1; }
    const uint64_t ncols = n_bp + 1; std::vector<uint64_t> h(2 * ncols); uint64_t start = 0;
    for (uint64_t c = 0; c < ncols; c++) {
        const uint64_t len = c < n_bp ? break_points[c] + 1 : p->ncells - start;
        if (start + len > p->ncells || len > ((uint64_t)1 << k) || len < 2) { set_error("h2w_fri_witness_batch_columns: break points do not fit the stream"); return -1; }
        h[c] = start; h[ncols + c] = len; start += len - (c < n_bp ? 1 : 0);
    }
    DeviceGuard dg(p->device);
    hipStream_t stream = (hipStream_t)stream_;
    if (h != p->h_col_tab || k != p->col_k) {      // (re)upload the column table; plans are single-threaded handles (include/h2w.h)
        H2W_HIP(hipDeviceSynchronize());             // a previous call on another stream may still read the old table
        p->h_col_tab.clear();                        // (a failed upload leaves no table: the next call starts over)
        if (p->d_col_tab.upload(h) != 0) return -1;
        p->h_col_tab = h; p->col_k = k;
    }
    ColMap cm; cm.starts = p->d_col_tab.get(); cm.ncols = (uint32_t)ncols; cm.k = (uint32_t)k;
    if (run_batch(p, proofs_dev, n_proofs, columns_dev, workspace_dev, stream_, stream_, cm, ncols << k, ShardSpec()) != 0) return -1;
    if (n_proofs) {
        if (n_proofs > 65535) { set_error("h2w_fri_witness_batch_columns: too many proofs per call"); return -1; }
        hipLaunchKernelGGL(k_columns_fixup, dim3(64, (unsigned)ncols, (unsigned)n_proofs), dim3(256), 0, stream, (ulonglong2 *)columns_dev, p->d_col_tab.get() + ncols, (uint32_t)ncols, (uint32_t)k);
        H2W_HIP(hipGetLastError());
    }
    return 0;
}
// (proof, query) sharding: this rank LAUNCHES only what it owns - the prologue block of the proofs p % world == rank and the
// query blocks of the units (proof * num_queries + query) % world == rank (every rank runs every prologue's values: it needs the
// challenges) - at their global offsets in advice_dev[n_proofs][num_cells]; the other blocks are left untouched.
int h2w_fri_witness_batch_shard(h2w_plan *p, const uint64_t *proofs_dev, uint64_t n_proofs, void *advice_dev, void *workspace_dev, void *stream_, int rank, int world) {
    if (bad_shard(rank, world)) { set_error("h2w_fri_witness_batch_shard: bad rank / world"); return -1; }
    if (const char *why = p ? traced_shard_refusal(p) : nullptr) { set_error(std::string("h2w_fri_witness_batch_shard: ") + why); return -1; }
    return run_batch(p, proofs_dev, n_proofs, advice_dev, workspace_dev, stream_, stream_, flat_cols(), p ? p->ncells : 0, shard_spec(rank, world));
}
// The same blocks packed into a buffer of h2w_plan_shard_cells cells: the rank's owned blocks back to back in (proof, block) order.
uint64_t h2w_plan_shard_cells(const h2w_plan *p, uint64_t n_proofs, int rank, int world) {
    if (!p || bad_shard(rank, world)) return 0;
    if (const char *why = traced_shard_refusal(p)) { set_error(std::string("h2w_plan_shard_cells: ") + why); return 0; }
    return own_count(n_proofs, rank, world) * p->st.pro_ncell + own_count(n_proofs * (uint64_t)p->shape.num_queries, rank, world) * shard_q_slot(p);
}
int h2w_plan_shard_block(const h2w_plan *p, int rank, int world, uint64_t proof, int query, uint64_t *local_cell, uint64_t *n_cells, uint64_t *global_cell) {
    if (!p || bad_shard(rank, world) || query >= p->shape.num_queries) { set_error("h2w_plan_shard_block: bad argument"); return -1; }
    if (const char *why = traced_shard_refusal(p)) { set_error(std::string("h2w_plan_shard_block: ") + why); return -1; }
    const uint64_t W = (uint64_t)world, r = (uint64_t)rank, nq = (uint64_t)p->shape.num_queries;
    if (!shard_owns(W, r, nq, proof, query)) return 1;
    const uint64_t local = packed_block_start(W, r, nq, p->st.pro_ncell, shard_q_slot(p), proof, query);
    uint64_t n = p->st.pro_ncell, g = 0;
    if (query >= 0) { n = p->st.q_ncell[query == 0 ? 0 : 1]; g = strand_q_cell(p->st, query); }
    if (local_cell) *local_cell = local; if (n_cells) *n_cells = n; if (global_cell) *global_cell = g;
    return 0;
}
int h2w_fri_witness_batch_shard_compact(h2w_plan *p, const uint64_t *proofs_dev, uint64_t n_proofs, void *shard_advice_dev, void *workspace_dev, void *stream_, int rank, int world) {
    if (bad_shard(rank, world)) { set_error("h2w_fri_witness_batch_shard_compact: bad rank / world"); return -1; }
    if (const char *why = p ? traced_shard_refusal(p) : nullptr) { set_error(std::string("h2w_fri_witness_batch_shard_compact: ") + why); return -1; }
    if (p && !(p->shape.lookup_bits == 21 || p->shape.lookup_bits == 13 || p->shape.lookup_bits == 8)) { set_error("h2w_fri_witness_batch_shard_compact: lookup_bits must be 21, 13 or 8 (the packed layout is written by expand_fast)"); return -1; }
    return run_batch(p, proofs_dev, n_proofs, shard_advice_dev, workspace_dev, stream_, stream_, flat_cols(), 0, shard_spec(rank, world, 1));
}
// Re-expands the block records a previous h2w_fri_witness_batch* call left in `workspace_dev` (same n_proofs) into advice_dev: the
// expansion kernel alone, for measuring its streaming rate (bench.py roofline).  Cells written by the value kernels are not touched.
int h2w_fri_expand_records(h2w_plan *p, uint64_t n_proofs, void *advice_dev, void *workspace_dev, void *stream_) {
    if (!p || p->device < 0) { set_error("h2w_fri_expand_records: no HIP device"); return -1; }
    if (p->traced) { set_error("h2w_fri_expand_records: not for traced plans"); return -1; }
    if (!advice_dev || !workspace_dev) { set_error("h2w_fri_expand_records: null buffer"); return -1; }
    if (n_proofs == 0) return 0;
    DeviceGuard dg(p->device);
    hipStream_t stream = (hipStream_t)stream_;
    const WsPtrs wp = ws_ptrs(workspace_dev, ws_layout(p, n_proofs));
    const ShardSpec one_rank{};
    if (launch_plan_expand(p, n_proofs, wp.recs, wp.ctr, (fr_t *)advice_dev, p->ncells, flat_cols(), &one_rank, plan_roam_per_cu(p), stream) != 0) return -1;
    H2W_HIP(hipGetLastError());
    return 0;
}
int h2w_plan_status(h2w_plan *p, const void *workspace_dev, uint64_t n_proofs, uint32_t *host_status, void *stream_) {
    if (!p || !workspace_dev || !host_status) { set_error("h2w_plan_status: null argument"); return -1; }
    WsLayout wl = ws_layout(p, n_proofs);
    if (p->traced) { wl.status = traced_status_offset(p, n_proofs, false); wl.lflag = traced_status_offset(p, n_proofs, true); }
    DeviceGuard dg(p->device);
    hipStream_t stream = (hipStream_t)stream_;
    std::vector<uint32_t> flag((size_t)n_proofs);
    H2W_HIP(hipMemcpyAsync(host_status, (const char *)workspace_dev + wl.status, n_proofs * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    H2W_HIP(hipMemcpyAsync(flag.data(), (const char *)workspace_dev + wl.lflag, n_proofs * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    H2W_HIP(hipStreamSynchronize(stream));
    for (uint64_t i = 0; i < n_proofs; i++) if (!host_status[i]) host_status[i] = flag[i];      // (the strands' conditions come first, as in round 2)
    return 0;
}
int h2w_plan_timing(h2w_plan *p, uint64_t back, float ms[5]) {   // `back` batches before the last one (ring of 64)
    const DevEvent *ev = call_events(p, back, "h2w_plan_timing: no such batch");
    if (!ev) return -1;
    DeviceGuard dg(p->device);
    H2W_HIP(hipEventSynchronize(ev[H2W_EV_CALL_END]));
    H2W_HIP(hipEventElapsedTime(&ms[0], ev[H2W_EV_CALL_START], ev[H2W_EV_PROLOGUE_END]));   // prologue strands: values (+ with PoseidonBN254 caps: their permutations' records)
    H2W_HIP(hipEventElapsedTime(&ms[1], ev[H2W_EV_GLUE_START], ev[H2W_EV_GLUE_END]));   // query glue strands (+ Goldilocks caps: Merkle strands, values, and every listed permutation's records)
    H2W_HIP(hipEventElapsedTime(&ms[2], ev[H2W_EV_CHAINS_START], ev[H2W_EV_CHAINS_END]));   // PoseidonBN254 Merkle chains: values + emission (on their side stream; 0 for Goldilocks-Poseidon Merkle)
    H2W_HIP(hipEventElapsedTime(&ms[3], ev[H2W_EV_EXPAND_START], ev[H2W_EV_EXPAND_END]));   // expansion kernel
    H2W_HIP(hipEventElapsedTime(&ms[4], ev[H2W_EV_CALL_START], ev[H2W_EV_CALL_END]));   // whole call
    return 0;
}
int h2w_plan_timing_ex(h2w_plan *p, uint64_t back, float ms[8]) {
    const DevEvent *ev = call_events(p, back, "h2w_plan_timing_ex: no such batch");
    if (!ev) return -1;
    DeviceGuard dg(p->device);
    H2W_HIP(hipEventSynchronize(ev[H2W_EV_CALL_END]));
    H2W_HIP(hipEventElapsedTime(&ms[0], ev[H2W_EV_CALL_START], ev[h2w_plan::EV_PROLOGUE_VALUES_END]));    // k_prologue_values
    H2W_HIP(hipEventElapsedTime(&ms[1], ev[h2w_plan::EV_GLP_START], ev[h2w_plan::EV_GLP_END]));  // k_glp_emit
    H2W_HIP(hipEventElapsedTime(&ms[2], ev[H2W_EV_GLUE_START], p->shape.hash_mode == 0 ? ev[h2w_plan::EV_GLP_START] : ev[H2W_EV_GLUE_END]));   // k_strands (+ k_merkle_gl_values)
    H2W_HIP(hipEventElapsedTime(&ms[3], ev[H2W_EV_CHAINS_START], ev[h2w_plan::EV_CHAIN_VALUES_END]));   // k_merkle_bn_values
    H2W_HIP(hipEventElapsedTime(&ms[4], ev[h2w_plan::EV_CHAIN_VALUES_END], ev[H2W_EV_CHAINS_END]));   // k_merkle_bn_emit
    H2W_HIP(hipEventElapsedTime(&ms[5], ev[H2W_EV_EXPAND_START], ev[H2W_EV_EXPAND_END]));    // expansion kernel
    H2W_HIP(hipEventElapsedTime(&ms[6], ev[H2W_EV_CALL_START], ev[H2W_EV_CALL_END]));    // whole call
    ms[7] = p->shape.hash_mode == 1 ? (float)p->passes_of[(p->n_batches - 1 - back) % h2w_plan::EV_RING] : 0.f;
    return 0;
}
int h2w_plan_last_timing(h2w_plan *p, float ms[5]) { return h2w_plan_timing(p, 0, ms); }
int h2w_plan_event_gap(h2w_plan *p, uint64_t back_a, int which_a, uint64_t back_b, int which_b, float *ms) {
    const char *none = "h2w_plan_event_gap: no such batch / event";
    if (!ms || which_a < 0 || which_a >= H2W_EV_COUNT || which_b < 0 || which_b >= H2W_EV_COUNT) { set_error(none); return -1; }
    const DevEvent *ev_a = call_events(p, back_a, none), *ev_b = call_events(p, back_b, none);
    if (!ev_a || !ev_b) return -1;
    if (p->shape.hash_mode == 0 && (which_a == H2W_EV_CHAINS_START || which_a == H2W_EV_CHAINS_END || which_b == H2W_EV_CHAINS_START || which_b == H2W_EV_CHAINS_END)) { set_error("h2w_plan_event_gap: no chain kernel with Goldilocks-Poseidon caps"); return -1; }
    hipEvent_t a = ev_a[which_a], b = ev_b[which_b];
    DeviceGuard dg(p->device);
    H2W_HIP(hipEventSynchronize(a)); H2W_HIP(hipEventSynchronize(b));
    H2W_HIP(hipEventElapsedTime(ms, a, b));
    return 0;
}
int h2w_plan_configure(h2w_plan *p, int option, int value) {
    if (!p) { set_error("h2w_plan_configure: null plan"); return -1; }
    if (option == H2W_OPT_FORK_CHAINS) { p->fork_chains = value != 0; return 0; }
    if (option == H2W_OPT_SERIAL_EXPAND) { p->serial_expand = value != 0; return 0; }      // (negative: the default, on)
    if (option == H2W_OPT_VALUES_FORM) { if (value < 0 || value > 2) { set_error("h2w_plan_configure: H2W_OPT_VALUES_FORM is 0 (by launch size), 1 (four lanes per path) or 2 (one wavefront per path)"); return -1; } p->values_form = value; return 0; }
    if (option == H2W_OPT_CHAIN_PASSES) { if (value < 0 || value > 2) { set_error("h2w_plan_configure: H2W_OPT_CHAIN_PASSES is 0 (by launch size), 1 or 2"); return -1; } p->chain_passes = value; return 0; }
    if (option == H2W_OPT_OUTPUT_FORM) {
        if (value != H2W_FORM_CANONICAL && value != H2W_FORM_MONTGOMERY) { set_error("h2w_plan_configure: H2W_OPT_OUTPUT_FORM is 0 (canonical cells) or 1 (Montgomery form, R = 2^256)"); return -1; }
        if (value == H2W_FORM_MONTGOMERY && p->traced && !p->trace_forms) { set_error("h2w_plan_configure: a traced plan (h2w_plan_from_trace) writes canonical cells only; convert its stream with h2w_advice_to_montgomery, or lower the trace with H2W_TRACE_OUTPUT_FORMS"); return -1; }
        if (value == H2W_FORM_MONTGOMERY && p->device >= 0 && !p->d_mont.get()) {      // first use: the form's constants (derived from r) and the direct-cell bitmap
            DeviceGuard dg(p->device);
            MontForm K; montform_init(K, p->tt.rb);
            DevBuf<uint64_t> bits, ranged; DevBuf<MontForm> d; DevBuf<fr_t> tabm;
            if (bits.upload(p->direct_bits) != 0 || d.upload(&K, 1) != 0) return -1;      // (nothing kept: the next call starts over)
            if (traced_mont_tables(p, tabm, ranged) != 0) return -1;      // (a traced plan with fused PoseidonBN254 permutations: the emitter's Montgomery cell table, the ranged kernel's map)
            p->d_direct_bits = std::move(bits); p->d_mont = std::move(d); p->d_bn_tab_mont = std::move(tabm); p->d_ranged_bits = std::move(ranged);
        }
        p->output_form = value; return 0;
    }
    set_error("h2w_plan_configure: unknown option"); return -1;
}

}  // extern "C"