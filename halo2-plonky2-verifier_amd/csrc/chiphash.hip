// chiphash.hip - batched hash and Merkle chip ops on the device (include/h2w.h 2c, ops 9-13): n independent instances of ONE of
//   PoseidonPermutationChip::permute / PoseidonBN254PermutationChip::permute   hash/poseidon/permutation.rs:270-284, poseidon_bn254/permutation.rs:190-203
//   HasherChip::hash_no_pad / two_to_one                                       hash/poseidon/hash.rs:161-214, hash/poseidon_bn254/hash.rs:156-209
//   MerkleTreeChip::verify_proof_to_cap                                        merkle/mod.rs:80-102
// each in a fresh Context, its operands loaded the way the verifier's WitnessChip loads them (chiphash.h hash_program), the shape of the reference's own chip
// tests (permutation.rs:325-347, poseidon_bn254/permutation.rs:266-301, hash.rs test_hash_no_pad / test_hash_two_to_one, merkle/mod.rs:136-265).
// The single-source chips (chips.h) on the device sinks the batched verifier runs them on, behind a front end that knows no proof shape:
//   Goldilocks-Poseidon (hash_mode 0, GL_PERMUTE)   k_chiphash_gl: one wavefront per instance walks the op wave-uniformly on the values-phase sink
//       (glcoop.h CoopSinkT<false, true, 0>): lane 0 stores the load / select records and direct cells, every permutation runs on values with
//       glp_permute_lanes and is listed {first record, input state}; k_chiphash_glp_emit: one wavefront per listed permutation writes its 2,604 records
//       (CoopSinkT::coop_poseidon_permute, as k_glp_emit_traced); the expansion kernel turns the records into cells.
//   PoseidonBN254 (hash_mode 1, BN_PERMUTE)         k_chiphash_bn: one quad per instance walks the op and emits every permutation's 4,032 cells itself
//       (bnquad.h QuadSinkT<false, QUAD_FUSED>::bn_emit_cells<false>, as k_merkle_bn_fused); lane 0 of the quad stores the Goldilocks-level records (leaf
//       loads) and the other direct cells.  The quads of a wavefront run the same program in lockstep; tail quads redo the last instance.
//   k_chiphash_check                                one lane per (instance, operand item): status 4 for a word outside its field / an index >= 2^depth.
//                                                   (also launched for h2w_chipbatch_values: chiphash_launch_check, the verdicts' status words two words apart)
// The layout of an instance (record metas, cells, listed permutations) is one host replay of the same program on the sequential gadgets.
// The program, its parameters and operand layout and the handle's part live in chiphash.h: chipvalues.hip runs the same program for results and verdicts.
#define H2W_FLATTEN_CHIPS 1      // the gadget stack inlined into the two value kernels (field.h HNI): the sinks below exist in this unit alone
#include <hip/hip_runtime.h>
#include <vector>
#include "chiphash.h"

namespace h2w {

constexpr uint64_t CHIPHASH_WS_BYTES = 512ull << 20;      // default bound of a call's internal workspace (records, permutation lists): instances per launch = this / bytes per instance
constexpr uint64_t CHIPHASH_MAX_CHUNK = 32768;            // instances per launch at most (grid.y of the expansion kernel)

// host: lays out the instance (record metas, cell count, listed Goldilocks-Poseidon permutations) - the sequential gadgets: a permutation's record block
// is the GLP_RECS records coop_poseidon_permute writes
struct HashLayoutSink : SinkBase {
    const TemplateTable *tt; std::vector<uint64_t> meta; uint64_t cell_off = 0; uint32_t nglp = 0;
    void rec(int t, uint64_t, uint64_t, uint64_t, uint64_t) { meta.push_back(meta_pack((uint32_t)t, cell_off)); cell_off += (uint64_t)tt->ncells(t); }
    void cell(const fr_t &) { cell_off++; }
    void skip(uint64_t, uint64_t) {}
    void glp_note() { nglp++; }
};

struct HashArgs {
    HashParams hp; int L; FrParams P; const uint64_t *operands; uint32_t nw; rec_t *recs; uint64_t nrec, ncells, n; fr_t *out; const uint16_t *tmpl_cells; const fr_t *inv;
    const h2w_poseidon_consts_t *consts; uint64_t *glist; uint32_t nglp; int small_mds;      // Goldilocks-Poseidon: the constants (+ derived tables), the list [instance][entry][GLP_LIST_WORDS]
    const fr_t *bn_tab;                                                                       // PoseidonBN254: the tables (bntab.h)
};
// (thin derived sinks: the flattened value backends of this unit are instantiated nowhere else - field.h HNI)
struct HashCoopSink : CoopSinkT<false, true, 0> {};
struct HashQuadSink : QuadSinkT<false, QUAD_FUSED> {};

__global__ __launch_bounds__(64) __attribute__((flatten)) void k_chiphash_gl(HashArgs A) {
    typedef ValBackend<HashCoopSink> CoopB;
    stage_glp_consts<true>(A.consts, threadIdx.x, 64);
    const uint64_t i = blockIdx.x;      // (the grid is the instances of the launch)
    HashCoopSink sink; sink.recs = A.recs + i * A.nrec; sink.out = A.out + i * A.ncells; sink.ncells = A.tmpl_cells; sink.lane = threadIdx.x; sink.cc.init(flat_cols());
    sink.glp = A.glist + i * (uint64_t)A.nglp * GLP_LIST_WORDS; sink.small_mds = A.small_mds != 0; sink.bind_lds();
    sink.nrec = 0; sink.cell_off = 0; sink.glp_slot = 0; sink.emit = true;
    CoopB be(sink, chiphash_cfg(0, A.L, A.P, A.inv, false), false);
    const HashParams hp = A.hp;
    hash_program<0>(be, hp, A.consts, A.operands + i * (uint64_t)A.nw, NoHashOut());
}

// one wavefront per listed permutation of the launch: its GLP_RECS records from the entry {first record, input state} (replay.hip k_glp_emit_traced)
struct HashEmitArgs { const h2w_poseidon_consts_t *consts; const uint64_t *list; rec_t *recs; uint64_t nrec; const uint16_t *tmpl_cells; uint32_t nglp; };
__global__ __launch_bounds__(64) void k_chiphash_glp_emit(HashEmitArgs A) {
    typedef CoopSinkT<false, false> Sink;
    const uint64_t i = blockIdx.x / A.nglp;
    stage_glp_consts(A.consts, threadIdx.x, 64);
    Sink sink; sink.recs = A.recs + i * A.nrec; sink.out = nullptr; sink.ncells = A.tmpl_cells; sink.lane = threadIdx.x; sink.bind_lds(); sink.cell_off = 0; sink.emit = true;
    const uint64_t *ent = A.list + (uint64_t)blockIdx.x * GLP_LIST_WORDS;
    const uint64_t w = threadIdx.x < GLP_LIST_WORDS ? g_load_u64(ent + threadIdx.x) : 0;
    uint64_t st[SPONGE_WIDTH];
#pragma unroll
    for (int j = 0; j < SPONGE_WIDTH; j++) st[j] = readlane64(w, j + 1);
    sink.nrec = readlane64(w, 0);
    sink.coop_poseidon_permute(st, A.consts);
}

// LDS: the tables (34.7 KB) + 10 KB of value slots per wavefront, as k_merkle_bn_fused.  The quads of a wavefront cooperate in the emitter's layer
// streams: no wavefront leaves early, tail quads redo the last instance and write identical bytes.
__global__ __launch_bounds__(QUAD_BLOCK) H2W_QUAD_ATTR __attribute__((flatten)) void k_chiphash_bn(HashArgs A) {
    typedef ValBackend<HashQuadSink> QuadB;
    stage_bn_consts(A.bn_tab, threadIdx.x, QUAD_BLOCK);      // (block-wide barrier inside: before any wavefront leaves)
    if ((((uint64_t)blockIdx.x * QUAD_BLOCK + (threadIdx.x & ~63u)) >> 2) >= A.n) return;      // a whole wavefront past the last instance
    uint64_t i = ((uint64_t)blockIdx.x * QUAD_BLOCK + threadIdx.x) >> 2;
    if (i >= A.n) i = A.n - 1;
    HashQuadSink sink; sink.recs = A.recs + i * A.nrec; sink.nrec = 0; sink.out = A.out + i * A.ncells; sink.cell_off = 0; sink.ncells = A.tmpl_cells; sink.l4 = threadIdx.x & 3;
    sink.cc.init(flat_cols()); sink.ustate = nullptr; sink.sbx = nullptr;
    QuadB be(sink, chiphash_cfg(1, A.L, A.P, A.inv, true), false);      // a fresh Context: its first permutation holds the cached load_zero cell
    const HashParams hp = A.hp;
    hash_program<1>(be, hp, nullptr, A.operands + i * (uint64_t)A.nw, NoHashOut());
}

// status 4: one lane per (instance, item) - a Goldilocks word, the leaf index, a hash (four Goldilocks words or one Fr); the argument block: chiphash.h
__global__ __launch_bounds__(256) void k_chiphash_check(CheckArgs C) {
    const uint32_t items = C.o.n_gl + C.o.has_idx + C.o.n_hash;
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x, i = g / items; const uint32_t j = (uint32_t)(g % items);
    if (i >= C.n) return;
    const uint64_t *w = C.operands + i * (uint64_t)C.o.nw;
    bool bad;
    if (j < C.o.n_gl) bad = g_load_u64(w + j) >= GL_P;
    else if (C.o.has_idx && j == C.o.n_gl) bad = (g_load_u64(w + j) >> C.depth) != 0;      // (depth <= 32)
    else {
        const uint64_t *h = w + C.o.n_gl + C.o.has_idx + 4ull * (j - C.o.n_gl - C.o.has_idx);
        fr_t v; for (int t = 0; t < 4; t++) v.l[t] = g_load_u64(h + t);
        bad = C.o.fr_hashes ? fr_geq_mod(v) : (v.l[0] >= GL_P || v.l[1] >= GL_P || v.l[2] >= GL_P || v.l[3] >= GL_P);
    }
    if (bad) atomicOr(&C.status[i * C.stride], 4u);
}
void chiphash_launch_check(const CheckArgs &K, hipStream_t stream) {
    const uint64_t items = (uint64_t)(K.o.n_gl + K.o.has_idx + K.o.n_hash) * K.n;
    hipLaunchKernelGGL(k_chiphash_check, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, K);
}

void chiphash_free(h2w_chipbatch *h) { delete h->hash; h->hash = nullptr; }

int chiphash_run(h2w_chipbatch *h, const uint64_t *operands_dev, uint64_t n, void *advice_dev, uint32_t *status_dev, void *stream_) {
    ChipHash *c = h->hash;
    DeviceGuard dg(h->device);
    hipStream_t stream = (hipStream_t)stream_;
    const size_t per_recs = (size_t)h->nrec * sizeof(rec_t), per_list = (size_t)c->nglp * GLP_LIST_WORDS * sizeof(uint64_t), per = per_recs + per_list + sizeof(uint32_t);
    uint64_t CH = c->chunk ? c->chunk : CHIPHASH_WS_BYTES / per;
    if (CH < 1) CH = 1; if (CH > CHIPHASH_MAX_CHUNK) CH = CHIPHASH_MAX_CHUNK; if (CH > n) CH = n;
    char *ws = nullptr; const size_t b_recs = CH * per_recs, b_list = CH * per_list, b_ctr = CH * sizeof(uint32_t);
    H2W_HIP(hipMallocAsync((void **)&ws, b_recs + b_list + b_ctr, stream));
    auto run = [&]() -> int {
        for (uint64_t first = 0; first < n; first += CH) {
            const uint64_t m = n - first < CH ? n - first : CH;
            HashArgs A; A.hp = c->hp; A.L = h->L; A.P = h->P; A.operands = operands_dev + first * (uint64_t)h->nw; A.nw = (uint32_t)h->nw; A.recs = (rec_t *)ws; A.nrec = h->nrec; A.ncells = h->ncells; A.n = m;
            A.out = (fr_t *)advice_dev + first * h->ncells; A.tmpl_cells = h->d_tmpl_cells.get(); A.inv = c->d_inv.get();
            A.consts = c->d_consts.get(); A.glist = (uint64_t *)(ws + b_recs); A.nglp = c->nglp; A.small_mds = c->small_mds; A.bn_tab = c->d_bn_tab.get();
            uint32_t *const status = status_dev + first;
            H2W_HIP(hipMemsetAsync(status, 0, m * sizeof(uint32_t), stream));
            CheckArgs K; K.operands = A.operands; K.o = c->o; K.depth = c->hp.depth; K.n = m; K.status = status; K.stride = 1;
            chiphash_launch_check(K, stream);
            if (c->bn) hipLaunchKernelGGL(k_chiphash_bn, dim3((unsigned)((m * 4 + QUAD_BLOCK - 1) / QUAD_BLOCK)), dim3(QUAD_BLOCK), 0, stream, A);
            else {
                hipLaunchKernelGGL(k_chiphash_gl, dim3((unsigned)m), dim3(64), 0, stream, A);
                HashEmitArgs G; G.consts = c->d_consts.get(); G.list = A.glist; G.recs = A.recs; G.nrec = h->nrec; G.tmpl_cells = h->d_tmpl_cells.get(); G.nglp = c->nglp;
                if (c->nglp) hipLaunchKernelGGL(k_chiphash_glp_emit, dim3((unsigned)(m * c->nglp)), dim3(64), 0, stream, G);
            }
            if (h->nrec) {      // expansion of the block records
                ExpandArgs E;
                E.meta = h->d_meta.get(); E.recs = A.recs; E.nrec = h->nrec; E.rec_stride = h->nrec; E.out = A.out; E.cell_stride = h->ncells; E.pool = nullptr;
                E.cm = flat_cols(); expand_unsharded(E);
                h->dt.fill(E);
                E.tile_ctr = (uint32_t *)(ws + b_recs + b_list);
                H2W_HIP(hipMemsetAsync(E.tile_ctr, 0, m * sizeof(uint32_t), stream));
                int gx = (int)(2048 / (m < 2048 ? m : 2048)); if (gx < 1) gx = 1;      // (launch_expand bounds it by the instance's tiles)
                if (launch_expand(E, m, gx, stream) != 0) return -1;
            }
            H2W_HIP(hipGetLastError());
        }
        return 0;
    };
    const int rc = run();
    (void)hipFreeAsync(ws, stream);
    return rc;
}

}  // namespace h2w

using namespace h2w;

extern "C" {

h2w_chipbatch *h2w_chipbatch_new_hash(int op, const h2w_poseidon_consts_t *consts, int hash_mode, uint32_t n_in, uint32_t depth, uint32_t cap_height, int lookup_bits, int device_id) {
    auto refuse = [](const char *why) -> h2w_chipbatch * { set_error(std::string("h2w_chipbatch_new_hash: ") + why); return nullptr; };
    if (op >= H2W_OP_GL_ADD && op <= H2W_OP_EXT_DIV) return refuse("the field ops (0-8) take no parameters: use h2w_chipbatch_new");
    if (op < H2W_OP_GL_PERMUTE || op > H2W_OP_MERKLE_VERIFY) return refuse("unknown op");
    if (!consts) return refuse("null argument");
    if (lookup_bits < 2 || lookup_bits > 28) return refuse("lookup_bits outside [2, 28]");
    const bool perm = op == H2W_OP_GL_PERMUTE || op == H2W_OP_BN_PERMUTE, uses_n_in = op == H2W_OP_HASH_NO_PAD || op == H2W_OP_MERKLE_VERIFY, merkle = op == H2W_OP_MERKLE_VERIFY;
    if (!perm && hash_mode != 0 && hash_mode != 1) return refuse("hash_mode is 0 (Goldilocks-Poseidon) or 1 (PoseidonBN254)");
    if (op == H2W_OP_BN_PERMUTE && hash_mode != 0) return refuse("BN_PERMUTE takes no hash_mode: an unused parameter must be 0");
    if ((!uses_n_in && n_in != 0) || (!merkle && (depth != 0 || cap_height != 0))) return refuse("an unused parameter must be 0");
    if (uses_n_in && (n_in < 1 || n_in > H2W_CHIPBATCH_MAX_N_IN)) return refuse("n_in outside [1, H2W_CHIPBATCH_MAX_N_IN]");
    if (merkle && (depth < 1 || depth > 32)) return refuse("depth outside [1, 32]");
    if (merkle && (cap_height > depth || cap_height > 6)) return refuse("cap_height above min(depth, 6)");
    h2w_chipbatch *h = new h2w_chipbatch(lookup_bits);
    ChipHash *c = new ChipHash; h->hash = c;
    c->hp = HashParams{op, op == H2W_OP_GL_PERMUTE ? 0 : op == H2W_OP_BN_PERMUTE ? 1 : hash_mode, n_in, depth, cap_height};
    c->o = operand_layout(c->hp); c->bn = c->hp.mode == 1; c->small_mds = glp_small_mds(*consts) ? 1 : 0;
    h->op = op; h->L = lookup_bits; h->device = device_id; h->nw = (int)c->o.nw; h->P = fr_params_init();
    const std::vector<fr_t> inv = inverse_table(h->P);      // Assigned::Rational(1, x) of is_zero (the cap lookup's indicator)
    HashLayoutSink ls; ls.tt = &h->tt;
    {   // layout of one instance: replay on harmless operands (all zero: in every field, index 0)
        ValBackend<HashLayoutSink> be(ls, chiphash_cfg(c->hp.mode, lookup_bits, h->P, inv.data(), false), false);
        const std::vector<uint64_t> zeros(c->o.nw, 0);
        hash_program<-1>(be, c->hp, consts, zeros.data(), NoHashOut());
    }
    h->nrec = ls.meta.size(); h->ncells = ls.cell_off; c->nglp = ls.nglp;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { h->device = -1; return h; }      // layout queries still work; h2w_chipbatch_run fails
    if (device_id < 0 || device_id >= ndev) { set_error("h2w_chipbatch_new_hash: device_id out of range"); h->device = -1; h2w_chipbatch_free(h); return nullptr; }
    DeviceGuard dg(device_id);
    // the tables of the op's hash: PoseidonBN254's (with the limb-form copy and the row constants of the values call), or the Goldilocks-Poseidon constants (handletabs.h)
    rf::RowConst rk; rf::rowconst_init(rk, h->P);
    if (h->dt.upload(h->tt) != 0 || h->d_meta.upload(ls.meta) != 0 || upload_tmpl_cells(h->d_tmpl_cells, h->tt) != 0 || c->d_inv.upload(inv) != 0 ||
        (c->bn ? (upload_bn_tab(c->d_bn_tab, *consts, h->P, &c->d_bn_tab9) != 0 || c->d_rowk.upload(&rk, 1) != 0) : upload_glp_consts(c->d_consts, *consts) != 0)) { h2w_chipbatch_free(h); return nullptr; }
    return h;
}

int h2w_chipbatch_configure(h2w_chipbatch *h, int option, uint64_t value) {
    if (!h) { set_error("h2w_chipbatch_configure: null argument"); return -1; }
    if (!h->hash) { set_error("h2w_chipbatch_configure: a handle of h2w_chipbatch_new has no options"); return -1; }
    if (option != H2W_CHIPBATCH_OPT_CHUNK) { set_error("h2w_chipbatch_configure: unknown option"); return -1; }
    if (value < 1 || value > CHIPHASH_MAX_CHUNK) { set_error("h2w_chipbatch_configure: H2W_CHIPBATCH_OPT_CHUNK outside [1, 32768]"); return -1; }
    h->hash->chunk = value;
    return 0;
}

}  // extern "C"
