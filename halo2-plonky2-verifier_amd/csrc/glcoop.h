// glcoop.h — the Goldilocks-Poseidon wavefront sink (device only; the PoseidonBN254 quad sink is bnquad.h).
//
// CoopSink: one 64-lane wavefront executes one strand of verifier.h *wave-uniformly* (every lane runs the same
// gadget code on the same values; lane 0 alone writes records / direct cells), and the lanes split up the one
// wide thing in it: the Goldilocks Poseidon permutation (hash/poseidon/permutation.rs:43-284), 12 lanes = the 12
// state elements / MDS rows.
//
// A strand's sponge is a serial chain of permutations, but only in its VALUES: the 2,604 block records of a permutation
// are a function of its input state alone.  So the strand kernels run in two phases:
//   values (CoopSinkT<COLS, true>)  the strand's wavefront computes each permutation's output with the state spread over 12
//                                   lanes (no records, no LDS exchange: broadcasts are v_readlane, the one cross-lane sum of a
//                                   partial round is a DPP row scan) and appends {record index, input state} to the proof's
//                                   permutation list;
//   records (k_glp_emit)            one wavefront per LISTED permutation replays it and writes its records - every permutation
//                                   of every strand of the launch side by side (CoopSinkT<COLS, false>::coop_poseidon_permute).
// Together they emit exactly the records the sequential template code (chips.h PoseidonPermutationChip) emits, at the same
// indices — tests/test_gpu_batch.py compares the resulting advice with the oracle byte for byte.
#pragma once
#include "valbackend.h"
#include "glptab.h"
#include "lanes.h"

namespace h2w {

constexpr int GLP_RECS_FULL = 12 + 48 + 1 + 12 * 14;           // constant_layer, sbox_layer, mds_layer
constexpr int GLP_RECS_PARTIAL_ROUND = 4 + 1 + 1 + 11 + 1 + 11; // sbox, +const, d = m00*s0, d chain, zeros, v row
constexpr int GLP_RECS_PARTIAL = 12 + 1 + 121 + N_PARTIAL_ROUNDS * GLP_RECS_PARTIAL_ROUND;
constexpr int GLP_CONST_WORDS = 360 + 12 + 12 + 12 + 22 + 121 + 242 + 242;   // u64 words of the Goldilocks block of h2w_poseidon_consts_t
constexpr int GLP_RECS = 2 * HALF_N_FULL_ROUNDS * GLP_RECS_FULL + GLP_RECS_PARTIAL;   // 2604

// Goldilocks-Poseidon round constants + MDS, staged in LDS by the cooperative kernels (stage_glp_consts) and read with
// ds_read (a namespace-scope __shared__ array keeps the LDS address space; a pointer member would decay to flat).
__shared__ uint64_t s_glp_k[GLP_CONST_WORDS];
__shared__ uint64_t s_glp_a[SPONGE_WIDTH], s_glp_b[SPONGE_WIDTH];      // the permutation's state exchange buffers
__shared__ uint64_t s_glp_in[CH_BUF];                                  // the challenger's input buffer (values phase of the prologue)
__shared__ uint64_t s_glp_m[SPONGE_WIDTH * SPONGE_WIDTH];              // MDS as a dense matrix, row-major: M[r][j] = circ[(j - r) mod 12] + [j == r] diag[r]  (values phase)
// LDS pointers are handed to the (out-of-line) permutation through the sink: a __shared__ array that several kernels use is reached
// from a non-kernel function through llvm.amdgcn.lds.offset.table - a GLOBAL load of the offset at every use, i.e. a vmcnt(0) wait
// for every record store in flight, inside the round loops (that was 60 of the 89 us of a permutation).  A kernel knows the
// addresses at compile time and passes them down.
__shared__ uint64_t s_glp_x[GLP_AUX_WORDS];                             // the derived tables of the partial rounds (glptab.h; values phase)
typedef __attribute__((address_space(3))) uint64_t lds64_t;
constexpr int KO_ARC = 0, KO_CIRC = 360, KO_DIAG = 372, KO_FIRST = 384, KO_PRC = 396, KO_INIT = 418, KO_WHAT = 539, KO_VS = 781;
static_assert(KO_VS + 242 == GLP_CONST_WORDS, "Goldilocks constant block layout");
// AUX: also the derived tables (the kernels of the values phase; they sit behind the struct: h2w_plan's device copy)
template <bool AUX = false> __device__ __forceinline__ void stage_glp_consts(const h2w_poseidon_consts_t *k, int tid, int nthreads) {
    const uint64_t *src = reinterpret_cast<const uint64_t *>(k);
    for (int i = tid; i < GLP_CONST_WORDS; i += nthreads) s_glp_k[i] = g_load_u64(src + i);
    if constexpr (AUX) { const uint64_t *ax = reinterpret_cast<const uint64_t *>(k + 1); for (int i = tid; i < GLP_AUX_WORDS; i += nthreads) s_glp_x[i] = g_load_u64(ax + i); }
    for (int i = tid; i < SPONGE_WIDTH * SPONGE_WIDTH; i += nthreads) {
        const int r = i / SPONGE_WIDTH, j = i % SPONGE_WIDTH; int d = j - r; if (d < 0) d += SPONGE_WIDTH;
        const uint64_t c = g_load_u64(src + KO_CIRC + d);
        s_glp_m[i] = j == r ? gl_reduce128((u128)c + g_load_u64(src + KO_DIAG + r)) : c;      // (c + diag) v = c v + diag v in the field
    }
    __syncthreads();
}
// plonky2's MDS entries are tiny (<= 41): a row is then two 64-bit sums of 32-bit halves and ONE reduction (the prover's trick, prover.hip).
// Below 2^26 each, a dense entry circ + diag is below 2^27 and a sum of 12 terms plus a constant word below 2^63 (glq_reduce96's precondition, glperm.h).
inline bool glp_small_mds(const h2w_poseidon_consts_t &k) {
    for (int i = 0; i < SPONGE_WIDTH; i++) if (k.mds_circ[i] >= (1ull << 26) || k.mds_diag[i] >= (1ull << 26)) return false;
    return true;
}

__device__ __forceinline__ uint64_t gl_add_c(uint64_t x, uint64_t y) {   // canonical x + y mod p
    uint64_t t = x + y;
    if (t < x || t >= GL_P) t -= GL_P;
    return t;
}
}      // namespace h2w
#include "glperm.h"
namespace h2w {
constexpr int GLP_LIST_WORDS = 1 + SPONGE_WIDTH;            // one listed permutation: {index of its first record, input state}

// VALPH: the values phase of a strand (see the top of the file); false: the record-emitting permutation (k_glp_emit)
template <bool COLS, bool VALPH = false, int HASH_MODE = -1> struct CoopSinkT : SinkBase {
    static constexpr bool kCoop = true, kDevSponge = VALPH; static constexpr int kHashMode = HASH_MODE;
    rec_t *recs; uint64_t nrec; fr_t *out; uint64_t cell_off; const uint16_t *ncells; int lane; ColPolicy<COLS> cc;
    lds64_t *lk = nullptr, *la = nullptr, *lb = nullptr, *lm = nullptr, *lx = nullptr;      // s_glp_k, s_glp_a, s_glp_b, s_glp_m (s_glp_x: values phase) of the running kernel (set by bind_lds)
    uint64_t *glp = nullptr; uint32_t glp_slot = 0; bool small_mds = false;   // values phase: this proof's permutation list, the next slot of this strand
    __device__ __forceinline__ void bind_lds() { lk = (lds64_t *)s_glp_k; la = (lds64_t *)s_glp_a; lb = (lds64_t *)s_glp_b; lm = (lds64_t *)s_glp_m; if constexpr (VALPH) lx = (lds64_t *)s_glp_x; }
    bool emit = true;            // false: values only (a sharded run computes every prologue for its challenges, but only the owning rank emits it)
    __device__ __forceinline__ void rec(int t, uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
        if (lane == 0 && emit) g_store_rec(recs + nrec, a, b, c, d);
        nrec++; cell_off += ncells[t];
    }
    __device__ __forceinline__ void cell(const fr_t &v) { if (lane == 0 && emit) g_store_fr(out + cc.map(cell_off), v); cell_off++; }
    __device__ __forceinline__ void skip(uint64_t nr, uint64_t nc) { nrec += nr; cell_off += nc; }
    // WitnessChip::load_proof_with_pis (witness/mod.rs:267-294) and the limb decompositions of the caps' BN254 hashes are k_prologue_load's
    // (every item is independent: one lane each); the strand only steps over their records and cells
    __device__ __forceinline__ bool coop_load_proof(const ValCfg &cfg) { nrec += cfg.load_nrec; cell_off += cfg.load_ncell; return true; }
    // ---- the Fiat-Shamir sponge of the values phase (ChallengerChip, challenger/mod.rs:19-126; overwrite-mode duplex, rate 8): the state
    // lives on the lanes (lane l: element l), the input buffer in LDS; every permutation is listed for k_glp_emit
    uint64_t sx = 0; int sp_in = 0, sp_out = 0; lds64_t *lin = nullptr;
    __device__ __forceinline__ void sponge_init() { sx = 0; sp_in = sp_out = 0; lin = (lds64_t *)s_glp_in; }
    __device__ __forceinline__ bool sponge_observe(uint64_t t) { sp_out = 0; if (sp_in >= CH_BUF) return false; lin[sp_in++] = t; return true; }
    template <class WordFn> __device__ __forceinline__ bool sponge_observe_words(const uint64_t *proof, int n, WordFn word) {      // n proof words, one lane each
        sp_out = 0; if (sp_in + n > CH_BUF) return false;
        for (int base = 0; base < n; base += 64) { const int i = base + lane; if (i < n) lin[sp_in + i] = g_load_u64(proof + word(i)); }
        sp_in += n; return true;
    }
    // proof words staged side by side in the (idle) input buffer, one lane a word: what the strand then reads one by one costs an LDS read each instead
    // of a dependent global load (~2.4 k cycles for a wavefront with nothing else to run)
    template <class WordFn> __device__ __forceinline__ void stage_words(const uint64_t *proof, int at, int n, WordFn word) {
        for (int base = 0; base < n; base += 64) { const int i = base + lane; if (i < n) lin[at + i] = g_load_u64(proof + word(i)); }
    }
    __device__ __forceinline__ uint64_t staged_word(int i) const { return lin[i]; }
    // observe_cap (challenger/mod.rs:65-74): hash j of the cap on lane j; Goldilocks hashes are their 4 words, BN254 hashes 5 limbs of 56 bits
    // (HashWire::to_goldilocks_vec, hash/poseidon_bn254/hash.rs:31-43: decompose_le(56, 5) - its cells are k_prologue_load's)
    __device__ __forceinline__ bool sponge_observe_cap(const uint64_t *proof, uint64_t w0, int n, int mode, int L) {      // (inlined, like sponge_challenge: an out-of-line member takes the sink's address, and a sink in memory pays a scratch round trip behind the record stores for every counter it bumps)
        const int per = mode == 0 ? 4 : 5;
        sp_out = 0; if (sp_in + per * n > CH_BUF) return false;
        for (int base = 0; base < n; base += 64) {
            const int j = base + lane;
            if (j < n) {
                fr_t x; for (int i = 0; i < 4; i++) x.l[i] = g_load_u64(proof + w0 + 4ull * j + i);
                if (mode == 0) for (int i = 0; i < 4; i++) lin[sp_in + 4 * j + i] = x.l[i];
                else for (int t = 0; t < 5; t++) lin[sp_in + 5 * j + t] = fr_bits(x, 56 * t, 56);
            }
        }
        sp_in += per * n;
        if (mode == 1) { const int nl = (56 + L - 1) / L, rem = 56 % L; cell_off += (uint64_t)n * (13 + 5ull * ((nl > 1 ? 1 + 3 * (nl - 1) : 0) + (rem ? 4 : 0))); }
        return true;
    }
    __device__ __forceinline__ void sponge_permute() {
        // list the permutation (lane 0: where its records start; lanes 1..12: the input state), then its values
        // (the list entry is STORED by the permutation, behind its entry: an out-of-line function waits at its entry for every memory operation in
        // flight, and a store issued just before the call was 2.5 k cycles of every permutation)
        const uint64_t up = row_shr64<1>(sx), w = lane == 0 ? nrec : up;
        uint64_t *at = emit && lane < GLP_LIST_WORDS ? glp + (uint64_t)glp_slot * GLP_LIST_WORDS + lane : nullptr;
        glp_slot++;
        sx = glp_permute_lanes(sx, lk, lm, lx, lane, small_mds, at, w);
        nrec += GLP_RECS;
        cell_off += perm_cell_count();
    }
    // cells of one permutation's records (a constant of the run: read from the template table once - a global load behind the list store above
    // waited, every permutation, for that store to drain)
    uint64_t perm_cells_ = 0;
    __device__ __forceinline__ uint64_t perm_cell_count() {
        if (perm_cells_ == 0) {
            const uint64_t nG = ncells[T_GLOP], nKA = ncells[T_KA_GLOP];
            perm_cells_ = 2 * HALF_N_FULL_ROUNDS * (12 * nKA + 48 * nG + 12 + 12 * (1 + 13 * nKA)) + 12 * nKA + 12 + 121 * nKA + (uint64_t)N_PARTIAL_ROUNDS * (4 * nG + nKA + nKA + 11 * nKA + 12 + 11 * nKA);
        }
        return perm_cells_;
    }
    __device__ __forceinline__ uint64_t sponge_challenge() {                   // ChallengerChip::get_challenge (:92-108, :260-277)
        if (sp_in) {
            for (int off = 0; off < sp_in; off += SPONGE_RATE) {
                const int len = sp_in - off < SPONGE_RATE ? sp_in - off : SPONGE_RATE;
                if ((lane & 15) < len) sx = lin[off + (lane & 15)];      // (every 16-lane row alike: glperm.h)
                sponge_permute();
            }
            sp_in = 0; sp_out = SPONGE_RATE;
        } else if (sp_out == 0) { sponge_permute(); sp_out = SPONGE_RATE; }
        return readlane64(sx, --sp_out);
    }

#if defined(H2W_FLATTEN_CHIPS)      // (glue.hip: the values strands, flattened - the state array stays in registers)
    __device__ __forceinline__
#else
    __device__ __noinline__
#endif
    void coop_poseidon_permute(uint64_t *st, const h2w_poseidon_consts_t *) {
        if constexpr (VALPH) {
            // values phase: list the permutation (lane 0: where its records start; lanes 1..12: the input state), compute its output
            uint64_t w = nrec, x = 0;
#pragma unroll
            for (int i = 0; i < SPONGE_WIDTH; i++) { if (lane == i + 1) w = st[i]; if ((lane & 15) == i) x = st[i]; }      // (every 16-lane row alike: glperm.h)
            uint64_t *at = emit && lane < GLP_LIST_WORDS ? glp + (uint64_t)glp_slot * GLP_LIST_WORDS + lane : nullptr;
            glp_slot++;
            x = glp_permute_lanes(x, lk, lm, lx, lane, small_mds, at, w);
#pragma unroll
            for (int i = 0; i < SPONGE_WIDTH; i++) st[i] = readlane64(x, i);
            nrec += GLP_RECS;
            cell_off += perm_cell_count();
            return;
        }
        lds64_t *const K = lk, *const s_a = la, *const s_b = lb;      // (by value: one read of the sink object per call)
        rec_t *R = recs + nrec;
        const int l = lane, grp13 = lane / 13, idx13 = lane % 13;
        const bool em = emit;
        auto W = [&](int idx, uint64_t A, uint64_t B, uint64_t C) { if (em) g_store_rec(R + idx, A, B, C, 0); };
        if (l < SPONGE_WIDTH) s_a[l] = st[l];
        wave_sync();
        int base = 0, round_ctr = 0;
        auto full_round = [&]() {
            if (l < SPONGE_WIDTH) {
                uint64_t x = s_a[l]; const uint64_t rc = K[KO_ARC + l + SPONGE_WIDTH * round_ctr];
                W(base + l, rc, 1, x); x = gl_add(x, rc);                                   // constant_layer
                const int sb = base + 12 + 4 * l;                                            // sbox_monomial: x^7
                const uint64_t x2 = gl_mul(x, x); W(sb, x, x, 0);
                const uint64_t x4 = gl_mul(x2, x2); W(sb + 1, x2, x2, 0);
                const uint64_t x6 = gl_mul(x4, x2); W(sb + 2, x4, x2, 0);
                const uint64_t x7 = gl_mul(x6, x); W(sb + 3, x6, x, 0);
                s_b[l] = x7;
            }
            wave_sync();
            const int mb = base + 60;                                                        // mds_layer
            // 12 rows x 13 terms: res_i = (sum_{j<=i} c_j v_j) mod p.  Products in parallel (lane = row_in_pass*13 + i, 4 rows
            // per pass), then a segmented inclusive scan over each 13-lane group: 1 product + 4 adds deep instead of 13 mul-adds.
            if (l == 0) W(mb, 0, 0, 0);
            uint64_t rowres = 0;
#pragma unroll
            for (int pass = 0; pass < 3; pass++) {
                const int rr = pass * 4 + grp13;
                uint64_t c = 0, v = 0, x = 0;
                if (l < 52) {
                    if (idx13 < 12) { c = K[KO_CIRC + idx13]; int vi = idx13 + rr; if (vi >= 12) vi -= 12; v = s_b[vi]; }
                    else { c = K[KO_DIAG + rr]; v = s_b[rr]; }
                    x = gl_mul(c, v);
                }
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) { const uint64_t y = shfl_up64(x, d); if (idx13 >= d) x = gl_add_c(x, y); }
                uint64_t prev = shfl_up64(x, 1); if (idx13 == 0) prev = 0;
                if (l < 52) {
                    const int rb = mb + 1 + 14 * rr;
                    if (idx13 == 0) W(rb, 0, 0, 0);
                    W(rb + 1 + idx13, c, v, prev);
                    if (idx13 == 12) rowres = x;
                }
                if (l < 52 && idx13 == 12) s_a[rr] = rowres;
            }
            wave_sync();
            base += GLP_RECS_FULL; round_ctr++;
        };
        for (int i = 0; i < HALF_N_FULL_ROUNDS; i++) full_round();
        // ---- partial rounds (hash/poseidon/permutation.rs:216-239)
        if (l < SPONGE_WIDTH) {                                                              // partial_first_constant_layer
            const uint64_t x = s_a[l], c = K[KO_FIRST + l];
            W(base + l, c, 1, x); s_b[l] = gl_add(x, c);
        }
        wave_sync();
        base += 12;
        if (l == 0) { W(base, 0, 0, 0); s_a[0] = s_b[0]; }                                   // mds_partial_layer_init
        else if (l < SPONGE_WIDTH) {
            uint64_t res = 0;
            for (int r = 1; r < SPONGE_WIDTH; r++) {
                const uint64_t t = K[KO_INIT + (r - 1) * 11 + (l - 1)], v = s_b[r];
                W(base + 1 + (r - 1) * 11 + (l - 1), t, v, res); res = gl_muladd(t, v, res);
            }
            s_a[l] = res;
        }
        wave_sync();
        base += 122;
        for (int r = 0; r < N_PARTIAL_ROUNDS; r++) {
            if (l == 0) {
                const uint64_t x = s_a[0];
                const uint64_t x2 = gl_mul(x, x); W(base, x, x, 0);
                const uint64_t x4 = gl_mul(x2, x2); W(base + 1, x2, x2, 0);
                const uint64_t x6 = gl_mul(x4, x2); W(base + 2, x4, x2, 0);
                const uint64_t x7 = gl_mul(x6, x); W(base + 3, x6, x, 0);
                const uint64_t c = K[KO_PRC + r];
                W(base + 4, c, 1, x7); s_a[0] = gl_add(x7, c);
            }
            wave_sync();
            const uint64_t s0 = s_a[0];                                                      // mds_partial_layer_fast
            {   // d = m00*s0 + sum_i w_hat_i * st_i as an inclusive scan over lanes 0..11 (records need every partial sum)
                uint64_t t = 0, v = 0, x = 0;
                if (l == 0) { t = K[KO_CIRC] + K[KO_DIAG]; v = s0; }
                else if (l < SPONGE_WIDTH) { t = K[KO_WHAT + r * 11 + (l - 1)]; v = s_a[l]; }
                if (l < SPONGE_WIDTH) x = gl_mul(t, v);
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) { const uint64_t y = shfl_up64(x, d); if (l >= d) x = gl_add_c(x, y); }
                uint64_t prev = shfl_up64(x, 1); if (l == 0) prev = 0;
                if (l < SPONGE_WIDTH) W(base + 5 + l, t, v, prev);
                if (l == 0) W(base + 17, 0, 0, 0);
                if (l == SPONGE_WIDTH - 1) s_b[0] = x;
                if (l > 0 && l < SPONGE_WIDTH) {
                    const uint64_t tv = K[KO_VS + r * 11 + (l - 1)];
                    W(base + 17 + l, tv, s0, v); s_b[l] = gl_muladd(tv, s0, v);
                }
            }
            wave_sync();
            if (l < SPONGE_WIDTH) s_a[l] = s_b[l];
            wave_sync();
            base += GLP_RECS_PARTIAL_ROUND;
        }
        round_ctr += N_PARTIAL_ROUNDS;
        for (int i = 0; i < HALF_N_FULL_ROUNDS; i++) full_round();
        for (int i = 0; i < SPONGE_WIDTH; i++) st[i] = s_a[i];
        wave_sync();
        const uint64_t nG = ncells[T_GLOP], nKA = ncells[T_KA_GLOP];
        const uint64_t full_cells = 12 * nKA + 48 * nG + 12 + 12 * (1 + 13 * nKA);
        const uint64_t part_cells = 12 * nKA + 12 + 121 * nKA + (uint64_t)N_PARTIAL_ROUNDS * (4 * nG + nKA + nKA + 11 * nKA + 12 + 11 * nKA);
        nrec += GLP_RECS; cell_off += 2 * HALF_N_FULL_ROUNDS * full_cells + part_cells;
    }
};
}  // namespace h2w
