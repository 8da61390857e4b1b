// proverhash.h — the prover's value hashers (prover.hip), host + device; plain C++ as well: tests/cpp/proverhash_check.cpp holds them to the
// oracle's orc_nv_gl_permute / orc_nv_bn_permute / orc_nv_hash_or_noop on the host.
//
// The two permutations on values, one whole permutation per thread, and the three hash functions of a Merkle oracle over them (a hash is four
// words, H4, in both modes).  They are NOT the replay's glpval.h / bnpval.h: those rotate the state to save code size, these are unrolled and
// use the small-MDS form - different schedules of the same exact arithmetic, each the faster one where it runs.
// ProverConsts is what a prover handle keeps on the host and on the device: the caller's tables and the PoseidonBN254 ones in Montgomery form.
#pragma once
#include "chips.h"

namespace h2w {

struct BnMont { fr_t c[88], s[392], m[4][4], p[4][4]; };                 // PoseidonBN254 tables in Montgomery form (x * 2^261)
struct ProverConsts { h2w_poseidon_consts_t k; BnMont bn; fr_t r2; uint64_t ninv; };
struct H4 { uint64_t w[4]; };

inline void prover_consts_init(ProverConsts &K, const h2w_poseidon_consts_t &consts) {
    const FrParams P = fr_params_init();
    K.k = consts; K.r2 = P.r2; K.ninv = P.ninv;
    for (int i = 0; i < 88; i++) K.bn.c[i] = fr_mont_mul(consts.bn_c[i], P.r2, P.ninv);
    for (int i = 0; i < 392; i++) K.bn.s[i] = fr_mont_mul(consts.bn_s[i], P.r2, P.ninv);
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) { K.bn.m[i][j] = fr_mont_mul(consts.bn_m[i][j], P.r2, P.ninv); K.bn.p[i][j] = fr_mont_mul(consts.bn_p[i][j], P.r2, P.ninv); }
}

// ---------------------------------------------------------------- Goldilocks Poseidon, plonky2 "fast" layout (hash/poseidon/permutation.rs:43-314)
// dot products of full-width words: 128-bit accumulator + overflow count, reduced once (2^128 = -2^32 mod p)
struct GlAcc { u128 lo; uint32_t carries; };
HD void glacc_mul(GlAcc &a, uint64_t x, uint64_t y) { const u128 pr = (u128)x * y; a.lo += pr; a.carries += a.lo < pr; }
HD uint64_t glacc_reduce(const GlAcc &a) { return gl_sub(gl_reduce128(a.lo), (uint64_t)a.carries << 32); }
// SMALL_MDS: every MDS_MATRIX_CIRC / _DIAG entry is below 2^28 (plonky2's are <= 41): a row is then two 64-bit accumulations over the
// 32-bit halves of the state (13 terms < 2^32 * 2^28 each) and ONE reduction, instead of 13 reduced 64x64 products - the full
// rounds' MDS layers are two thirds of a permutation's instructions otherwise.  Same values either way (exact arithmetic).
template <bool SMALL_MDS> HDN inline void gl_permute_t(const h2w_poseidon_consts_t *k, uint64_t *st) {
    int rc = 0;
    for (int half = 0; half < 2; half++) {
        if (half == 1) {
#pragma unroll
            for (int i = 0; i < 12; i++) st[i] = gl_add(st[i], k->fast_partial_first_round_constant[i]);
            uint64_t res[12];
            res[0] = st[0];
#pragma unroll
            for (int c = 1; c < 12; c++) {
                GlAcc a; a.lo = 0; a.carries = 0;
#pragma unroll
                for (int r = 1; r < 12; r++) glacc_mul(a, k->fast_partial_round_initial_matrix[r - 1][c - 1], st[r]);
                res[c] = glacc_reduce(a);
            }
#pragma unroll
            for (int c = 0; c < 12; c++) st[c] = res[c];
            const uint64_t m00 = gl_add(k->mds_circ[0], k->mds_diag[0]);
#pragma unroll 1
            for (int r = 0; r < N_PARTIAL_ROUNDS; r++) {
                uint64_t x = st[0], x2 = gl_mul(x, x), x4 = gl_mul(x2, x2), x6 = gl_mul(x4, x2);
                const uint64_t s0 = gl_add(gl_mul(x6, x), k->fast_partial_round_constants[r]);
                GlAcc a; a.lo = (u128)m00 * s0; a.carries = 0;
#pragma unroll
                for (int i = 1; i < 12; i++) glacc_mul(a, k->fast_partial_round_w_hats[r][i - 1], st[i]);
#pragma unroll
                for (int i = 1; i < 12; i++) st[i] = gl_muladd(k->fast_partial_round_vs[r][i - 1], s0, st[i]);
                st[0] = glacc_reduce(a);
            }
            rc += N_PARTIAL_ROUNDS;
        }
#pragma unroll 1
        for (int f = 0; f < HALF_N_FULL_ROUNDS; f++) {
#pragma unroll
            for (int i = 0; i < 12; i++) {
                uint64_t x = gl_add(st[i], k->all_round_constants[i + 12 * rc]);
                uint64_t x2 = gl_mul(x, x), x4 = gl_mul(x2, x2), x6 = gl_mul(x4, x2); st[i] = gl_mul(x6, x);
            }
            uint64_t res[12];
            if (SMALL_MDS) {
                uint32_t lo32[12], hi32[12];
#pragma unroll
                for (int i = 0; i < 12; i++) { lo32[i] = (uint32_t)st[i]; hi32[i] = (uint32_t)(st[i] >> 32); }
#pragma unroll
                for (int r = 0; r < 12; r++) {
                    const uint32_t dg = (uint32_t)k->mds_diag[r];
                    uint64_t lo = (uint64_t)lo32[r] * dg, hi = (uint64_t)hi32[r] * dg;
#pragma unroll
                    for (int i = 0; i < 12; i++) { const uint32_t c = (uint32_t)k->mds_circ[i]; lo += (uint64_t)lo32[(i + r) % 12] * c; hi += (uint64_t)hi32[(i + r) % 12] * c; }
                    res[r] = gl_reduce128((u128)lo + ((u128)hi << 32));
                }
            } else {
#pragma unroll
                for (int r = 0; r < 12; r++) {
                    uint64_t acc = 0;
#pragma unroll
                    for (int i = 0; i < 12; i++) acc = gl_muladd(k->mds_circ[i], st[(i + r) % 12], acc);
                    res[r] = gl_muladd(k->mds_diag[r], st[r], acc);
                }
            }
#pragma unroll
            for (int r = 0; r < 12; r++) st[r] = res[r];
            rc++;
        }
    }
}

HDN inline bool gl_mds_is_small(const h2w_poseidon_consts_t *k) {
    bool small = true;
    for (int i = 0; i < 12; i++) small = small && k->mds_circ[i] < (1ull << 28) && k->mds_diag[i] < (1ull << 28);
    return small;
}
HDN inline void gl_permute(const h2w_poseidon_consts_t *k, uint64_t *st) { if (gl_mds_is_small(k)) gl_permute_t<true>(k, st); else gl_permute_t<false>(k, st); }

// ---------------------------------------------------------------- PoseidonBN254 (hash/poseidon_bn254/permutation.rs:48-203), Montgomery-form state
HOL inline fr_t mmul(fr_t a, fr_t b, uint64_t ninv) { return fr_mont_mul(a, b, ninv); }
HDN inline fr_t bn_pow5(fr_t x, uint64_t ni) { fr_t x2 = mmul(x, x, ni), x4 = mmul(x2, x2, ni); return mmul(x4, x, ni); }
HDN inline void bn_mix(fr_t *st, const fr_t m[4][4], uint64_t ni) {
    fr_t ns[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        ns[i] = mmul(m[0][i], st[0], ni);
#pragma unroll
        for (int j = 1; j < 4; j++) ns[i] = fr_add(ns[i], mmul(m[j][i], st[j], ni));
    }
#pragma unroll
    for (int i = 0; i < 4; i++) st[i] = ns[i];
}
HDN inline void bn_permute_m(const ProverConsts *K, fr_t *st) {
    const uint64_t ni = K->ninv; const BnMont &B = K->bn;
#pragma unroll
    for (int j = 0; j < 4; j++) st[j] = fr_add(st[j], B.c[j]);
    for (int half = 0; half < 2; half++) {
        if (half == 1) {
#pragma unroll 1
            for (int r = 0; r < BN_PARTIAL_ROUNDS; r++) {
                st[0] = fr_add(bn_pow5(st[0], ni), B.c[bn_c_partial(r)]);
                fr_t ns0 = mmul(B.s[bn_s_row(r)], st[0], ni);
#pragma unroll
                for (int j = 1; j < 4; j++) ns0 = fr_add(ns0, mmul(B.s[bn_s_row(r) + j], st[j], ni));
#pragma unroll
                for (int kk = 1; kk < 4; kk++) st[kk] = fr_add(st[kk], mmul(B.s[bn_s_row(r) + BN_WIDTH + kk - 1], st[0], ni));
                st[0] = ns0;
            }
        }
#pragma unroll 1
        for (int i = 0; i < BN_FULL_ROUNDS / 2 - 1; i++) {
            const int it = bn_c_full(half, i);
#pragma unroll
            for (int j = 0; j < 4; j++) st[j] = fr_add(bn_pow5(st[j], ni), B.c[it + j]);
            bn_mix(st, B.m, ni);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) st[j] = bn_pow5(st[j], ni);
        if (half == 0) {
#pragma unroll
            for (int j = 0; j < 4; j++) st[j] = fr_add(st[j], B.c[(BN_FULL_ROUNDS / 2) * BN_WIDTH + j]);
            bn_mix(st, B.p, ni);
        } else bn_mix(st, B.m, ni);
    }
}
HDN inline fr_t to_mont(const ProverConsts *K, fr_t x) { return mmul(x, K->r2, K->ninv); }
HDN inline fr_t from_mont(const ProverConsts *K, fr_t x) { return mmul(x, fr_from_u64(1), K->ninv); }

// ---------------------------------------------------------------- hashers (hash/poseidon/hash.rs:63-215, hash/poseidon_bn254/hash.rs:67-210): a hash is 4 words
HD H4 h4_of_state(const uint64_t *st) {                          // the first four words of a Goldilocks sponge state
    H4 h;
#pragma unroll
    for (int i = 0; i < 4; i++) h.w[i] = st[i];
    return h;
}
HD H4 h4_of_mont(const ProverConsts *K, const fr_t &x) { return h4_of_state(from_mont(K, x).l); }      // the canonical limbs of a Montgomery-form element
template <int MAXN> HDN inline H4 hash_no_pad(const ProverConsts *K, int mode, const uint64_t (&in)[MAXN], int n) {
    if (mode == 0) {
        uint64_t st[12];
#pragma unroll
        for (int i = 0; i < 12; i++) st[i] = 0;
#pragma unroll
        for (int off = 0; off < MAXN; off += SPONGE_RATE) {
            if (off < n) {
#pragma unroll
                for (int i = 0; i < SPONGE_RATE; i++) if (off + i < MAXN && off + i < n) st[i] = in[off + i];
                gl_permute(&K->k, st);
            }
        }
        return h4_of_state(st);
    }
    fr_t st[4];
#pragma unroll
    for (int i = 0; i < 4; i++) st[i] = fr_zero();
#pragma unroll
    for (int off = 0; off < MAXN; off += 9) {
        if (off < n) {
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const int o = off + 3 * j;
                if (o < MAXN && o < n) {
                    fr_t v = fr_zero();
#pragma unroll
                    for (int l = 0; l < 3; l++) if (o + l < MAXN && o + l < n) v.l[l] = in[o + l];
                    st[j + 1] = to_mont(K, v);
                }
            }
            bn_permute_m(K, st);
        }
    }
    return h4_of_mont(K, st[0]);
}
template <int MAXN> HDN inline H4 hash_or_noop(const ProverConsts *K, int mode, const uint64_t (&in)[MAXN], int n) {
    if (n > (mode == 0 ? 4 : 3)) return hash_no_pad<MAXN>(K, mode, in, n);
    H4 h;
#pragma unroll
    for (int i = 0; i < 4; i++) h.w[i] = (i < MAXN && i < n) ? in[i < MAXN ? i : 0] : 0;
    return h;
}
HDN inline H4 two_to_one(const ProverConsts *K, int mode, const H4 &l, const H4 &r) {
    if (mode == 0) {
        uint64_t st[12];
#pragma unroll
        for (int i = 0; i < 4; i++) { st[i] = l.w[i]; st[4 + i] = r.w[i]; st[8 + i] = 0; }
        gl_permute(&K->k, st);
        return h4_of_state(st);
    }
    fr_t st[4], a, b;
#pragma unroll
    for (int i = 0; i < 4; i++) { a.l[i] = l.w[i]; b.l[i] = r.w[i]; }
    st[0] = fr_zero(); st[1] = fr_zero(); st[2] = to_mont(K, a); st[3] = to_mont(K, b);
    bn_permute_m(K, st);
    return h4_of_mont(K, st[0]);
}

}  // namespace h2w
