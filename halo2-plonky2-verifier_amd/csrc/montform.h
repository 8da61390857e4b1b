// montform.h — canonical cell -> Montgomery form of BN254 Fr (halo2curves bn256::Fr in memory: v * 2^256 mod r), by the WIDTH of v.
//
// The expansion kernel's cells are bit-fields of values below 2^128 (expand.hip); a full 254 x 254-bit Montgomery product per cell is
// what a second pass pays (advicetools.hip k_to_montgomery), not what they need.  Route for a value of N 32-bit words w_0 .. w_{N-1}:
//     S = sum_i w_i * C_i,   C_i = 2^(256 + 32 i) mod r            N rows of eight 32 x 32-bit multiply-adds; S <= (2^32 - 1) sum_i C_i, nine words: up to
//                                                                  N = 4 because S < 4 2^32 r < 2^288, for N = 8 because C_0 + .. + C_7 < 2^256 for this r
//                                                                  (montform_init checks it; montform_check.cpp runs the all-ones input)
//     q = floor(floor(S / 2^224) * mu / 2^93),   mu = floor(2^317 / r)    S / r - 1 < q' <= S / r for the real quotient q':
//                                                                  (S mod 2^224) / r < 2^-29 and floor(S / 2^224) (2^224 / r - mu / 2^93) < 2^-29
//     T = (S - q r) mod 2^256 in [0, 2 r),  one conditional subtraction of r.
// N = 2 (a Goldilocks word): 16 + 4 + 15 products.  N = 3 (below 2^96: x + 2^RB - p and its kin): 24 + 4 + 15.  N = 4 (below 2^128): 32 + 4 + 15.
// N = 8: any canonical value (the literal cells of the generic expansion kernel), 64 + 4 + 15 - the price of a full product.
// The number of rows may be a run-time value (mf_convert_upto): the expansion kernel's flush is unrolled, so it folds to the class of the step's cells.
// Every constant is derived from r on the host (montform_init); nothing is typed in.  Host + device: tests/cpp/montform_check.cpp runs the same
// source against unsigned __int128 / wide integers.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include "field.h"

namespace h2w {

struct MontForm {
    uint32_t c[8][8];      // c[i] = 2^(256 + 32 i) mod r, little-endian 32-bit words
    uint32_t mu[2];        // floor(2^317 / r) < 2^64
    uint32_t neg_rb[8];    // the Montgomery form of -2^rb mod r (the one full-width constant of check_less_than's cells)
};

HD uint32_t mf_r(int j) { const uint64_t l = fr_mod_limb(j >> 1); return (j & 1) ? (uint32_t)(l >> 32) : (uint32_t)l; }

HD uint64_t mf_mulhi64(uint64_t a, uint64_t b) {
    const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

// o[0..8) = (value of the first n of the N words w) * 2^256 mod r, n <= N; the value may be anything below 2^(32 n) (n = 8: below 2^256)
template <int N> HD void mf_convert_upto(const uint32_t *w, int n, const MontForm &K, uint32_t *o) {
    static_assert(N >= 1 && N <= 8, "one to eight 32-bit words");
    uint32_t s[9];
#pragma unroll
    for (int j = 0; j < 9; j++) s[j] = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        if (i >= n) break;
        uint64_t cy = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) { const uint64_t t = (uint64_t)w[i] * K.c[i][j] + s[j] + cy; s[j] = (uint32_t)t; cy = t >> 32; }
        s[8] += (uint32_t)cy;
    }
    const uint64_t q = mf_mulhi64(((uint64_t)s[8] << 32) | s[7], ((uint64_t)K.mu[1] << 32) | K.mu[0]) >> 29;      // < 2^35
    const uint32_t q0 = (uint32_t)q, q1 = (uint32_t)(q >> 32);
    uint32_t p[8];
    {
        uint64_t cy = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) { const uint64_t t = (uint64_t)q0 * mf_r(j) + cy; p[j] = (uint32_t)t; cy = t >> 32; }
    }
    if (N > 1) {      // (one word: S < 2^32 r, the quotient has one word)
        uint64_t cy = 0;
#pragma unroll
        for (int j = 0; j < 7; j++) { const uint64_t t = (uint64_t)q1 * mf_r(j) + p[j + 1] + cy; p[j + 1] = (uint32_t)t; cy = t >> 32; }
    }
    uint32_t t[8], u[8]; uint64_t bw = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) { const uint64_t d = (uint64_t)s[j] - p[j] - bw; t[j] = (uint32_t)d; bw = (d >> 32) & 1; }
    bw = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) { const uint64_t d = (uint64_t)t[j] - mf_r(j) - bw; u[j] = (uint32_t)d; bw = (d >> 32) & 1; }
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = bw ? t[j] : u[j];
}
template <int N> HD void mf_convert(const uint32_t *w, const MontForm &K, uint32_t *o) { mf_convert_upto<N>(w, N, K, o); }

// the routes by class, on 64-bit limbs
HD fr_t mf_pack(const uint32_t *o) { fr_t z; for (int j = 0; j < 4; j++) z.l[j] = ((uint64_t)o[2 * j + 1] << 32) | o[2 * j]; return z; }
HD fr_t mont_from_u64(uint64_t x, const MontForm &K) { const uint32_t w[2] = {(uint32_t)x, (uint32_t)(x >> 32)}; uint32_t o[8]; mf_convert<2>(w, K, o); return mf_pack(o); }
HD fr_t mont_from_u96(uint64_t lo, uint32_t hi, const MontForm &K) { const uint32_t w[3] = {(uint32_t)lo, (uint32_t)(lo >> 32), hi}; uint32_t o[8]; mf_convert<3>(w, K, o); return mf_pack(o); }
HD fr_t mont_from_u128(uint64_t lo, uint64_t hi, const MontForm &K) {
    const uint32_t w[4] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)}; uint32_t o[8]; mf_convert<4>(w, K, o); return mf_pack(o);
}
HD fr_t mont_from_fr(const fr_t &v, const MontForm &K) {
    uint32_t w[8], o[8];
    for (int j = 0; j < 4; j++) { w[2 * j] = (uint32_t)v.l[j]; w[2 * j + 1] = (uint32_t)(v.l[j] >> 32); }
    mf_convert<8>(w, K, o); return mf_pack(o);
}
// a canonical cell of unknown class: the route its width allows
HD fr_t mont_from_cell(const fr_t &v, const MontForm &K) {
    if ((v.l[2] | v.l[3]) != 0) return mont_from_fr(v, K);
    if (v.l[1] != 0) return mont_from_u128(v.l[0], v.l[1], K);
    return mont_from_u64(v.l[0], K);
}

// ---- host: the constants, from r
inline void mf_host_double(uint32_t *x) {      // x = 2 x mod r, x < r
    uint32_t cy = 0;
    for (int j = 0; j < 8; j++) { const uint32_t n = (x[j] << 1) | cy; cy = x[j] >> 31; x[j] = n; }
    uint32_t u[8]; uint64_t bw = 0;
    for (int j = 0; j < 8; j++) { const uint64_t d = (uint64_t)x[j] - mf_r(j) - bw; u[j] = (uint32_t)d; bw = (d >> 32) & 1; }
    if (!bw) for (int j = 0; j < 8; j++) x[j] = u[j];      // (2 x < 2^255: no carry out of the eight words)
}
inline void mf_host_pow2(int e, uint32_t *x) { for (int j = 0; j < 8; j++) x[j] = j == 0 ? 1u : 0u; for (int i = 0; i < e; i++) mf_host_double(x); }
inline void montform_init(MontForm &K, int rb) {
    for (int i = 0; i < 8; i++) mf_host_pow2(256 + 32 * i, K.c[i]);
    // mu = floor(2^317 / r): restoring division, one bit of the dividend at a time (the remainder stays below r < 2^254)
    uint32_t rem[8] = {0, 0, 0, 0, 0, 0, 0, 0}; uint64_t q = 0;
    for (int bit = 317; bit >= 0; bit--) {
        uint32_t cy = bit == 317 ? 1u : 0u;
        for (int j = 0; j < 8; j++) { const uint32_t n = (rem[j] << 1) | cy; cy = rem[j] >> 31; rem[j] = n; }
        uint32_t u[8]; uint64_t bw = 0;
        for (int j = 0; j < 8; j++) { const uint64_t d = (uint64_t)rem[j] - mf_r(j) - bw; u[j] = (uint32_t)d; bw = (d >> 32) & 1; }
        q <<= 1;
        if (!bw) { q |= 1; for (int j = 0; j < 8; j++) rem[j] = u[j]; }
    }
    K.mu[0] = (uint32_t)q; K.mu[1] = (uint32_t)(q >> 32);
    { uint32_t sum[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};      // the nine-word accumulator holds the eight-word route: sum C_i < 2^256
      for (int i = 0; i < 8; i++) { uint64_t cy = 0; for (int j = 0; j < 8; j++) { const uint64_t t = (uint64_t)sum[j] + K.c[i][j] + cy; sum[j] = (uint32_t)t; cy = t >> 32; } sum[8] += (uint32_t)cy; }
      if (sum[8]) abort(); }
    // -2^rb * 2^256 = r - 2^(256 + rb) mod r
    uint32_t x[8]; mf_host_pow2(256 + rb, x); uint64_t bw = 0;
    for (int j = 0; j < 8; j++) { const uint64_t d = (uint64_t)mf_r(j) - x[j] - bw; K.neg_rb[j] = (uint32_t)d; bw = (d >> 32) & 1; }
}
// 2^(256 + 261) mod r: the device product divides by 2^261, so a product with this constant is the Montgomery form with R = 2^256 (the full-product
// passes: batch.hip k_direct_to_montgomery, advicetools.hip k_to_montgomery)
inline const fr_t &mont_k() { static const fr_t K = [] { fr_t x = fr_from_u64(1); for (int i = 0; i < 256 + FR_MONT_BITS; i++) x = fr_add(x, x); return x; }(); return K; }

}  // namespace h2w
