// bnpval.h — the PoseidonBN254 permutation on VALUES, one whole permutation per thread (host + device; plain C++ as well:
// tests/cpp/bnperm_values_check.cpp).
//
// What chips.h PoseidonBN254PermutationChip::permute computes (hash/poseidon_bn254/permutation.rs:48-203: ark, full rounds, the sparse partial
// rounds, full rounds), without its cells: the state stays times R (Montgomery form, R = 2^261), every product is ONE fr_mont_mul against a
// table entry that is times R as well (bntab.h bn_table_build: the second half of the table), x^5 is three products, and the four outputs go
// back to canonical form at the end - they equal the gadget's word for word.  It is what one lane of the replay interpreter runs for a fused
// stretch of its tape (replay.hip DOP_BNPERM): the lane keeps the four outputs, the permutation's 4,032 cells are written afterwards by a quad
// of their own from the listed input state (k_bn_emit_traced).
//
// Registers, not scratch: the state is only ever indexed by constants; the loops that must not be unrolled (code size: a product is ~340
// instructions) ROTATE the state instead of indexing it.
// K: anything callable as k(entry) -> the times-R table entry BK_C / BK_S / BK_M / BK_P + i as an fr_t (on the device: scalar loads, the index
// is uniform over the wavefront).  An input at or above r (a proof word h2w_plan_status flags with 4) is taken as it is: the result is then
// some value below r, as the cells of such a proof are "unreduced" (include/h2w.h).
#pragma once
#include "bntab.h"

#if defined(__HIPCC__)
#define BV_UNROLL _Pragma("unroll")
#define BV_LOOP _Pragma("unroll 1")
#else
#define BV_UNROLL
#define BV_LOOP
#endif

namespace h2w {

HD void bnv_rotate(fr_t (&s)[BN_WIDTH], const fr_t &in) {      // s[i] <- s[i + 1], s[3] <- in
    BV_UNROLL
    for (int i = 0; i + 1 < BN_WIDTH; i++) s[i] = s[i + 1];
    s[BN_WIDTH - 1] = in;
}
HD fr_t bnv_exp5(const fr_t &x, uint64_t ninv) { const fr_t x2 = fr_mont_mul(x, x, ninv), x4 = fr_mont_mul(x2, x2, ninv); return fr_mont_mul(x4, x, ninv); }

template <class K> HF void bn_permute_values(fr_t (&s)[BN_WIDTH], const FrParams &P, K k) {
    const uint64_t ninv = P.ninv;
    BV_LOOP
    for (int i = 0; i < BN_WIDTH; i++) bnv_rotate(s, fr_add(fr_mont_mul(s[0], P.r2, ninv), k(BK_C + i)));      // times R, and ark(0)
    BV_LOOP
    for (int half = 0; half < 2; half++) {
        if (half == 1) {
            // ---- the partial rounds (:83-110): x^5 and the round constant on s0, the sparse row into s0, the sparse column into s1..s3
            BV_LOOP
            for (int r = 0; r < BN_PARTIAL_ROUNDS; r++) {
                const int ix = BK_S + bn_s_row(r);
                const fr_t s0 = fr_add(bnv_exp5(s[0], ninv), k(BK_C + bn_c_partial(r)));
                fr_t row = fr_mont_mul(k(ix), s0, ninv);
                row = fr_add(fr_mont_mul(k(ix + 1), s[1], ninv), row);
                row = fr_add(fr_mont_mul(k(ix + 2), s[2], ninv), row);
                row = fr_add(fr_mont_mul(k(ix + 3), s[3], ninv), row);
                s[1] = fr_add(fr_mont_mul(k(ix + BN_WIDTH), s0, ninv), s[1]);
                s[2] = fr_add(fr_mont_mul(k(ix + BN_WIDTH + 1), s0, ninv), s[2]);
                s[3] = fr_add(fr_mont_mul(k(ix + BN_WIDTH + 2), s0, ninv), s[3]);
                s[0] = row;
            }
        }
        // ---- four full rounds (:112-160): x^5, the round constants (not behind the last round of all), the matrix (P behind the first four, else M)
        BV_LOOP
        for (int r = 0; r < BN_FULL_ROUNDS / 2; r++) {
            const bool last = r == BN_FULL_ROUNDS / 2 - 1;
            const bool ark = !(half == 1 && last);
            const int it = BK_C + bn_c_full(half, r);
            BV_LOOP
            for (int i = 0; i < BN_WIDTH; i++) {
                fr_t x = bnv_exp5(s[0], ninv);
                if (ark) x = fr_add(x, k(it + i));
                bnv_rotate(s, x);
            }
            const int mb = half == 0 && last ? BK_P : BK_M;
            fr_t acc[BN_WIDTH];
            BV_UNROLL
            for (int i = 0; i < BN_WIDTH; i++) acc[i] = fr_zero();
            BV_LOOP
            for (int j = 0; j < BN_WIDTH; j++) {      // s is rotated by j here: s[0] is element j
                BV_UNROLL
                for (int i = 0; i < BN_WIDTH; i++) acc[i] = fr_add(fr_mont_mul(s[0], k(mb + 4 * j + i), ninv), acc[i]);
                bnv_rotate(s, s[0]);
            }
            BV_UNROLL
            for (int i = 0; i < BN_WIDTH; i++) s[i] = acc[i];
        }
    }
    BV_LOOP
    for (int i = 0; i < BN_WIDTH; i++) bnv_rotate(s, fr_mont_mul(s[0], fr_from_u64(1), ninv));      // back to canonical
}

}      // namespace h2w
#undef BV_UNROLL
#undef BV_LOOP
