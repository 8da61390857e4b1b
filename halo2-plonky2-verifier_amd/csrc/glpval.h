// glpval.h — the Goldilocks Poseidon permutation on VALUES, one whole permutation per thread (host + device; plain C++ as well:
// tests/cpp/glperm_values_check.cpp).
//
// plonky2's fast form, layer by layer as the gadget walks it (chips.h PoseidonPermutationChip, hash/poseidon/permutation.rs:43-284): every
// intermediate value is the canonical one the gadget's cells show, so the output equals the gadget's word for word.  It is what one lane of the
// replay interpreter runs for a fused stretch of its tape (replay.hip DOP_GLPERM): the lane keeps the 12 outputs, the permutation's records are
// written afterwards by a wavefront of their own from the listed input state (k_glp_emit_traced).
//
// Registers, not scratch: the state is only ever indexed by constants.  The loops over rows / elements that must not be unrolled (code size: an
// unrolled MDS layer is 156 multiply-adds) ROTATE the state instead of indexing it.
// K: anything callable as k(word) -> the u64 word of the Goldilocks block of h2w_poseidon_consts_t (on the device: a scalar load, the index is
// uniform over the wavefront).
#pragma once
#include <stddef.h>
#include "field.h"

#if defined(__HIPCC__)
#define GV_UNROLL _Pragma("unroll")
#define GV_LOOP _Pragma("unroll 1")
#else
#define GV_UNROLL
#define GV_LOOP
#endif

namespace h2w {

constexpr int GV_W = 12, GV_HALF_FULL = 4, GV_PARTIAL = 22;
constexpr int GV_ARC = 0, GV_CIRC = 360, GV_DIAG = 372, GV_FIRST = 384, GV_PRC = 396, GV_INIT = 418, GV_WHAT = 539, GV_VS = 781, GV_WORDS = 1023;
static_assert(offsetof(h2w_poseidon_consts_t, mds_circ) == 8 * GV_CIRC && offsetof(h2w_poseidon_consts_t, mds_diag) == 8 * GV_DIAG &&
              offsetof(h2w_poseidon_consts_t, fast_partial_first_round_constant) == 8 * GV_FIRST && offsetof(h2w_poseidon_consts_t, fast_partial_round_constants) == 8 * GV_PRC &&
              offsetof(h2w_poseidon_consts_t, fast_partial_round_initial_matrix) == 8 * GV_INIT && offsetof(h2w_poseidon_consts_t, fast_partial_round_w_hats) == 8 * GV_WHAT &&
              offsetof(h2w_poseidon_consts_t, fast_partial_round_vs) == 8 * GV_VS, "Goldilocks constant block layout");

HD uint64_t glv_sbox(uint64_t x) { const uint64_t x2 = gl_mul(x, x), x4 = gl_mul(x2, x2), x6 = gl_mul(x4, x2); return gl_mul(x6, x); }
HD void glv_rotate(uint64_t (&s)[GV_W], uint64_t in) {      // s[i] <- s[i + 1], s[11] <- in
    GV_UNROLL
    for (int i = 0; i + 1 < GV_W; i++) s[i] = s[i + 1];
    s[GV_W - 1] = in;
}

template <class K> HF void glp_permute_values(uint64_t (&s)[GV_W], K k) {
    int round_ctr = 0;
    GV_LOOP
    for (int fr = 0; fr < 2 * GV_HALF_FULL; fr++) {
        if (fr == GV_HALF_FULL) {
            // ---- partial rounds (:216-239)
            GV_LOOP
            for (int i = 0; i < GV_W; i++) glv_rotate(s, gl_add(s[0], k(GV_FIRST + i)));          // partial_first_constant_layer
            {   // mds_partial_layer_init: res[c] = sum_r init[r - 1][c - 1] st[r]
                uint64_t t[GV_W], res[GV_W];
                GV_UNROLL
                for (int c = 0; c < GV_W; c++) { t[c] = s[c]; res[c] = 0; }
                GV_LOOP
                for (int r = 1; r < GV_W; r++) {
                    glv_rotate(t, 0);      // t[0] = st[r]
                    GV_UNROLL
                    for (int c = 1; c < GV_W; c++) res[c] = gl_muladd(k(GV_INIT + (r - 1) * 11 + (c - 1)), t[0], res[c]);
                }
                GV_UNROLL
                for (int c = 1; c < GV_W; c++) s[c] = res[c];
            }
            const uint64_t m00 = k(GV_CIRC) + k(GV_DIAG);      // (as the gadget forms it: chips.h mds_partial_layer_fast)
            GV_LOOP
            for (int r = 0; r < GV_PARTIAL; r++) {
                const uint64_t s0 = gl_add(glv_sbox(s[0]), k(GV_PRC + r));
                uint64_t d = gl_mul(m00, s0);
                GV_UNROLL
                for (int i = 1; i < GV_W; i++) d = gl_muladd(k(GV_WHAT + r * 11 + (i - 1)), s[i], d);
                GV_UNROLL
                for (int i = 1; i < GV_W; i++) s[i] = gl_muladd(k(GV_VS + r * 11 + (i - 1)), s0, s[i]);
                s[0] = d;
            }
            round_ctr += GV_PARTIAL;
        }
        // ---- one full round (:241-254): constant_layer, sbox_layer, mds_layer
        GV_LOOP
        for (int i = 0; i < GV_W; i++) glv_rotate(s, glv_sbox(gl_add(s[0], k(GV_ARC + GV_W * round_ctr + i))));
        uint64_t res[GV_W];
        GV_UNROLL
        for (int c = 0; c < GV_W; c++) res[c] = 0;
        GV_LOOP
        for (int r = 0; r < GV_W; r++) {      // row r: sum_i circ[i] v[(i + r) % 12] + diag[r] v[r]; s is rotated by r here
            uint64_t acc = 0;
            GV_UNROLL
            for (int i = 0; i < GV_W; i++) acc = gl_muladd(k(GV_CIRC + i), s[i], acc);
            acc = gl_muladd(k(GV_DIAG + r), s[0], acc);
            glv_rotate(res, acc);
            glv_rotate(s, s[0]);
        }
        GV_UNROLL
        for (int c = 0; c < GV_W; c++) s[c] = res[c];
        round_ctr++;
    }
}

}      // namespace h2w
#undef GV_UNROLL
#undef GV_LOOP
