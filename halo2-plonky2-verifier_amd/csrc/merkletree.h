// merkletree.h — what the public Merkle builder (merkletree.hip, include/h2w.h 2e) is made of that is plain arithmetic, host + device; plain C++ as
// well: tests/cpp/merkletree_check.cpp holds the sponge to the oracle's orc_nv_hash_or_noop on the host.
//   the layout of a tree's hash store (levels from the leaves upward, the cap last) and of an opening row (chiphash.h operand_layout of MERKLE_VERIFY)
//   hash_or_noop over a leaf of RUN-TIME length read from memory: proverhash.h hash_no_pad<MAXN> is a compile-time-bounded register array - right for
//   the prover's 16 / 32 words, no form for a leaf of up to H2W_CHIPBATCH_MAX_N_IN.  The same permutations and the same absorb rule, block by block.
#pragma once
#include "proverhash.h"

namespace h2w {

constexpr uint32_t MERKLE_MAX_DEPTH = 24, MERKLE_MAX_CAP = 6;

// word offset of level l (0: the leaf digests) in a tree's hash store, and the store's size: level l has 2^(depth - l) hashes of four words
HD uint64_t mt_level_off(uint32_t depth, uint32_t l) { return 4ull * ((2ull << depth) - (2ull << (depth - l))); }
HD uint64_t mt_tree_words(uint32_t depth, uint32_t cap_height) { return 4ull * ((2ull << depth) - (1ull << cap_height)); }
// words of an opening row: leaf[n_in], leaf_index, cap[2^cap_height][4], siblings[depth - cap_height][4]
HD uint32_t mt_row_words(uint32_t n_in, uint32_t depth, uint32_t cap_height) { return n_in + 1 + 4 * ((1u << cap_height) + depth - cap_height); }

// hash_or_noop (hash/poseidon/hash.rs:63-120, hash/poseidon_bn254/hash.rs:67-120) of n words at `in`
HDN inline H4 hash_or_noop_words(const ProverConsts *K, int mode, const uint64_t *in, uint32_t n) {
    if (n <= (mode == 0 ? 4u : 3u)) {
        H4 h;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) h.w[i] = i < n ? g_load_u64(in + i) : 0;
        return h;
    }
    if (mode == 0) {      // overwrite-mode sponge at rate 8: a short last block leaves the other rate words as they are
        uint64_t st[12];
#pragma unroll
        for (int i = 0; i < 12; i++) st[i] = 0;
        const bool small = gl_mds_is_small(&K->k);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
        for (uint32_t off = 0; off < n; off += SPONGE_RATE) {
#pragma unroll
            for (uint32_t i = 0; i < SPONGE_RATE; i++) if (off + i < n) st[i] = g_load_u64(in + off + i);
            if (small) gl_permute_t<true>(&K->k, st); else gl_permute_t<false>(&K->k, st);
        }
        return h4_of_state(st);
    }
    fr_t st[4];      // nine words a permutation: three Fr of three words each into state elements 1 .. 3, a short last Fr zero-padded
#pragma unroll
    for (int i = 0; i < 4; i++) st[i] = fr_zero();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (uint32_t off = 0; off < n; off += 9) {
#pragma unroll
        for (uint32_t j = 0; j < 3; j++) {
            const uint32_t o = off + 3 * j;
            if (o < n) {
                fr_t v = fr_zero();
#pragma unroll
                for (uint32_t l = 0; l < 3; l++) if (o + l < n) v.l[l] = g_load_u64(in + o + l);
                st[j + 1] = to_mont(K, v);
            }
        }
        bn_permute_m(K, st);
    }
    return h4_of_mont(K, st[0]);
}

}  // namespace h2w
