// Host check of csrc/merkletree.h: the leaf hasher of the public Merkle builder (what a lane of merkletree.hip's k_mt_leaves runs) - hash_or_noop over
// a leaf of RUN-TIME length read from memory -, compiled as plain C++, against the oracle's orc_nv_hash_or_noop; and the layout functions against
// the formulas of include/h2w.h 2e.
// The driver (tests/test_merkle_tree_host.py) writes the cases: groups of [u64 n][h2w_poseidon_consts_t][n cases], a case being
//   mode n in[n] want[4]
// The leaf sits in a buffer of exactly n words with guard words behind it, so a read past the leaf shows (and a sanitizer build of this program
// alone sees it).  The constants of a group go through prover_consts_init, as a handle's do.  The counts printed at the end are asserted by the driver.
// g++ -O2 -std=c++17 -I halo2-plonky2-verifier_amd/csrc -I include tests/cpp/merkletree_check.cpp && ./a.out cases.bin
#include <cstdio>
#include <cstring>
#include <vector>
#include "merkletree.h"
using namespace h2w;

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: merkletree_check cases.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    int bad = 0, groups = 0; uint64_t n_cases, noop = 0, hashed = 0, longest = 0;
    // the layout: level offsets add up to the store, the cap is its last level, a row is leaf + index + cap + siblings
    for (uint32_t depth = 1; depth <= MERKLE_MAX_DEPTH; depth++) for (uint32_t cap = 0; cap <= depth && cap <= MERKLE_MAX_CAP; cap++) {
        uint64_t at = 0;
        for (uint32_t l = 0; l <= depth - cap; l++) { if (mt_level_off(depth, l) != at) bad++; at += 4ull << (depth - l); }
        if (at != mt_tree_words(depth, cap) || mt_row_words(7, depth, cap) != 7 + 1 + 4 * ((1u << cap) + depth - cap)) bad++;
    }
    if (bad) printf("layout: %d mismatches\n", bad);
    while (fread(&n_cases, 8, 1, f) == 1) {
        static h2w_poseidon_consts_t k; static ProverConsts K;
        if (fread(&k, sizeof k, 1, f) != 1) { printf("truncated constants\n"); return 2; }
        prover_consts_init(K, k);
        for (uint64_t c = 0; c < n_cases; c++) {
            uint64_t hdr[2], want[4];
            if (fread(hdr, 8, 2, f) != 2 || hdr[0] > 1 || hdr[1] < 1 || hdr[1] > H2W_CHIPBATCH_MAX_N_IN) { printf("bad case\n"); return 2; }
            const uint32_t n = (uint32_t)hdr[1];
            std::vector<uint64_t> leaf(n);      // (exactly n words: the hasher reads nothing behind them)
            if (fread(leaf.data(), 8, n, f) != n || fread(want, 8, 4, f) != 4) { printf("truncated case\n"); return 2; }
            const H4 h = hash_or_noop_words(&K, (int)hdr[0], leaf.data(), n);
            for (int i = 0; i < 4; i++) if (h.w[i] != want[i]) {
                if (bad < 8) printf("group %d case %llu mode %d n %u word %d: %016llx, want %016llx\n", groups, (unsigned long long)c, (int)hdr[0], n, i, (unsigned long long)h.w[i], (unsigned long long)want[i]);
                bad++;
            }
            (n <= (hdr[0] == 0 ? 4u : 3u) ? noop : hashed)++;
            if (n > longest) longest = n;
        }
        groups++;
    }
    fclose(f);
    printf("groups: %d noop: %llu hashed: %llu longest: %llu\n", groups, (unsigned long long)noop, (unsigned long long)hashed, (unsigned long long)longest);
    printf(bad || noop + hashed == 0 ? "FAILED\n" : "OK\n");
    return bad != 0 || noop + hashed == 0;
}
