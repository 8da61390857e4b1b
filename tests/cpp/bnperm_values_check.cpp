// Host check of csrc/bnpval.h: the per-thread PoseidonBN254 value permutation (what a lane of the replay interpreter runs for a fused stretch,
// csrc/replay.hip DOP_BNPERM), compiled as plain C++, against known answers.
// The driver (tests/test_bnperm_values.py) writes the cases: groups of [u64 n][h2w_poseidon_consts_t][n x {in[4], want[4]}] (32-byte little-endian
// field elements) - the published circomlib vector on the published tables, the oracle's gadget on random and edge states.  The table the
// permutation reads is built from the constants as a plan builds it (bntab.h bn_table_build: the times-R half).
// g++ -O2 -std=c++17 -I halo2-plonky2-verifier_amd/csrc -I include tests/cpp/bnperm_values_check.cpp && ./a.out cases.bin
#include <cstdio>
#include <cstring>
#include <vector>
#include "bnpval.h"
using namespace h2w;

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: bnperm_values_check cases.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    const FrParams P = fr_params_init();
    int bad = 0, groups = 0; uint64_t total = 0, n;
    std::vector<fr_t> tab(BK_ALL);
    while (fread(&n, 8, 1, f) == 1) {
        static h2w_poseidon_consts_t k;
        if (fread(&k, sizeof k, 1, f) != 1) { printf("truncated constants\n"); return 2; }
        bn_table_build(k, P, tab.data());
        const fr_t *kr = tab.data() + BK_T;
        for (uint64_t c = 0; c < n; c++) {
            fr_t io[8];
            if (fread(io, sizeof(fr_t), 8, f) != 8) { printf("truncated case\n"); return 2; }
            fr_t st[BN_WIDTH]; memcpy(st, io, sizeof st);
            bn_permute_values(st, P, [&](int i) { return kr[i]; });
            for (int i = 0; i < BN_WIDTH; i++) if (!fr_eq(st[i], io[4 + i])) {
                if (bad < 8) printf("group %d case %llu element %d: %016llx..%016llx, want %016llx..%016llx\n", groups, (unsigned long long)c, i, (unsigned long long)st[i].l[3], (unsigned long long)st[i].l[0],
                                    (unsigned long long)io[4 + i].l[3], (unsigned long long)io[4 + i].l[0]);
                bad++;
            }
        }
        groups++; total += n;
    }
    fclose(f);
    printf("groups: %d cases: %llu\n", groups, (unsigned long long)total);
    printf(bad || total == 0 ? "FAILED\n" : "OK\n");
    return bad != 0 || total == 0;
}
