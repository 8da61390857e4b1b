// Host check of csrc/glpval.h: the per-thread Goldilocks-Poseidon value permutation (what a lane of the replay interpreter runs for a fused
// stretch, csrc/replay.hip DOP_GLPERM), compiled as plain C++, against known answers.
// The driver (tests/test_glperm_values.py) writes the cases: groups of [u64 n][h2w_poseidon_consts_t][n x {in[12], want[12]}] - plonky2's
// published vectors on the published tables, the oracle's value permutation on random states with full-width seeded tables.
// g++ -O2 -std=c++17 -I halo2-plonky2-verifier_amd/csrc -I include tests/cpp/glperm_values_check.cpp && ./a.out cases.bin
#include <cstdio>
#include <cstring>
#include <vector>
#include "glpval.h"
using namespace h2w;

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: glperm_values_check cases.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    static_assert(sizeof(h2w_poseidon_consts_t) >= 8 * GV_WORDS, "the Goldilocks block leads the constants");
    int bad = 0, groups = 0; uint64_t total = 0, n;
    while (fread(&n, 8, 1, f) == 1) {
        static h2w_poseidon_consts_t k;
        if (fread(&k, sizeof k, 1, f) != 1) { printf("truncated constants\n"); return 2; }
        const uint64_t *kw = reinterpret_cast<const uint64_t *>(&k);
        for (uint64_t c = 0; c < n; c++) {
            uint64_t io[24];
            if (fread(io, 8, 24, f) != 24) { printf("truncated case\n"); return 2; }
            uint64_t st[GV_W]; memcpy(st, io, sizeof st);
            glp_permute_values(st, [&](int i) { return kw[i]; });
            for (int i = 0; i < GV_W; i++) if (st[i] != io[12 + i]) { if (bad < 8) printf("group %d case %llu element %d: %016llx, want %016llx\n", groups, (unsigned long long)c, i, (unsigned long long)st[i], (unsigned long long)io[12 + i]); bad++; }
        }
        groups++; total += n;
    }
    fclose(f);
    printf("groups: %d cases: %llu\n", groups, (unsigned long long)total);
    printf(bad || total == 0 ? "FAILED\n" : "OK\n");
    return bad != 0 || total == 0;
}
