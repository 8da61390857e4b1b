// Host check of csrc/proverhash.h: the prover's value hashers (what the lanes of prover.hip's leaf, tree-level and proof-of-work kernels and its host
// transcript run), compiled as plain C++, against the oracle's values.
// The driver (tests/test_proverhash_host.py) writes the cases: groups of [u64 kind][u64 n][h2w_poseidon_consts_t][n cases], a case being
//   kind 0  gl_permute      in[12] want[12]                      small-MDS tables: gl_permute_t<true>, gl_permute_t<false> and the dispatcher; others: <false> and the dispatcher
//   kind 1  bn_permute_m    in[4][4] want[4][4]                  canonical elements; to_mont before, from_mont behind
//   kind 2  hash_or_noop    mode maxn n in[32] want[4]           maxn = MAX_BATCH_POLYS or 2 * MAX_ARITY: the two instantiations of the kernels
//   kind 3  two_to_one      mode l[4] r[4] want[4]
// The constants of a group go through prover_consts_init, as a prover handle's do.  The counts printed at the end are asserted by the driver.
// g++ -O2 -std=c++17 -I halo2-plonky2-verifier_amd/csrc -I include tests/cpp/proverhash_check.cpp && ./a.out cases.bin
#include <cstdio>
#include <cstring>
#include "proverhash.h"
using namespace h2w;

static int bad = 0;
static void hold(const char *what, int group, uint64_t c, const uint64_t *got, const uint64_t *want, int n) {
    for (int i = 0; i < n; i++) if (got[i] != want[i]) { if (bad < 8) printf("group %d case %llu %s word %d: %016llx, want %016llx\n", group, (unsigned long long)c, what, i, (unsigned long long)got[i], (unsigned long long)want[i]); bad++; }
}
template <int MAXN> static H4 run_hash(const ProverConsts *K, int mode, const uint64_t *in, int n) {
    uint64_t buf[MAXN]; memcpy(buf, in, sizeof buf);
    return hash_or_noop<MAXN>(K, mode, buf, n);
}

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: proverhash_check cases.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    static_assert(MAX_BATCH_POLYS == 16 && 2 * MAX_ARITY == 32, "the case layout holds 32 input words");
    int groups = 0; uint64_t hdr[2], gl_small = 0, gl_full = 0, bn = 0, hash16 = 0, hash32 = 0, two = 0;
    while (fread(hdr, 8, 2, f) == 2) {
        static h2w_poseidon_consts_t k; static ProverConsts K;
        if (fread(&k, sizeof k, 1, f) != 1) { printf("truncated constants\n"); return 2; }
        prover_consts_init(K, k);
        const int words = hdr[0] == 0 ? 24 : hdr[0] == 1 ? 32 : hdr[0] == 2 ? 39 : hdr[0] == 3 ? 13 : 0;
        if (!words) { printf("unknown group kind\n"); return 2; }
        for (uint64_t c = 0; c < hdr[1]; c++) {
            uint64_t io[39];
            if (fread(io, 8, (size_t)words, f) != (size_t)words) { printf("truncated case\n"); return 2; }
            if (hdr[0] == 0) {
                uint64_t st[12];
                memcpy(st, io, sizeof st); gl_permute(&K.k, st); hold("gl_permute", groups, c, st, io + 12, 12);
                memcpy(st, io, sizeof st); gl_permute_t<false>(&K.k, st); hold("gl_permute_t<false>", groups, c, st, io + 12, 12);
                if (gl_mds_is_small(&K.k)) { memcpy(st, io, sizeof st); gl_permute_t<true>(&K.k, st); hold("gl_permute_t<true>", groups, c, st, io + 12, 12); gl_small++; } else gl_full++;
            } else if (hdr[0] == 1) {
                fr_t st[4]; memcpy(st, io, sizeof st);
                for (int i = 0; i < 4; i++) st[i] = to_mont(&K, st[i]);
                bn_permute_m(&K, st);
                for (int i = 0; i < 4; i++) st[i] = from_mont(&K, st[i]);
                hold("bn_permute_m", groups, c, st[0].l, io + 16, 16); bn++;
            } else if (hdr[0] == 2) {
                const int mode = (int)io[0], n = (int)io[2];
                if ((io[1] != 16 && io[1] != 32) || n < 0 || n > (int)io[1]) { printf("bad hash case\n"); return 2; }
                const H4 h = io[1] == 16 ? run_hash<MAX_BATCH_POLYS>(&K, mode, io + 3, n) : run_hash<2 * MAX_ARITY>(&K, mode, io + 3, n);
                hold("hash_or_noop", groups, c, h.w, io + 35, 4); (io[1] == 16 ? hash16 : hash32)++;
            } else {
                H4 l, r; memcpy(l.w, io + 1, 32); memcpy(r.w, io + 5, 32);
                const H4 h = two_to_one(&K, (int)io[0], l, r);
                hold("two_to_one", groups, c, h.w, io + 9, 4); two++;
            }
        }
        groups++;
    }
    fclose(f);
    const uint64_t total = gl_small + gl_full + bn + hash16 + hash32 + two;
    printf("groups: %d gl_small: %llu gl_full: %llu bn: %llu hash16: %llu hash32: %llu two: %llu\n", groups, (unsigned long long)gl_small, (unsigned long long)gl_full,
           (unsigned long long)bn, (unsigned long long)hash16, (unsigned long long)hash32, (unsigned long long)two);
    printf(bad || total == 0 ? "FAILED\n" : "OK\n");
    return bad != 0 || total == 0;
}
