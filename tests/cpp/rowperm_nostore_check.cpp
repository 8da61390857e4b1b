// Host check of the store-free instantiation of the row-cooperative PoseidonBN254 permutation (csrc/rowperm.h bn_permute_rows<false>: what
// k_verdict_merkle_row runs on the device), with the 64 lanes of a wavefront simulated as in rowfr_check.cpp:
//   * bn_permute_rows<false>(st, K, L, nullptr) stores nothing - a store through the null pointer, or an address formed from it, ends this program
//     (the test also builds it with -fsanitize=address,undefined);
//   * its output state equals that of bn_permute_rows<true> (whose S-box buffer is written: every value slot changes) and of the plain reference walk
//     on canonical values (chips.h PoseidonBN254PermutationChip; hash/poseidon_bn254/permutation.rs:83-203);
//   * on the published circomlib tables and on full-width random tables; inputs: the all-zero state, a state of r - 1, random states;
//   * no sum wraps on the simulated lanes.
// Built and run by tests/test_rowperm_nostore.py (g++).
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include "bntab.h"
static uint32_t g_tab9[h2w::BK9_N * h2w::BK9_W];
#define RF_TAB9 g_tab9
#include "rowperm.h"
#include "poseidon_tables.h"
using namespace h2w;
namespace h2w { namespace rf { bool g_overflow = false; } }

static uint64_t rng_s = 0xD1B54A32D192ED03ull;
static uint64_t rnd() { rng_s ^= rng_s << 7; rng_s ^= rng_s >> 9; return rng_s * 0x2545F4914F6CDD1Dull; }
static fr_t rnd_fr() {      // 254 random bits, reduced (r > 2^253: at most three subtractions)
    fr_t x; x.l[0] = rnd(); x.l[1] = rnd(); x.l[2] = rnd(); x.l[3] = rnd() >> 2;
    while (fr_geq_mod(x)) x = fr_sub_mod_raw(x);
    return x;
}
static bool eq(const fr_t &a, const fr_t &b) { return a.l[0] == b.l[0] && a.l[1] == b.l[1] && a.l[2] == b.l[2] && a.l[3] == b.l[3]; }

// the reference walk of rowfr_check.cpp: ark; 4 full rounds [P on the last]; 56 partial; 4 full
static void reference_permute(const h2w_poseidon_consts_t &kc, const FrParams &P, fr_t ref[4]) {
    auto mul = [&](const fr_t &x, const fr_t &y) { return fr_mul(x, y, P); };
    auto exp5 = [&](const fr_t &x) { const fr_t x2 = mul(x, x), x4 = mul(x2, x2); return mul(x4, x); };
    auto mixm = [&](const h2w_fr_t m[4][4]) { fr_t ns[4]; for (int i = 0; i < 4; i++) { ns[i] = fr_zero(); for (int j = 0; j < 4; j++) ns[i] = fr_add(mul(m[j][i], ref[j]), ns[i]); } for (int i = 0; i < 4; i++) ref[i] = ns[i]; };
    auto ark = [&](int at) { for (int i = 0; i < 4; i++) ref[i] = fr_add(ref[i], kc.bn_c[at + i]); };
    ark(0);
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 4; j++) ref[j] = exp5(ref[j]); ark((i + 1) * 4); mixm(kc.bn_m); }
    for (int j = 0; j < 4; j++) ref[j] = exp5(ref[j]);
    ark(16); mixm(kc.bn_p);
    for (int r = 0; r < 56; r++) {
        ref[0] = exp5(ref[0]); ref[0] = fr_add(ref[0], kc.bn_c[20 + r]);
        fr_t ns0 = fr_zero(); for (int j = 0; j < 4; j++) ns0 = fr_add(mul(kc.bn_s[7 * r + j], ref[j]), ns0);
        for (int k = 1; k < 4; k++) ref[k] = fr_add(mul(kc.bn_s[7 * r + 4 + k - 1], ref[0]), ref[k]);
        ref[0] = ns0;
    }
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 4; j++) ref[j] = exp5(ref[j]); ark(20 + 56 + i * 4); mixm(kc.bn_m); }
    for (int j = 0; j < 4; j++) ref[j] = exp5(ref[j]);
    mixm(kc.bn_m);
}

int main() {
    const FrParams P = fr_params_init();
    rf::RowConst K; rf::rowconst_init(K, P);
    const rf::LaneK L = rf::lane_consts();
    int fails = 0, runs = 0;
    for (int tabs = 0; tabs < 2; tabs++) {
        h2w_poseidon_consts_t kc = H2W_POSEIDON_PUBLISHED;
        if (tabs == 1) { for (auto &x : kc.bn_c) x = rnd_fr(); for (auto &x : kc.bn_s) x = rnd_fr(); for (auto &rw : kc.bn_m) for (auto &x : rw) x = rnd_fr(); for (auto &rw : kc.bn_p) for (auto &x : rw) x = rnd_fr(); }
        std::vector<fr_t> tab(BK_ALL); bn_table_build(kc, P, tab.data()); bn_table9_build(tab.data(), g_tab9);
        for (int it = 0; it < 6; it++, runs++) {
            fr_t in[4], ref[4], bare[4], stored[4];
            for (int i = 0; i < 4; i++) {
                in[i] = it == 0 ? fr_zero() : rnd_fr();
                if (it == 1) { for (int j = 0; j < 4; j++) in[i].l[j] = fr_mod_limb(j); in[i].l[0] -= 1; }      // r - 1
                ref[i] = bare[i] = stored[i] = in[i];
            }
            reference_permute(kc, P, ref);
            rf::g_overflow = false;
            rf::bn_permute_rows<false>(bare, K, L, nullptr);
            if (rf::g_overflow) { printf("a sum wrapped inside the store-free permutation (tables %d, input %d)\n", tabs, it); fails++; }
            std::vector<uint32_t> sbx9(56 * 3 * rf::SBX9_W, 0xdeadbeefu);
            rf::bn_permute_rows<true>(stored, K, L, sbx9.data());
            for (int v = 0; v < 56 * 3; v++) if (sbx9[(size_t)v * rf::SBX9_W] == 0xdeadbeefu) { printf("bn_permute_rows<true> left S-box value %d unwritten\n", v); fails++; break; }
            fr_t dflt[4]; for (int i = 0; i < 4; i++) dflt[i] = in[i];
            std::vector<uint32_t> sbx9d(56 * 3 * rf::SBX9_W, 0u);
            rf::bn_permute_rows(dflt, K, L, sbx9d.data());      // the default argument is the storing form
            if (sbx9d != sbx9) { printf("bn_permute_rows without an argument is not bn_permute_rows<true>\n"); fails++; }
            for (int i = 0; i < 4; i++) {
                if (!eq(bare[i], ref[i])) { printf("store-free output differs from the reference (tables %d, input %d, element %d)\n", tabs, it, i); fails++; }
                if (!eq(bare[i], stored[i]) || !eq(bare[i], dflt[i])) { printf("store-free output differs from the storing form's (tables %d, input %d, element %d)\n", tabs, it, i); fails++; }
            }
        }
    }
    if (fails) { printf("FAILED: %d\n", fails); return 1; }
    printf("OK %d permutations\n", runs);
    return 0;
}
