// The largest lazy value the row-cooperative PoseidonBN254 permutation (csrc/rowperm.h bn_permute_rows) holds, on the case file of the device
// checks' `bn` group (tests/devcheck_ref.py bn_pack): the 64 lanes of a wavefront simulated as in rowfr_check.cpp, with every operand and result of
// rf::mont and every result of rf::tighten inside the permutation looked at on the way (rowperm.h calls them by these names: the two are renamed for
// that one include; the arithmetic is the product's own).  Nothing is judged here but wrapped sums: tests/test_devcheck_refs.py reads the figures.
//   rowperm_reach <case file>   ->   one line per case: its index, its table, the largest value (hex), the output state (hex), "wrapped" if a sum wrapped
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include "bntab.h"
static uint32_t g_tab9[h2w::BK9_N * h2w::BK9_W];
#define RF_TAB9 g_tab9
#include "rowfr.h"
namespace h2w { namespace rf {
bool g_overflow = false;
struct Big { uint64_t w[5]; };
static Big g_peak;
static Big big_from_limbs(const uint32_t *t) { Big r = {{0, 0, 0, 0, 0}}; for (int i = 8; i >= 0; i--) { uint64_t carry = t[i]; for (int j = 0; j < 5; j++) { const unsigned __int128 x = ((unsigned __int128)r.w[j] << 29) + carry; r.w[j] = (uint64_t)x; carry = (uint64_t)(x >> 64); } } return r; }
static bool big_less(const Big &a, const Big &b) { for (int j = 4; j >= 0; j--) if (a.w[j] != b.w[j]) return a.w[j] < b.w[j]; return false; }
static void look(const V &v) {
    for (int row = 0; row < 4; row++) { uint32_t t[9]; for (int k = 0; k < 9; k++) t[k] = v.l[16 * row + k]; const Big x = big_from_limbs(t); if (big_less(g_peak, x)) g_peak = x; }
}
inline V tighten_seen(const V &v) { const V r = tighten(v); look(r); return r; }
inline V mont_seen(const A9 &A, const V &b, const RowConst &K, const LaneK &L) { look(b); const V r = mont(A, b, K, L); look(r); return r; }
} }
#define tighten tighten_seen
#define mont mont_seen
#include "rowperm.h"
#undef tighten
#undef mont
using namespace h2w;

int main(int argc, char **argv) {
    if (argc != 2) { printf("usage: rowperm_reach <case file>\n"); return 2; }
    std::vector<uint64_t> in;
    {
        FILE *f = fopen(argv[1], "rb"); if (!f) { printf("cannot read %s\n", argv[1]); return 2; }
        fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
        if (bytes < 16 || bytes % 8) { printf("case file: not whole 64-bit words\n"); fclose(f); return 2; }
        in.resize((size_t)bytes / 8);
        const size_t got = fread(in.data(), 8, in.size(), f); fclose(f);
        if (got != in.size()) { printf("short read\n"); return 2; }
    }
    constexpr size_t KW = sizeof(h2w_poseidon_consts_t) / 8;
    const size_t nt = in[0], nc = in[1];
    if (in.size() != 2 + nt * KW + nc * 20) { printf("case file: unexpected size\n"); return 2; }
    const FrParams P = fr_params_init();
    rf::RowConst K; rf::rowconst_init(K, P);
    const rf::LaneK L = rf::lane_consts();
    std::vector<fr_t> tab(BK_ALL); std::vector<uint32_t> sbx9(56 * 3 * rf::SBX9_W);
    for (size_t i = 0; i < nc; i++) {
        const uint64_t *cs = &in[2 + nt * KW + i * 20];
        if (cs[0] >= nt) { printf("case %zu: bad table\n", i); return 2; }
        bn_table_build(*reinterpret_cast<const h2w_poseidon_consts_t *>(&in[2 + cs[0] * KW]), P, tab.data()); bn_table9_build(tab.data(), g_tab9);
        fr_t st[4]; for (int e = 0; e < 4; e++) for (int j = 0; j < 4; j++) st[e].l[j] = cs[4 + 4 * e + j];
        rf::g_overflow = false; rf::g_peak = rf::Big{{0, 0, 0, 0, 0}};
        rf::bn_permute_rows(st, K, L, sbx9.data());
        printf("case %zu table %llu peak 0x%llx%016llx%016llx%016llx%016llx state", i, (unsigned long long)cs[0], (unsigned long long)rf::g_peak.w[4], (unsigned long long)rf::g_peak.w[3],
               (unsigned long long)rf::g_peak.w[2], (unsigned long long)rf::g_peak.w[1], (unsigned long long)rf::g_peak.w[0]);
        for (int e = 0; e < 4; e++) printf(" 0x%016llx%016llx%016llx%016llx", (unsigned long long)st[e].l[3], (unsigned long long)st[e].l[2], (unsigned long long)st[e].l[1], (unsigned long long)st[e].l[0]);
        printf("%s\n", rf::g_overflow ? " wrapped" : "");
    }
    return 0;
}
