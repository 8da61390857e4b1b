// Host check of csrc/montform.h: every route of the canonical -> Montgomery conversion (two, three, four and eight 32-bit words, a run-time
// row count, and the dispatch by width) against v * 2^256 mod r computed here by 256 modular doublings on 64-bit limbs (unsigned __int128 carries), on the
// edge values of every class and 10^5 random values per class; the constants montform_init derives are printed so that the pytest wrapper
// (tests/test_montform_host.py) compares them, and a sample of (value, result) pairs, with Python integers.
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include "montform.h"
using namespace h2w;

typedef unsigned __int128 u128_t;
struct V4 { uint64_t w[4]; };
static const V4 RMOD = {{H2W_FR_M0, H2W_FR_M1, H2W_FR_M2, H2W_FR_M3}};
static bool geq(const V4 &a, const V4 &b) { for (int j = 3; j >= 0; j--) if (a.w[j] != b.w[j]) return a.w[j] > b.w[j]; return true; }
static V4 sub(const V4 &a, const V4 &b) { V4 r; u128_t bw = 0; for (int j = 0; j < 4; j++) { const u128_t t = (u128_t)a.w[j] - b.w[j] - (uint64_t)bw; r.w[j] = (uint64_t)t; bw = (t >> 64) & 1; } return r; }
static V4 dbl(const V4 &a) { V4 r; uint64_t c = 0; for (int j = 0; j < 4; j++) { r.w[j] = (a.w[j] << 1) | c; c = a.w[j] >> 63; } if (c) { printf("doubling overflowed\n"); exit(1); } return geq(r, RMOD) ? sub(r, RMOD) : r; }
static V4 ref_mont(V4 v) { while (geq(v, RMOD)) v = sub(v, RMOD); for (int i = 0; i < 256; i++) v = dbl(v); return v; }
static bool eq(const fr_t &a, const V4 &b) { return a.l[0] == b.w[0] && a.l[1] == b.w[1] && a.l[2] == b.w[2] && a.l[3] == b.w[3]; }
static uint64_t rng_s = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_s ^= rng_s << 7; rng_s ^= rng_s >> 9; return rng_s * 0x2545F4914F6CDD1Dull; }
static void hex(const char *name, const uint32_t *w, int n) { printf("%s 0x", name); for (int j = n - 1; j >= 0; j--) printf("%08x", w[j]); printf("\n"); }
static void hex4(const char *name, const uint64_t *w) { printf("%s 0x%016llx%016llx%016llx%016llx", name, (unsigned long long)w[3], (unsigned long long)w[2], (unsigned long long)w[1], (unsigned long long)w[0]); }

static MontForm K;
static long n_checked = 0; static int n_samples = 0;
// v through every route whose range holds it
static void check(const V4 &v, bool sample) {
    const V4 want = ref_mont(v);
    fr_t in; for (int j = 0; j < 4; j++) in.l[j] = v.w[j];
    auto bad = [&](const char *route) { printf("route %s wrong for ", route); hex4("v", v.w); printf("\n"); exit(1); };
    const bool w64 = (v.w[1] | v.w[2] | v.w[3]) == 0, w128 = (v.w[2] | v.w[3]) == 0;
    if (w64 && !eq(mont_from_u64(v.w[0], K), want)) bad("u64");
    if (w128 && (v.w[1] >> 32) == 0 && !eq(mont_from_u96(v.w[0], (uint32_t)v.w[1], K), want)) bad("u96");
    if (w128 && !eq(mont_from_u128(v.w[0], v.w[1], K), want)) bad("u128");
    if (w128) {      // the run-time row count of the expansion kernel's flush: any count that covers the value
        const uint32_t w[4] = {(uint32_t)v.w[0], (uint32_t)(v.w[0] >> 32), (uint32_t)v.w[1], (uint32_t)(v.w[1] >> 32)};
        for (int n = w64 ? 2 : (v.w[1] >> 32) ? 4 : 3; n <= 4; n++) { uint32_t o[8]; mf_convert_upto<4>(w, n, K, o); if (!eq(mf_pack(o), want)) bad("upto"); }
    }
    if (!eq(mont_from_fr(in, K), want)) bad("full");
    if (!eq(mont_from_cell(in, K), want)) bad("by width");
    if (geq(want, RMOD)) bad("range");
    n_checked++;
    if (sample && n_samples < 400) { hex4("sample", v.w); hex4(" ->", want.w); printf("\n"); n_samples++; }
}
static V4 v_u64(uint64_t x) { V4 v = {{x, 0, 0, 0}}; return v; }
static V4 v_pow2(int e) { V4 v = {{0, 0, 0, 0}}; v.w[e / 64] = 1ull << (e % 64); return v; }
static V4 v_dec(V4 v) { return sub(v, v_u64(1)); }

int main() {
    const int RBS[3] = {84, 65, 64};      // rb of lookup_bits 21, 13, 8
    montform_init(K, 84);
    for (int i = 0; i < 8; i++) { char nm[16]; snprintf(nm, sizeof nm, "c%d", i); hex(nm, K.c[i], 8); }
    hex("mu", K.mu, 2);
    for (int k = 0; k < 3; k++) { MontForm T; montform_init(T, RBS[k]); char nm[16]; snprintf(nm, sizeof nm, "neg%d", RBS[k]); hex(nm, T.neg_rb, 8);
        // the fixed cell agrees with the full route on -2^rb mod r
        fr_t n; const V4 nv = sub(RMOD, v_pow2(RBS[k])); for (int j = 0; j < 4; j++) n.l[j] = nv.w[j];
        const fr_t got = mont_from_fr(n, K);
        for (int j = 0; j < 4; j++) if (got.l[j] != (((uint64_t)T.neg_rb[2 * j + 1] << 32) | T.neg_rb[2 * j])) { printf("neg_rb constant wrong (rb %d)\n", RBS[k]); return 1; } }
    // edges
    check(v_u64(0), true); check(v_u64(1), true);
    const int LS[3] = {21, 13, 8};
    for (int k = 0; k < 3; k++) { check(v_u64((1ull << LS[k]) - 1), true); check(v_u64(1ull << LS[k]), true); }
    check(v_u64(0xffffffffull), true); check(v_u64(1ull << 32), true);
    check(v_u64(1ull << 63), true); check(v_u64(~0ull), true); check(v_u64(GL_P - 1), true); check(v_u64(GL_P), true);
    check(v_pow2(64), true); check(v_pow2(65), true); check(v_pow2(84), true); check(v_dec(v_pow2(84)), true); check(v_pow2(127), true);
    check(v_dec(v_pow2(128)), true); check(v_pow2(128), true);
    check(v_dec(RMOD), true); check(RMOD, true);
    for (int k = 0; k < 3; k++) { check(sub(RMOD, v_pow2(RBS[k])), true); check(v_pow2(RBS[k]), true); }
    { V4 top = {{~0ull, ~0ull, ~0ull, ~0ull}}; check(top, true); }      // (not canonical: the route's own range is 2^256)
    // random values per class
    for (int i = 0; i < 100000; i++) {
        const bool s = i < 20;
        check(v_u64(rnd() >> 43), s); check(v_u64(rnd() >> 32), s); check(v_u64(rnd()), s);
        { V4 v = {{rnd(), rnd() >> 32, 0, 0}}; check(v, s); }
        { V4 v = {{rnd(), rnd() >> (i % 64), 0, 0}}; check(v, s); }
        { V4 v = {{rnd(), rnd(), rnd(), rnd() >> 2}}; while (geq(v, RMOD)) v = sub(v, RMOD); check(v, s); }
    }
    printf("checked %ld values\nOK\n", n_checked);
    return 0;
}
