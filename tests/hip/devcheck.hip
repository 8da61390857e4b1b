// Device harness of tests/test_gpu_devcheck.py: runs the product's own __device__ arithmetic (csrc/glperm.h, rowfr.h, rowperm.h, field.h, montform.h)
// on words a test wrote (csrc/bnquad.h bn_values too), and writes the raw results back.  No reference arithmetic lives here: the expected values are Python integers
// (tests/devcheck_ref.py).  Files are raw little-endian 64-bit words (32-bit arrays are packed two to a word); the layout of every group is spelled out
// at its function and mirrored by the test.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I halo2-plonky2-verifier_amd/csrc -I include tests/hip/devcheck.hip -o devcheck
//   devcheck <glq|mds|perm|mont|bn|quad|plain> <case file> <result file>
// One process, one group, one device context.  Exit status 0: every kernel ran and the result file is complete; anything else: a message on stdout,
// and nothing was launched after the first HIP error.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "common.h"
#include "batchargs.h"
#define RF_TAB9 s_bn_tab9
#include "rowperm.h"
#include "montform.h"
using namespace h2w;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
#define RAN(name) do { CK(hipGetLastError()); hipError_t e_ = hipDeviceSynchronize(); if (e_ != hipSuccess) { printf("%s: %s\n", name, hipGetErrorString(e_)); return 1; } } while (0)

constexpr int KW = sizeof(h2w_poseidon_consts_t) / 8;      // 64-bit words of a constant block
static_assert(sizeof(h2w_poseidon_consts_t) % 8 == 0, "constant block in 64-bit words");

// ---------------------------------------------------------------------------------------------- (a) glq: per-lane primitives, every lane its own case
enum { GLQ_REDUCE = 0, GLQ_REDUCE96, GLQ_MUL, GLQ_MULADD, GLQ_ADD, GLQ_OPS };
__global__ __launch_bounds__(64) void k_glq_single(int op, const uint64_t *a, const uint64_t *b, const uint64_t *c, uint64_t *out) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    const uint64_t x = a[i], y = b[i], z = c[i]; uint64_t r = 0;
    switch (op) {
    case GLQ_REDUCE: r = glq_reduce(x, (uint32_t)y, (uint32_t)z); break;
    case GLQ_REDUCE96: r = glq_reduce96(x, (uint32_t)y, (uint32_t)z); break;
    case GLQ_MUL: r = glq_mul(x, y); break;
    case GLQ_MULADD: r = glq_muladd(x, y, z); break;
    default: r = glq_add(x, y); break;
    }
    out[i] = r;
}
// the same cases as chains: the result of one asm block is the operand of the next one, or is read by another lane right behind it
//   GLQ_REDUCE  out[i] = reduce(reduce(x, y, z), y, z)
//   GLQ_MUL     out[i] = (x y) z;   out[n + i] = the S-box shape of glp_permute_lanes on x: x^2, x^3 (even rows) | x^4 (odd rows), lane swap, product
//   GLQ_MULADD  four rounds of { acc = y s0 + acc; s0 = lane 16 + k's acc } from acc = z, s0 = lane 0's x:   out[i] = acc, out[n + i] = s0
__global__ __launch_bounds__(64) void k_glq_chain(int op, size_t n, const uint64_t *a, const uint64_t *b, const uint64_t *c, uint64_t *out) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    const uint64_t x = a[i], y = b[i], z = c[i];
    if (op == GLQ_REDUCE) {
        out[i] = glq_reduce(glq_reduce(x, (uint32_t)y, (uint32_t)z), (uint32_t)y, (uint32_t)z);
    } else if (op == GLQ_MUL) {
        out[i] = glq_mul(glq_mul(x, y), z);
        const bool odd_row = (threadIdx.x >> 4) & 1;
        const uint64_t v2 = glq_mul(x, x); uint64_t t = glq_mul(v2, odd_row ? v2 : x);
        uint64_t e, o; glq_pair_rows(t, e, o);
        out[n + i] = glq_mul(e, o);
    } else {
        uint64_t acc = z, s0 = readlane64(x, 0);
#pragma unroll 1
        for (int k = 0; k < 4; k++) {
            acc = glq_muladd(y, s0, acc);
            glq_lane_fence<0>(acc);
            s0 = readlane64(acc, 16 + k);
        }
        out[i] = acc; out[n + i] = s0;
    }
}
// in:  n[8] (reduce, reduce96, mul, muladd, add, 0, 0, 0: multiples of 64), then per op three arrays of n words (32-bit operands in the low half)
// out: reduce n, its chain n | reduce96 n | mul n, its chains 2 n | muladd n, its chains 2 n | add n
static int run_glq(const std::vector<uint64_t> &in, const uint64_t *din, std::vector<uint64_t> &res, uint64_t *&dout) {
    if (in.size() < 8) { printf("short case file\n"); return 1; }
    size_t need = 8, outw = 0;
    for (int op = 0; op < GLQ_OPS; op++) { if (in[op] % 64) { printf("whole wavefronts only\n"); return 1; } need += 3 * in[op]; outw += in[op] * (op == GLQ_REDUCE ? 2 : op == GLQ_MUL || op == GLQ_MULADD ? 3 : 1); }
    if (in.size() != need) { printf("case file: %zu words, expected %zu\n", in.size(), need); return 1; }
    res.assign(outw, 0); CK(hipMalloc(&dout, outw * 8 + 8)); CK(hipMemset(dout, 0xA5, outw * 8 + 8));
    size_t at = 8, o = 0;
    for (int op = 0; op < GLQ_OPS; op++) {
        const size_t n = in[op]; const uint64_t *a = din + at, *b = a + n, *c = b + n;
        if (n) {
            hipLaunchKernelGGL(k_glq_single, dim3(n / 64), dim3(64), 0, 0, op, a, b, c, dout + o); RAN("k_glq_single");
            o += n;
            if (op == GLQ_REDUCE || op == GLQ_MUL || op == GLQ_MULADD) { hipLaunchKernelGGL(k_glq_chain, dim3(n / 64), dim3(64), 0, 0, op, n, a, b, c, dout + o); RAN("k_glq_chain"); o += op == GLQ_REDUCE ? n : 2 * n; }
        }
        at += 3 * n;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- (b) the hand-scheduled v_readlane blocks, one wavefront per case
// case: x[64], next[64] (words), m[64][12] (dwords: this lane's row entries)  ->  r[64]
__global__ __launch_bounds__(64) void k_mds_small(const uint64_t *in, uint64_t *out) {
    const uint64_t *cs = in + (size_t)blockIdx.x * 512; const int lane = threadIdx.x;
    const uint32_t *mp = reinterpret_cast<const uint32_t *>(cs + 128) + lane * SPONGE_WIDTH;
    uint32_t m[SPONGE_WIDTH];
#pragma unroll
    for (int j = 0; j < SPONGE_WIDTH; j++) m[j] = mp[j];
    out[(size_t)blockIdx.x * 64 + lane] = glq_mds_small(cs[lane], m, cs[64 + lane]);
}
// case: a0[64], a1[64] (words), limb[64], wl[64][12], wh[64][12] (dwords)  ->  a0[64], a1[64]
__global__ __launch_bounds__(64) void k_dense12(const uint64_t *in, uint64_t *out) {
    const uint64_t *cs = in + (size_t)blockIdx.x * 928; const int lane = threadIdx.x;
    const uint32_t *d = reinterpret_cast<const uint32_t *>(cs + 128);
    uint32_t wl[SPONGE_WIDTH], wh[SPONGE_WIDTH];
#pragma unroll
    for (int j = 0; j < SPONGE_WIDTH; j++) { wl[j] = d[64 + lane * SPONGE_WIDTH + j]; wh[j] = d[64 + 64 * SPONGE_WIDTH + lane * SPONGE_WIDTH + j]; }
    uint64_t a0 = cs[lane], a1 = cs[64 + lane];
    glq_dense12(d[lane], wl, wh, a0, a1);
    out[(size_t)blockIdx.x * 128 + lane] = a0; out[(size_t)blockIdx.x * 128 + 64 + lane] = a1;
}
// in: n_mds, n_d12, then the cases of glq_mds_small (512 words each), then those of glq_dense12 (928 words each);  out: 64 words each, then 128 each
static int run_mds(const std::vector<uint64_t> &in, const uint64_t *din, std::vector<uint64_t> &res, uint64_t *&dout) {
    if (in.size() < 2 || in.size() != 2 + in[0] * 512 + in[1] * 928) { printf("case file: unexpected size\n"); return 1; }
    const size_t nm = in[0], nd = in[1], outw = nm * 64 + nd * 128;
    res.assign(outw, 0); CK(hipMalloc(&dout, outw * 8 + 8)); CK(hipMemset(dout, 0xA5, outw * 8 + 8));
    if (nm) { hipLaunchKernelGGL(k_mds_small, dim3(nm), dim3(64), 0, 0, din + 2, dout); RAN("k_mds_small"); }
    if (nd) { hipLaunchKernelGGL(k_dense12, dim3(nd), dim3(64), 0, 0, din + 2 + nm * 512, dout + nm * 64); RAN("k_dense12"); }
    return 0;
}

// ---------------------------------------------------------------------------------------------- (c) glp_permute_lanes, one wavefront per case
// case (16 words): table, small, n, list, state[12]  ->  80 words: every lane's output of the n-th permutation, then the 13 words the first permutation lists
// (lane 0: a tag, lanes 1..12: the input state, as glcoop.h coop_poseidon_permute lists them; untouched when `list` is 0)
__global__ __launch_bounds__(64) void k_perm(const uint64_t *tabs, const uint64_t *cases, uint64_t *out) {
    const uint64_t *cs = cases + (size_t)blockIdx.x * 16;
    const int tab = __builtin_amdgcn_readfirstlane((int)cs[0]), small = __builtin_amdgcn_readfirstlane((int)cs[1]), n = __builtin_amdgcn_readfirstlane((int)cs[2]),
              list = __builtin_amdgcn_readfirstlane((int)cs[3]);
    stage_glp_consts<true>(reinterpret_cast<const h2w_poseidon_consts_t *>(tabs + (size_t)tab * (KW + GLP_AUX_WORDS)), threadIdx.x, 64);
    const int lane = threadIdx.x;
    uint64_t *o = out + (size_t)blockIdx.x * 80;
    uint64_t x = (lane & 15) < SPONGE_WIDTH ? cs[4 + (lane & 15)] : 0;      // every 16-lane row alike
    const uint64_t w = lane == 0 ? 0xC0DE000000000000ull + blockIdx.x : lane <= SPONGE_WIDTH ? cs[4 + lane - 1] : 0;
    for (int i = 0; i < n; i++) {
        uint64_t *at = list && i == 0 && lane < GLP_LIST_WORDS ? o + 64 + lane : nullptr;
        x = glp_permute_lanes(x, (lds64_t *)s_glp_k, (lds64_t *)s_glp_m, (lds64_t *)s_glp_x, lane, small != 0, at, w);
    }
    o[lane] = x;
}
// in: n_tab, n_case, the constant blocks (KW words each), the cases;  out: 80 words per case
static int run_perm(const std::vector<uint64_t> &in, const uint64_t *din, std::vector<uint64_t> &res, uint64_t *&dout) {
    if (in.size() < 2 || in.size() != 2 + in[0] * KW + in[1] * 16) { printf("case file: unexpected size\n"); return 1; }
    const size_t nt = in[0], nc = in[1], stride = KW + GLP_AUX_WORDS;
    for (size_t i = 0; i < nc; i++) { const uint64_t *cs = &in[2 + nt * KW + i * 16]; if (cs[0] >= nt || cs[2] > 64) { printf("case %zu: bad table or chain length\n", i); return 1; } }
    std::vector<uint64_t> tabs(nt * stride);
    for (size_t t = 0; t < nt; t++) {      // the derived tables behind each block, as the plan keeps them on the device
        memcpy(&tabs[t * stride], &in[2 + t * KW], KW * 8);
        glp_aux_tables(*reinterpret_cast<const h2w_poseidon_consts_t *>(&in[2 + t * KW]), &tabs[t * stride + KW]);
    }
    uint64_t *dt; CK(hipMalloc(&dt, tabs.size() * 8 + 8)); CK(hipMemcpy(dt, tabs.data(), tabs.size() * 8, hipMemcpyHostToDevice));
    res.assign(nc * 80, 0); CK(hipMalloc(&dout, nc * 80 * 8 + 8)); CK(hipMemset(dout, 0xA5, nc * 80 * 8 + 8));
    if (nc) { hipLaunchKernelGGL(k_perm, dim3(nc), dim3(64), 0, 0, dt, din + 2 + nt * KW, dout); RAN("k_perm"); }
    return 0;
}

// ---------------------------------------------------------------------------------------------- (d) the lane-cooperative Montgomery product, one wavefront per case
// case (136 dwords): a[4][9], b[4][9] (the limbs of row r's operands), v[64] (tighten's input)
//   ->  1344 dwords: A built by replicate + put_rows [9][64], A built by replicate_rows [9][64], mont of the first [64], mont of the second [64], tighten(v) [64]
__global__ __launch_bounds__(64) void k_mont(rf::RowConst K, const uint32_t *in, uint32_t *out) {
#if defined(__HIP_DEVICE_COMPILE__)      // (on the host rowfr.h is the simulated-lanes form)
    const uint32_t *cs = in + (size_t)blockIdx.x * 136; uint32_t *o = out + (size_t)blockIdx.x * 1344;
    const rf::LaneK L = rf::lane_consts();
    const unsigned lane = threadIdx.x, row = lane >> 4, k = lane & 15;
    const uint32_t va = k < 9 ? cs[row * 9 + k] : 0u, vb = k < 9 ? cs[36 + row * 9 + k] : 0u;
    rf::A9 A1;
#pragma unroll
    for (int i = 0; i < 9; i++) A1.a[i] = 0u;
#pragma unroll
    for (int r = 0; r < 4; r++) { uint32_t t[9]; rf::replicate(va, r, t); rf::put_rows(A1, row == (unsigned)r, t); }
    const rf::A9 A2 = rf::replicate_rows(va);
#pragma unroll
    for (int i = 0; i < 9; i++) { o[i * 64 + lane] = A1.a[i]; o[(9 + i) * 64 + lane] = A2.a[i]; }
    o[18 * 64 + lane] = rf::mont(A1, vb, K, L);
    o[19 * 64 + lane] = rf::mont(A2, vb, K, L);
    o[20 * 64 + lane] = rf::tighten(cs[72 + lane]);
#endif
}
// in: n_case, the cases (68 words each);  out: 672 words per case
static int run_mont(const std::vector<uint64_t> &in, const uint64_t *din, std::vector<uint64_t> &res, uint64_t *&dout) {
    if (in.size() < 1 || in.size() != 1 + in[0] * 68) { printf("case file: unexpected size\n"); return 1; }
    const size_t nc = in[0];
    const FrParams P = fr_params_init(); rf::RowConst K; rf::rowconst_init(K, P);
    res.assign(nc * 672, 0); CK(hipMalloc(&dout, nc * 672 * 8 + 8)); CK(hipMemset(dout, 0xA5, nc * 672 * 8 + 8));
    if (nc) { hipLaunchKernelGGL(k_mont, dim3(nc), dim3(64), 0, 0, K, reinterpret_cast<const uint32_t *>(din + 1), reinterpret_cast<uint32_t *>(dout)); RAN("k_mont"); }
    return 0;
}

// ---------------------------------------------------------------------------------------------- (e) bn_permute_rows, one wavefront per case
// case (20 words): table, 0, 0, 0, state[4][4]  ->  BN_OUT words: the output state [4][4], the 56 x 3 x SBX9_W S-box dwords, then the output state [4][4] of the
// no-store form bn_permute_rows<false> (what k_verdict_merkle_row runs) on the same input
constexpr int BN_OUT = 16 + BN_PARTIAL_ROUNDS * 3 * rf::SBX9_W / 2 + 16;
__global__ __launch_bounds__(64) void k_bn(const uint32_t *tab9s, const rf::RowConst *rowk, const uint64_t *cases, uint64_t *out) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint64_t *cs = cases + (size_t)blockIdx.x * 20;
    const int tab = __builtin_amdgcn_readfirstlane((int)cs[0]);
    stage_bn_consts9(tab9s + (size_t)tab * (BK9_N * BK9_W), threadIdx.x, 64);
    rf::RowConst K;
    {   // wave-uniform: scalar loads (batchargs.h load_row_consts)
        const uint32_t *src = reinterpret_cast<const uint32_t *>(rowk); uint32_t *dst = reinterpret_cast<uint32_t *>(&K);
#pragma unroll
        for (unsigned i = 0; i < sizeof(rf::RowConst) / 4; i++) dst[i] = *(const __attribute__((address_space(4))) uint32_t *)(src + i);
    }
    const rf::LaneK L = rf::lane_consts();
    fr_t st[4], bare[4];
#pragma unroll
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) bare[i].l[j] = st[i].l[j] = H2W_CLOAD64(cs + 4 + 4 * i + j);
    uint64_t *o = out + (size_t)blockIdx.x * BN_OUT;
    rf::bn_permute_rows(st, K, L, reinterpret_cast<uint32_t *>(o + 16));
    rf::bn_permute_rows<false>(bare, K, L, nullptr);
    const unsigned lane = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 4; i++) if (lane == (unsigned)i) { g_store_fr(reinterpret_cast<fr_t *>(o) + i, st[i]); g_store_fr(reinterpret_cast<fr_t *>(o + BN_OUT - 16) + i, bare[i]); }
#endif
}
// in: n_tab, n_case, the constant blocks (KW words each), the cases;  out: BN_OUT words per case
static int run_bn(const std::vector<uint64_t> &in, const uint64_t *din, std::vector<uint64_t> &res, uint64_t *&dout) {
    if (in.size() < 2 || in.size() != 2 + in[0] * KW + in[1] * 20) { printf("case file: unexpected size\n"); return 1; }
    const size_t nt = in[0], nc = in[1];
    for (size_t i = 0; i < nc; i++) if (in[2 + nt * KW + i * 20] >= nt) { printf("case %zu: bad table\n", i); return 1; }
    const FrParams P = fr_params_init(); rf::RowConst rk; rf::rowconst_init(rk, P);
    std::vector<uint32_t> tab9(nt * BK9_N * BK9_W);
    for (size_t t = 0; t < nt; t++) {
        std::vector<fr_t> tab(BK_ALL);
        bn_table_build(*reinterpret_cast<const h2w_poseidon_consts_t *>(&in[2 + t * KW]), P, tab.data());
        bn_table9_build(tab.data(), &tab9[t * BK9_N * BK9_W]);
    }
    uint32_t *dt; rf::RowConst *dk;
    CK(hipMalloc(&dt, tab9.size() * 4 + 16)); CK(hipMemcpy(dt, tab9.data(), tab9.size() * 4, hipMemcpyHostToDevice));
    CK(hipMalloc(&dk, sizeof rk)); CK(hipMemcpy(dk, &rk, sizeof rk, hipMemcpyHostToDevice));
    res.assign(nc * BN_OUT, 0); CK(hipMalloc(&dout, nc * BN_OUT * 8 + 8)); CK(hipMemset(dout, 0xA5, nc * BN_OUT * 8 + 8));
    if (nc) { hipLaunchKernelGGL(k_bn, dim3(nc), dim3(64), 0, 0, dt, dk, din + 2 + nt * KW, dout); RAN("k_bn"); }
    return 0;
}

// ---------------------------------------------------------------------------------------------- (e') QuadSinkT::bn_values, sixteen quads per wavefront, one wavefront per launch record
// record (QL_IN words): table, live quads (bit q), unit_local, 0, state[16][4][4]
//   ->  per quad QQ_FR field elements: ustate [QUAD_UNITS][4], sbx [QUAD_UNITS][56 * 3], st[] behind QUAD_VALUES [4], st[] behind QUAD_VERDICT [4] (lane l stores st[l]).
// A quad that is not live returns before the call.  QUAD_VERDICT gets the same ustate / sbx pointers and must not store through them: its run comes second, and
// the harness stores its st[] itself.
constexpr int QUAD_UNITS = 2, QQ_FR = QUAD_UNITS * 4 + QUAD_UNITS * BN_PARTIAL_ROUNDS * 3 + 4 + 4, QL_IN = 4 + 16 * 16, QL_OUT = 16 * QQ_FR * 4;
__global__ __launch_bounds__(64) __attribute__((flatten)) void k_quad(const uint32_t *tab9s, FrParams P, const uint64_t *recs, uint64_t *out) {
    const uint64_t *rc = recs + (size_t)blockIdx.x * QL_IN;
    const int tab = __builtin_amdgcn_readfirstlane((int)rc[0]), live = __builtin_amdgcn_readfirstlane((int)rc[1]), unit = __builtin_amdgcn_readfirstlane((int)rc[2]);
    stage_bn_consts9(tab9s + (size_t)tab * (BK9_N * BK9_W), threadIdx.x, 64);      // (the barrier inside: before any quad leaves)
    const int q = threadIdx.x >> 2, l = threadIdx.x & 3;
    if (!((live >> q) & 1)) return;
    fr_t *o = reinterpret_cast<fr_t *>(out + (size_t)blockIdx.x * QL_OUT) + (size_t)q * QQ_FR;
    ValCfg cfg; cfg.P = P;
    fr_t in[4], st[4];
#pragma unroll
    for (int i = 0; i < 4; i++) in[i] = g_load_fr(reinterpret_cast<const fr_t *>(rc + 4) + q * 4 + i);
    {
        QuadSinkT<false, QUAD_VALUES> s; s.recs = nullptr; s.nrec = 0; s.out = nullptr; s.cell_off = 0; s.ncells = nullptr; s.l4 = l;
        s.ustate = o; s.sbx = o + QUAD_UNITS * 4; s.unit_local = unit;
#pragma unroll
        for (int i = 0; i < 4; i++) st[i] = in[i];
        s.bn_values(st, cfg);
        g_store_fr(o + QQ_FR - 8 + l, fr_sel(l < 2, fr_sel(l == 0, st[0], st[1]), fr_sel(l == 2, st[2], st[3])));
    }
    {
        QuadSinkT<false, QUAD_VERDICT> s; s.recs = nullptr; s.nrec = 0; s.out = nullptr; s.cell_off = 0; s.ncells = nullptr; s.l4 = l;
        s.ustate = o; s.sbx = o + QUAD_UNITS * 4; s.unit_local = unit;
#pragma unroll
        for (int i = 0; i < 4; i++) st[i] = in[i];
        s.bn_values(st, cfg);
        g_store_fr(o + QQ_FR - 4 + l, fr_sel(l < 2, fr_sel(l == 0, st[0], st[1]), fr_sel(l == 2, st[2], st[3])));
    }
}
// in: n_tab, n_rec, the constant blocks (KW words each), the records;  out: QL_OUT words per record
static int run_quad(const std::vector<uint64_t> &in, const uint64_t *din, std::vector<uint64_t> &res, uint64_t *&dout) {
    if (in.size() < 2 || in.size() != 2 + in[0] * KW + in[1] * QL_IN) { printf("case file: unexpected size\n"); return 1; }
    const size_t nt = in[0], nc = in[1];
    for (size_t i = 0; i < nc; i++) { const uint64_t *rc = &in[2 + nt * KW + i * QL_IN]; if (rc[0] >= nt || rc[1] >> 16 || rc[2] >= (uint64_t)QUAD_UNITS) { printf("record %zu: bad table, quads or unit\n", i); return 1; } }
    const FrParams P = fr_params_init();
    std::vector<uint32_t> tab9(nt * BK9_N * BK9_W);
    for (size_t t = 0; t < nt; t++) {
        std::vector<fr_t> tab(BK_ALL);
        bn_table_build(*reinterpret_cast<const h2w_poseidon_consts_t *>(&in[2 + t * KW]), P, tab.data());
        bn_table9_build(tab.data(), &tab9[t * BK9_N * BK9_W]);
    }
    uint32_t *dt; CK(hipMalloc(&dt, tab9.size() * 4 + 16)); CK(hipMemcpy(dt, tab9.data(), tab9.size() * 4, hipMemcpyHostToDevice));
    res.assign(nc * QL_OUT, 0); CK(hipMalloc(&dout, nc * QL_OUT * 8 + 8)); CK(hipMemset(dout, 0xA5, nc * QL_OUT * 8 + 8));
    if (nc) { hipLaunchKernelGGL(k_quad, dim3(nc), dim3(64), 0, 0, dt, P, din + 2 + nt * KW, dout); RAN("k_quad"); }
    return 0;
}

// ---------------------------------------------------------------------------------------------- (f) the plain C++ per-lane routes, as the device compiler builds them
enum { PL_REDUCE128 = 0, PL_DIVMOD, PL_FRMONT, PL_FR9, PL_MF2, PL_MF3, PL_MF4, PL_MF8, PL_CANON9, PL_OPS };
constexpr int PL_HDR = 16;      // words of the case file's header
// words per case, in and out (fr9: 18 / 9 dwords, padded to whole words)
__host__ __device__ constexpr int pl_in(int op) { return op == PL_REDUCE128 ? 2 : op == PL_DIVMOD ? 3 : op == PL_FRMONT ? 8 : op == PL_FR9 ? 9 : op == PL_MF2 ? 1 : op == PL_MF8 ? 4 : op == PL_CANON9 ? 6 : 2; }
__host__ __device__ constexpr int pl_out(int op) { return op == PL_REDUCE128 ? 1 : op == PL_DIVMOD ? 2 : op == PL_FR9 ? 5 : 4; }
__global__ __launch_bounds__(64) void k_plain(int op, uint64_t ninv, const MontForm *mf, const uint64_t *in, uint64_t *out) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    const uint64_t *c = in + i * pl_in(op); uint64_t *o = out + i * pl_out(op);
    if (op == PL_REDUCE128) o[0] = gl_reduce128(((u128)c[1] << 64) | c[0]);
    else if (op == PL_DIVMOD) { uint64_t q, r; gl_divmod128((u128)c[0] * c[1] + c[2], q, r); o[0] = q; o[1] = r; }
    else if (op == PL_FRMONT) {
        fr_t A, B; for (int j = 0; j < 4; j++) { A.l[j] = c[j]; B.l[j] = c[4 + j]; }
        const fr_t r = fr_mont_mul(A, B, ninv); for (int j = 0; j < 4; j++) o[j] = r.l[j];
    } else if (op == PL_FR9) {
        const uint32_t *d = reinterpret_cast<const uint32_t *>(c); uint32_t *od = reinterpret_cast<uint32_t *>(o);
        fr9_t A, B; for (int j = 0; j < 9; j++) { A.t[j] = d[j]; B.t[j] = d[9 + j]; }
        const fr9_t r = fr9_norm(fr9_mont(A, B, (uint32_t)ninv & rf::M29)); for (int j = 0; j < 9; j++) od[j] = r.t[j];
        od[9] = 0;
    } else if (op == PL_CANON9) {      // the sequence of k_sbox_canon9 (batch.hip) on twelve dwords as the row-cooperative values pass leaves them
        const uint32_t *t = reinterpret_cast<const uint32_t *>(c);
        fr9_t n; uint32_t cy = 0;
        for (int j = 0; j < 8; j++) { const uint32_t x = t[j] + cy; n.t[j] = x & rf::M29; cy = x >> 29; }
        n.t[8] = t[8] + cy;
        fr9_t one9; for (int j = 0; j < 9; j++) one9.t[j] = j == 0 ? 1u : 0u;
        fr_t s = fr9_pack(fr9_mont(n, one9, (uint32_t)ninv & rf::M29));
        if (fr_geq_mod(s)) s = fr_sub_mod_raw(s);
        for (int j = 0; j < 4; j++) o[j] = s.l[j];
    } else {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(c); uint32_t *od = reinterpret_cast<uint32_t *>(o);
        if (op == PL_MF2) mf_convert<2>(w, *mf, od); else if (op == PL_MF3) mf_convert<3>(w, *mf, od); else if (op == PL_MF4) mf_convert<4>(w, *mf, od); else mf_convert<8>(w, *mf, od);
    }
}
// in: n[PL_HDR] (one count per routine, multiples of 64, then zeros), then the cases of every routine: reduce128 {lo, hi} | divmod {a, b, c: a b + c} | fr_mont_mul {A[4], B[4]} | fr9 {A[9], B[9] dwords} |
// mf_convert<2> {w[2] dwords} | <3> {w[3], 0} | <4> {w[4]} | <8> {w[8]} | canon9 {t[12] dwords};  out: r | q, r | [4] | [9] dwords, 0 | [8] dwords each | [4]
static int run_plain(const std::vector<uint64_t> &in, const uint64_t *din, std::vector<uint64_t> &res, uint64_t *&dout) {
    if (in.size() < (size_t)PL_HDR) { printf("short case file\n"); return 1; }
    size_t need = PL_HDR, outw = 0;
    for (int op = 0; op < PL_OPS; op++) { if (in[op] % 64) { printf("whole wavefronts only\n"); return 1; } need += in[op] * pl_in(op); outw += in[op] * pl_out(op); }
    if (in.size() != need) { printf("case file: %zu words, expected %zu\n", in.size(), need); return 1; }
    const FrParams P = fr_params_init(); MontForm K; montform_init(K, 64);
    MontForm *dk; CK(hipMalloc(&dk, sizeof K)); CK(hipMemcpy(dk, &K, sizeof K, hipMemcpyHostToDevice));
    res.assign(outw, 0); CK(hipMalloc(&dout, outw * 8 + 8)); CK(hipMemset(dout, 0xA5, outw * 8 + 8));
    size_t at = PL_HDR, o = 0;
    for (int op = 0; op < PL_OPS; op++) {
        const size_t n = in[op];
        if (n) { hipLaunchKernelGGL(k_plain, dim3(n / 64), dim3(64), 0, 0, op, P.ninv, dk, din + at, dout + o); RAN("k_plain"); }
        at += n * pl_in(op); o += n * pl_out(op);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 4) { printf("usage: devcheck <glq|mds|perm|mont|bn|quad|plain> <case file> <result file>\n"); return 2; }
    std::vector<uint64_t> in;
    {
        FILE *f = fopen(argv[2], "rb"); if (!f) { printf("cannot read %s\n", argv[2]); return 2; }
        fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
        if (bytes < 8 || bytes % 8) { printf("case file: not whole 64-bit words\n"); fclose(f); return 2; }
        in.resize((size_t)bytes / 8);
        const size_t got = fread(in.data(), 8, in.size(), f); fclose(f);
        if (got != in.size()) { printf("short read\n"); return 2; }
    }
    uint64_t *din = nullptr, *dout = nullptr; std::vector<uint64_t> res;
    CK(hipMalloc(&din, in.size() * 8 + 8)); CK(hipMemcpy(din, in.data(), in.size() * 8, hipMemcpyHostToDevice));
    const std::string g = argv[1]; int rc;
    if (g == "glq") rc = run_glq(in, din, res, dout); else if (g == "mds") rc = run_mds(in, din, res, dout); else if (g == "perm") rc = run_perm(in, din, res, dout);
    else if (g == "mont") rc = run_mont(in, din, res, dout); else if (g == "bn") rc = run_bn(in, din, res, dout); else if (g == "quad") rc = run_quad(in, din, res, dout); else if (g == "plain") rc = run_plain(in, din, res, dout);
    else { printf("unknown group %s\n", argv[1]); return 2; }
    if (rc) return rc;
    if (!res.empty()) CK(hipMemcpy(res.data(), dout, res.size() * 8, hipMemcpyDeviceToHost));
    FILE *f = fopen(argv[3], "wb"); if (!f) { printf("cannot write %s\n", argv[3]); return 2; }
    const size_t put = fwrite(res.data(), 8, res.size(), f);
    if (fclose(f) != 0 || put != res.size()) { printf("short write\n"); return 2; }
    printf("%s: %zu words in, %zu words out\n", argv[1], in.size(), res.size());
    return 0;
}
