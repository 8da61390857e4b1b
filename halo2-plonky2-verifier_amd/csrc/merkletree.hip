// merkletree.hip - Merkle trees on the device (include/h2w.h 2e): h2w_merkle_build, h2w_merkle_open and their handle.  plonky2's
// MerkleTree::new(leaves, cap_height) and tree.prove(i) in both hash modes - the producer side of H2W_OP_MERKLE_VERIFY (chiphash.hip, chipvalues.hip):
// an opening row is that op's operand row (chiphash.h operand_layout).  The prover keeps its own builder (prover.hip k_leaves_initial / k_tree_level).
// A tree's work is throughput-bound at its wide levels and latency-bound at its crown, so a level is built in one of two forms:
//   wide    k_mt_leaves    one lane per leaf: hash_or_noop over a leaf of run-time length read from memory (merkletree.h hash_or_noop_words)
//           k_mt_level     one lane per node of ONE level of all trees of the call: proverhash.h two_to_one (one whole permutation per lane)
//   crown   k_mt_crown_gl  one wavefront per node, four levels a launch: a workgroup of four wavefronts owns one node of the launch's top level and
//           k_mt_crown_bn  walks the subtree under it - 8, 4, 2, 1 nodes - bottom-up; a level's hashes go to the tree and, for the next level, to LDS
//                          behind a __syncthreads.  Workgroups meet at kernel boundaries only; nothing waits on global memory.  The permutations are
//                          the wavefront-cooperative ones of the values calls: glp_permute_lanes (glperm.h; hash_mode 0: the state on the lanes of
//                          every 16-lane row) and rf::bn_permute_rows<false> (rowfr.h / rowperm.h; hash_mode 1: the four rows = the four elements)
//   k_mt_check   status 4 of a build: a grid-stride walk over the leaf words, atomicOr into the tree's word
//   k_mt_open    one wavefront per query gathers its row: leaf, index, cap, siblings; its status word is a plain store by lane 0
// Which levels are the crown's: H2W_MERKLE_OPT_CROWN_BITS (merkle_crown_of).  Both forms store the same canonical words: a hash is a permutation's
// output reduced below its modulus, whichever schedule computed it.
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "batchargs.h"
#include "handletabs.h"
#include "merkletree.h"
#define RF_TAB9 s_bn_tab9
#include "rowperm.h"

struct h2w_merkle {
    int mode = 0; uint32_t n_in = 0, depth = 0, cap_height = 0; int device = -1;
    uint64_t crown_opt = H2W_MERKLE_CROWN_AUTO; int small_mds = 0;
    h2w::DevBuf<h2w::ProverConsts> d_k;                                            // the wide kernels: proverhash.h
    h2w::DevBuf<h2w::GlpConsts> d_consts;                                          // the crown, hash_mode 0 (handletabs.h)
    h2w::DevBuf<uint32_t> d_bn_tab9; h2w::DevBuf<h2w::rf::RowConst> d_rowk;        // the crown, hash_mode 1
};

namespace h2w {

constexpr uint64_t MERKLE_MAX_LEAVES = 1ull << 30, MERKLE_MAX_TREES = 65535, MERKLE_MAX_QUERIES = 1ull << 26;
constexpr int CROWN_WAVES = QUAD_WAVES, CROWN_LEVELS = 4, CROWN_BOTTOM = 1 << (CROWN_LEVELS - 1);      // levels a launch, nodes of a workgroup's lowest level
static_assert(CROWN_WAVES == 4 && QUAD_BLOCK == 256, "a crown workgroup is four wavefronts (stage_bn_consts9's block)");
// H2W_MERKLE_CROWN_AUTO: the crown takes the levels of at most 2^b nodes per tree for the largest b with n_trees x 2^b <= this, per hash mode.
// Measured, a call alone on the chip (tools/bench_merkle.py --crossover: depth 12, 16, 20, leaves of 5 and 20 words, 1, 8 and 64 trees, each level count
// against H2W_MERKLE_CROWN_NONE in alternation; profiles/merkle_tree_forms.jsonl): the build time falls with every level the crown takes up
// to n_trees x 2^b = 16,384 (hash_mode 0) / 8,192 (hash_mode 1) and rises beyond it, at every depth and tree count of the sweep that reaches the figure
// (64 trees of depth 12, hash_mode 0, leaves of 5: 0.796 ms at b = 8, 0.847 at b = 9; hash_mode 1, leaves of 20: 10.45 ms at b = 7, 10.71 at b = 8; single
// configurations of long builds land one level either side).  One lane per node, a level is a
// launch as long as ONE permutation on a lone lane (~0.09 ms Goldilocks-Poseidon, ~0.6 ms PoseidonBN254) whatever its width; the crown's wavefronts
// run out of SIMDs at these counts.  0 would mean not measured: no level, AUTO = H2W_MERKLE_CROWN_NONE.
constexpr uint64_t MERKLE_CROWN_MAX_NODES[2] = {16384, 8192};

// what a build of n_trees runs with: 0 .. depth or H2W_MERKLE_CROWN_NONE
static int merkle_crown_of(const h2w_merkle *h, uint64_t n_trees) {
    if (h->crown_opt != H2W_MERKLE_CROWN_AUTO) return (int)h->crown_opt;
    const uint64_t most = MERKLE_CROWN_MAX_NODES[h->mode];
    int b = H2W_MERKLE_CROWN_NONE;
    for (uint32_t i = 0; i <= h->depth; i++) if ((n_trees ? n_trees : 1) <= most >> i) b = (int)i;
    return b;
}

struct MtArgs { const ProverConsts *K; int mode; uint32_t n_in, depth; const uint64_t *leaves; uint64_t *trees; uint64_t n_trees, tree_words; uint32_t *status; };

__global__ __launch_bounds__(256) void k_mt_check(MtArgs A, uint64_t total) {
    const uint64_t per_tree = (uint64_t)A.n_in << A.depth, step = (uint64_t)gridDim.x * 256;
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += step)
        if (g_load_u64(A.leaves + g) >= GL_P) atomicOr(&A.status[g / per_tree], 4u);
}

__device__ __forceinline__ void mt_store_hash(uint64_t *at, const H4 &h) {
    unsigned long long *q = reinterpret_cast<unsigned long long *>(at);
    H2W_GSTORE64(q, h.w[0]); H2W_GSTORE64(q + 1, h.w[1]); H2W_GSTORE64(q + 2, h.w[2]); H2W_GSTORE64(q + 3, h.w[3]);
}
__device__ __forceinline__ H4 mt_load_hash(const uint64_t *at) { H4 h; for (int i = 0; i < 4; i++) h.w[i] = g_load_u64(at + i); return h; }

// g = tree << depth | leaf over the leaves of the call
__global__ __launch_bounds__(64) void k_mt_leaves(MtArgs A) {
    const uint64_t g = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (g >= A.n_trees << A.depth) return;
    const uint64_t t = g >> A.depth, j = g & ((1ull << A.depth) - 1);
    const H4 h = hash_or_noop_words(A.K, A.mode, A.leaves + g * A.n_in, A.n_in);
    mt_store_hash(A.trees + t * A.tree_words + 4 * j, h);
}
// level l >= 1: g = tree << (depth - l) | node
__global__ __launch_bounds__(64) void k_mt_level(MtArgs A, uint32_t l) {
    const uint32_t lb = A.depth - l;
    const uint64_t g = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (g >= A.n_trees << lb) return;
    const uint64_t t = g >> lb, i = g & ((1ull << lb) - 1);
    uint64_t *tree = A.trees + t * A.tree_words;
    const uint64_t *in = tree + mt_level_off(A.depth, l - 1) + 8 * i;
    const H4 h = two_to_one(A.K, A.mode, mt_load_hash(in), mt_load_hash(in + 4));
    mt_store_hash(tree + mt_level_off(A.depth, l) + 4 * i, h);
}

// A launch of the crown: the levels of lb_bottom, lb_bottom - 1, .., lb_bottom - nlev + 1 bits (2^bits nodes per tree; nlev <= CROWN_LEVELS).
// Workgroup b = tree << tb | node of the top level (tb its bits); at step s it owns the 2^(nlev - 1 - s) nodes under that node, wavefront w the nodes
// w, w + 4, ..  A node's children are eight consecutive words: of the level below in the tree (step 0) or of the hand-over buffer (s_mt[(s - 1) & 1]).
struct CrownArgs { uint64_t *trees; uint64_t tree_words; uint32_t depth, lb_bottom, nlev; const h2w_poseidon_consts_t *consts; int small_mds; const uint32_t *bn_tab9; const rf::RowConst *rowk; };
__shared__ uint64_t s_mt[2][CROWN_BOTTOM * 4];

template <class NodeFn> __device__ __forceinline__ void crown_walk(const CrownArgs &A, NodeFn node) {
    const uint32_t tb = A.lb_bottom - (A.nlev - 1), wave = threadIdx.x >> 6;
    const uint64_t t = blockIdx.x >> tb, j = blockIdx.x & ((1u << tb) - 1);
    uint64_t *tree = A.trees + t * A.tree_words;
    for (uint32_t s = 0; s < A.nlev; s++) {
        const uint32_t l = A.depth - (A.lb_bottom - s), cnt = 1u << (A.nlev - 1 - s);
        const uint64_t first = j * cnt;      // the subtree's first node of level l
        const uint64_t *below = tree + mt_level_off(A.depth, l - 1) + 8 * first;
        uint64_t *out = tree + mt_level_off(A.depth, l) + 4 * first;
        for (uint32_t i = wave; i < cnt; i += CROWN_WAVES) node(s == 0 ? below + 8 * i : &s_mt[(s - 1) & 1][8 * i], out + 4 * i, &s_mt[s & 1][4 * i]);
        __syncthreads();      // (every wavefront of the block comes here nlev times: the loop bounds are the block's)
    }
}

// LDS: the Goldilocks-Poseidon constants and derived tables, the hand-over buffer
__global__ __launch_bounds__(QUAD_BLOCK) void k_mt_crown_gl(CrownArgs A) {
    stage_glp_consts<true>(A.consts, threadIdx.x, QUAD_BLOCK);
    lds64_t *const lk = (lds64_t *)s_glp_k, *const lm = (lds64_t *)s_glp_m, *const lx = (lds64_t *)s_glp_x;
    const int lane = threadIdx.x & 63, l15 = lane & 15;
    const bool small = A.small_mds != 0;
    crown_walk(A, [&](const uint64_t *children, uint64_t *out, uint64_t *hand) {
        uint64_t x = l15 < 8 ? children[l15] : 0;      // (left, right, 0^4) on the lanes of every 16-lane row
        x = glp_permute_lanes(x, lk, lm, lx, lane, small);
        if (lane < 4) { H2W_GSTORE64(reinterpret_cast<unsigned long long *>(out + lane), x); hand[lane] = x; }
    });
}
// LDS: the nine-limb tables, the hand-over buffer
__global__ __launch_bounds__(QUAD_BLOCK) void k_mt_crown_bn(CrownArgs A) {
    stage_bn_consts9(A.bn_tab9, threadIdx.x, QUAD_BLOCK);
    const int lane = threadIdx.x & 63;
    const rf::RowConst K = load_row_consts(A.rowk);
    const rf::LaneK L = rf::lane_consts();
    crown_walk(A, [&](const uint64_t *children, uint64_t *out, uint64_t *hand) {
        fr_t st[4]; st[0] = fr_zero(); st[1] = fr_zero();      // (0, 0, left, right): the same on every lane
        for (int i = 0; i < 4; i++) { st[2].l[i] = children[i]; st[3].l[i] = children[4 + i]; }
        rf::bn_permute_rows<false>(st, K, L, nullptr);
        if (lane == 0) for (int i = 0; i < 4; i++) { H2W_GSTORE64(reinterpret_cast<unsigned long long *>(out + i), st[0].l[i]); hand[i] = st[0].l[i]; }
    });
}

struct OpenArgs { const uint64_t *leaves, *trees, *queries; uint64_t n_trees, tree_words; uint32_t n_in, depth, cap_height, nw; uint64_t *out; uint32_t *status; };
__global__ __launch_bounds__(64) void k_mt_open(OpenArgs A) {
    const uint64_t i = blockIdx.x, t = g_load_u64(A.queries + 2 * i), idx = g_load_u64(A.queries + 2 * i + 1);
    const bool bad = t >= A.n_trees || (idx >> A.depth) != 0;
    if (threadIdx.x == 0) A.status[i] = bad ? 4u : 0u;
    if (bad) return;      // (nothing is read through the query's indices)
    const uint64_t *leaf = A.leaves + ((t << A.depth) + idx) * A.n_in, *tree = A.trees + t * A.tree_words;
    const uint32_t cap_words = 4u << A.cap_height;
    const uint64_t cap_off = mt_level_off(A.depth, A.depth - A.cap_height);
    unsigned long long *row = reinterpret_cast<unsigned long long *>(A.out + i * (uint64_t)A.nw);
    for (uint32_t w = threadIdx.x; w < A.nw; w += 64) {
        uint64_t v;
        if (w < A.n_in) v = g_load_u64(leaf + w);
        else if (w == A.n_in) v = idx;
        else if (w - A.n_in - 1 < cap_words) v = g_load_u64(tree + cap_off + (w - A.n_in - 1));
        else {
            const uint32_t u = w - A.n_in - 1 - cap_words, lv = u >> 2;      // sibling lv: node (index >> lv) ^ 1 of level lv
            v = g_load_u64(tree + mt_level_off(A.depth, lv) + 4 * ((idx >> lv) ^ 1) + (u & 3));
        }
        H2W_GSTORE64(row + w, v);
    }
}

static inline unsigned blocks_of(uint64_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

static int merkle_build(h2w_merkle *h, const uint64_t *leaves_dev, uint64_t n_trees, uint64_t *trees_dev, uint32_t *status_dev, hipStream_t stream) {
    DeviceGuard dg(h->device);
    const uint32_t depth = h->depth, cap = h->cap_height;
    MtArgs A; A.K = h->d_k.get(); A.mode = h->mode; A.n_in = h->n_in; A.depth = depth; A.leaves = leaves_dev; A.trees = trees_dev; A.n_trees = n_trees;
    A.tree_words = mt_tree_words(depth, cap); A.status = status_dev;
    H2W_HIP(hipMemsetAsync(status_dev, 0, n_trees * sizeof(uint32_t), stream));
    const uint64_t words = (n_trees << depth) * h->n_in, check_blocks = (words + 255) / 256;
    hipLaunchKernelGGL(k_mt_check, dim3((unsigned)(check_blocks < 65536 ? check_blocks : 65536)), dim3(256), 0, stream, A, words);
    hipLaunchKernelGGL(k_mt_leaves, dim3(blocks_of(n_trees << depth, 64)), dim3(64), 0, stream, A);
    // the levels of cap .. hb bits are the crown's (none: hb < cap), those above them one lane per node
    const int crown = merkle_crown_of(h, n_trees);
    int hb = crown == H2W_MERKLE_CROWN_NONE ? -1 : crown < (int)depth - 1 ? crown : (int)depth - 1;
    if (hb < (int)cap) hb = (int)cap - 1;
    for (uint32_t l = 1; (int)(depth - l) > hb && l <= depth - cap; l++) hipLaunchKernelGGL(k_mt_level, dim3(blocks_of(n_trees << (depth - l), 64)), dim3(64), 0, stream, A, l);
    CrownArgs C; C.trees = trees_dev; C.tree_words = A.tree_words; C.depth = depth; C.consts = h->d_consts.get(); C.small_mds = h->small_mds; C.bn_tab9 = h->d_bn_tab9.get(); C.rowk = h->d_rowk.get();
    for (int lb = hb; lb >= (int)cap;) {
        const int nlev = lb - (int)cap + 1 < CROWN_LEVELS ? lb - (int)cap + 1 : CROWN_LEVELS;
        C.lb_bottom = (uint32_t)lb; C.nlev = (uint32_t)nlev;
        const dim3 grid((unsigned)(n_trees << (lb - nlev + 1)));
        if (h->mode == 0) hipLaunchKernelGGL(k_mt_crown_gl, grid, dim3(QUAD_BLOCK), 0, stream, C);
        else hipLaunchKernelGGL(k_mt_crown_bn, grid, dim3(QUAD_BLOCK), 0, stream, C);
        lb -= nlev;
    }
    H2W_HIP(hipGetLastError());
    return 0;
}

}  // namespace h2w

using namespace h2w;

extern "C" {

h2w_merkle *h2w_merkle_new(const h2w_poseidon_consts_t *consts, int hash_mode, uint32_t n_in, uint32_t depth, uint32_t cap_height, int device_id) {
    auto refuse = [](const char *why) -> h2w_merkle * { set_error(std::string("h2w_merkle_new: ") + why); return nullptr; };
    if (!consts) return refuse("null argument");
    if (hash_mode != 0 && hash_mode != 1) return refuse("hash_mode is 0 (Goldilocks-Poseidon) or 1 (PoseidonBN254)");
    if (n_in < 1 || n_in > H2W_CHIPBATCH_MAX_N_IN) return refuse("n_in outside [1, H2W_CHIPBATCH_MAX_N_IN]");
    if (depth < 1 || depth > MERKLE_MAX_DEPTH) return refuse("depth outside [1, 24]");
    if (cap_height > depth || cap_height > MERKLE_MAX_CAP) return refuse("cap_height above min(depth, 6)");
    h2w_merkle *h = new h2w_merkle;
    h->mode = hash_mode; h->n_in = n_in; h->depth = depth; h->cap_height = cap_height; h->small_mds = glp_small_mds(*consts) ? 1 : 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { h->device = -1; return h; }      // layout queries still work; h2w_merkle_build / _open fail
    if (device_id < 0 || device_id >= ndev) { delete h; return refuse("device_id out of range"); }
    h->device = device_id;
    DeviceGuard dg(device_id);
    const FrParams P = fr_params_init();
    std::vector<ProverConsts> k(1); prover_consts_init(k[0], *consts);
    rf::RowConst rk; rf::rowconst_init(rk, P);
    DevBuf<fr_t> tab;      // (upload_bn_tab's canonical table: the crown reads the limb-form copy alone)
    if (h->d_k.upload(k) != 0 || (hash_mode == 1 ? (upload_bn_tab(tab, *consts, P, &h->d_bn_tab9) != 0 || h->d_rowk.upload(&rk, 1) != 0) : upload_glp_consts(h->d_consts, *consts) != 0)) {
        const std::string why = g_last_error;
        delete h; set_error("h2w_merkle_new: " + why);
        return nullptr;
    }
    return h;
}

void h2w_merkle_free(h2w_merkle *h) {
    if (!h) return;
    DeviceGuard dg(h->device);
    delete h;
}

uint64_t h2w_merkle_tree_words(const h2w_merkle *h) {
    if (!h) { set_error("h2w_merkle_tree_words: null argument"); return 0; }
    return mt_tree_words(h->depth, h->cap_height);
}

int h2w_merkle_layout(const h2w_merkle *h, uint64_t *out, size_t n_out) {
    if (!h) { set_error("h2w_merkle_layout: null argument"); return -1; }
    const uint32_t n_levels = h->depth - h->cap_height + 1;
    const int n = (int)n_levels + 3;
    if (!out) return n;
    if (n_out < (size_t)n) { set_error("h2w_merkle_layout: out holds fewer than n_levels + 3 words"); return -1; }
    out[0] = n_levels;
    for (uint32_t l = 0; l < n_levels; l++) out[1 + l] = mt_level_off(h->depth, l);
    out[1 + n_levels] = mt_level_off(h->depth, n_levels - 1);
    out[2 + n_levels] = mt_row_words(h->n_in, h->depth, h->cap_height);
    return n;
}

int h2w_merkle_configure(h2w_merkle *h, int option, uint64_t value) {
    if (!h) { set_error("h2w_merkle_configure: null argument"); return -1; }
    if (option != H2W_MERKLE_OPT_CROWN_BITS) { set_error("h2w_merkle_configure: unknown option"); return -1; }
    if (value > h->depth && value != H2W_MERKLE_CROWN_NONE && value != H2W_MERKLE_CROWN_AUTO) {
        set_error("h2w_merkle_configure: H2W_MERKLE_OPT_CROWN_BITS is 0 .. depth, H2W_MERKLE_CROWN_NONE or H2W_MERKLE_CROWN_AUTO"); return -1;
    }
    h->crown_opt = value;
    return 0;
}

int h2w_merkle_crown_bits(const h2w_merkle *h, uint64_t n_trees) {
    if (!h) { set_error("h2w_merkle_crown_bits: null argument"); return -1; }
    return merkle_crown_of(h, n_trees);
}

int h2w_merkle_build(h2w_merkle *h, const uint64_t *leaves_dev, uint64_t n_trees, uint64_t *trees_dev, uint32_t *status_dev, void *stream) {
    if (!h) { set_error("h2w_merkle_build: null handle"); return -1; }
    if (n_trees > MERKLE_MAX_TREES || n_trees << h->depth > MERKLE_MAX_LEAVES) { set_error("h2w_merkle_build: batch too large (more than 2^30 leaves or 65,535 trees); split the batch"); return -1; }
    if (h->device < 0) { set_error("h2w_merkle_build: no HIP device - the tree kernels only run on the GPU (no CPU fallback)"); return -1; }
    if (n_trees == 0) return 0;
    if (!leaves_dev || !trees_dev || !status_dev) { set_error("h2w_merkle_build: null buffer"); return -1; }
    return merkle_build(h, leaves_dev, n_trees, trees_dev, status_dev, (hipStream_t)stream);
}

int h2w_merkle_open(h2w_merkle *h, const uint64_t *leaves_dev, const uint64_t *trees_dev, uint64_t n_trees, const uint64_t *queries_dev, uint64_t n,
                    uint64_t *operands_dev, uint32_t *status_dev, void *stream) {
    if (!h) { set_error("h2w_merkle_open: null handle"); return -1; }
    if (n_trees > MERKLE_MAX_TREES || n_trees << h->depth > MERKLE_MAX_LEAVES || n > MERKLE_MAX_QUERIES) {
        set_error("h2w_merkle_open: batch too large (more than 2^30 leaves, 65,535 trees or 2^26 queries); split the batch"); return -1;
    }
    if (h->device < 0) { set_error("h2w_merkle_open: no HIP device - the gather kernel only runs on the GPU (no CPU fallback)"); return -1; }
    if (n == 0) return 0;
    if (!queries_dev || !operands_dev || !status_dev || (n_trees != 0 && (!leaves_dev || !trees_dev))) { set_error("h2w_merkle_open: null buffer"); return -1; }
    DeviceGuard dg(h->device);
    OpenArgs A; A.leaves = leaves_dev; A.trees = trees_dev; A.queries = queries_dev; A.n_trees = n_trees; A.tree_words = mt_tree_words(h->depth, h->cap_height);
    A.n_in = h->n_in; A.depth = h->depth; A.cap_height = h->cap_height; A.nw = mt_row_words(h->n_in, h->depth, h->cap_height); A.out = operands_dev; A.status = status_dev;
    hipLaunchKernelGGL(k_mt_open, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, A);
    H2W_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
