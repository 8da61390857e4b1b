// chiphash.h - what the two units of the batched hash and Merkle chip ops share (include/h2w.h 2c, ops 9-13): chiphash.hip runs an op for its cells
// (h2w_chipbatch_run), chipvalues.hip for its results and verdicts (h2w_chipbatch_values).  The op's parameters and operand layout, the one program
// both run (hash_program), the handle's part of either (ChipHash) and the status check's argument block.
#pragma once
#include "batchargs.h"
#include "chipbatch.h"

namespace h2w {

struct HashParams { int op, mode; uint32_t n_in, depth, cap_height; };

// operand words of an instance and what the status check makes of them: [n_gl Goldilocks words][the leaf index, if has_idx][n_hash hashes x 4 words]
struct OperandLayout { uint32_t nw, n_gl, has_idx, n_hash, fr_hashes; };
inline OperandLayout operand_layout(const HashParams &hp) {
    OperandLayout o{0, 0, 0, 0, hp.mode == 1 ? 1u : 0u};
    switch (hp.op) {
        case H2W_OP_GL_PERMUTE: o.n_gl = SPONGE_WIDTH; break;
        case H2W_OP_BN_PERMUTE: o.n_hash = BN_WIDTH; o.fr_hashes = 1; break;
        case H2W_OP_HASH_NO_PAD: o.n_gl = hp.n_in; break;
        case H2W_OP_TWO_TO_ONE: o.n_hash = 2; break;
        default: o.n_gl = hp.n_in; o.has_idx = 1; o.n_hash = (1u << hp.cap_height) + (hp.depth - hp.cap_height); break;
    }
    o.nw = o.n_gl + o.has_idx + 4 * o.n_hash;
    return o;
}

// operand words as wires: on the value backends a wire IS its value, so a loaded operand is read again where the op uses it
struct WordView { const uint64_t *w; HF uint64_t operator[](int i) const { return g_load_u64(w + i); } };
template <class B> HF HashW<B> hash_words(int mode, const uint64_t *w) {
    HashW<B> h; h.f = fr_zero();
    for (int i = 0; i < 4; i++) { const uint64_t x = g_load_u64(w + i); h.e[i] = mode == 0 ? x : 0; if (mode != 0) h.f.l[i] = x; }
    return h;
}
// the op's output wires, handed to the caller of hash_program: gl(v, n) n Goldilocks wires, fr(v, n) n native wires (permutations: the state;
// hashes: the hash wires, by the hash mode; MERKLE_VERIFY: none).  The runs that are after the cells take nothing: NoHashOut
struct NoHashOut {
    template <class W> HF void gl(const W *, int) const {}
    template <class W> HF void fr(const W *, int) const {}
};
// FAM: the ops a backend is instantiated for - 0: Goldilocks-Poseidon (GL_PERMUTE, hash_mode 0), 1: PoseidonBN254 (BN_PERMUTE, hash_mode 1), -1: all (host)
template <int FAM, class B, class Out> HF void hash_program(B &be, const HashParams &hp, const h2w_poseidon_consts_t *k, const uint64_t *w, const Out &out) {
    typedef typename B::Gl Gl; typedef typename B::Bool Bool; typedef typename B::Fr Fr; typedef HashW<B> H;
    GoldilocksChip<B> gl(be);
    if (hp.op == H2W_OP_GL_PERMUTE) {
        if constexpr (FAM != 1) {
            PoseidonPermutationChip<B> pg(be, k); Gl st[SPONGE_WIDTH];
            for (int i = 0; i < SPONGE_WIDTH; i++) st[i] = gl.load_witness(g_load_u64(w + i));
            pg.permute(st);
            out.gl(st, SPONGE_WIDTH);
        }
        return;
    }
    if (hp.op == H2W_OP_BN_PERMUTE) {
        if constexpr (FAM != 0) {
            PoseidonBN254PermutationChip<B> pb(be, k); Fr st[BN_WIDTH];
            for (int i = 0; i < BN_WIDTH; i++) st[i] = be.fr_witness(hash_words<B>(1, w + 4 * i).f);      // NativeChip::load_witness
            pb.permute(st);
            out.fr(st, BN_WIDTH);
        }
        return;
    }
    const int mode = hp.mode;
    auto load_hash = [&](const uint64_t *p) { uint64_t t[4]; for (int i = 0; i < 4; i++) t[i] = g_load_u64(p + i); HasherChip<B> hs(be, mode, k); return hs.load_witness(t); };
    auto hand_out = [&](const HasherChip<B> &hs, const H &h) { if (hs.md() == 0) out.gl(h.e, NUM_HASH_OUT_ELTS); else out.fr(&h.f, 1); };
    if (hp.op == H2W_OP_HASH_NO_PAD) {
        const WordView in{w};
        for (uint32_t i = 0; i < hp.n_in; i++) gl.load_witness(in[(int)i]);
        HasherChip<B> hs(be, mode, k); const H h = hs.hash_no_pad(in, (int)hp.n_in);
        hand_out(hs, h);
        return;
    }
    if (hp.op == H2W_OP_TWO_TO_ONE) {
        const H l = load_hash(w), r = load_hash(w + 4);
        HasherChip<B> hs(be, mode, k); const H h = hs.two_to_one(l, r);
        hand_out(hs, h);
        return;
    }
    // MERKLE_VERIFY: leaf, index -> bits, cap, siblings, cap_index, the path
    const int depth = (int)hp.depth, ch = (int)hp.cap_height, n_cap = 1 << ch, n_sib = depth - ch;
    const WordView leaf{w}; const uint64_t *cap0 = w + hp.n_in + 1, *sib0 = cap0 + 4 * n_cap;
    for (uint32_t i = 0; i < hp.n_in; i++) gl.load_witness(leaf[(int)i]);
    const Gl idx = gl.load_witness(g_load_u64(w + hp.n_in));
    Bool bits[32]; gl.num_to_bits(idx, depth, bits);
    for (int i = 0; i < n_cap; i++) load_hash(cap0 + 4 * i);
    for (int i = 0; i < n_sib; i++) load_hash(sib0 + 4 * i);
    const Gl cap_index = gl.bits_to_num(bits + n_sib, ch);
    MerkleTreeChip<B> mk(be, mode, k);
    mk.verify_proof_to_cap_with_cap_index(leaf, (int)hp.n_in, bits, depth, cap_index, n_cap,
                                          [&](int i) { return hash_words<B>(mode, cap0 + 4 * i); }, n_sib, [&](int i) { return hash_words<B>(mode, sib0 + 4 * i); });
}

HF ValCfg chiphash_cfg(int mode, int L, const FrParams &P, const fr_t *inv, bool split_bn) {
    ValCfg cfg; cfg.fri = nullptr; cfg.proof = nullptr; cfg.mode = mode; cfg.L = L; cfg.P = P; cfg.inv_pos = inv; cfg.inv_neg = inv + INV_TAB; cfg.st = nullptr; cfg.split = false; cfg.split_bn = split_bn;
    cfg.load_items = nullptr; cfg.n_load_items = 0; cfg.load_nrec = cfg.load_ncell = 0; cfg.n_cap_items = 0;
    return cfg;
}

// status 4 (k_chiphash_check, chiphash.hip): one lane per (instance, item) - a Goldilocks word, the leaf index, a hash (four Goldilocks words or one Fr).
// Instance i's word is status[i * stride], zeroed by the caller: 1 for the status array of h2w_chipbatch_run, 2 for the verdicts of h2w_chipbatch_values
struct CheckArgs { const uint64_t *operands; OperandLayout o; uint32_t depth; uint64_t n; uint32_t *status; uint32_t stride; };
void chiphash_launch_check(const CheckArgs &K, hipStream_t stream);      // chiphash.hip

struct ChipHash {
    HashParams hp; OperandLayout o; bool bn; uint32_t nglp = 0; int small_mds = 0; uint64_t chunk = 0;      // chunk 0: by CHIPHASH_WS_BYTES
    DevBuf<GlpConsts> d_consts; DevBuf<fr_t> d_bn_tab, d_inv;
    DevBuf<uint32_t> d_bn_tab9; DevBuf<rf::RowConst> d_rowk;      // PoseidonBN254: the limb-form tables and the row form's constants (chipvalues.hip)
};

}  // namespace h2w
