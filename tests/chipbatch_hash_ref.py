"""What tests/test_chipbatch_hash_layout.py and tests/test_gpu_chipbatch_hash.py share: the cases of the batched hash / Merkle chip ops
(include/h2w.h 2c, ops 9-13), their operand layout, and the oracle's run of ONE instance - a fresh context, the operands loaded the way
the verifier's WitnessChip loads them, then the op."""
import ctypes as C
import random

P = 2**64 - 2**32 + 1
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617

GL_PERMUTE, BN_PERMUTE, HASH_NO_PAD, TWO_TO_ONE, MERKLE_VERIFY = 9, 10, 11, 12, 13
MAX_N_IN = 4096

# (op, hash_mode, n_in, depth, cap_height): every parameter set the GPU tests run
HASH_N_IN = {0: (1, 8, 9, 20), 1: (1, 3, 9, 10, 20)}       # mode 0: one absorb, exactly the rate, one word into the second, the reference's 20; mode 1: nine words per permutation
MERKLE_SHAPES = ((20, 3, 1), (3, 3, 0), (4, 2, 2), (5, 1, 0), (20, 3, 2))
PARAMS = [(GL_PERMUTE, 0, 0, 0, 0), (BN_PERMUTE, 0, 0, 0, 0)]
PARAMS += [(HASH_NO_PAD, m, n, 0, 0) for m in (0, 1) for n in HASH_N_IN[m]]
PARAMS += [(TWO_TO_ONE, m, 0, 0, 0) for m in (0, 1)]
PARAMS += [(MERKLE_VERIFY, m, n, d, c) for m in (0, 1) for (n, d, c) in MERKLE_SHAPES]


def family(op, mode):
    """1: the PoseidonBN254 kernels run the op, 0: the Goldilocks-Poseidon ones."""
    return 0 if op == GL_PERMUTE else 1 if op == BN_PERMUTE else mode


def operand_kinds(op, mode, n_in, depth, cap_height):
    """The operand words of an instance as a list of ('gl' | 'idx' | 'hash') items; a hash is four words."""
    if op == GL_PERMUTE:
        return ["gl"] * 12
    if op == BN_PERMUTE:
        return ["hash"] * 4
    if op == HASH_NO_PAD:
        return ["gl"] * n_in
    if op == TWO_TO_ONE:
        return ["hash"] * 2
    return ["gl"] * n_in + ["idx"] + ["hash"] * ((1 << cap_height) + depth - cap_height)


def num_operands(op, mode, n_in, depth, cap_height):
    return sum(4 if k == "hash" else 1 for k in operand_kinds(op, mode, n_in, depth, cap_height))


def random_items(rnd, op, mode, n_in, depth, cap_height, fill=None, index=None):
    """One instance's operands as items (a Goldilocks word, the index, or a hash: 4 Goldilocks words / one Fr as an integer).
    fill: 'zero' | 'max' (p - 1, r - 1) instead of random values; index: the leaf index (random otherwise)."""
    fr = family(op, mode) == 1
    out = []
    for k in operand_kinds(op, mode, n_in, depth, cap_height):
        if k == "gl":
            out.append(0 if fill == "zero" else P - 1 if fill == "max" else rnd.randrange(P))
        elif k == "idx":
            out.append(index if index is not None else 0 if fill == "zero" else (1 << depth) - 1 if fill == "max" else rnd.randrange(1 << depth))
        elif fr:
            out.append(0 if fill == "zero" else R - 1 if fill == "max" else rnd.randrange(R))
        else:
            out.append([0 if fill == "zero" else P - 1 if fill == "max" else rnd.randrange(P) for _ in range(4)])
    return out


def words_of(op, mode, n_in, depth, cap_height, items):
    """items -> words, hashes of the PoseidonBN254 family always as four little-endian words (also a small Fr)."""
    fr = family(op, mode) == 1
    w = []
    for k, it in zip(operand_kinds(op, mode, n_in, depth, cap_height), items):
        if k == "hash" and fr:
            w += [(it >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
        elif k == "hash":
            w += it
        else:
            w.append(it)
    return w


def oracle_instance(oracle, ko, lookup_bits, op, mode, n_in, depth, cap_height, items):
    """Runs the op on a fresh oracle context.  Returns (ctx, out): out = the op's output wires (permutations: the state; hashes: the hash
    wires; MERKLE_VERIFY: none).  The caller closes ctx."""
    OL = oracle.lib(); ctx = oracle.Ctx(lookup_bits); AV = oracle.AV
    kinds = operand_kinds(op, mode, n_in, depth, cap_height)
    fr = family(op, mode) == 1
    hw = 1 if fr else 4

    def load_hash(it):      # HasherChip::load_witness: four CONSTANTS (poseidon/hash.rs:86-96) / one native witness (poseidon_bn254/hash.rs:89-98)
        if fr:
            return [OL.orc_load_witness(ctx.p, oracle.Fr.from_int(it))]
        return [OL.orc_gl_load_constant(ctx.p, x) for x in it]

    def hash4(wires):       # the oracle's hash argument: 4 wires, the Fr wire in [0]
        a = (AV * 4)()
        for i, w in enumerate(wires):
            a[i] = w
        return a

    if op == GL_PERMUTE:
        st = (AV * 12)(*[OL.orc_gl_load_witness(ctx.p, x) for x in items]); out = (AV * 12)()
        OL.orc_gl_poseidon_permute(ctx.p, C.byref(ko), st, out)
        return ctx, list(out)
    if op == BN_PERMUTE:
        st = (AV * 4)(*[OL.orc_load_witness(ctx.p, oracle.Fr.from_int(x)) for x in items]); out = (AV * 4)()
        OL.orc_bn_poseidon_permute(ctx.p, C.byref(ko), st, out)
        return ctx, list(out)
    if op == HASH_NO_PAD:
        pre = (AV * n_in)(*[OL.orc_gl_load_witness(ctx.p, x) for x in items]); out = (AV * 4)()
        OL.orc_hash_no_pad(ctx.p, C.byref(ko), mode, pre, n_in, out)
        return ctx, list(out)[:hw]
    if op == TWO_TO_ONE:
        l = hash4(load_hash(items[0])); r = hash4(load_hash(items[1])); out = (AV * 4)()
        OL.orc_two_to_one(ctx.p, C.byref(ko), mode, l, r, out)
        return ctx, list(out)[:hw]
    n_cap, n_sib = 1 << cap_height, depth - cap_height
    leaf = (AV * n_in)(*[OL.orc_gl_load_witness(ctx.p, x) for x in items[:n_in]])
    idx = OL.orc_gl_load_witness(ctx.p, items[n_in])
    bits = (AV * depth)()
    OL.orc_num_to_bits(ctx.p, idx, depth, bits)
    cap = [w for it in items[n_in + 1:n_in + 1 + n_cap] for w in load_hash(it)]
    sib = [w for it in items[n_in + 1 + n_cap:] for w in load_hash(it)]
    assert len(kinds) == n_in + 1 + n_cap + n_sib
    top = (AV * max(cap_height, 1))(*list(bits)[n_sib:])
    cap_index = OL.orc_bits_to_num(ctx.p, top, cap_height)
    OL.orc_merkle_verify(ctx.p, C.byref(ko), mode, leaf, n_in, bits, depth, cap_index, (AV * len(cap))(*cap), n_cap,
                         (AV * len(sib))(*sib) if sib else None, n_sib)
    return ctx, []


def case_seed(op, mode, n_in, depth, cap_height, extra=0):
    return random.Random(1000003 * op + 10007 * mode + 101 * n_in + 13 * depth + cap_height + 7919 * extra)
