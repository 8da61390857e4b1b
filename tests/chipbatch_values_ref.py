"""What h2w_chipbatch_values (include/h2w.h 2c, csrc/chipvalues.hip) must store for an instance, from the CPU oracle alone - shared by
tests/test_chipbatch_values_host.py and tests/test_gpu_chipbatch_values.py.

The oracle runs the instance on a KEYGEN context (witness_gen_only=False), which records every copy constraint.  The constraints of the op's own
wiring hold for any operands inside their fields, so a pair of ctx.equalities() whose two cells differ is one of the chips' assert_equal calls -
the root check of MERKLE_VERIFY - and their number is the verdict's n_failed (tests/verdict_ref.py derives a proof's the same way).  The result
words are the op's output wires: a Goldilocks wire is one word, a native wire four little-endian words.
"""
import numpy as np

import chipbatch_hash_ref as ref
from chipbatch_hash_ref import BN_PERMUTE, GL_PERMUTE, HASH_NO_PAD, MERKLE_VERIFY, TWO_TO_ONE

NUM_RESULTS = {GL_PERMUTE: 12, BN_PERMUTE: 16, HASH_NO_PAD: 4, TWO_TO_ONE: 4, MERKLE_VERIFY: 0}
FORM_AUTO, FORM_QUAD, FORM_ROW = 0, 1, 2
MASK64 = 0xFFFFFFFFFFFFFFFF


def forms_of(op, mode):
    """The forms the op's hash admits, AUTO aside: the PoseidonBN254 family has two kernels."""
    return (FORM_QUAD, FORM_ROW) if ref.family(op, mode) == 1 else (FORM_QUAD,)


class _Keygen:
    """pyoracle as ref.oracle_instance uses it, its contexts keygen ones."""

    def __init__(self, oracle):
        self.o, self.AV, self.Fr = oracle, oracle.AV, oracle.Fr

    def lib(self):
        return self.o.lib()

    def Ctx(self, lookup_bits):
        return self.o.Ctx(lookup_bits, witness_gen_only=False)


def result_words(op, mode, out):
    """The op's output wires -> the instance's result words."""
    vals = [o.v.to_int() for o in out]
    if ref.family(op, mode) == 0:
        assert all(v < ref.P for v in vals)
        return vals
    assert all(v < ref.R for v in vals)
    return [(v >> (64 * i)) & MASK64 for v in vals for i in range(4)]


def oracle_values(oracle, ko, lookup_bits, params, items, want_cells=False):
    """One keygen run of the instance: (result words, failing pairs as [((cell, value), (cell, value)), ..] in program order) and, with want_cells,
    the output wires' cell offsets and the advice bytes (the witness call's cells)."""
    ctx, out = ref.oracle_instance(_Keygen(oracle), ko, lookup_bits, *params, items)
    try:
        assert not ctx.error(), ctx.error()
        adv = ctx.advice_array()
        val = lambda c: sum(int(adv[c][j]) << (64 * j) for j in range(4))
        n_eq = int(ctx.L.orc_num_equalities(ctx.p))      # (ctx.equalities(), without a Python tuple per pair: tests/verdict_ref.py)
        eq = np.zeros(max(2 * n_eq, 1), dtype=np.uint64)
        ctx.L.orc_equalities(ctx.p, eq.ctypes.data)
        eq = eq[:2 * n_eq].astype(np.int64).reshape(-1, 2)
        differ = eq[(adv[eq[:, 0]] != adv[eq[:, 1]]).any(axis=1)].tolist()
        failing = sorted((((a, val(a)), (b, val(b))) for a, b in differ), key=lambda p: max(p[0][0], p[1][0]))
        words = result_words(params[0], params[1], out)
        assert len(words) == NUM_RESULTS[params[0]]
        if want_cells:
            return words, failing, [int(o.cell) for o in out], ctx.advice_bytes()
        return words, failing
    finally:
        ctx.close()


def expected(oracle, ko, lookup_bits, params, items):
    """(result words, n_failed) of one instance."""
    words, failing = oracle_values(oracle, ko, lookup_bits, params, items)
    return words, len(failing)


def cap_slot(params, items):
    """The item index of the cap entry the leaf index selects."""
    op, mode, n_in, depth, cap = params
    return n_in + 1 + (items[n_in] >> (depth - cap))


def computed_node(oracle, ko, lookup_bits, params, items):
    """The cap-level node the path computes, as a hash item (four Goldilocks words / one Fr): read off the failing root pairs of a run whose cap
    entry differs from it in every word - of a pair, the side that is not the selected cap entry's word."""
    op, mode, n_in, depth, cap = params
    assert op == MERKLE_VERIFY
    _, failing = oracle_values(oracle, ko, lookup_bits, params, items)
    entry = items[cap_slot(params, items)]
    root = [entry] if mode == 1 else list(entry)
    assert len(failing) == len(root), (len(failing), "a random cap entry fails every word of the root check")
    node = []
    for (a, b), r in zip(failing, root):
        sides = [v for _, v in (a, b) if v != r]
        assert len(sides) == 1, (a, b, r)
        node.append(sides[0])
    return node[0] if mode == 1 else node


def valid_merkle(oracle, ko, lookup_bits, params, rnd, index=None):
    """A valid opening: random operands, the computed node put into the cap entry the index selects; a second run must fail nothing."""
    items = ref.random_items(rnd, *params, index=index)
    items[cap_slot(params, items)] = computed_node(oracle, ko, lookup_bits, params, items)
    _, failing = oracle_values(oracle, ko, lookup_bits, params, items)
    assert failing == [], failing
    return items


def bump_item(params, items, at, word=0):
    """A copy of the instance with item `at` + 1 in its field (a hash: its word `word`)."""
    op, mode, n_in, depth, cap = params
    out = [list(x) if isinstance(x, list) else x for x in items]
    kind = ref.operand_kinds(*params)[at]
    if kind == "gl":
        out[at] = (out[at] + 1) % ref.P
    elif kind == "hash" and mode == 1:
        out[at] = (out[at] + 1) % ref.R
    elif kind == "hash":
        out[at][word] = (out[at][word] + 1) % ref.P
    else:
        raise ValueError("the index is not bumped")
    return out


def invalid_row(params, items):
    """The instance with one operand outside its field: a Goldilocks word = p, an Fr = r, a Goldilocks hash word = p, the leaf index = 2^depth."""
    op, mode, n_in, depth, cap = params
    bad = [list(x) if isinstance(x, list) else x for x in items]
    if op in (GL_PERMUTE, HASH_NO_PAD):
        bad[len(bad) // 2] = ref.P
    elif op == BN_PERMUTE or (op == TWO_TO_ONE and mode == 1):
        bad[-1] = ref.R
    elif op == TWO_TO_ONE:
        bad[0] = [1, 2, ref.P, 3]
    else:
        bad[n_in] = 1 << depth
    return bad
