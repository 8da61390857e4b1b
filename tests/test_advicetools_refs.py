"""The references of tests/test_gpu_advicetools.py (tests/advicetools_ref.py) held to the oracle, without a GPU, before they judge a kernel: the gate,
lookup and equality counts against the oracle's MockProver on a valid proof, on random proof words and on streams corrupted in the oracle's own memory;
the two column layouts byte for byte; the digest against the streaming context's.  And the argument checks of the layout entry points that refuse
before any device work."""
import ctypes as C
import random

import numpy as np
import pytest

import advicetools_ref as ref

SHAPE = dict(d=6, q=1, cap=0)      # the smallest streams of the Fibonacci shapes: 1.8 M cells with PoseidonBN254 caps


def _oshape(oracle, mode, lookup_bits=21):
    return oracle.fibonacci_shape(SHAPE["d"], SHAPE["q"], cap_height=SHAPE["cap"], hash_mode=mode, lookup_bits=lookup_bits)


class _Keygen:
    """An oracle keygen context with its lists, and its cells as Python integers kept in step with what is written into the context's own memory."""

    def __init__(self, oracle, osh, ko, proof):
        self.bits = osh.lookup_bits
        self.ctx = oracle.Ctx(self.bits, witness_gen_only=False)
        assert oracle.verify_stark(self.ctx, osh, ko, proof) == 0
        self.n = self.ctx.num_cells()
        self.adv = self.ctx.advice_array()                      # no copy: orc_mock_prover reads what is written here
        self.ints = ref.ints(self.adv)
        self.sel, self.lk, self.eqs, self.ceq = self.ctx.selectors(), self.ctx.lookup_cells(), self.ctx.equalities(), self.ctx.const_equalities()
        self.gates = ref.gate_cells(self.sel, self.n)

    def put(self, cell, v):
        self.adv[cell] = ref.to_limbs(v); self.ints[cell] = v

    def counts(self):
        e, c = ref.bad_equalities(self.ints, self.eqs, [x for x, _ in self.ceq], [v for _, v in self.ceq])
        return ref.bad_gates(self.ints, self.sel, self.n), ref.bad_lookups(self.ints, self.lk, self.bits), e, c

    def oracle_total(self):
        mp = self.ctx.mock_prover()
        assert mp["gates"] == len(self.gates) and mp["lookups"] == len(self.lk) and mp["equalities"] <= len(self.eqs) + len(self.ceq)
        return mp["bad"] + mp["semantic_failed"], mp


def test_counts_equal_the_oracles_mock_prover(oracle, consts):
    """orc_mock_prover reports ONE sum of failed gates, copy constraints, constant equalities and lookups, with the chip-level (semantic) pairs and
    lookups counted apart, and the lists it exports hold both kinds: so the sums are compared.  Zero on the valid proof; the failed semantic checks
    on random words; and on the valid stream with one cell changed at a time in the oracle's own memory, each cell chosen so that only one of the
    four counts can move - which holds every count to the oracle by itself."""
    ko, _ = consts
    osh = _oshape(oracle, 1)
    rng = random.Random(7)
    k = _Keygen(oracle, osh, ko, oracle.synth_proof(osh, 11))
    base = k.counts()
    total, mp = k.oracle_total()
    assert mp["bad"] == 0 and base[0] == 0 and sum(base) == total > 0, (base, mp)
    k.ctx.close()

    k = _Keygen(oracle, osh, ko, oracle.prove_fri(osh, ko, 2024))
    assert k.counts() == (0, 0, 0, 0) and k.oracle_total()[0] == 0
    lk, in_pair, in_const = set(k.lk), {x for ab in k.eqs for x in ab}, {c for c, _ in k.ceq}
    in_gate = {g + t for g in k.gates for t in range(4)}
    alone = [[g + 3 for g in k.gates if g + 3 not in lk and g + 3 not in in_pair and g + 3 not in in_const],
             [c for c in k.lk if c not in in_gate and c not in in_pair and c not in in_const],
             [a for ab in k.eqs for a in ab if a not in in_gate and a not in lk and a not in in_const],
             [c for c in in_const if c not in in_gate and c not in lk and c not in in_pair]]
    print("cells that move one count alone (gates, lookups, pairs, constants):", [len(x) for x in alone])
    moved = [0, 0, 0, 0]
    for which, cands in enumerate(alone):
        if not cands:
            continue
        cell = rng.choice(sorted(cands))
        old = k.ints[cell]
        k.put(cell, (old + (1 << 30)) % ref.R)
        now = k.counts()
        assert sum(now) == k.oracle_total()[0], (which, cell, now)
        assert now[which] >= 1 and all(now[i] == 0 for i in range(4) if i != which), (which, cell, now)
        moved[which] = now[which]
        k.put(cell, old)
    assert moved[0] >= 1 and sum(1 for m in moved if m) >= 3, moved
    # the lookup bound and the limbs.  Every looked-up cell of these streams lies in a gate, so the gates it breaks are known first (a value that
    # leaves the lookup alone) and the lookup's own step is what comes on top: 2^bits - 1 holds, 2^bits and a value with only limb 3 set do not.
    # A pair that differs in limb 3 only is a failed equality.
    for cell in (k.lk[0], k.lk[-1]):
        old = k.ints[cell]
        seen = []
        for v in ((1 << 21) - 1, 1 << 21, 1 << 192):
            if v == old:
                v -= 1
            k.put(cell, v)
            now = k.counts()
            assert sum(now) == k.oracle_total()[0], (cell, hex(v), now)
            seen.append(now)
        k.put(cell, old)
        assert [s[1] for s in seen] == [0, 1, 1] and seen[0][0] == seen[1][0] == seen[2][0] >= 1, (cell, seen)
    cell = sorted(alone[2])[0]
    old = k.ints[cell]
    k.put(cell, old ^ (1 << 200))
    now = k.counts()
    assert sum(now) == k.oracle_total()[0] and now[2] >= 1 and now[0] == now[1] == now[3] == 0, now
    k.put(cell, old)
    # every kind at once, cells that several checks share included
    for cell in (k.gates[0], k.gates[-1] + 3, k.lk[0], k.lk[-1], k.eqs[0][0], k.eqs[-1][1], k.ceq[0][0], k.ceq[-1][0]):
        k.put(cell, (k.ints[cell] + (1 << 40)) % ref.R)
    now = k.counts()
    assert sum(now) == k.oracle_total()[0] and min(now) >= 1, now
    k.ctx.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_layouts_equal_the_oracles_byte_for_byte(oracle, consts, mode):
    ko, _ = consts
    osh = _oshape(oracle, mode)
    ctx = oracle.Ctx(21, witness_gen_only=False)
    assert oracle.verify_stark(ctx, osh, ko, oracle.synth_proof(osh, 5)) == 0
    cells = ctx.advice_array().copy()
    for k, unusable in ((12, 9), (14, 9), (10, 0), (10, 700)):
        if k != 10:
            bp = ctx.break_points(k, unusable)
            assert ref.columns(cells, bp, k).tobytes() == ctx.layout_columns(bp, k), k
        ncols, want = ctx.layout_lookup_columns(k, unusable)
        got = ref.lookup_columns(cells, ctx.lookup_cells(), k, unusable)
        assert got.shape[0] == ncols and got.tobytes() == want, (k, unusable)
    assert len(ctx.break_points(12)) > 4
    ctx.close()


def test_columns_edges_by_hand():
    """What the layout means at the edges the device test uses, on eight cells written out: the boundary cell is repeated, a column may be exactly 2^k long,
    the last column may be the repeated cell alone."""
    cells = ref.pack(range(100, 108))
    v = lambda a: [int(x) for x in a[:, 0]]
    assert v(ref.columns(cells, [], 3)[0]) == list(range(100, 108))
    two = ref.columns(cells, [7], 3)
    assert v(two[0]) == list(range(100, 108)) and v(two[1]) == [107, 0, 0, 0, 0, 0, 0, 0]
    three = ref.columns(cells, [2, 3], 3)
    assert v(three[0]) == [100, 101, 102, 0, 0, 0, 0, 0] and v(three[1]) == [102, 103, 104, 105, 0, 0, 0, 0] and v(three[2]) == [105, 106, 107, 0, 0, 0, 0, 0]


def test_digest_equals_the_oracles_streaming_checksum(oracle, consts):
    ko, _ = consts
    for mode in (1,):
        osh = _oshape(oracle, mode)
        pr = oracle.synth_proof(osh, 9)
        a = oracle.Ctx(21); assert oracle.verify_stark(a, osh, ko, pr) == 0
        b = oracle.Ctx(21, streaming=True); assert oracle.verify_stark(b, osh, ko, pr) == 0
        assert a.num_cells() == b.num_cells()
        assert ref.digest(a.advice_array().copy()) == b.digest()
        a.close(); b.close()
    ones = np.full((3, 4), ref.M64, dtype=np.uint64)
    m = [(((i + 1) * 0x9E3779B97F4A7C15) % 2**64) | 1 for i in range(3)]
    assert ref.digest(ones) == [(-sum(x + 2 * j for x in m)) % 2**64 for j in range(4)]      # (2^64 - 1) w = -w mod 2^64
    assert ref.digest(np.zeros((0, 4), dtype=np.uint64)) == [0, 0, 0, 0]


def test_montgomery_reference():
    assert ref.to_montgomery(0) == 0 and ref.to_montgomery(1) == (1 << 256) % ref.R
    assert (ref.to_montgomery(ref.R - 1) + ref.to_montgomery(1)) % ref.R == 0


def test_pass_sizes_are_the_launch_lines():
    """The device tests place corruptions in the last lane of a first pass and in second passes: the sizes they go by are the unit's launch lines."""
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "halo2-plonky2-verifier_amd", "csrc", "advicetools.hip")).read()
    blocks, threads = ref.launch_blocks(src)
    assert blocks == ref.BLOCKS and threads == {ref.THREADS}
    assert "byte * 8" in src and "(uint64_t)2 << k" in src      # a selector byte a thread in k_check_gates, a half cell in k_layout_columns
    assert (ref.GATE_PASS_CELLS, ref.LOOKUP_PASS, ref.EQUALITY_PASS, ref.COLUMN_PASS_ROWS, ref.DIGEST_PASS, ref.MONTGOMERY_PASS) == (4194304, 262144, 262144, 1 << 19, 524288, 1048576)


# ---- refusals that happen on the host, before any device work (so they can be told from a later failure on a machine without a device)

def test_layout_columns_refuses_break_points_that_wrap(h2w):
    """break_points[c] = 2^64 - 1 made a column of 2^64 cells: its length wrapped to 0, the next column's start to 2^64 - 1, and the check of the column
    after it wrapped again - a source one cell before the buffer.  Refused as break points that do not fit; so are 0 (a column that breaks holds
    two cells at least) and 2^k (longer than a column)."""
    L = h2w.lib()
    fake_in, fake_out = C.c_void_p(0x1000), C.c_void_p(0x2000)      # never dereferenced: the refusal comes first
    for bp, k in (([2**64 - 1, 1], 5), ([3, 2**64 - 1, 1], 5), ([2**64 - 1], 5), ([0], 5), ([1 << 5], 5), ([4, 2**63], 34), ([40], 5), ([31, 31], 5), ([31, 2**64 - 2], 5)):
        arr = (C.c_uint64 * len(bp))(*bp)
        assert L.h2w_layout_columns(fake_in, 40, 40, 1, arr, len(bp), k, fake_out, None) == -1, bp
        assert h2w.last_error() == "h2w_layout_columns: break points do not fit the stream", (bp, h2w.last_error())


def test_lookup_columns_refuse_unusable_rows_that_leave_no_column(h2w, h2w_api, consts):
    """unusable_rows = 2^k made max_rows zero (a division by zero in the size query), more wrapped.  The rule is h2w_break_points': 2^k > unusable_rows + 4."""
    _, kh = consts
    plan = h2w_api.Plan(h2w.fibonacci_shape(5, 1), kh)
    nl = len(plan.lookup_cells())
    assert nl > 0
    for k, unusable in ((10, 1024), (10, 1025), (10, 1020), (10, 2**31 - 1), (3, 4), (3, 8)):
        with pytest.raises(h2w.H2WError, match="h2w_layout_lookup_columns: bad argument"):
            plan.num_lookup_columns(k, unusable)
    n = C.c_uint64()
    assert h2w.lib().h2w_break_points((C.c_uint8 * 2)(), 10, 10, 1020, None, 0, C.byref(n)) != 0      # the same bound there
    assert plan.num_lookup_columns(10, 1019) == (nl + 4) // 5
    assert plan.num_lookup_columns(10, 1000) == (nl + 23) // 24
    assert plan.num_lookup_columns(10, 0) == (nl + 1023) // 1024
    plan.close()
