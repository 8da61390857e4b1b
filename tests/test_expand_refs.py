"""The reference, generators, packer and checker of the record-level expansion tests (tests/expand_ref.py, tests/test_gpu_expandcheck.py), as far as they can
be checked without a GPU: the Python expansion of every template equals the cells the oracle appends for the operation the template stands for, at
lookup_bits 21, 13, 8 and 17, on the edge operands and on random ones; the generated cases hold the operand and geometry classes they claim; the case file
round-trips; the checker reports the four faults of the issue's sensitivity list when they are applied to a copy of the reference; and the harness
cross-compiles for gfx950 together with the product's expand.hip."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import expand_ref as ref

P, R, M64 = ref.P, ref.R, ref.M64
LS = [21, 13, 8, 17]


class Orc:
    """an oracle context and the cells an operation appended"""

    def __init__(self, oracle, L):
        self.O, self.L, self.ctx = oracle, oracle.lib(), oracle.Ctx(L)
        self.p = self.ctx.p

    def wit(self, v): return self.L.orc_load_witness(self.p, self.O.Fr.from_int(v))      # one cell, no range check: an operand load

    def cells(self, n0):
        a = self.ctx.advice_array()[n0:]
        return [sum(int(a[i, j]) << (64 * j) for j in range(4)) for i in range(len(a))]

    def run(self, loads, op):
        """loads: operand values (their cells are excluded); op(handles) appends the cells to compare"""
        hs = [self.wit(v) for v in loads]
        n0 = self.ctx.num_cells()
        op(*hs)
        return self.cells(n0)


def _pairs(L):
    """(a, b, c) operand triples: the Goldilocks-op classes, then random ones on and off the domain"""
    rng = random.Random(500 + L)
    return ref.GLOP_EDGES + [(rng.randrange(P), rng.randrange(P), rng.randrange(P)) for _ in range(40)] + [(rng.randrange(1 << 64), rng.randrange(1 << 64), rng.randrange(1 << 64)) for _ in range(40)]


@pytest.mark.parametrize("L", LS)
def test_reference_equals_the_oracle_for_every_template_with_an_operation(oracle, L):
    o = Orc(oracle, L); lib, p = o.L, o.p
    n = {}
    def same(name, got, t, rec):
        want = ref.expand(t, rec, L)
        assert got == want, "%s L=%d %s: oracle %s\nreference %s" % (name, L, [hex(x) for x in rec], [hex(x) for x in got], [hex(x) for x in want])
        assert len(got) == ref.ncells(t, L)
        n[name] = n.get(name, 0) + 1
    rng = random.Random(600 + L)
    xs = ref.witness_edges(L) + [rng.randrange(P) for _ in range(30)] + [rng.randrange(1 << 64) for _ in range(30)]
    for x in xs:
        n0 = o.ctx.num_cells(); lib.orc_gl_load_witness(p, x)
        same("orc_gl_load_witness -> T_LOADW", o.cells(n0), ref.T_LOADW, (x, 0, 0, 0))
        same("orc_check_less_than_safe(p) -> T_CLT_SAFE", o.run([x], lambda h: lib.orc_check_less_than_safe(p, h, P)), ref.T_CLT_SAFE, (x, 0, 0, 0))
    for a, b, c in _pairs(L):
        same("orc_mul_add -> T_GATE", o.run([a, b, c], lambda ha, hb, hc: lib.orc_mul_add(p, ha, hb, hc)), ref.T_GATE, (a, b, c, 0))
        same("orc_gl_mul_add -> T_GLOP", o.run([a, b, c], lambda ha, hb, hc: lib.orc_gl_mul_add(p, ha, hb, hc)), ref.T_GLOP, (a, b, c, 0))
        same("orc_gl_mul -> T_GLOP", o.run([a, b], lambda ha, hb: lib.orc_gl_mul(p, ha, hb)), ref.T_GLOP, (a, b, 0, 0))
        same("orc_gl_add -> T_GLOP", o.run([a, b], lambda ha, hb: lib.orc_gl_add(p, ha, hb)), ref.T_GLOP, (b, 1, a, 0))            # gate.add: [a, b, 1, a + b]
        # a constant operand, loaded right in front of the operation (its cell is the template's prefix)
        same("orc_gl_load_constant, orc_gl_mul_add -> T_KA_GLOP", o.run([b, c], lambda hb, hc: lib.orc_gl_mul_add(p, lib.orc_gl_load_constant(p, a), hb, hc)), ref.T_KA_GLOP, (a, b, c, 0))
        same("orc_gl_load_constant, orc_gl_mul -> T_KA_GLOP", o.run([b], lambda hb: lib.orc_gl_mul(p, lib.orc_gl_load_constant(p, a), hb)), ref.T_KA_GLOP, (a, b, 0, 0))
        same("orc_gl_load_constant, orc_gl_add -> T_KA_GLOP", o.run([b], lambda hb: lib.orc_gl_add(p, hb, lib.orc_gl_load_constant(p, a))), ref.T_KA_GLOP, (a, 1, b, 0))   # [K] [b, K, 1, b + K]
        if a + b * (P - 1) < 1 << 128:
            got = o.run([a, b], lambda ha, hb: lib.orc_gl_sub(p, ha, hb))                                                             # [p-1] [a, b, p-1, b (p-1) + a], reduce
            same("orc_gl_sub -> T_KB_GLOP", got, ref.T_KB_GLOP, (b, P - 1, a, 0))
            same("orc_gl_sub, its first five cells -> T_KB_GATE", got[:5], ref.T_KB_GATE, (b, P - 1, a, 0))
    for V in ref.REDUCE_EDGES + [rng.randrange(1 << 128) for _ in range(60)]:
        same("orc_gl_reduce -> T_REDUCE", o.run([V], lambda h: lib.orc_gl_reduce(p, h)), ref.T_REDUCE, (V & M64, V >> 64, 0, 0))
    # orc_gl_mul_sub emits mul_no_reduce, sub_no_reduce, reduce: T_GATE, T_KB_GATE (C = the product: a record holds it while it is below 2^64), T_REDUCE
    for a, b, c in [(0, 0, 0), (M64, 1, M64), (1 << 32, (1 << 32) - 1, P - 1), (3, 5, 7)] + [(rng.randrange(1 << 32), rng.randrange(1 << 32), rng.randrange(1 << 64)) for _ in range(30)]:
        got = o.run([a, b, c], lambda ha, hb, hc: lib.orc_gl_mul_sub(p, ha, hb, hc))
        V = c * (P - 1) + a * b
        same("orc_gl_mul_sub -> T_GATE", got[:4], ref.T_GATE, (a, b, 0, 0))
        same("orc_gl_mul_sub -> T_KB_GATE", got[4:9], ref.T_KB_GATE, (c, P - 1, a * b, 0))
        same("orc_gl_mul_sub -> T_REDUCE", got[9:], ref.T_REDUCE, (V & M64, V >> 64, 0, 0))
    # T_CONST1 is a lone load; the oracle has no operation for T_CONST4 (four loads), T_REP12 (twelve loads of one constant) and T_LOADW2 (a pair of loads):
    # they are concatenations of what is pinned above
    for x in (0, M64, 12345):
        n0 = o.ctx.num_cells(); lib.orc_gl_load_constant(p, x)
        same("orc_gl_load_constant -> T_CONST1", o.cells(n0), ref.T_CONST1, (x, 0, 0, 0))
        assert ref.expand(ref.T_REP12, (x, 0, 0, 0), L) == 12 * ref.expand(ref.T_CONST1, (x, 0, 0, 0), L)
        assert ref.expand(ref.T_CONST4, (x, 1, 2, 3), L) == [x, 1, 2, 3]
        assert ref.expand(ref.T_LOADW2, (x, P, 0, 0), L) == ref.expand(ref.T_LOADW, (x, 0, 0, 0), L) + ref.expand(ref.T_LOADW, (P, 0, 0, 0), L)
    assert o.ctx.error() == "", o.ctx.error()
    for name in sorted(n): print("  L=%d %-55s %4d operand sets agree" % (L, name, n[name]))
    o.ctx.close()


def test_montgomery_expectation_and_column_contract():
    assert ref.to_mont(1) == (1 << 256) % R and ref.to_mont(R - 1) == R - ref.to_mont(1) and ref.to_mont(0) == 0
    starts, k = [0, 10, 11, 40], 5
    assert [ref.col_map(i, starts, k) for i in (0, 9, 10, 11, 39, 40, 45)] == [0, 9, 32, 64, 64 + 28, 96, 101]


def _print_counts(cs):
    ops, geo = ref.class_counts(cs)
    print("  %s -> %s: %s | %s" % (cs.name, cs.kernel(), ", ".join("%s %d" % x for x in ops.items()), ", ".join("%s %d" % x for x in geo.items())))
    return ops, geo


@pytest.mark.parametrize("L", [21, 13, 8])
def test_fast_kernel_cases_hold_what_they_claim(L):
    for nrec in ref.STATIC_NREC:
        cs = ref.static_case(L, nrec)
        ops, geo = _print_counts(cs)
        assert cs.kernel() == "expand_fast<%d, false, false>" % L and cs.nproofs in (2, 3) and cs.rec_stride > cs.nrec and cs.cell_stride > cs.flat_end
        if nrec >= 255:      # every operand class, in every long case; the groups of four of both kinds; the own-lane templates
            assert min(ops.values()) >= 1, ops
            assert geo["all_glop_groups"] >= 10 and geo["mixed_groups"] >= 10 and geo["own_lane"] >= 10 and geo["gaps"] >= 30 and geo["templates"] == 12
            have = {(t, r) for p in range(cs.nproofs) for t, r in zip(cs.tmpls, cs.recs[p])}
            for t in range(12):      # the whole edge list of every template (ref.operands puts it first)
                edges = ref.operands(t, L, 0, 0)
                assert all((t, e) in have for e in edges), ref.TNAMES[t]
        assert geo["cells"] <= 400000
    assert {ref.static_case(L, n).tmpls[0] for n in ref.STATIC_NREC} >= {ref.T_LOADW, ref.T_CLT_SAFE, ref.T_CONST1}      # each at flat cell 0 in some case
    assert {n % 16 != 0 for n in ref.STATIC_NREC} == {True, False} and {n % 64 != 0 for n in ref.STATIC_NREC} == {True, False}
    big = ref.static_case(L, 1025)
    have = {(t, r) for p in range(big.nproofs) for t, r in zip(big.tmpls, big.recs[p])}
    for t in range(12):
        assert sum(1 for (tt, r) in have if tt == t) >= (200 if t in ref.GLOPS else 60), ref.TNAMES[t]      # distinct records per template in the static test's largest case (by its share of PATTERN) ...
    for per_cu, nproofs in ref.ROAM_SHAPES:
        cs = ref.roam_case(L, per_cu, nproofs, mont=True)
        ops, geo = _print_counts(cs)
        assert cs.kernel() == "expand_fast_mont<%d, true, false>" % L and geo["units"] >= 16 and geo["cells"] <= 2500000
        have = {(t, r) for p in range(cs.nproofs) for t, r in zip(cs.tmpls, cs.recs[p])}
        if nproofs == 3:      # ... and a few hundred per template (its whole pool: the edge list and 200 random ones) in the roaming test's
            for t in range(12): assert sum(1 for (tt, r) in have if tt == t) >= 200, ref.TNAMES[t]
        else: assert len(have) <= 1000
    cs = ref.column_case(L)
    _print_counts(cs)
    assert cs.kernel() == "expand_fast<%d, false, true>" % L and len(cs.starts) <= 64
    print("  column boundaries: " + ", ".join("%s @ %d" % x for x in cs.bounds.items()))
    assert len(set(cs.bounds.values())) == len(cs.bounds) == 13
    order = sorted(range(cs.nrec), key=lambda i: cs.offs[i])
    for i in order:      # a record crosses at most one boundary
        assert sum(1 for s in cs.starts if cs.offs[i] < s < cs.offs[i] + cs.sizes[cs.tmpls[i]]) <= 1
    gap = cs.bounds["between two records"]
    assert not any(cs.offs[i] <= gap < cs.offs[i] + cs.sizes[cs.tmpls[i]] for i in order)


def test_generic_kernel_cases_hold_what_they_claim():
    for L in (17, 20):
        for nrec in ref.GENERIC_NREC:
            for counter in (0, 1):
                for cols in (0, 1):
                    cs = ref.generic_case(L, nrec, counter, cols, mont=bool(counter ^ cols))
                    assert cs.kernel() == "%s<32, 5, %s>" % ("expand_kernel_mont" if cs.mont else "expand_kernel_t", "true" if cols else "false")
                    assert not cols or 200 <= len(cs.starts) < 1000
            _print_counts(ref.generic_case(L, nrec, 1, 0, False))
    # no work counter: the generic kernel even at a lookup_bits the fast kernel has; more than 64 columns: the same
    assert ref.generic_case(21, 33, 0, 0, False).kernel() == "expand_kernel_t<32, 5, false>"
    assert ref.column_case(21, generic_cols=200).kernel() == "expand_kernel_t<32, 5, true>"
    a, b = ref.shared_layout_cases()
    assert a.offs == b.offs and a.tmpls == b.tmpls and a.recs == b.recs and a.kernel() == "expand_kernel_t<32, 5, false>" and b.kernel() == "expand_fast<21, false, false>"


def test_case_file_round_trips():
    for cs in (ref.static_case(13, 65, mont=True), ref.column_case(8), ref.generic_case(17, 33, 0, 1, True)):
        blob = ref.pack_case(cs)
        assert len(blob) == 8 * (ref.HEADER + len(cs.starts) + cs.nrec + cs.nproofs * cs.rec_stride * 4)
        u = ref.unpack_case(blob)
        for key in ("L", "nproofs", "nrec", "rec_stride", "cell_stride", "grid_x", "roam_per_cu", "counter", "mont", "starts", "k", "tmpls", "offs"):
            assert u[key] == getattr(cs, key), key
        for p in range(cs.nproofs):
            assert [tuple(int(x) for x in r) for r in u["recs"][p, :cs.nrec]] == cs.recs[p]
        want = ref.expected_buffer(cs)
        assert want.shape == (cs.total_cells(), 32) and (want[:ref.GUARD] == ref.SENTINEL).all() and (want[-ref.GUARD:] == ref.SENTINEL).all()
        assert ref.check(cs, want.copy()) == []
        # every record cell of the expectation is where the contract of records.h puts it
        p = cs.nproofs - 1; i = cs.nrec // 2; cells = ref.expand(cs.tmpls[i], cs.recs[p][i], cs.L)
        for s, v in enumerate(cells):
            f = cs.offs[i] + s; d = ref.col_map(f, cs.starts, cs.k) if cs.starts else f
            assert int.from_bytes(want[ref.GUARD + p * cs.cell_stride + d].tobytes(), "little") == (ref.to_mont(v) if cs.mont else v)


def test_checker_reports_the_faults_of_the_sensitivity_list():
    """Each fault of the issue's list, applied to a copy of the reference (expected_buffer(fault=...)) and shown to the checker as if it were the device's
    output.  The case named is the GPU test that catches the same fault in expand.hip."""
    def msgs(cs, fault):
        m = ref.check(cs, ref.expected_buffer(cs, fault))
        print("  %-8s %s: %d cells reported, e.g. %s" % (fault, cs.name, len(m), m[0] if m else "-"))
        return m
    # fast_step_words returning 2 for a three-word step: the Montgomery form of x + 2^RB - p and its kin loses its third word
    for L in (21, 13, 8):
        m = msgs(ref.static_case(L, 257, mont=True), "words2")
        assert m and all("wrong cell" in x for x in m) and any("T_LOADW" in x for x in m)
        assert msgs(ref.static_case(L, 257, mont=False), "words2") == []      # (the canonical stream has no such step)
    # the qhi line removed: V div p >= 2^64 loses its top bit before the reduction mod p
    m = msgs(ref.static_case(21, 257), "no_qhi")
    assert m and all("T_GLOP" in x or "T_KA_GLOP" in x or "T_KB_GLOP" in x or "T_REDUCE" in x for x in m)
    assert any("0xffffffffffffffff 0xffffffffffffffff" in x for x in m)
    # c_lo off by one: the first flush step of a record is not stored
    m = msgs(ref.static_case(13, 65), "c_lo")
    assert m and all("left as sentinel" in x for x in m) and any("slot 0," in x for x in m)
    # the over_b shift dropped: behind a column boundary, cells 8 .. 15 of a step land with the previous column's shift
    cs = ref.column_case(8, mont=True)
    m = msgs(cs, "over_b")
    assert any("left as sentinel" in x for x in m) and any("sentinel overwritten" in x or "wrong cell" in x for x in m)
    # and a store outside every record, into a guard
    want = ref.expected_buffer(cs); want[3] = 0; want[-1] = 7
    m = ref.check(cs, want)
    assert len(m) == 2 and "front guard" in m[0] and "rear guard" in m[1]


def test_expansion_harness_cross_compiles(tmp_path):
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc")
    exe = os.path.join(str(tmp_path), "expandcheck")
    r = subprocess.run(ref.harness_command(exe), capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(exe), r.stdout + r.stderr
