"""h2w_trace_verdict_batch on the device (include/h2w.h 2d, csrc/traceverdict.hip): per-proof verdicts of a TRACED plan, from the assert_equal calls
the trace recorded.

Verifier traces: the batch of tests/verdict_ref.py (the valid proof, one corrupted word per check, a random proof, a status-4 proof, the valid proof
again; the layout from the compiled plan of the shape).  Every proof's first three words equal the oracle's expectation, all four equal the compiled
plan's h2w_fri_verdict_batch, and status equals h2w_plan_status after a witness call of the traced plan on the same buffer.

Hand-driven programs (tests/replay_prog.py's backend interface, with eq / site added): the expectation is an integer model - every eq whose sides
differ counts, ORs the site word in force and names the depth-1 instance it lies in; a range check follows RangeChip::range_check (a value beyond
its bits: the flag; beyond its ceil(bits / lookup_bits) limbs, with more than one limb: + 1, the copy constraint on the limb sum).
check_less_than_safe(a, p): the oracle's keygen run of orc_check_less_than_safe breaks no constraint at p - 1 and exactly one copy constraint (the
limb sum of a + 2^rb - p) at p, p + 1 and 2^64 - 1, at lookup_bits 8, 13 and 21: a >= p counts + 1 and raises the flag."""
import ctypes as C

import numpy as np
import pytest

import replay_prog as RP
import verdict_ref as R

pytestmark = pytest.mark.gpu

NO = 0xFFFFFFFF
RANGE = 1
P = RP.P
FUSE = {"unfused": None, "fuse_gl": (True, False), "fuse_gl_bn": (True, True)}


def _traced(h2w_api, sh, kh, words, fuse=None):
    c = h2w_api.Context(sh.lookup_bits, True, 0); c.trace_begin()
    h2w_api.verify_stark(c, sh, kh, np.asarray(words, dtype=np.uint64))
    kw = {} if fuse is None else dict(fuse_consts=kh, fuse_gl=fuse[0], fuse_bn=fuse[1])
    plan = h2w_api.Plan.from_trace(c, len(words), **kw); c.close()
    return plan


def _upload(words):
    import torch
    return torch.from_numpy(np.concatenate([np.asarray(w, dtype=np.uint64) for w in words]).view(np.int64)).cuda()


def _ws(plan, n):
    import torch
    return torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda:0")


def _witness_status(plan, d, n, ws=None):
    import torch
    advice = torch.empty(n * plan.num_cells * 32, dtype=torch.uint8, device="cuda:0")
    ws = _ws(plan, n) if ws is None else ws
    plan.run(d.data_ptr(), n, advice.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return plan.status(ws.data_ptr(), n), advice


_BATCHES = {}


def _batch(h2w, h2w_api, oracle, consts, mode, name):
    """(shapes, the batch of verdict_ref.build_batch, the compiled plan's verdicts): computed once per shape, shared by the fuse-flag cases"""
    if (mode, name) not in _BATCHES:
        _BATCHES[(mode, name)] = _make_batch(h2w, h2w_api, oracle, consts, mode, name)
    return _BATCHES[(mode, name)]


def _make_batch(h2w, h2w_api, oracle, consts, mode, name):
    ko, kh = consts
    (db, nq, rb, ch), over = {"one_fold_step": ((6, 2, 1, 2), {}), "three_steps": ((8, 2, 2, 2), dict(arity_bits=2, final_poly_bits=3))}[name]
    sh, osh = R.shape_pair(h2w, oracle, mode, db, nq, rb, ch, **over)
    cplan = h2w_api.Plan(sh, kh)
    names, words, want, noncanonical, siblings = R.build_batch(osh, ko, cplan.proof_layout())
    d = _upload(words)      # (held until the call has run)
    compiled = cplan.verdict(d.data_ptr(), len(words))
    cplan.close()
    return sh, osh, names, words, want, noncanonical, compiled


CASES = [("one_fold_step", 1, f) for f in FUSE] + [("one_fold_step", 0, "unfused"), ("three_steps", 1, "unfused")]


@pytest.mark.parametrize("name,mode,fuse", CASES)
def test_verifier_trace_verdicts_are_the_oracles_and_the_compiled_plans(h2w, h2w_api, oracle, consts, name, mode, fuse):
    sh, osh, names, words, want, noncanonical, compiled = _batch(h2w, h2w_api, oracle, consts, mode, name)
    n = len(words)
    plan = _traced(h2w_api, sh, consts[1], np.frombuffer(bytes(oracle.synth_proof(osh, 43)), dtype=np.uint64), FUSE[fuse])
    info = plan.trace_verdict_info()
    assert info["available"] == 1 and info["recorded"] == info["equalities"] and info["range_sites"] == 1, info
    d = _upload(words); ws = _ws(plan, n)
    got = plan.trace_verdict(d.data_ptr(), n, ws.data_ptr())
    status, _ = _witness_status(plan, d, n)
    for i, nm in enumerate(names):
        print(f"{i:2d} {nm:45s} oracle {want[i]} traced {got[i]} compiled {compiled[i]} witness status {status[i]}")
    assert want[0] == want[-1] == (0, 0, NO)
    assert [g[:3] for g in got] == want
    assert got == compiled
    assert [g[3] for g in got] == status
    for i in noncanonical:
        assert status[i] == 4
    plan.close()


def test_65_units_a_second_wavefront_of_table_lanes_and_of_quiet_lanes(h2w, h2w_api, oracle, consts):
    """5 proofs x 13 queries, PoseidonBN254 caps: unit 64 is the first quiet lane of the query template's second wavefront and of the table lanes'; its
    proof, the last, has a sibling of its LAST query changed.  Nothing counts twice."""
    ko, kh = consts
    sh, osh = R.shape_pair(h2w, oracle, 1, 6, 13, 1, 2)
    cplan = h2w_api.Plan(sh, kh); L = cplan.proof_layout()
    valid = np.frombuffer(bytes(oracle.prove_fri(osh, ko, 77)), dtype=np.uint64)
    rand = np.frombuffer(bytes(oracle.synth_proof(osh, 5)), dtype=np.uint64)
    smap = R.semantic_map(osh, *R.oracle_run(osh, ko, rand))
    words = [valid, R.bump(valid, R.sibling_word(L, 7, L["oracles"][1], 2)), rand, valid, R.bump(valid, R.sibling_word(L, 12, L["steps"][0], 0) + 2)]
    want = R.expected_many(osh, ko, words, smap)
    assert want[1] == (R.MERKLE_PERM_Z, 1, 7) and want[4] == (R.MERKLE_STEP, 1, 12) and want[2][1] >= 13 * len(R.site_flags(osh))
    d = _upload(words)
    compiled = cplan.verdict(d.data_ptr(), 5); cplan.close()
    plan = _traced(h2w_api, sh, kh, np.frombuffer(bytes(oracle.synth_proof(osh, 43)), dtype=np.uint64))
    ws = _ws(plan, 5)
    got = plan.trace_verdict(d.data_ptr(), 5, ws.data_ptr())
    print(want, got)
    assert [g[:3] for g in got] == want and got == compiled
    assert [g[3] for g in got] == _witness_status(plan, d, 5)[0]
    plan.close()


# ---------------------------------------------------------------- hand-driven programs
class VTrace(RP.TraceBackend):
    def eq(self, a, b):
        assert self.lib.h2w_constrain_equal(self.ctx.p, C.byref(a), C.byref(b)) == 0

    def site(self, w): self.ctx.trace_site(w)


class VInt(RP.IntBackend):
    """The integer model of a verdict: (flags, n_failed, first_query) beside IntBackend's status."""

    def __init__(self, words, L, units=("inst", "outer")):
        super().__init__(words)
        self.L, self.units, self.cur_site, self.flags, self.n_failed, self.first = L, units, 0, 0, 0, NO
        self.stack, self.next_unit = [], 0

    def push(self, name):
        unit = None
        if name in self.units and not any(u is not None for u in self.stack):
            unit = self.next_unit; self.next_unit += 1
        self.stack.append(unit)

    def pop(self): self.stack.pop()
    def site(self, w): self.cur_site = w

    def eq(self, a, b):
        if a != b:
            self.n_failed += 1; self.flags |= self.cur_site
            unit = next((u for u in self.stack if u is not None), None)
            if unit is not None:
                self.first = min(self.first, unit)

    def range_check(self, a, bits):
        n = (bits + self.L - 1) // self.L
        if a >> bits:
            self.flags |= self.cur_site | RANGE
        if n > 1 and a >> (n * self.L):
            self.n_failed += 1

    def check_less_than_safe(self, a, bound):
        if a >= bound:      # (the oracle: one copy constraint, the limb sum of a + 2^rb - bound; module docstring)
            self.flags |= self.cur_site | RANGE; self.n_failed += 1

    def gl_div(self, a, b):      # GoldilocksChip::div's own assert_equal(a, b * res)
        res = super().gl_div(a, b)
        self.eq(a % P, b * res % P)
        return res

    def ext_inv(self, a):        # assert_equal(a * inverse, one), component by component
        inv = super().ext_inv(a)
        pr = RP._ext_mul(a, inv)
        self.eq(pr[0], 1); self.eq(pr[1], 0)
        return inv

    def verdict(self):
        return (self.flags, self.n_failed, self.first, self.status())


def _run_program(h2w, h2w_api, prog, proof_a, proofs, L=13, scopes=("inst", "outer", "inner")):
    """prog traced on proof A, lowered, judged on `proofs` in one batch: every proof's four words against the integer model; status against
    h2w_plan_status after a witness call of the plan on the same buffer."""
    tb = VTrace(h2w, h2w_api, proof_a, L)
    try:
        prog(tb)
        plan = h2w_api.Plan.from_trace(tb.ctx, len(proof_a), parallel_scopes=tuple(scopes))
    finally:
        tb.ctx.close()
    info = plan.trace_verdict_info()
    assert info["available"] == 1, info
    n = len(proofs); d = _upload(proofs)
    ws = _ws(plan, n)
    got = plan.trace_verdict(d.data_ptr(), n, ws.data_ptr())
    want = []
    for p in proofs:
        ib = VInt(p, L); prog(ib); want.append(ib.verdict())
    status, _ = _witness_status(plan, d, n)
    plan.close()
    print(want, got, status)
    assert got == want
    assert [g[3] for g in got] == status
    return got


def test_a_goldilocks_result_against_a_proof_word(h2w, h2w_api):
    def prog(b):
        x, y, w = b.gl_in(0), b.gl_in(1), b.gl_in(2)
        b.site(0x10); b.eq(b.gl_mul(x, y), w)
    mk = lambda x, y, d: [x, y, (x * y + d) % P]
    got = _run_program(h2w, h2w_api, prog, mk(5, 7, 0), [mk(3, P - 1, 0), mk(3, P - 1, 1), mk(2**63, 2**32, 0), mk(0, 9, P - 1)])
    assert [g[:3] for g in got] == [(0, 0, NO), (0x10, 1, NO), (0, 0, NO), (0x10, 1, NO)]


def test_widths_literals_and_site_words(h2w, h2w_api):
    """Two Fr values that differ in word 3 only; a one-word value against a four-word one with equal low words; a 64-bit and a wide literal operand;
    site words 0, 1 << 31 and two different words failing in one proof (their OR)."""
    LIT, WIDE = 0x123456789, 2**200 + 5

    def prog(b):
        h0, h1, n, h2, x, h3 = b.hash_in(0), b.hash_in(4), b.nat_in(8), b.hash_in(9), b.nat_in(13), b.hash_in(14)
        b.eq(h0, h1)                                       # site 0: counted, no flag
        b.site(1 << 31); b.eq(n, h2)
        b.site(0x2); b.eq(x, b.const(LIT))
        b.site(0x4); b.eq(h3, b.const(WIDE))

    def mk(h0, h1, n, h2, x, h3):
        return RP.fr_words(h0) + RP.fr_words(h1) + [n] + RP.fr_words(h2) + [x] + RP.fr_words(h3)
    v = 2**192 * 3 + 2**64 * 5 + 9
    ok = mk(v, v, 77, 77, LIT, WIDE)
    got = _run_program(h2w, h2w_api, prog, ok, [ok, mk(v, v + 2**192, 77, 77, LIT, WIDE), mk(v, v, 77, 77 + 2**192, LIT, WIDE), mk(v, v, 77, 77 + 2**64, LIT + 1, WIDE + 2**128),
                                                mk(1, 1, 2**64 - 1, 2**64 - 1, LIT, WIDE)])
    assert [g[:3] for g in got] == [(0, 0, NO), (0, 1, NO), (1 << 31, 1, NO), ((1 << 31) | 6, 3, NO), (0, 0, NO)]


@pytest.mark.parametrize("dist", [255, 256, 257])
def test_an_operand_far_behind_comes_from_the_value_store(h2w, h2w_api, dist):
    def prog(b):
        v = b.nat_in(0)                     # two slots: the value and the fetched proof word
        for _ in range((dist - 2) // 2):
            bit = b.nat_in(1)
        if (dist - 2) % 2:
            bit = b.select(bit, bit, bit)
        w = b.nat_in(2)
        b.site(0x8); b.eq(v, w); b.eq(bit, w)
    got = _run_program(h2w, h2w_api, prog, [6, 1, 6], [[9, 1, 9], [9, 1, 8], [1, 1, 1], [2**64 - 1, 0, 2**64 - 1]])
    assert [g[:3] for g in got] == [(0x8, 1, NO), (0x8, 2, NO), (0, 0, NO), (0x8, 1, NO)]


@pytest.mark.parametrize("ninst", [1, 64, 65])
def test_the_failing_instance_names_its_unit(h2w, h2w_api, ninst):
    """ninst instances of a parallel scope, each comparing its own word with a root value (an import at depth 1): the failure in the LAST instance only."""
    def prog(b):
        x = b.gl_in(0)
        for k in range(ninst):
            with b.scope("inst"):
                a = b.gl_in(1 + k); b.site(0x40); b.eq(b.gl_mul(a, a), b.gl_mul(x, x))
    mk = lambda x, bad: [x] + [x if k != bad else x + 1 for k in range(ninst)]
    got = _run_program(h2w, h2w_api, prog, mk(5, -1), [mk(7, -1), mk(11, ninst - 1), mk(13, -1), mk(2, 0)])
    assert [g[:3] for g in got] == [(0, 0, NO), (0x40, 1, ninst - 1), (0, 0, NO), (0x40, 1, 0)]


def test_depth_2_imports_and_the_root_behind_the_scopes(h2w, h2w_api):
    """At depth 2: a root value against the instance's own word (an import across two levels), and a four-word root value against a four-word value of
    the enclosing depth-1 instance (imports from depth 0 and depth 1) - the unit is the enclosing depth-1 instance; then an equality in the root
    behind the scopes (no unit).  words: 0 x, 1.. h, per outer instance k from 5 + 6 k: its hash (4 words), its two inner words; 17 the root's last word."""
    def prog(b):
        x, h = b.gl_in(0), b.hash_in(1)
        for k in range(2):
            with b.scope("outer"):
                o4 = b.hash_in(5 + 6 * k)
                for j in range(2):
                    with b.scope("inner"):
                        i = b.gl_in(9 + 6 * k + j)
                        b.site(0x100); b.eq(i, x)
                        b.site(0x200); b.eq(h, o4)
        b.site(0x400); b.eq(x, b.gl_in(17))
    H = 2**250 + 2**130 + 17

    def mk(x, inner, outer, last):
        p = [x] + RP.fr_words(H) + [0] * 13
        for k in range(2):
            p[5 + 6 * k:9 + 6 * k] = RP.fr_words(outer[k]); p[9 + 6 * k], p[10 + 6 * k] = inner[2 * k], inner[2 * k + 1]
        p[17] = last
        return p
    got = _run_program(h2w, h2w_api, prog, mk(5, [5] * 4, [H, H], 5),
                       [mk(9, [9] * 4, [H, H], 9), mk(9, [9, 9, 9, 8], [H, H], 9), mk(9, [9] * 4, [H + 2**192, H], 9), mk(9, [9] * 4, [H, H], 10)])
    assert [g[:3] for g in got] == [(0, 0, NO), (0x100, 1, 1), (0x200, 2, 0), (0x400, 1, NO)]


def test_the_root_alone_fails(h2w, h2w_api):
    def prog(b):
        x = b.gl_in(0)
        for k in range(3):
            with b.scope("inst"):
                a = b.gl_in(1 + k); b.site(0x40); b.eq(a, x)
        b.site(0x400); b.eq(x, b.gl_in(4))
    got = _run_program(h2w, h2w_api, prog, [5] * 5, [[9, 9, 9, 9, 9], [9, 9, 9, 9, 8], [9, 9, 8, 9, 8]])
    assert [g[:3] for g in got] == [(0, 0, NO), (0x400, 1, NO), (0x440, 2, 1)]


@pytest.mark.parametrize("L", [13, 21])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_range_sites(h2w, h2w_api, L, which):
    bits = (L - 1, L, 2 * L + 1)[which]; n = (bits + L - 1) // L

    def prog(b):
        b.site(0x20); b.range_check(b.nat_in(0), bits)
    vals = [2**bits - 1, 2**bits, 2**(n * L) - 1, 2**(n * L)]
    got = _run_program(h2w, h2w_api, prog, [1], [[v] for v in vals], L=L)
    want = [(0, 0, NO)] + [((0x21, 1 if (n > 1 and v >> (n * L)) else 0, NO) if v >> bits else (0, 0, NO)) for v in vals[1:]]
    assert [g[:3] for g in got] == want


def test_check_less_than_safe(h2w, h2w_api):
    def prog(b):
        b.site(0x20); b.check_less_than_safe(b.nat_in(0), P)
    got = _run_program(h2w, h2w_api, prog, [1], [[P - 1], [P], [2**64 - 1], [0]])
    assert got == [(0, 0, NO, 0), (0x21, 1, NO, 4), (0x21, 1, NO, 4), (0, 0, NO, 0)]      # (a word >= p is outside its field as well: status 4)


def test_status_1_and_2_beside_a_failing_equality(h2w, h2w_api):
    def prog(b):
        x, dv, e, w = b.gl_in(0), b.gl_in(1), [b.gl_in(2), b.gl_in(3)], b.gl_in(4)
        b.site(0x2); b.gl_div(x, dv)
        b.site(0x4); b.ext_inv(e)
        b.site(0x8); b.eq(x, w)
    got = _run_program(h2w, h2w_api, prog, [5, 3, 1, 2, 5], [[7, 3, 1, 2, 7], [7, 0, 1, 2, 8], [7, 3, 0, 0, 8], [7, 0, 0, 0, 7], [0, 0, 4, 5, 0]])
    # a zero divisor: status 1, and the hint's own check a == b * res fails unless a is zero; a zero extension element: status 2, and component 0 of
    # a * inverse == one fails
    assert got == [(0, 0, NO, 0), (0xA, 2, NO, 1), (0xC, 2, NO, 2), (0x6, 2, NO, 1), (0, 0, NO, 1)]


def test_status_5_of_the_off_domain_select_batch_is_the_witness_calls(h2w, h2w_api):
    """The batch of tests/replay_prog.py's off_select (selectors above 1 on either side of a zero divisor): the verdict call runs the same interpreter on
    values only, and its status word is h2w_plan_status after a witness call on the same buffer - 0, 1 or 5 as the integer model says, per proof."""
    prog = next(p for p in RP.PROGRAMS if p.name == "off_select")
    proofs = prog.batch(130); n = len(proofs)
    tb = VTrace(h2w, h2w_api, prog.proof_a(), prog.lookup_bits)
    try:
        prog.fn(tb)
        plan = h2w_api.Plan.from_trace(tb.ctx, prog.nwords)
    finally:
        tb.ctx.close()
    assert plan.trace_verdict_info()["available"] == 1
    d = _upload(proofs); ws = _ws(plan, n)
    got = plan.trace_verdict(d.data_ptr(), n, ws.data_ptr())
    status, _ = _witness_status(plan, d, n)
    plan.close()
    want = [RP.int_run(prog.fn, p)[1].status() for p in proofs]
    print(want, [g[3] for g in got], status)
    assert set(want) == {0, 1, 5} and want == [prog.off.expected_status(i) for i in range(n)]
    assert [g[3] for g in got] == want and status == want


# ---------------------------------------------------------------- the call among others
def test_the_call_among_witness_calls_on_one_workspace(h2w, h2w_api, oracle, consts):
    """verdict, sharded witness calls (world 2, both ranks), verdict again on one plan and one workspace: equal verdicts, shard streams byte-equal to
    those of a plan that never ran a verdict; an unsharded witness call behind a verdict call gives the oracle's stream."""
    import torch
    ko, kh = consts
    sh, osh = R.shape_pair(h2w, oracle, 1, 6, 2, 1, 2)
    valid = np.frombuffer(bytes(oracle.prove_fri(osh, ko, 77)), dtype=np.uint64)
    rand = np.frombuffer(bytes(oracle.synth_proof(osh, 5)), dtype=np.uint64)
    words = [valid, rand, R.bump(valid, 3)]; n = len(words); d = _upload(words)
    tr_words = np.frombuffer(bytes(oracle.synth_proof(osh, 43)), dtype=np.uint64)
    plan, fresh = _traced(h2w_api, sh, kh, tr_words), _traced(h2w_api, sh, kh, tr_words)
    st = torch.cuda.current_stream().cuda_stream
    ws = _ws(plan, n); ws2 = _ws(fresh, n)
    first = plan.trace_verdict(d.data_ptr(), n, ws.data_ptr())
    assert first[0] == (0, 0, NO, 0) and first[1][1] > 0 and first[2][1] > 0
    for rank in (0, 1):
        a = torch.zeros(n * plan.num_cells * 32, dtype=torch.uint8, device="cuda:0"); b = torch.zeros_like(a)
        plan.run_shard(d.data_ptr(), n, a.data_ptr(), ws.data_ptr(), rank, 2, st)
        fresh.run_shard(d.data_ptr(), n, b.data_ptr(), ws2.data_ptr(), rank, 2, st)
        torch.cuda.synchronize()
        assert torch.equal(a, b), f"rank {rank}: the shard stream changed behind a verdict call"
        assert plan.trace_verdict(d.data_ptr(), n, ws.data_ptr()) == first
    status, advice = _witness_status(plan, d, n, ws)
    assert status == [g[3] for g in first]
    got = advice.cpu().numpy().reshape(n, -1)
    for i, w in enumerate(words):
        ctx = oracle.Ctx(sh.lookup_bits)
        assert oracle.verify_stark(ctx, osh, ko, (C.c_uint64 * len(w))(*[int(x) for x in w])) == 0
        assert got[i].tobytes() == ctx.advice_bytes(), f"proof {i}: the stream behind a verdict call is not the oracle's"
        ctx.close()
    plan.close(); fresh.close()


def test_no_proof(h2w, h2w_api, oracle, consts):
    import torch
    sh, osh = R.shape_pair(h2w, oracle, 1, 6, 2, 1, 2)
    plan = _traced(h2w_api, sh, consts[1], np.frombuffer(bytes(oracle.synth_proof(osh, 43)), dtype=np.uint64))
    assert plan.trace_verdict(0, 0, 0) == []
    out = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    assert plan.trace_verdict(0, 0, 0, verdict_ptr=out.data_ptr()) is None      # (nothing is read or written)
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [0x5A5A5A5A] * 4
    with pytest.raises(h2w_api.H2WError, match="null buffer"):
        plan.trace_verdict(0, 1, 0, verdict_ptr=out.data_ptr())
    cplan = h2w_api.Plan(sh, consts[1])
    with pytest.raises(h2w_api.H2WError, match="h2w_fri_verdict_batch"):
        cplan.trace_verdict(out.data_ptr(), 1, out.data_ptr(), verdict_ptr=out.data_ptr())
    plan.close(); cplan.close()


def _hip_current_device():
    """hipGetDevice of the one HIP runtime this process holds (the one libh2w.so is bound to)."""
    paths = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    assert len(paths) == 1, paths
    dev = C.c_int(-1)
    assert C.CDLL(paths[0]).hipGetDevice(C.byref(dev)) == 0
    return dev.value


def test_the_callers_device_stays_current(h2w, h2w_api, oracle, consts):
    import torch
    ko, kh = consts
    sh, osh = R.shape_pair(h2w, oracle, 1, 6, 2, 1, 2)
    valid = np.frombuffer(bytes(oracle.prove_fri(osh, ko, 77)), dtype=np.uint64)
    rand = np.frombuffer(bytes(oracle.synth_proof(osh, 5)), dtype=np.uint64)
    words = [valid, rand, valid]
    plan = _traced(h2w_api, sh, kh, rand)
    d = _upload(words).to("cuda:0"); ws = _ws(plan, 3)
    out = torch.zeros(12, dtype=torch.int32, device="cuda:0")
    cur = torch.cuda.device_count() - 1
    torch.cuda.set_device(cur)
    try:
        assert _hip_current_device() == cur
        plan.trace_verdict(d.data_ptr(), 3, ws.data_ptr(), 0, verdict_ptr=out.data_ptr())
        assert _hip_current_device() == cur
        torch.cuda.synchronize(0)
        w = out.cpu().tolist()
        assert w[0:2] == [0, 0] and w[8:12] == w[0:4] and w[5] > 0
    finally:
        torch.cuda.set_device(0)
    plan.close()
