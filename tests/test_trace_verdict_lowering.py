"""The verdict stage of the traced-plan lowering (include/h2w.h 2d: h2w_trace_site, h2w_plan_trace_verdict_info), without a device.

A trace of verify_stark keeps every chip-level assert_equal of the run beside its tape and lowers all of them.  Their number is reconciled from two
sides that do not read the recorded list: the protocol's checks - the semantic pairs tests/verdict_ref.py's semantic_map enumerates on a uniformly
random proof's oracle run, num_queries x len(site_flags) - plus the never-failing hint checks, one per GoldilocksChip::div (the assert_equal inside
h2w_gl_div) and two per extension inverse (the caller's assert_equal of a * inverse against one, component by component).  The hint sites are counted
on the TAPE: a plan lowered from the same run with no parallel scope is one segment, so its op counts are the run's - DOP_LOADW_DIV ops (one per
division) + DOP_LOADW_EXTINV ops (two per inverse).  One range site: the PoW response's.
Recording changes no witness plan: a hand-driven program traced with its equalities and sites, and traced again on a backend whose eq / site do
nothing, lowers to plans with equal sizes, op counts and workspaces."""
import ctypes as C

import numpy as np
import pytest

import replay_prog as RP
import verdict_ref as R

SHAPES = {"one_fold_step-bn": (1, (6, 2, 1, 2), {}), "one_fold_step-gl": (0, (6, 2, 1, 2), {}), "arity_4": (1, (8, 2, 2, 2), dict(arity_bits=2))}
FUSE = {"unfused": None, "fuse_gl": (True, False), "fuse_gl_bn": (True, True)}


def _trace(h2w_api, sh, kh, words):
    c = h2w_api.Context(sh.lookup_bits, True, 0); c.trace_begin()
    h2w_api.verify_stark(c, sh, kh, words)
    return c


def _from_trace(h2w_api, ctx, nwords, kh, fuse, **kw):
    if fuse is not None:
        kw.update(fuse_consts=kh, fuse_gl=fuse[0], fuse_bn=fuse[1])
    return h2w_api.Plan.from_trace(ctx, nwords, **kw)


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_assert_equal_of_the_protocol_is_recorded_and_lowered(h2w, h2w_api, oracle, consts, name):
    ko, kh = consts
    mode, (db, nq, rb, ch), over = SHAPES[name]
    sh, osh = R.shape_pair(h2w, oracle, mode, db, nq, rb, ch, **over)
    rand = oracle.synth_proof(osh, 5)
    smap = R.semantic_map(osh, *R.oracle_run(osh, ko, rand)[:3])
    assert len(smap) == osh.num_queries * len(R.site_flags(osh))
    words = np.frombuffer(bytes(oracle.synth_proof(osh, 43)), dtype=np.uint64)
    ctx = _trace(h2w_api, sh, kh, words)
    E = RP.tape_enums()
    flat = h2w_api.Plan.from_trace(ctx, len(words), parallel_scopes=())      # one segment: its op counts are the run's
    oc = flat.trace_op_counts(); hints = oc[E["DOP_LOADW_DIV"]] + oc[E["DOP_LOADW_EXTINV"]]
    assert flat.trace_info()["segments"] == 1 and hints > 0
    want = len(smap) + hints
    vi = flat.trace_verdict_info()
    assert (vi["recorded"], vi["equalities"], vi["range_sites"], vi["available"], vi["templates"]) == (want, want, 1, 1, 1), (vi, want)
    flat.close()
    for fname, fuse in FUSE.items():
        plan = _from_trace(h2w_api, ctx, len(words), kh, fuse)
        vi = plan.trace_verdict_info()
        print(name, fname, vi, "semantic", len(smap), "hints", hints)
        assert (vi["recorded"], vi["equalities"], vi["range_sites"], vi["available"]) == (want, want, 1, 1), (fname, vi, want)
        assert vi["why"] == "" and 1 <= vi["templates"] <= plan.trace_info()["templates"]
        plan.close()
    ctx.close()


class _Recording(RP.TraceBackend):
    def eq(self, a, b):
        assert self.lib.h2w_constrain_equal(self.ctx.p, C.byref(a), C.byref(b)) == 0

    def site(self, w): self.ctx.trace_site(w)


class _Silent(RP.TraceBackend):      # constrain_equal replaced by nothing
    def eq(self, a, b): pass
    def site(self, w): pass


def _prog(b):
    x, n0, h = b.gl_in(0), b.nat_in(1), b.hash_in(2)
    g = b.mul(n0, n0)
    b.site(1); b.range_check(n0, 30); b.eq(x, b.gl_in(6))
    for k in range(3):
        with b.scope("inst"):
            a = b.gl_in(12 + k); m = b.gl_mul_add(a, x, a)
            b.site(2 + k); b.eq(m, a); b.eq(b.add(g, a), g)
    for k in range(2):
        with b.scope("outer"):
            o4 = b.hash_in(8)
            for j in range(2):
                with b.scope("inner"):
                    b.site(0x100); b.eq(b.add(h, o4), h); b.check_less_than_safe(b.nat_in(7), RP.P)
    q = b.gl_div(x, b.gl_in(6))
    b.site(0x400); b.eq(q, x); b.eq(b.const(5), n0)


@pytest.mark.parametrize("fuse", list(FUSE))
def test_recording_equalities_changes_no_witness_plan(h2w, h2w_api, consts, fuse):
    proof = RP.safe_proof(15); proof[5] = proof[11] = 1      # (the two hashes below r)
    plans = []
    for cls in (_Recording, _Silent):
        tb = cls(h2w, h2w_api, proof, 13)
        _prog(tb)
        plans.append(_from_trace(h2w_api, tb.ctx, len(proof), consts[1], FUSE[fuse], parallel_scopes=RP.SCOPE_NAMES)); tb.ctx.close()
    rec, sil = plans
    facts = lambda p: (p.trace_info(), p.trace_info_bn(), p.trace_op_counts(), p.num_cells, p.num_records, [p.workspace_bytes(n) for n in (1, 3, 64)])
    assert facts(rec) == facts(sil)
    vi, vs = rec.trace_verdict_info(), sil.trace_verdict_info()
    # 1 + 3 x 2 + 4 + 2 of the program's own, + the one inside h2w_gl_div (which both traces record); range sites: the root's, a bound check per inner instance
    assert (vi["recorded"], vi["equalities"], vi["range_sites"], vi["available"]) == (14, 14, 5, 1), vi
    assert (vs["recorded"], vs["equalities"], vs["range_sites"], vs["available"]) == (1, 1, 5, 1), vs
    rec.close(); sil.close()


def _forged(h2w_api, like, offset):
    h = h2w_api.Assigned()
    C.memmove(C.byref(h), C.byref(like), C.sizeof(h))
    h.offset = offset
    return h


def test_an_equality_on_a_cell_that_is_no_result_handle_leaves_the_plan_without_a_verdict(h2w, h2w_api, consts):
    proof = RP.safe_proof(3)
    tb = _Recording(h2w, h2w_api, proof, 13)
    x, y = tb.gl_in(0), tb.gl_in(1)
    m = tb.gl_mul(x, y)
    tb.eq(_forged(h2w_api, m, int(m.offset) - 1), x)      # a cell inside gl_mul's record block: no call handed it out
    plan = h2w_api.Plan.from_trace(tb.ctx, 3, parallel_scopes=()); tb.ctx.close()
    vi = plan.trace_verdict_info()
    assert (vi["recorded"], vi["equalities"], vi["range_sites"], vi["available"], vi["templates"]) == (1, 0, 0, 0, 0), vi
    assert "no traced call's result handle" in vi["why"] and f"cell {int(m.offset) - 1}" in vi["why"], vi
    assert plan.num_cells > 0 and plan.trace_info()["ops"] == 3      # the witness plan is built as before
    with pytest.raises(h2w_api.H2WError, match="no traced call's result handle"):
        plan.trace_verdict(1, 1, 1, verdict_ptr=1)      # (refused before any device work: nothing is dereferenced)
    plan.close()


def test_an_equality_on_a_value_interior_to_a_fused_permutation(h2w, h2w_api, consts):
    """The fusing pass does not look at equalities (that could un-fuse a permutation of an existing plan): the stretch stays fused, its interior values
    are not in the value store, and only the verdict is unavailable; without the fuse flag the same trace's forged cell is just no result handle."""
    ko, kh = consts
    proof = RP.safe_proof(12)
    tb = _Recording(h2w, h2w_api, proof, 13)
    ins = [tb.gl_in(k) for k in range(12)]
    out = (h2w_api.Assigned * 12)()
    assert tb.lib.h2w_chip_gl_poseidon_permute(tb.ctx.p, C.byref(kh), h2w_api._arr(ins), out) == 0
    tb.eq(_forged(h2w_api, out[0], int(out[0].offset) - 1), ins[0])
    fused = h2w_api.Plan.from_trace(tb.ctx, 12, parallel_scopes=(), fuse_consts=kh)
    plain = h2w_api.Plan.from_trace(tb.ctx, 12, parallel_scopes=()); tb.ctx.close()
    assert fused.trace_info()["fused"] == 1
    vf, vp = fused.trace_verdict_info(), plain.trace_verdict_info()
    assert vf["available"] == 0 and "interior to a fused permutation" in vf["why"], vf
    assert vp["available"] == 0 and "no traced call's result handle" in vp["why"], vp
    fused.close(); plain.close()


def test_a_compiled_plan_has_no_trace_verdict_info(h2w, h2w_api, consts):
    plan = h2w_api.Plan(h2w.fibonacci_shape(6, 2, rate_bits=1, cap_height=2), consts[1])
    out = (C.c_uint64 * 6)()
    assert h2w.lib().h2w_plan_trace_verdict_info(plan.p, out) == -1 and "h2w_fri_verdict_batch" in h2w_api.last_error()
    with pytest.raises(h2w_api.H2WError, match="use h2w_fri_verdict_batch"):
        plan.trace_verdict(1, 1, 1, verdict_ptr=1)
    plan.close()


def test_trace_site_on_a_context_that_is_not_tracing(h2w, h2w_api):
    ctx = h2w_api.Context(13, True, 0)
    a = h2w_api.NativeChip(ctx).load_constant(7)
    before = ctx.num_cells()
    assert h2w.lib().h2w_trace_site(ctx.p, 0x55) == 0
    ctx.trace_site(1 << 31)
    assert ctx.num_cells() == before == 1 and a.has_cell
    ctx.close()
