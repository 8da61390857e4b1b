"""Hand-driven operator programs through h2w_plan_from_trace, the host side (no GPU): every program of tests/replay_prog.py lowers, to the oracle's
cell count, and h2w_plan_trace_op_counts shows that it reaches the part of the lowering it was written for - the ring's 256 slots, the LDS part of the
constant pools, every DOP_FETCH kind, runs of 255, several templates, imports into depth 2; what csrc/tracelower.cpp documents as not replayable is
refused by its message.  tests/test_gpu_replay_programs.py replays the same programs on the device."""
import os
import re

import pytest

import replay_prog as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = rp.tape_enums()
_counts = {}


def _lowered_counts(h2w, h2w_api, oracle, prog):
    if prog.name not in _counts:
        lw = rp.lower(h2w, h2w_api, prog.fn, prog.proof_a(), prog.lookup_bits, prog.scopes)
        stream, cells, _ = rp.oracle_run(oracle, prog.fn, prog.proof_a(), prog.lookup_bits)
        c = lw.plan.trace_op_counts(); lw.plan.close()
        _counts[prog.name] = (c, lw.num_cells, len(stream) // 32, lw.offsets == cells)
    return _counts[prog.name]


def test_the_enums_are_read_from_the_tape_format():
    assert E["DOP_END"] == 0 and E["RK_LOCAL"] == 0 and E["RK_RING"] == E["RK_LITFR"] + 1
    assert E["DOP_COUNT"] == E["DOP_BNPERM"] + 1 and E["DOP_GLOPRUN"] == E["DOP_FETCH"] + 1 and E["DOP_GLPERM"] == E["DOP_GLOPRUN"] + 1


@pytest.mark.parametrize("prog", rp.PROGRAMS, ids=lambda p: p.name)
def test_a_program_lowers_to_the_oracles_cells_and_reaches_what_it_was_written_for(h2w, h2w_api, oracle, prog):
    counts, ncells, oracle_cells, same_handles = _lowered_counts(h2w, h2w_api, oracle, prog)
    assert len(counts) == E["DOP_COUNT"] + E["RK_RING"] + 1
    assert ncells == oracle_cells and same_handles
    assert all(len(p) == prog.nwords for p in prog.batch(3))
    prog.expect(counts, E)


def test_the_programs_together_reach_every_interpreter_op_and_every_fetch_kind(h2w, h2w_api, oracle):
    total = [0] * (E["DOP_COUNT"] + E["RK_RING"] + 1)
    for prog in rp.PROGRAMS:
        total = [a + b for a, b in zip(total, _lowered_counts(h2w, h2w_api, oracle, prog)[0])]
    names = {v: k for k, v in E.items() if k.startswith("DOP_")}
    missing = [names[op] for op in range(E["DOP_SKIP"], E["DOP_GLOPRUN"] + 1) if total[op] == 0]      # DOP_GLPERM, DOP_BNPERM: the fused tests'
    assert not missing, missing
    kinds = ("RK_LOCAL", "RK_IMPORT", "RK_LIT64", "RK_INPUT", "RK_LITFR")
    assert not [k for k in kinds if total[E["DOP_COUNT"] + E[k]] == 0]
    assert sorted(E[k] for k in kinds) == list(range(E["RK_RING"]))


def test_a_constant_loaded_in_front_of_its_op_is_one_record_in_the_middle_of_a_run(h2w, h2w_api):
    """T_KA_GLOP: the same program with the constant loaded early has one record more, and the same runs."""
    a = rp.lower(h2w, h2w_api, rp.prog_runs(True), rp.safe_proof(3)); b = rp.lower(h2w, h2w_api, rp.prog_runs(False), rp.safe_proof(3))
    assert a.plan.num_records + 1 == b.plan.num_records and a.num_cells == b.num_cells
    ca, cb = a.plan.trace_op_counts(), b.plan.trace_op_counts()
    assert ca[E["DOP_GLOPRUN"]] == cb[E["DOP_GLOPRUN"]] == 5 and rp.longest_run(ca, E) == rp.longest_run(cb, E) == 255
    a.plan.close(); b.plan.close()


def test_op_counts_of_a_compiled_plan_are_refused(h2w, h2w_api):
    plan = h2w_api.Plan(h2w.fibonacci_shape(6, 2), h2w.published_consts())
    with pytest.raises(h2w.H2WError, match="not a traced plan"):
        plan.trace_op_counts()
    plan.close()


def test_header_rust_block_and_library_declare_the_op_counts(h2w):
    hdr = open(os.path.join(ROOT, "include", "h2w.h")).read()
    rs = open(os.path.join(ROOT, "rust", "h2w-sys", "src", "lib.rs")).read()
    assert re.search(r"^int h2w_plan_trace_op_counts\(const h2w_plan \*, uint64_t \*out, size_t n_out\);$", hdr, flags=re.M)
    assert "pub fn h2w_plan_trace_op_counts(a0: *const H2wPlan, out: *mut u64, n_out: usize) -> c_int;" in rs
    assert hasattr(h2w.lib(), "h2w_plan_trace_op_counts") and "h2w_plan_trace_op_counts" in h2w.SYMBOLS


def test_the_status_cases_of_the_goldilocks_program_are_all_there():
    """What the batch of the Goldilocks program holds: proofs with a zero divisor (1), with a zero extension element (2), never both; non-canonical
    words (4); a zero divisor AND a non-canonical word (1: the chip status wins, h2w_plan_status); proofs with none of them (0)."""
    proofs = next(p for p in rp.PROGRAMS if p.fn is rp.prog_gl_ops).batch(130)
    runs = [rp.int_run(rp.prog_gl_ops, p)[1] for p in proofs]
    assert {r.status() for r in runs} == {0, 1, 2, 4}
    assert any(r.chip == 1 and r.flagged for r in runs) and any(r.chip == 1 and not r.flagged for r in runs)
    assert not any(p[8] == 0 and p[11] == 0 and p[12] == 0 for p in proofs)


# ---- batches that leave proof A's value domain (status 5)
def test_the_off_domain_programs_together_show_the_ops_that_can_raise_5(h2w, h2w_api, oracle):
    total = [0] * (E["DOP_COUNT"] + E["RK_RING"] + 1)
    for prog in rp.OFF_PROGRAMS:
        total = [a + b for a, b in zip(total, _lowered_counts(h2w, h2w_api, oracle, prog)[0])]
    ops = ("DOP_SELECT", "DOP_FR_SELECT", "DOP_SELIND", "DOP_FR_SELIND", "DOP_BITS2NUM", "DOP_NUM2BITS", "DOP_RANGE", "DOP_FR_MULADD", "DOP_REDUCE")
    assert not [op for op in ops if total[E[op]] == 0]
    assert {p.name for p in rp.OFF_PROGRAMS} == {"off_select", "off_selind", "off_reduce", "off_bits-L21", "off_bits-L13", "off_bits-L8"}


@pytest.mark.parametrize("prog", rp.OFF_PROGRAMS, ids=lambda p: p.name)
def test_an_off_domain_batch_holds_what_it_is_built_for(oracle, prog):
    """Per proof of every batch the device test replays: the oracle (total on these inputs) and the integer model agree on every handle; the model's
    status is the batch's stated one - 0 for the proofs in domain, 5 for one offence, 5 where the offence stands in front of a zero divisor, 1 where
    the zero divisor stands in front; an off-domain proof has exactly one offending op, and the cells in front of it are fewer than the stream.  At
    least a quarter of every batch is in domain, proof 0 is, and the batch of 130 holds every kind of offence."""
    od = prog.off
    assert prog.sizes == (1, 130) and len(od.kinds) == len({k[0] for k in od.kinds})
    for n in prog.sizes:
        proofs = prog.batch(n); in_domain = 0; kinds = set()
        for i, p in enumerate(proofs):
            assert len(p) == prog.nwords and all(0 <= w < 2**64 for w in p)
            want_vals, ib = rp.int_run(prog.fn, p)
            stream, cells, vals, entries = rp.oracle_run(oracle, prog.fn, p, prog.lookup_bits, entries=True)
            assert vals == want_vals, (i, od.kind(i) and od.kind(i)[0], [k for k in range(len(vals)) if vals[k] != want_vals[k]][:8])
            assert ib.status() == od.expected_status(i), (i, ib.status(), od.kind(i) and od.kind(i)[0])
            held = rp.held_cells(ib, entries, len(stream) // 32)
            if od.kind(i) is None:
                assert ib.status() == 0 and ib.off is None and not ib.flagged and held == len(stream) // 32
                in_domain += 1
            else:
                assert ib.n_off == 1 and 0 < held < len(stream) // 32, (i, od.kind(i)[0], ib.n_off)
                kinds.add(od.kind(i)[0])
        assert 4 * in_domain >= n and od.kind(0) is None
        if n == 130:
            assert kinds == {k[0] for k in od.kinds}
            assert {od.expected_status(i) for i in range(n)} == {0, 1, 5} and any(i % 16 == 5 for i in range(n))


def test_the_integer_model_states_the_cases_of_the_status_5_rule():
    """select(5, 9, 2) = 1; bits_to_num([2^63, 2^63]) = 3 * 2^63; entries (5, 9) by indicators (2, p - 1); mul_sub(p - 1, p - 1, p - 1) = 2: the field's
    values, each under status 5; the same ops on bits: status 0."""
    P = rp.P
    for run, want in ((lambda b: b.select(5, 9, 2), 1), (lambda b: b.bits_to_num([2**63, 2**63]), 0x18000000000000000),
                      (lambda b: b.select_array_by_indicator([[5], [9]], [2, P - 1])[0], 0x8fffffff70000000a), (lambda b: b.gl_mul_sub(P - 1, P - 1, P - 1), 2),
                      (lambda b: b.gl_reduce(2**128), 2**128 % P), (lambda b: b.select_array_by_indicator([[2**63], [2**63]], [1, 1])[0], 2**64)):
        ib = rp.IntBackend([]); assert run(ib) == want and ib.status() == 5 and ib.off == 0
    for run, want in ((lambda b: b.select(5, 9, 1), 5), (lambda b: b.select(5, 9, 0), 9), (lambda b: b.bits_to_num([1] * 64), 2**64 - 1), (lambda b: b.gl_reduce(2**128 - 1), (2**128 - 1) % P),
                      (lambda b: b.select_array_by_indicator([[2**64], [2**253]], [1, 1])[0], 2**64 + 2**253), (lambda b: b.gl_mul_sub(P - 1, P - 1, 0), 1)):
        ib = rp.IntBackend([]); assert run(ib) == want and ib.status() == 0 and ib.off is None
    ib = rp.IntBackend([]); ib.gl_div(3, 0); ib.select(1, 2, 3)
    assert ib.status() == 1 and ib.off == 0      # the first condition wins; the offending op is still remembered
    ib = rp.IntBackend([2**64 - 1]); ib.nat_in(0); ib.select(1, 2, 3)
    assert ib.status() == 5 and ib.flagged      # ... and 5 wins over 4


# ---- what cannot be replayed
def _refused(h2w, h2w_api, fn, nwords, match, scopes=()):
    proof = rp.safe_proof(nwords)
    proof[3:6] = [0, 0, 0]      # the four-word value at word 2 is below 2^64 on proof A: the eager call takes it, the lowering goes by the static width
    with pytest.raises(h2w.H2WError, match=match):
        lw = rp.lower(h2w, h2w_api, fn, proof, 21, scopes)
        lw.plan.close()


def _bits(b, n):
    return [b.nat_in(1) for _ in range(n)]


REFUSALS = [
    ("idx_to_indicator-65", lambda b: b.idx_to_indicator(b.nat_in(0), 65), "idx_to_indicator: a wide index or more than 64 entries"),
    ("select_by_indicator-65", lambda b: b.select_array_by_indicator([[x] for x in _bits(b, 65)], _bits(b, 65)), "select_by_indicator: more than 64 entries"),
    ("num_to_bits-65", lambda b: b.num_to_bits(b.nat_in(0), 65), "num_to_bits: a wide value or more than 64 bits"),
    ("bits_to_num-65", lambda b: b.bits_to_num(_bits(b, 65)), "bits_to_num: more than 64 bits"),
    ("decompose_le-32x3", lambda b: b.decompose_le(b.nat_in(0), 32, 3), r"decompose_le: only \(56 bits, 5 limbs\) is replayable"),
    ("decompose_le-56x4", lambda b: b.decompose_le(b.nat_in(0), 56, 4), r"decompose_le: only \(56 bits, 5 limbs\) is replayable"),
    ("limbs_to_num-5", lambda b: b.limbs_to_num(_bits(b, 5), 64), "limbs_to_num: only up to four 64-bit limbs are replayable"),
    ("limbs_to_num-32bit", lambda b: b.limbs_to_num(_bits(b, 2), 32), "limbs_to_num: only up to four 64-bit limbs are replayable"),
    ("check_less_than_safe-bound", lambda b: b.check_less_than_safe(b.nat_in(0), 2**63), "check_less_than_safe: only .* is replayable"),
    ("range_check-wide", lambda b: b.range_check(b.hash_in(0), 200), "range_check: a wide value"),
    ("select-wide-selector", lambda b: b.select(b.nat_in(0), b.nat_in(1), b.hash_in(2)), "select: the selector is not a bit"),
    ("gl-wide-operand", lambda b: b.gl_mul(b.gl_in(0), b.hash_in(2)), "a Goldilocks op on a wide value"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: c[0])
def test_what_the_lowering_documents_as_not_replayable_is_refused(h2w, h2w_api, case):
    def prog(b):
        case[1](b)
        return []
    _refused(h2w, h2w_api, prog, 8, case[2])


def test_a_tagged_constant_of_four_words_is_refused(h2w, h2w_api):
    def prog(b):
        b._tag(0, 4); b.nat.load_constant(b.hash_value(0))
        return []
    _refused(h2w, h2w_api, prog, 8, "a constant that is a proof value must be one Goldilocks word")


# ---- more fetched operands than the lane's ring holds (include/h2w.h 2d)
@pytest.mark.parametrize("scoped", [True, False])
@pytest.mark.parametrize("n", [52, 64])
def test_a_wide_select_of_more_entries_than_the_ring_holds_is_refused(h2w, h2w_api, n, scoped):
    """4 n + n operand words of a wide select_by_indicator: from n = 52 on they are more than the 256 slots, and before the bound the later fetches
    overwrote the earlier ones (slot mod 256) - the plan lowered and the op read the wrong entries."""
    _refused(h2w, h2w_api, rp.prog_far_operands(n, scoped), 4 * n + 1, rf"select_by_indicator with {2 * n} operands: {5 * n} slots of them have to be fetched .* more than the 256 value slots", ("sel",) if scoped else ())


@pytest.mark.parametrize("n,L", [(63, 8), (64, 21)])
def test_the_list_program_with_its_wide_array_is_refused_at_63_and_64(h2w, h2w_api, n, L):
    _refused(h2w, h2w_api, rp.prog_lists(n, L, True, False), 8 + 5 * n, "select_by_indicator with .* more than the 256 value slots")


def _traced_verifier(h2w, h2w_api, oracle, cap_height):
    import numpy as np
    sh = h2w.fibonacci_shape(7, 2, rate_bits=1, hash_mode=1, cap_height=cap_height); osh = oracle.fibonacci_shape(7, 2, rate_bits=1, hash_mode=1, cap_height=cap_height)
    proof = oracle.synth_proof(osh, 1)
    ctx = h2w_api.Context(21, True, 0); ctx.trace_begin()
    h2w_api.verify_stark(ctx, sh, h2w.published_consts(), np.frombuffer(bytes(proof), dtype=np.uint64))
    return ctx, len(proof)


def test_a_traced_bn254_verifier_with_64_cap_entries_is_refused(h2w, h2w_api, oracle):
    """cap_height 6: 64 wide cap entries imported from the root into verify_proof_to_cap_with_cap_index.  (Goldilocks-Poseidon caps are one-word
    entries: that trace replays, tests/test_gpu_replay_programs.py.)"""
    ctx, nwords = _traced_verifier(h2w, h2w_api, oracle, 6)
    try:
        with pytest.raises(h2w.H2WError, match="select_by_indicator with 128 operands: .* more than the 256 value slots"):
            h2w_api.Plan.from_trace(ctx, nwords).close()
    finally:
        ctx.close()


def test_a_traced_bn254_verifier_with_32_cap_entries_lowers(h2w, h2w_api, oracle):
    ctx, nwords = _traced_verifier(h2w, h2w_api, oracle, 5)
    try:
        plan = h2w_api.Plan.from_trace(ctx, nwords)
        assert plan.num_cells == ctx.num_cells()
        plan.close()
    finally:
        ctx.close()
