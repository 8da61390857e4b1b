"""H2W_TRACE_SPLIT_SELECTS, the host side (no GPU): the flag's value in the header, the package and the Rust block, flags 4 and 16 still refused; the
programs of tests/replay_prog.py that h2w_plan_from_trace refuses for a wide select on 52 to 64 entries lower with the flag, to the oracle's cells,
with the select as two or more DOP_FR_SELIND parts; a flag that splits nothing leaves the plan what it is without it; the PoseidonBN254 verifier at
cap_height 6 lowers with every combination of the other flags, with a verdict and with fused permutations.  tests/test_gpu_replay_split_selects.py
replays the same plans on the device; tests/test_tapefmt_chain.py holds tape_check to the shape of a chain of parts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import replay_prog as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = rp.tape_enums()
SPLIT = 32
RING_K = 256
VERIFIER_SCOPES = ("verify_query_round", "verify_proof_to_cap_with_cap_index")
CAP6_CELLS = 25942538      # the oracle's cell count of fibonacci_shape(7, 2, rate_bits=1, hash_mode=1, cap_height=6) at lookup_bits 21


def plan_ex(h2w, api, ctx, nwords, scopes, flags, kh=None):
    """h2w_plan_from_trace_ex with `flags` as given (Plan.from_trace has a keyword per flag) -> Plan; raises H2WError where it refuses."""
    names = (C.c_char_p * len(scopes))(*[s.encode() for s in scopes])
    h = h2w.lib().h2w_plan_from_trace_ex(ctx.p, nwords, names, len(scopes), 0, C.byref(kh) if kh is not None else None, flags)
    if not h:
        raise h2w.H2WError("h2w_plan_from_trace_ex: " + h2w.last_error())
    return api.Plan(None, None, 0, _handle=h)


def lower(h2w, api, prog, proof_a, flags, lookup_bits=21, scopes=()):
    """rp.lower with the lowering's flags"""
    tb = rp.TraceBackend(h2w, api, proof_a, lookup_bits)
    try:
        hs = rp.flatten(prog(tb))
        assert all(h.has_cell for h in hs)
        plan = plan_ex(h2w, api, tb.ctx, len(proof_a), tuple(scopes), flags) if flags else api.Plan.from_trace(tb.ctx, len(proof_a), parallel_scopes=tuple(scopes))
        assert plan.num_cells == tb.ctx.num_cells() and plan.proof_words == len(proof_a)
        return rp.Lowered(plan, [int(h.offset) for h in hs], tb.ctx.num_cells())
    finally:
        tb.ctx.close()


def far_program(n, scoped):
    return rp.Program(f"far_operands-{n}-{'scoped' if scoped else 'flat'}", rp.prog_far_operands(n, scoped), 4 * n + 1, None, 21, ("sel",) if scoped else ())


def list_program(n, L):
    return rp.Program(f"lists-n{n}-wide", rp.prog_lists(n, L, True, True), 8 + 5 * n, None, L)


# name -> (program, wide selects that have to be split)
SPLIT_PROGRAMS = [(far_program(n, scoped), 1) for n in (52, 64) for scoped in (True, False)] + [(list_program(63, 8), 2), (list_program(64, 21), 2)]


def traced_verifier(h2w, api, oracle, mode, cap_height):
    """The Fibonacci verifier at (7, 2, rate_bits 1) recorded on one synthetic proof -> (context, proof words)"""
    sh = h2w.fibonacci_shape(7, 2, rate_bits=1, hash_mode=mode, cap_height=cap_height); osh = oracle.fibonacci_shape(7, 2, rate_bits=1, hash_mode=mode, cap_height=cap_height)
    proof = oracle.synth_proof(osh, 1)
    ctx = api.Context(21, True, 0); ctx.trace_begin()
    api.verify_stark(ctx, sh, h2w.published_consts(), np.frombuffer(bytes(proof), dtype=np.uint64))
    return ctx, len(proof)


def quantities(plan):
    return plan.trace_op_counts(), plan.num_records, [plan.workspace_bytes(n) for n in (1, 70)], plan.trace_info()


# ---------------------------------------------------------------- the flag
def test_the_flag_is_32_in_the_header_the_package_and_the_rust_block(h2w):
    hdr = open(os.path.join(ROOT, "include", "h2w.h")).read()
    rs = open(os.path.join(ROOT, "rust", "h2w-sys", "src", "lib.rs")).read()
    assert re.search(r"^#define H2W_TRACE_SPLIT_SELECTS 32\s*$", hdr, flags=re.M)
    assert h2w.H2W_TRACE_SPLIT_SELECTS == SPLIT
    assert "pub const H2W_TRACE_SPLIT_SELECTS: c_int = 32;" in rs


def test_flags_4_and_16_are_still_unknown_alone_and_with_the_flag(h2w, h2w_api):
    kh = h2w.published_consts()
    tb = rp.TraceBackend(h2w, h2w_api, rp.safe_proof(205), 21)
    try:
        rp.prog_far_operands(51, False)(tb)
        for flags in (4, 16, 4 | SPLIT, 16 | SPLIT, 4 | 16 | SPLIT, 64, 64 | SPLIT):
            with pytest.raises(h2w.H2WError, match="unknown flag"):
                plan_ex(h2w, h2w_api, tb.ctx, 205, (), flags, kh)
        plan_ex(h2w, h2w_api, tb.ctx, 205, (), SPLIT).close()                  # alone the flag needs no tables (as flag 8)
        plan_ex(h2w, h2w_api, tb.ctx, 205, (), SPLIT | 8).close()
        for flags in (SPLIT | 1, SPLIT | 2):                                     # the fuse flags still do
            with pytest.raises(h2w.H2WError, match="needs the Poseidon tables"):
                plan_ex(h2w, h2w_api, tb.ctx, 205, (), flags)
        h2w_api.Plan.from_trace(tb.ctx, 205, parallel_scopes=(), split_selects=True).close()
        h2w_api.Plan.from_trace(tb.ctx, 205, parallel_scopes=(), split_selects=True, fuse_consts=kh, fuse_bn=True, output_forms=True).close()
    finally:
        tb.ctx.close()


# ---------------------------------------------------------------- programs that were refused
@pytest.mark.parametrize("case", SPLIT_PROGRAMS, ids=lambda c: c[0].name)
def test_a_refused_program_lowers_with_the_flag(h2w, h2w_api, oracle, case):
    prog, n_selects = case
    with pytest.raises(h2w.H2WError, match="more than the 256 value slots"):
        lower(h2w, h2w_api, prog.fn, prog.proof_a(), 0, prog.lookup_bits, prog.scopes)
    lw = lower(h2w, h2w_api, prog.fn, prog.proof_a(), SPLIT, prog.lookup_bits, prog.scopes)      # (num_cells is the tracing context's: asserted there)
    stream, cells, _ = rp.oracle_run(oracle, prog.fn, prog.proof_a(), prog.lookup_bits)
    c = lw.plan.trace_op_counts(); lw.plan.close()
    assert lw.num_cells == len(stream) // 32 and lw.offsets == cells
    parts = c[E["DOP_FR_SELIND"]]
    assert parts >= 2 * n_selects, parts
    if prog.fn.__qualname__.startswith("prog_far_operands"):
        # 4 n + n slots have to be fetched (the refusal's count), at most 256 in front of a part: two parts are the fewest, and what the lowering makes
        n = (prog.nwords - 1) // 4
        assert parts == 2 == -(-5 * n // RING_K)
        wide = rp.fetches(c, E, "RK_IMPORT") if prog.scopes else None
        local = rp.fetches(c, E, "RK_LOCAL")
        if prog.scopes:      # the entries are the imports, four slots each; the local fetches are the indicators pushed out of the ring
            assert wide == n and local <= n and 4 * wide + local <= RING_K * parts, (wide, local)
        else:                # entries and indicators are both local: at least cnt - n of the cnt fetches are entries
            assert local <= 2 * n and 4 * max(local - n, 0) + min(local, n) <= RING_K * parts, local


# the same select with its indicators read from the proof (tests/test_gpu_replay_split_selects.py puts indicators that are no bits into every part)
IND_PROGRAM = rp.Program("ind_words_select-64-scoped", rp.prog_ind_words_select(64, True), 5 * 64, None, 21, ("sel",))


def test_a_select_by_indicators_from_the_proof_is_refused_without_the_flag_and_split_with_it(h2w, h2w_api, oracle):
    prog = IND_PROGRAM
    with pytest.raises(h2w.H2WError, match="more than the 256 value slots"):
        lower(h2w, h2w_api, prog.fn, prog.proof_a(), 0, prog.lookup_bits, prog.scopes)
    lw = lower(h2w, h2w_api, prog.fn, prog.proof_a(), SPLIT, prog.lookup_bits, prog.scopes)
    stream, cells, _ = rp.oracle_run(oracle, prog.fn, prog.proof_a(), prog.lookup_bits)
    parts = lw.plan.trace_op_counts()[E["DOP_FR_SELIND"]]; lw.plan.close()
    assert lw.num_cells == len(stream) // 32 and lw.offsets == cells
    assert parts >= 2, parts


@pytest.mark.parametrize("n", [52, 64])
def test_the_public_keyword_routes_the_flag(h2w, h2w_api, n):
    tb = rp.TraceBackend(h2w, h2w_api, rp.safe_proof(4 * n + 1), 21)
    try:
        rp.prog_far_operands(n, True)(tb)
        with pytest.raises(h2w.H2WError, match="more than the 256 value slots"):
            h2w_api.Plan.from_trace(tb.ctx, 4 * n + 1, parallel_scopes=("sel",))
        for kw in (dict(), dict(output_forms=True), dict(fuse_consts=h2w.published_consts()), dict(fuse_consts=h2w.published_consts(), fuse_bn=True, output_forms=True)):
            plan = h2w_api.Plan.from_trace(tb.ctx, 4 * n + 1, parallel_scopes=("sel",), split_selects=True, **kw)
            assert plan.num_cells == tb.ctx.num_cells() and plan.trace_op_counts()[E["DOP_FR_SELIND"]] == 2
            plan.close()
    finally:
        tb.ctx.close()


def test_other_ops_with_too_many_fetched_operands_are_still_refused(h2w, h2w_api):
    """Only the wide select is split.  Its refusal without the flag keeps its words; with the flag the documented refusals of the lowering stay."""
    def too_many(b):
        b.select_array_by_indicator([[x] for x in [b.nat_in(1) for _ in range(65)]], [b.nat_in(1) for _ in range(65)])
        return []
    with pytest.raises(h2w.H2WError, match="select_by_indicator: more than 64 entries"):
        lower(h2w, h2w_api, too_many, rp.safe_proof(8), SPLIT)
    with pytest.raises(h2w.H2WError, match=r"decompose_le: only \(56 bits, 5 limbs\) is replayable"):
        lower(h2w, h2w_api, lambda b: b.decompose_le(b.nat_in(0), 32, 3) and [], rp.safe_proof(8), SPLIT)


# ---------------------------------------------------------------- a flag that splits nothing changes nothing
@pytest.mark.parametrize("scoped", [True, False])
def test_a_select_that_fits_stays_one_op(h2w, h2w_api, scoped):
    prog = rp.prog_far_operands(51, scoped); scopes = ("sel",) if scoped else ()
    a = lower(h2w, h2w_api, prog, rp.safe_proof(205), 0, 21, scopes); b = lower(h2w, h2w_api, prog, rp.safe_proof(205), SPLIT, 21, scopes)
    assert quantities(a.plan) == quantities(b.plan) and a.offsets == b.offsets
    assert a.plan.trace_op_counts()[E["DOP_FR_SELIND"]] == 1
    a.plan.close(); b.plan.close()


@pytest.mark.parametrize("mode,cap_height", [(1, 5), (0, 6)], ids=["bn254-cap5", "goldilocks-cap6"])
def test_a_verifier_without_such_a_select_lowers_to_the_same_plan(h2w, h2w_api, oracle, mode, cap_height):
    kh = h2w.published_consts()
    ctx, nwords = traced_verifier(h2w, h2w_api, oracle, mode, cap_height)
    try:
        for other in (0, 1 | 2 | 8):
            a = plan_ex(h2w, h2w_api, ctx, nwords, VERIFIER_SCOPES, other, kh) if other else h2w_api.Plan.from_trace(ctx, nwords)
            b = plan_ex(h2w, h2w_api, ctx, nwords, VERIFIER_SCOPES, other | SPLIT, kh)
            assert quantities(a) == quantities(b), other
            assert a.num_cells == b.num_cells == ctx.num_cells() and a.trace_info_bn() == b.trace_info_bn() and a.trace_verdict_info() == b.trace_verdict_info()
            if other & 8:
                assert np.array_equal(a.direct_cells(), b.direct_cells())
            a.close(); b.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------- the PoseidonBN254 verifier at cap_height 6
def test_the_bn254_verifier_with_64_cap_entries_lowers_with_every_combination_of_flags(h2w, h2w_api, oracle):
    kh = h2w.published_consts()
    ctx, nwords = traced_verifier(h2w, h2w_api, oracle, 1, 6)
    try:
        with pytest.raises(h2w.H2WError, match="select_by_indicator with 128 operands: .* more than the 256 value slots"):
            h2w_api.Plan.from_trace(ctx, nwords)
        assert ctx.num_cells() == CAP6_CELLS
        seen = {}
        for flags in (SPLIT, SPLIT | 1, SPLIT | 1 | 2, SPLIT | 8, SPLIT | 1 | 2 | 8):
            plan = plan_ex(h2w, h2w_api, ctx, nwords, VERIFIER_SCOPES, flags, kh if flags & 3 else None)
            assert plan.num_cells == ctx.num_cells() == CAP6_CELLS and plan.proof_words == nwords
            assert plan.trace_verdict_info()["available"] == 1, h2w.last_error()      # (out[3] of h2w_plan_trace_verdict_info)
            c = plan.trace_op_counts()
            seen[flags] = (c[E["DOP_FR_SELIND"]], plan.num_records, plan.workspace_bytes(1))
            if flags & 2:
                assert plan.trace_info_bn()["fused"] > 0 and c[E["DOP_BNPERM"]] > 0
            if flags & 1:
                assert plan.trace_info()["fused"] > 0
            if flags & 8:      # the direct cells are the complement of the records: the 1 + 3 n cells of every select, parts or not, among them
                direct = np.unpackbits(plan.direct_cells(), bitorder="little")
                assert int(direct.sum()) + plan.num_record_cells == plan.num_cells
            plan.close()
        # the split depends on the tape alone: the same parts whatever else the lowering does, and no record or slot for them with the output forms
        assert len({v[0] for v in seen.values()}) == 1 and seen[SPLIT][0] >= 2
        assert seen[SPLIT] == seen[SPLIT | 8] and seen[SPLIT | 1 | 2] == seen[SPLIT | 1 | 2 | 8]
    finally:
        ctx.close()
