"""H2W_TRACE_OUTPUT_FORMS, the host side (no GPU): the flag's value in the header, the package and the Rust block; flag 4 stays refused; a plan lowered
with the flag maps its direct cells as the complement of its record ranges and takes H2W_OPT_OUTPUT_FORM without a device; a plan lowered without it
refuses all three as before."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BN_PERM_CELLS = 4032
# flags -> Plan.from_trace keywords (kh: the Poseidon tables)
FLAG_KW = {8: lambda kh: dict(), 9: lambda kh: dict(fuse_consts=kh), 10: lambda kh: dict(fuse_consts=kh, fuse_bn=True, fuse_gl=False), 11: lambda kh: dict(fuse_consts=kh, fuse_bn=True)}


def traced_fibonacci(h2w, h2w_api, oracle, consts, mode, d=6, q=2, rb=1, cap=4, lookup_bits=21, seed=42, witness_gen_only=True):
    """A context that recorded the Fibonacci verifier on one synthetic proof -> (context, proof words)"""
    ko, kh = consts
    sh = h2w.fibonacci_shape(d, q, rate_bits=rb, cap_height=cap, hash_mode=mode, lookup_bits=lookup_bits)
    osh = oracle.fibonacci_shape(d, q, rate_bits=rb, cap_height=cap, hash_mode=mode, lookup_bits=lookup_bits)
    proof = oracle.synth_proof(osh, seed)
    ctx = h2w_api.Context(lookup_bits, witness_gen_only, 0); ctx.trace_begin()
    h2w_api.verify_stark(ctx, sh, kh, np.frombuffer(bytes(proof), dtype=np.uint64))
    return ctx, proof


def test_the_flag_is_8_in_the_header_the_package_and_the_rust_block(h2w):
    hdr = open(os.path.join(ROOT, "include", "h2w.h")).read()
    rs = open(os.path.join(ROOT, "rust", "h2w-sys", "src", "lib.rs")).read()
    assert re.search(r"^#define H2W_TRACE_OUTPUT_FORMS 8\s*$", hdr, flags=re.M)
    assert h2w.H2W_TRACE_OUTPUT_FORMS == 8
    assert "pub const H2W_TRACE_OUTPUT_FORMS: c_int = 8;" in rs


def test_flag_4_is_still_an_unknown_flag(h2w, h2w_api, oracle, consts):
    ko, kh = consts
    ctx, proof = traced_fibonacci(h2w, h2w_api, oracle, consts, 1)
    L = h2w.lib(); names = (C.c_char_p * 0)()
    for flags in (4, 4 | 8, 16):
        assert not L.h2w_plan_from_trace_ex(ctx.p, len(proof), names, 0, 0, C.byref(kh), flags) and "unknown flag" in h2w.last_error(), flags
    p = L.h2w_plan_from_trace_ex(ctx.p, len(proof), names, 0, 0, None, 8)      # the flag alone needs no tables
    assert p, h2w.last_error()
    L.h2w_plan_free(p)
    ctx.close()


@pytest.mark.parametrize("flags", sorted(FLAG_KW))
@pytest.mark.parametrize("mode", [1, 0])
def test_direct_cells_and_record_ranges_tile_the_stream(h2w, h2w_api, oracle, consts, mode, flags):
    ko, kh = consts
    ctx, proof = traced_fibonacci(h2w, h2w_api, oracle, consts, mode)
    plan = h2w_api.Plan.from_trace(ctx, len(proof), output_forms=True, **FLAG_KW[flags](kh))
    base = h2w_api.Plan.from_trace(ctx, len(proof), **FLAG_KW[flags](kh)); ctx.close()
    n = plan.num_cells
    assert (n, plan.num_records, plan.num_record_cells) == (base.num_cells, base.num_records, base.num_record_cells)
    assert [plan.workspace_bytes(k) for k in (1, 3)] == [base.workspace_bytes(k) for k in (1, 3)]
    direct = np.unpackbits(plan.direct_cells(), bitorder="little")
    assert not direct[n:].any()
    direct = direct[:n].astype(bool)
    rr = plan.record_ranges().astype(np.int64)
    assert rr.shape == (plan.num_records, 2) and int(rr[:, 1].sum()) == plan.num_record_cells
    cover = np.zeros(n + 1, dtype=np.int64)
    assert rr[:, 0].min() >= 0 and (rr[:, 0] + rr[:, 1]).max() <= n and (rr[:, 1] > 0).all()
    np.add.at(cover, rr[:, 0], 1); np.add.at(cover, rr[:, 0] + rr[:, 1], -1)
    cover = np.cumsum(cover)[:n]
    assert cover.max() <= 1, "two records on one cell"
    assert np.array_equal(cover == 0, direct), "the direct cells are not the complement of the record ranges"
    assert int(direct.sum()) + plan.num_record_cells == n
    if flags & 2:      # every cell of every fused PoseidonBN254 permutation is direct
        fused = plan.trace_info_bn()["fused"]
        assert (fused > 0) == (mode == 1)
        runs = np.diff(np.concatenate(([0], direct.astype(np.int8), [0])))
        lens = np.nonzero(runs == -1)[0] - np.nonzero(runs == 1)[0]
        assert int((lens // BN_PERM_CELLS).sum()) >= fused and int(direct.sum()) >= fused * BN_PERM_CELLS
    plan.close(); base.close()


def test_fused_permutations_lie_whole_inside_runs_of_direct_cells(h2w, h2w_api, oracle, consts):
    """Flag 8 against 8|2 on one trace: a PoseidonBN254 permutation's cells are wide values, direct cells whether the interpreter or the emission kernel
    writes them - fusing changes neither map -, and every fused permutation lies whole inside a run of direct cells."""
    ko, kh = consts
    ctx, proof = traced_fibonacci(h2w, h2w_api, oracle, consts, 1)
    plain = h2w_api.Plan.from_trace(ctx, len(proof), output_forms=True)
    fused = h2w_api.Plan.from_trace(ctx, len(proof), output_forms=True, **FLAG_KW[10](kh)); ctx.close()
    n = plain.num_cells; nf = fused.trace_info_bn()["fused"]
    a = np.unpackbits(plain.direct_cells(), bitorder="little")[:n].astype(np.int8); b = np.unpackbits(fused.direct_cells(), bitorder="little")[:n].astype(np.int8)
    assert nf > 0 and np.array_equal(a, b) and plain.num_record_cells == fused.num_record_cells
    spans = np.diff(np.concatenate(([0], b, [0])))
    s1, e1 = np.nonzero(spans == 1)[0], np.nonzero(spans == -1)[0]
    assert int(((e1 - s1) // BN_PERM_CELLS).sum()) >= nf      # every fused permutation lies whole inside a run of direct cells
    plain.close(); fused.close()


def test_selecting_the_form_needs_no_call(h2w, h2w_api, oracle, consts):
    """Without a device the plan is a layout object: the option is taken, nothing is uploaded, and a witness call still says why it cannot run."""
    import torch
    ko, kh = consts
    ctx, proof = traced_fibonacci(h2w, h2w_api, oracle, consts, 1)
    plan = h2w_api.Plan.from_trace(ctx, len(proof), output_forms=True, **FLAG_KW[11](kh)); ctx.close()
    plan.set_output_form(h2w_api.FORM_MONTGOMERY); plan.set_output_form(h2w_api.FORM_CANONICAL); plan.set_output_form(h2w_api.FORM_MONTGOMERY)
    with pytest.raises(h2w_api.H2WError, match="OUTPUT_FORM"):
        plan.configure(h2w_api.OPT_OUTPUT_FORM, 2)
    if not torch.cuda.is_available():
        with pytest.raises(h2w_api.H2WError, match="no HIP device"):
            plan.run(1, 1, 1, 1)
    plan.close()


@pytest.mark.parametrize("flags", [0, 1, 3])
def test_plans_without_the_flag_refuse_as_before(h2w, h2w_api, oracle, consts, flags):
    ko, kh = consts
    ctx, proof = traced_fibonacci(h2w, h2w_api, oracle, consts, 1)
    assert h2w.H2W_TRACE_OUTPUT_FORMS == 8      # (on the parent commit: no such flag)
    kw = FLAG_KW[8 | flags](kh) if flags else {}
    plan = h2w_api.Plan.from_trace(ctx, len(proof), **kw); ctx.close()
    for call in (plan.direct_cells, plan.record_ranges, lambda: plan.set_output_form(h2w_api.FORM_MONTGOMERY)):
        with pytest.raises(h2w_api.H2WError, match="H2W_TRACE_OUTPUT_FORMS"):
            call()
    with pytest.raises(h2w_api.H2WError, match="a traced plan .* writes canonical cells only"):
        plan.set_output_form(h2w_api.FORM_MONTGOMERY)
    plan.set_output_form(h2w_api.FORM_CANONICAL)
    plan.close()
