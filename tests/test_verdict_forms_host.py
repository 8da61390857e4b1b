"""The host side of h2w_fri_verdict_batch_ex and h2w_plan_verdict_form (include/h2w.h 3b; no GPU): the symbols are declared and exported with the
binding's signatures; every refusal of `flags` comes before any device work - so it is the answer on a machine without a device too - and names
its reason; what FORM_AUTO resolves to: the one kernel there is with Goldilocks caps at any size, with PoseidonBN254 caps the wavefront-per-path form
up to a crossover in Merkle paths and the four-lane form beyond it.  The crossover is read back by bisection and not restated here: it must be one
threshold in n_proofs x num_queries x trees, the same for every shape."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(h2w, h2w_api, consts, mode, degree_bits=6, queries=2, **over):
    sh = h2w.fibonacci_shape(degree_bits, queries, rate_bits=1, cap_height=2, hash_mode=mode)
    for k, v in over.items():
        setattr(sh, k, v)
    return h2w_api.Plan(sh, consts[1])


def _trees(plan):
    L = plan.proof_layout()
    return len(L["oracles"]) + len(L["steps"])


def test_the_symbols_are_declared_exported_and_bound(h2w, h2w_api):
    header = open(os.path.join(ROOT, "include", "h2w.h")).read()
    assert re.search(r"int h2w_fri_verdict_batch_ex\(h2w_plan \*, const uint64_t \*proofs_dev, uint64_t n_proofs,\s*h2w_verdict_t \*verdict_dev, void \*stream, uint32_t flags\);", header)
    assert re.search(r"int h2w_plan_verdict_form\(const h2w_plan \*, uint64_t n_proofs\);", header)
    for name, value in (("AUTO", 0), ("QUAD", 1), ("ROW", 2), ("MASK", 0xFF)):
        m = re.search(r"#define H2W_VERDICT_FORM_%s\s+(\w+)u" % name, header)
        assert m and int(m.group(1), 0) == value == getattr(h2w, "H2W_VERDICT_FORM_" + name)
    m = re.search(r"#define H2W_VERDICT_FORK\s+(\w+)u", header)
    assert m and int(m.group(1), 0) == 0x100 == h2w.H2W_VERDICT_FORK == h2w_api.VERDICT_FORK
    assert (h2w_api.VERDICT_FORM_AUTO, h2w_api.VERDICT_FORM_QUAD, h2w_api.VERDICT_FORM_ROW) == (0, 1, 2)
    L = h2w.lib()
    ex, form = L.h2w_fri_verdict_batch_ex, L.h2w_plan_verdict_form      # (exported: ctypes resolves them)
    assert ex.restype is C.c_int and list(ex.argtypes) == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32]
    assert form.restype is C.c_int and list(form.argtypes) == [C.c_void_p, C.c_uint64]


def test_a_null_plan_is_refused(h2w):
    L = h2w.lib()
    out = (C.c_uint32 * 4)(); words = (C.c_uint64 * 4)()
    assert L.h2w_fri_verdict_batch_ex(None, C.addressof(words), 1, C.addressof(out), None, 0) == -1
    assert "h2w_fri_verdict_batch_ex: null plan" in h2w.last_error()
    assert L.h2w_plan_verdict_form(None, 1) == -1
    assert "h2w_plan_verdict_form: null plan" in h2w.last_error()


@pytest.mark.parametrize("mode", [1, 0])
def test_every_refusal_of_flags_names_its_reason(h2w, h2w_api, consts, mode):
    """Before any device work: the answers are the same with and without a device, and the verdict buffer is host memory nobody may touch."""
    plan = _plan(h2w, h2w_api, consts, mode)
    words = (C.c_uint64 * plan.proof_words)(); out = (C.c_uint32 * 4)(*([0x5A5A5A5A] * 4))
    call = lambda flags, n=1: plan.verdict(C.addressof(words), n, verdict_ptr=C.addressof(out), flags=flags)
    for stray in (0x200, 0x80000000, h2w_api.VERDICT_FORM_ROW | h2w_api.VERDICT_FORK | 0x1000):
        with pytest.raises(h2w_api.H2WError, match="h2w_fri_verdict_batch_ex: unknown flag bits %d" % (stray & ~0x1FF)):
            call(stray)
    for form in (3, 0xFF, 3 | h2w_api.VERDICT_FORK):
        with pytest.raises(h2w_api.H2WError, match="h2w_fri_verdict_batch_ex: unknown form %d" % (form & 0xFF)):
            call(form)
    if mode == 0:
        for f in (h2w_api.VERDICT_FORM_ROW, h2w_api.VERDICT_FORM_ROW | h2w_api.VERDICT_FORK):
            with pytest.raises(h2w_api.H2WError, match="H2W_VERDICT_FORM_ROW is a PoseidonBN254 form and the plan's hash_mode is 0"):
                call(f)
            with pytest.raises(h2w_api.H2WError, match="hash_mode is 0"):
                call(f, 0)      # (a refusal of the flags, not of the batch: no proof changes it)
    with pytest.raises(h2w_api.H2WError, match="unknown flag bits"):
        call(0x200, 0)
    assert list(out) == [0x5A5A5A5A] * 4
    if h2w.lib().h2w_device_count() == 0:      # accepted flags reach the device check, under the entry point's own name
        for f in (0, 1, h2w_api.VERDICT_FORK) + ((2, 2 | h2w_api.VERDICT_FORK) if mode == 1 else ()):
            with pytest.raises(h2w_api.H2WError, match="h2w_fri_verdict_batch_ex: no HIP device"):
                call(f)
    plan.close()


def test_a_traced_plan_is_refused(h2w, h2w_api, oracle):
    osh = oracle.fibonacci_shape(6, 2, rate_bits=1, hash_mode=1, cap_height=2)
    sh = h2w.fibonacci_shape(6, 2, rate_bits=1, hash_mode=1, cap_height=2)
    proof = oracle.synth_proof(osh, 43)
    ctx = h2w_api.Context(21, True, 0); ctx.trace_begin()
    h2w_api.verify_stark(ctx, sh, h2w.published_consts(), np.frombuffer(bytes(proof), dtype=np.uint64))
    rplan = h2w_api.Plan.from_trace(ctx, len(proof)); ctx.close()
    words = (C.c_uint64 * len(proof))(); out = (C.c_uint32 * 4)()
    for flags in (h2w_api.VERDICT_FORM_AUTO, h2w_api.VERDICT_FORM_QUAD, h2w_api.VERDICT_FORM_ROW | h2w_api.VERDICT_FORK):
        with pytest.raises(h2w_api.H2WError, match="h2w_fri_verdict_batch_ex: a traced plan"):
            rplan.verdict(C.addressof(words), 1, verdict_ptr=C.addressof(out), flags=flags)
    with pytest.raises(h2w_api.H2WError, match="h2w_plan_verdict_form: a traced plan"):
        rplan.verdict_form(1)
    assert h2w.lib().h2w_plan_verdict_form(rplan.p, 1) == -1
    rplan.close()


def test_auto_is_the_one_kernel_with_goldilocks_caps_at_any_size(h2w, h2w_api, consts):
    plan = _plan(h2w, h2w_api, consts, 0)
    for n in (0, 1, 2, 7, 64, 1 << 20, (1 << 64) - 1):
        assert plan.verdict_form(n) == h2w_api.VERDICT_FORM_QUAD
    plan.close()


def _last_row_batch(h2w_api, plan):
    """The largest n_proofs FORM_AUTO gives the wavefront-per-path form, by bisection; the decision is monotone (checked on the way)."""
    assert plan.verdict_form(1) == h2w_api.VERDICT_FORM_ROW, "one proof of a small shape is below any crossover"
    lo, hi = 1, 1 << 40
    assert plan.verdict_form(hi) == h2w_api.VERDICT_FORM_QUAD and plan.verdict_form((1 << 64) - 1) == h2w_api.VERDICT_FORM_QUAD
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if plan.verdict_form(mid) == h2w_api.VERDICT_FORM_ROW:
            lo = mid
        else:
            hi = mid
    return lo


def test_auto_switches_at_one_crossover_in_merkle_paths(h2w, h2w_api, consts):
    """ROW below, QUAD above, for PoseidonBN254 caps; the crossover read off three shapes with different paths per proof is one number of paths:
    floor(crossover / paths per proof) proofs are the last ROW batch of every shape."""
    found = []
    for queries, over in ((2, {}), (3, {}), (5, dict(n_perm_z=0))):
        plan = _plan(h2w, h2w_api, consts, 1, queries=queries, **over)
        per_proof = queries * _trees(plan)
        n = _last_row_batch(h2w_api, plan)
        for k in (1, 2, n // 2, n - 1, n):
            assert k < 1 or plan.verdict_form(k) == h2w_api.VERDICT_FORM_ROW
        for k in (n + 1, n + 2, 2 * n, 1000 * n):
            assert plan.verdict_form(k) == h2w_api.VERDICT_FORM_QUAD
        found.append((per_proof, n))      # crossover in [n * per_proof, (n + 1) * per_proof)
        plan.close()
    lo = max(n * per for per, n in found); hi = min((n + 1) * per for per, n in found)
    print("paths per proof, last ROW batch:", found, "-> crossover in [%d, %d)" % (lo, hi))
    assert lo < hi, "the three shapes do not switch at one path count"
