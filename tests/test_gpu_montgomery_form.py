"""H2W_OPT_OUTPUT_FORM = Montgomery: every entry point that generates cells for a compiled plan leaves v * 2^256 mod r in every cell it writes.

The yardstick is never the code under test: the expected bytes are the canonical stream of the same call (pinned to the CPU oracle by
test_gpu_batch.py and its neighbours) put through h2w_advice_to_montgomery (pinned to Python integers by test_montgomery_form_output), compared
over EVERY byte, plus (v << 256) % r in Python on a sample that holds the first and the last 2,000 cells."""
import random

import pytest

pytestmark = pytest.mark.gpu

R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
OPT_CHAIN_PASSES, OPT_VALUES_FORM, OPT_OUTPUT_FORM = 3, 4, 5
CANONICAL, MONTGOMERY = 0, 1


def _shapes(h2w, oracle, d, q, rb=1, mode=1, lookup_bits=21, cap=4, **kw):
    sh = h2w.fibonacci_shape(d, q, rate_bits=rb, cap_height=cap, hash_mode=mode, lookup_bits=lookup_bits)
    osh = oracle.fibonacci_shape(d, q, rate_bits=rb, cap_height=cap, hash_mode=mode, lookup_bits=lookup_bits)
    for k, v in kw.items():
        setattr(sh, k, v); setattr(osh, k, v)
    return sh, osh


def _upload(oracle, osh, plan, seeds, proofs=None):
    import torch
    proofs = proofs or [oracle.synth_proof(osh, s) for s in seeds]
    host = torch.empty(len(proofs) * plan.proof_words, dtype=torch.int64)
    for i, p in enumerate(proofs):
        host[i * plan.proof_words:(i + 1) * plan.proof_words] = torch.frombuffer(bytearray(bytes(p)), dtype=torch.int64)
    return host.cuda()


def _to_int(row):
    return sum(int(x) << (64 * j) for j, x in enumerate(row))


def _check_sample(canon, mont, what):
    """canon, mont: int64 device tensors [cells][4].  Python integers on the first and last 2,000 cells and 2,000 random ones."""
    import torch
    n = canon.shape[0]
    rnd = random.Random(n)
    idx = sorted(set(list(range(min(n, 2000))) + list(range(max(0, n - 2000), n)) + [rnd.randrange(n) for _ in range(2000)]))
    sel = torch.tensor(idx, dtype=torch.int64, device=canon.device)
    a = canon.index_select(0, sel).cpu().numpy().view("uint64"); b = mont.index_select(0, sel).cpu().numpy().view("uint64")
    for i, ra, rb in zip(idx, a, b):
        v = _to_int(ra)
        assert _to_int(rb) == (v << 256) % R_MOD, f"{what}: cell {i} holds {hex(_to_int(rb))}, canonical value {hex(v)}"


def _assert_equal_cells(want, got, what):
    import torch
    if not torch.equal(want, got):
        bad = torch.nonzero((want != got).any(dim=1)).flatten()
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {want.shape[0]} cells differ, first at {bad[:8].tolist()}: got {got[i].tolist()} want {want[i].tolist()}")


def _flat_pair(plan, d_proofs, n, what, expect_status=None):
    """The flat stream of one call in both forms: (canonical, Montgomery) int64 tensors [n * cells][4]; checks every byte and the sample."""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    cells = n * plan.num_cells
    out = []
    status = []
    for form in (CANONICAL, MONTGOMERY):
        plan.set_output_form(form)
        adv = torch.full((cells, 4), -1, dtype=torch.int64, device="cuda")
        ws = torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda")
        plan.run(d_proofs.data_ptr(), n, adv.data_ptr(), ws.data_ptr(), st)
        torch.cuda.synchronize()
        status.append(plan.status(ws.data_ptr(), n, st))
        out.append(adv)
    plan.set_output_form(CANONICAL)
    assert status[0] == status[1] == (expect_status or [0] * n), (what, status)
    canon, mont = out
    want = canon.clone()
    assert plan.L.h2w_advice_to_montgomery(want.data_ptr(), cells, st) == 0
    torch.cuda.synchronize()
    _assert_equal_cells(want, mont, what)
    _check_sample(canon, mont, what)
    return canon, mont


@pytest.mark.parametrize("mode", [1, 0])
def test_small_shapes_every_cell(h2w, h2w_api, oracle, consts, mode):
    """One proof and three: the fast expansion kernel at its three lookup_bits, the generic one (lookup_bits 17), and the canonical stream against the oracle once."""
    ko, kh = consts
    for lb, (d, q, rb) in [(21, (6, 2, 1)), (13, (7, 3, 2)), (8, (6, 2, 1)), (17, (6, 2, 1)), (21, (5, 1, 1))]:
        sh, osh = _shapes(h2w, oracle, d, q, rb, mode, lb)
        plan = h2w_api.Plan(sh, kh)
        for seeds in ([21], [22, 23, 24]):
            proofs = [oracle.synth_proof(osh, s) for s in seeds]
            canon, _ = _flat_pair(plan, _upload(oracle, osh, plan, seeds, proofs), len(seeds), f"mode {mode} lookup_bits {lb} seeds {seeds}")
        ctx = oracle.Ctx(lb)
        assert oracle.verify_stark(ctx, osh, ko, proofs[-1]) == 0
        assert ctx.advice_bytes() == canon[-plan.num_cells:].cpu().numpy().tobytes()
        ctx.close(); plan.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_shape_variants(h2w, h2w_api, oracle, consts, mode):
    """The arity / cap-height / column-count variants of test_gpu_batch.test_shape_edge_cases."""
    ko, kh = consts
    cases = [dict(d=6, q=2, n_perm_z=0), dict(d=6, q=1, cap=0), dict(d=8, q=2, rb=2, cap=2, arity_bits=2, final_poly_bits=3),
             dict(d=6, q=2, pow_bits=10, n_cols=6, n_quotient=4, n_pis=1, num_challenges=3), dict(d=9, q=2, rb=3, cap=1, arity_bits=3),
             dict(d=5, q=2, cap=1, arity_bits=1, final_poly_bits=2)]
    for kw in cases:
        kw = dict(kw); sh, osh = _shapes(h2w, oracle, kw.pop("d"), kw.pop("q"), kw.pop("rb", 1), mode, 21, kw.pop("cap", 4), **kw)
        plan = h2w_api.Plan(sh, kh)
        _flat_pair(plan, _upload(oracle, osh, plan, [11, 12]), 2, f"mode {mode} {kw}")
        plan.close()


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("passes,form", [(1, 0), (2, 1), (2, 2)])
def test_batch_on_the_roaming_grid(h2w, h2w_api, oracle, consts, mode, passes, form):
    """A batch whose proofs have more than 16 work units each (the roaming grid of expand_fast), with the Merkle paths in one pass and in two,
    the values pass in both of its forms."""
    ko, kh = consts
    sh, osh = _shapes(h2w, oracle, 8, 4, 1, mode)
    plan = h2w_api.Plan(sh, kh)
    assert plan.num_records > 16 * 256      # (expand.hip launch_expand: at least 16 work units of 256 records per proof)
    plan.configure(OPT_CHAIN_PASSES, passes)
    if form:
        plan.configure(OPT_VALUES_FORM, form)
    _flat_pair(plan, _upload(oracle, osh, plan, list(range(300, 304))), 4, f"mode {mode} passes {passes} values form {form}")
    plan.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_columns(h2w, h2w_api, oracle, consts, mode):
    """run_columns in Montgomery form = run_columns canonical converted cell by cell: repeated boundary cells, zero unused rows.  k = 12: a column boundary every ~4,000 cells, thousands of columns (the generic expansion
    kernel); k = 18: a few dozen columns (expand_fast's column form).  Either way most boundaries fall inside a record."""
    import torch
    ko, kh = consts
    sh, osh = _shapes(h2w, oracle, 7, 3, 2, mode)
    plan = h2w_api.Plan(sh, kh)
    n = 3; d_proofs = _upload(oracle, osh, plan, [61, 62, 63])
    st = torch.cuda.current_stream().cuda_stream
    for k in (12, 18):
        bp = plan.break_points(k); ncol = len(bp) + 1
        assert ncol > 2 and (k != 18 or ncol <= 64)
        rr = plan.record_ranges().astype("int64"); starts = [0]
        for b in bp:
            starts.append(starts[-1] + b)
        assert sum(1 for s in starts[1:] if ((rr[:, 0] < s) & (rr[:, 0] + rr[:, 1] > s)).any()) >= 2, "no record straddles a column boundary"
        res = []
        for f in (CANONICAL, MONTGOMERY):
            plan.set_output_form(f)
            cols = torch.full(((n * ncol) << k, 4), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
            ws = torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda")
            plan.run_columns(d_proofs.data_ptr(), n, bp, k, cols.data_ptr(), ws.data_ptr(), st)
            torch.cuda.synchronize()
            assert plan.status(ws.data_ptr(), n, st) == [0] * n
            res.append(cols)
        plan.set_output_form(CANONICAL)
        want = res[0].clone()
        assert plan.L.h2w_advice_to_montgomery(want.data_ptr(), want.shape[0], st) == 0
        torch.cuda.synchronize()
        _assert_equal_cells(want, res[1], f"columns k={k} mode {mode}")
        _check_sample(res[0], res[1], f"columns k={k} mode {mode}")
        rows = 1 << k
        for c, b in enumerate(bp):      # the repeated boundary cell, converted once: (c, last) == (c + 1, 0)
            assert torch.equal(res[1][c * rows + b], res[1][(c + 1) * rows]) and bool((res[1][c * rows + b + 1:(c + 1) * rows] == 0).all())
    plan.close()


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("world", [2, 8])
def test_sharding(h2w, h2w_api, oracle, consts, mode, world):
    """Plain and packed: a rank's blocks equal the converted full stream at h2w_plan_shard_block's offsets; everything else keeps its sentinel."""
    import torch
    ko, kh = consts
    sh, osh = _shapes(h2w, oracle, 7, 5, 2, mode)
    plan = h2w_api.Plan(sh, kh)
    n = 5; d_proofs = _upload(oracle, osh, plan, [140 + i for i in range(n)])
    st = torch.cuda.current_stream().cuda_stream
    _, full = _flat_pair(plan, d_proofs, n, f"unsharded mode {mode}")
    full = full.reshape(n, plan.num_cells, 4)
    plan.set_output_form(MONTGOMERY)
    SENT = -0x0123456789ABCDEF
    for rank in range(world):
        cells = plan.shard_cells(n, rank, world)
        packed = torch.full((cells + 8, 4), SENT, dtype=torch.int64, device="cuda")
        ws = torch.zeros(plan.shard_workspace_bytes(n, rank, world), dtype=torch.uint8, device="cuda")
        plan.run_shard_compact(d_proofs.data_ptr(), n, packed.data_ptr(), ws.data_ptr(), rank, world, st)
        plain = torch.full((n, plan.num_cells, 4), SENT, dtype=torch.int64, device="cuda")
        ws2 = torch.zeros(plan.shard_workspace_bytes(n, rank, world), dtype=torch.uint8, device="cuda")
        plan.run_shard(d_proofs.data_ptr(), n, plain.data_ptr(), ws2.data_ptr(), rank, world, st)
        torch.cuda.synchronize()
        assert plan.status(ws.data_ptr(), n, st) == [0] * n and plan.status(ws2.data_ptr(), n, st) == [0] * n
        used = torch.zeros(cells + 8, dtype=torch.bool, device="cuda"); owned = torch.zeros((n, plan.num_cells), dtype=torch.bool, device="cuda")
        for p_ in range(n):
            for q in range(-1, sh.num_queries):
                blk = plan.shard_block(rank, world, p_, q)
                if blk is None:
                    continue
                lo, cnt, g = blk
                _assert_equal_cells(full[p_, g:g + cnt], packed[lo:lo + cnt], f"packed rank {rank}/{world} proof {p_} query {q}")
                _assert_equal_cells(full[p_, g:g + cnt], plain[p_, g:g + cnt], f"plain rank {rank}/{world} proof {p_} query {q}")
                used[lo:lo + cnt] = True; owned[p_, g:g + cnt] = True
        assert bool((packed[~used] == SENT).all()), f"rank {rank}/{world}: packed buffer touched outside its blocks"
        assert bool((plain[~owned] == SENT).all()), f"rank {rank}/{world}: blocks of other ranks touched"
    plan.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_full_size_config3(h2w, h2w_api, oracle, consts, mode):
    """cfg 3 (2^20 rows, 28 queries), one proof: whole-stream equality on the device."""
    ko, kh = consts
    sh, osh = _shapes(h2w, oracle, 20, 28, 1, mode)
    plan = h2w_api.Plan(sh, kh)
    _flat_pair(plan, _upload(oracle, osh, plan, [0xF1B00003]), 1, f"cfg 3 mode {mode}")
    plan.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_noncanonical_proof_words(h2w, h2w_api, oracle, consts, mode):
    """Status 4 (test_gpu_batch.test_noncanonical_proof_words_are_flagged) in both forms, cells = the converted canonical stream."""
    ko, kh = consts
    P = 2**64 - 2**32 + 1
    sh, osh = _shapes(h2w, oracle, 6, 2, 1, mode)
    plan = h2w_api.Plan(sh, kh)
    rnd = random.Random(3)
    pr = oracle.synth_proof(osh, 101)
    for _ in range(10):
        pr[rnd.randrange(len(pr))] = rnd.choice([P, P + 1, 2**64 - 1])
    _flat_pair(plan, _upload(oracle, osh, plan, None, [pr]), 1, f"non-canonical words, mode {mode}", expect_status=[4])
    plan.close()


def test_option_handling(h2w, h2w_api, oracle, consts):
    import numpy as np
    import torch
    ko, kh = consts
    sh, osh = _shapes(h2w, oracle, 6, 2, 1, 1)
    st = torch.cuda.current_stream().cuda_stream
    plan = h2w_api.Plan(sh, kh); other = h2w_api.Plan(sh, kh)
    for bad in (2, -1):
        with pytest.raises(h2w_api.H2WError, match="OUTPUT_FORM"):
            plan.configure(OPT_OUTPUT_FORM, bad)
    d_proofs = _upload(oracle, osh, plan, [7])

    def run(p):
        adv = torch.zeros((p.num_cells, 4), dtype=torch.int64, device="cuda"); ws = torch.zeros(p.workspace_bytes(1), dtype=torch.uint8, device="cuda")
        p.run(d_proofs.data_ptr(), 1, adv.data_ptr(), ws.data_ptr(), st); torch.cuda.synchronize()
        return adv
    fresh = run(other)                        # a plan that never saw the option
    plan.set_output_form(h2w_api.FORM_MONTGOMERY)
    m1 = run(plan); c_other = run(other)      # two plans of different forms side by side
    plan.set_output_form(h2w_api.FORM_CANONICAL)
    back = run(plan)
    assert torch.equal(fresh, c_other) and torch.equal(fresh, back) and not torch.equal(fresh, m1)
    other.set_output_form(MONTGOMERY)
    assert torch.equal(run(other), m1) and torch.equal(run(plan), fresh)
    plan.close(); other.close()
    # a traced plan refuses the form and keeps writing canonical cells
    pr = oracle.synth_proof(osh, 7)
    tctx = h2w_api.Context(21, True, 0); tctx.trace_begin()
    h2w_api.verify_stark(tctx, sh, kh, np.frombuffer(bytes(pr), dtype=np.uint64))
    rplan = h2w_api.Plan.from_trace(tctx, len(pr)); tctx.close()
    with pytest.raises(h2w_api.H2WError, match="traced"):
        rplan.set_output_form(MONTGOMERY)
    rplan.set_output_form(CANONICAL)
    radv = torch.zeros((rplan.num_cells, 4), dtype=torch.int64, device="cuda"); rws = torch.zeros(rplan.workspace_bytes(1), dtype=torch.uint8, device="cuda")
    rplan.run(d_proofs.data_ptr(), 1, radv.data_ptr(), rws.data_ptr(), st); torch.cuda.synchronize()
    assert torch.equal(radv, fresh)
    rplan.close()
