"""H2W_TRACE_OUTPUT_FORMS on the device: a traced plan lowered with the flag writes its stream in Montgomery form (H2W_OPT_OUTPUT_FORM) through every
entry point that works on a traced plan - flat, columns, sharded, packed.

The yardstick is never the code under test: the expected bytes are the SAME plan's canonical stream (pinned to the CPU oracle by test_gpu_replay*.py)
put through h2w_advice_to_montgomery (pinned to Python integers by test_gpu_batch.py test_montgomery_form_output), compared over every byte, plus
(v << 256) % r in Python on the first and last 2,000 cells and 2,000 random ones (the helpers of tests/test_gpu_montgomery_form.py, which hold a
compiled plan to the same yardstick)."""
import random

import numpy as np
import pytest

import replay_prog as RP
from test_gpu_montgomery_form import CANONICAL, MONTGOMERY, R_MOD, _assert_equal_cells, _check_sample, _flat_pair, _to_int
from test_trace_output_forms_host import FLAG_KW, traced_fibonacci

pytestmark = pytest.mark.gpu

SHAPES = {"A": dict(d=6, q=2, rb=1, cap=4, lookup_bits=21), "B": dict(d=7, q=3, rb=2, cap=4, lookup_bits=13)}


def _upload(proofs):
    import torch
    return torch.from_numpy(np.concatenate([np.frombuffer(bytes(p), dtype=np.int64) for p in proofs])).cuda()


def _plans(h2w, h2w_api, oracle, consts, mode, flags, seeds, witness_gen_only=True, with_base=False, **shape):
    """The verifier traced on one proof and lowered with `flags` (8 set); proofs of other seeds, uploaded -> (plan[, the plan without 8], proofs on the device)"""
    ko, kh = consts
    ctx, proof_a = traced_fibonacci(h2w, h2w_api, oracle, consts, mode, seed=41, witness_gen_only=witness_gen_only, **shape)
    plan = h2w_api.Plan.from_trace(ctx, len(proof_a), output_forms=True, **FLAG_KW[flags](kh))
    base = h2w_api.Plan.from_trace(ctx, len(proof_a), **FLAG_KW[flags](kh)) if with_base else None
    ctx.close()
    osh = oracle.fibonacci_shape(shape["d"], shape["q"], rate_bits=shape["rb"], cap_height=shape.get("cap", 4), hash_mode=mode, lookup_bits=shape.get("lookup_bits", 21))
    d_proofs = _upload([oracle.synth_proof(osh, s) for s in seeds])
    return (plan, base, d_proofs) if with_base else (plan, d_proofs)


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("flags", sorted(FLAG_KW))
def test_flat_every_byte(h2w, h2w_api, oracle, consts, flags, mode, shape):
    """One proof and three, none of them the traced one: status 0 in both forms, Montgomery == the converted canonical stream, the Python sample."""
    plan, d_proofs = _plans(h2w, h2w_api, oracle, consts, mode, flags, [21, 22, 23, 24], **SHAPES[shape])
    if flags & 2:
        assert (plan.trace_info_bn()["fused"] > 0) == (mode == 1)
    W = plan.proof_words
    _flat_pair(plan, d_proofs[:W], 1, f"flags {flags} mode {mode} shape {shape}, 1 proof")
    _flat_pair(plan, d_proofs[W:], 3, f"flags {flags} mode {mode} shape {shape}, 3 proofs")
    plan.close()


def test_switching_the_form_and_a_plan_beside_it(h2w, h2w_api, oracle, consts):
    """canonical -> Montgomery -> canonical on one plan gives the first stream again; a plan of the same trace without the flag, run in between, is not
    touched by any of it (and still refuses the form)."""
    import torch
    plan, other, d_proofs = _plans(h2w, h2w_api, oracle, consts, 1, 11, [7, 8], with_base=True, **SHAPES["A"])
    st = torch.cuda.current_stream().cuda_stream

    def run(p):
        adv = torch.full((2 * p.num_cells, 4), -1, dtype=torch.int64, device="cuda"); ws = torch.zeros(p.workspace_bytes(2), dtype=torch.uint8, device="cuda")
        p.run(d_proofs.data_ptr(), 2, adv.data_ptr(), ws.data_ptr(), st); torch.cuda.synchronize()
        assert p.status(ws.data_ptr(), 2, st) == [0, 0]
        return adv
    first = run(plan); fresh = run(other)
    assert torch.equal(first, fresh)
    plan.set_output_form(MONTGOMERY)
    m1 = run(plan); beside = run(other)
    plan.set_output_form(CANONICAL)
    back = run(plan)
    assert torch.equal(back, first) and torch.equal(beside, fresh) and not torch.equal(m1, first)
    want = first.clone()
    assert plan.L.h2w_advice_to_montgomery(want.data_ptr(), want.shape[0], st) == 0
    torch.cuda.synchronize()
    _assert_equal_cells(want, m1, "Montgomery form between two canonical calls")
    plan.set_output_form(MONTGOMERY)
    assert torch.equal(run(plan), m1)
    with pytest.raises(h2w_api.H2WError, match="H2W_TRACE_OUTPUT_FORMS"):
        other.set_output_form(MONTGOMERY)
    assert torch.equal(run(other), fresh)
    plan.close(); other.close()


# words: 0 n0, 1 n1, 2.. h0, 6.. h1, 10 a selector bit, 11 a canonical word
WIDE_K = [2**200 + 7 * 2**64 + 5, R_MOD - 1, 2**253 + 1]


def _prog_cells(b):
    """Hand-written: wide literal cells, wide witnesses, gates, selects of one- and four-word values, check_less_than_safe (the -2^rb constant)."""
    n0, n1, h0, h1, s, c = b.nat_in(0), b.nat_in(1), b.hash_in(2), b.hash_in(6), b.nat_in(10), b.nat_in(11)
    ks = [b.const(v) for v in WIDE_K]; zero, one = b.const(0), b.const(1)
    g = b.mul_add(n0, n1, n0)
    out = [g, b.mul(h0, ks[0]), b.add(h1, ks[1]), b.mul_add(ks[2], h0, h1), b.add(g, ks[0])]
    for sel in (s, zero, one):
        out += [b.select(n0, n1, sel), b.select(h0, ks[1], sel), b.select(ks[2], g, sel)]
    b.check_less_than_safe(c, RP.P); b.check_less_than_safe(n0, RP.P)
    out += b.decompose_le(h1, 56, 5)
    return out + ks


def _make_cells(i):
    p = [RP.pick(RP.GL_EDGES, i, 0), RP.pick(RP.GL_EDGES, i, 1)] + [0] * 8 + [(i // 3) & 1, RP.pick(RP.GL_EDGES, i, 11)]
    RP._put_fr(p, 2, RP.pick(RP.FR_EDGES, i, 2)); RP._put_fr(p, 6, RP.pick(RP.FR_EDGES, i, 3))
    return p


@pytest.mark.parametrize("lookup_bits", [8, 17])
def test_hand_written_program_at_lookup_bits_8_and_17(h2w, h2w_api, lookup_bits):
    """lookup_bits 17 expands through the generic kernel, 8 through the fast one; 70 proofs: more than a wavefront of lanes."""
    import torch
    tb = RP.TraceBackend(h2w, h2w_api, RP.safe_proof(12), lookup_bits)
    _prog_cells(tb)
    plan = h2w_api.Plan.from_trace(tb.ctx, 12, parallel_scopes=(), output_forms=True); tb.ctx.close()
    direct = np.unpackbits(plan.direct_cells(), bitorder="little")[:plan.num_cells]
    assert 0 < int(direct.sum()) < plan.num_cells and plan.num_records > 0
    n = 70
    proofs = [_make_cells(i) for i in range(n)]
    assert {RP.int_run(_prog_cells, p)[1].status() for p in proofs} == {0}
    d_proofs = torch.from_numpy(np.array(proofs, dtype=np.uint64).reshape(-1).view(np.int64)).cuda()
    _flat_pair(plan, d_proofs, n, f"hand-written program, lookup_bits {lookup_bits}")
    plan.close()


@pytest.mark.parametrize("k", [12, 18])
@pytest.mark.parametrize("mode", [1, 0])
def test_columns(h2w, h2w_api, oracle, consts, mode, k):
    """h2w_fri_witness_batch_columns: Montgomery columns == canonical columns converted; every boundary cell equals its repeat, unused rows are zero.
    Shape B; with Goldilocks caps its stream at lookup_bits 13 needs more than the call's 4,096 columns of 2^12 rows, so that one case runs the
    shape at lookup_bits 21 (the stream of tests/test_gpu_montgomery_form.py test_columns)."""
    import torch
    shape = dict(SHAPES["B"], lookup_bits=21) if (mode, k) == (0, 12) else SHAPES["B"]
    plan, d_proofs = _plans(h2w, h2w_api, oracle, consts, mode, 11, [61, 62, 63], witness_gen_only=False, **shape)
    n = 3; st = torch.cuda.current_stream().cuda_stream
    bp = plan.break_points(k); ncol = len(bp) + 1; rows = 1 << k
    assert ncol >= 2
    res = []
    for f in (CANONICAL, MONTGOMERY):
        plan.set_output_form(f)
        cols = torch.full(((n * ncol) << k, 4), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
        ws = torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda")
        plan.run_columns(d_proofs.data_ptr(), n, bp, k, cols.data_ptr(), ws.data_ptr(), st)
        torch.cuda.synchronize()
        assert plan.status(ws.data_ptr(), n, st) == [0] * n
        res.append(cols)
    want = res[0].clone()
    assert plan.L.h2w_advice_to_montgomery(want.data_ptr(), want.shape[0], st) == 0
    torch.cuda.synchronize()
    _assert_equal_cells(want, res[1], f"columns k={k} mode {mode}")
    _check_sample(res[0], res[1], f"columns k={k} mode {mode}")
    for p_ in range(n):
        for c, b in enumerate(bp):
            lo = (p_ * ncol + c) * rows
            assert torch.equal(res[1][lo + b], res[1][lo + rows]), f"proof {p_} column {c}: the boundary cell is not its repeat"
            assert bool((res[1][lo + b + 1:lo + rows] == 0).all()), f"proof {p_} column {c}: unused rows are not zero"
    plan.close()


@pytest.mark.parametrize("world", [2, 8])
@pytest.mark.parametrize("mode", [1, 0])
def test_sharding(h2w, h2w_api, oracle, consts, mode, world):
    """Plain and packed: a rank's blocks equal the converted unsharded stream at h2w_plan_shard_block's offsets; everything else keeps its sentinel."""
    import torch
    n = 5
    plan, d_proofs = _plans(h2w, h2w_api, oracle, consts, mode, 11, [140 + i for i in range(n)], d=7, q=5, rb=2)
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
            for q in range(-1, 5):
                blk = plan.shard_block(rank, world, p_, q)
                if blk is None:
                    continue
                lo, cnt, g = blk
                _assert_equal_cells(full[p_, g:g + cnt], packed[lo:lo + cnt], f"packed rank {rank}/{world} proof {p_} query {q}")
                _assert_equal_cells(full[p_, g:g + cnt], plain[p_, g:g + cnt], f"plain rank {rank}/{world} proof {p_} query {q}")
                used[lo:lo + cnt] = True; owned[p_, g:g + cnt] = True
        assert bool(used.any()) or cells == 0
        assert bool((packed[~used] == SENT).all()), f"rank {rank}/{world}: packed buffer touched outside its blocks"
        assert bool((plain[~owned] == SENT).all()), f"rank {rank}/{world}: blocks of other ranks touched"
    plan.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_noncanonical_proof_words(h2w, h2w_api, oracle, consts, mode):
    """Status 4 with the seeding of test_gpu_montgomery_form.test_noncanonical_proof_words: the status words do not depend on the form; a cell whose
    canonical value is below r is byte-equal to its conversion, a cell loaded from a hash at or above r is congruent to it modulo r."""
    import torch
    P = 2**64 - 2**32 + 1
    ko, kh = consts
    ctx, proof_a = traced_fibonacci(h2w, h2w_api, oracle, consts, mode, seed=41)
    plan = h2w_api.Plan.from_trace(ctx, len(proof_a), output_forms=True, **FLAG_KW[11](kh)); ctx.close()
    osh = oracle.fibonacci_shape(6, 2, rate_bits=1, cap_height=4, hash_mode=mode, lookup_bits=21)
    rnd = random.Random(3)
    pr = oracle.synth_proof(osh, 101)
    for _ in range(10):
        pr[rnd.randrange(len(pr))] = rnd.choice([P, P + 1, 2**64 - 1])
    d_proofs = _upload([pr]); st = torch.cuda.current_stream().cuda_stream
    out, status = [], []
    for form in (CANONICAL, MONTGOMERY):
        plan.set_output_form(form)
        adv = torch.full((plan.num_cells, 4), -1, dtype=torch.int64, device="cuda"); ws = torch.zeros(plan.workspace_bytes(1), dtype=torch.uint8, device="cuda")
        plan.run(d_proofs.data_ptr(), 1, adv.data_ptr(), ws.data_ptr(), st); torch.cuda.synchronize()
        status.append(plan.status(ws.data_ptr(), 1, st)); out.append(adv)
    assert status[0] == status[1] == [4]
    canon, mont = out
    want = canon.clone()
    assert plan.L.h2w_advice_to_montgomery(want.data_ptr(), want.shape[0], st) == 0
    torch.cuda.synchronize()
    differ = torch.nonzero((want != mont).any(dim=1)).flatten().tolist()
    assert len(differ) <= 64, f"{len(differ)} cells differ from the converted canonical stream"
    c_h = canon.cpu().numpy().view("uint64"); m_h = mont.cpu().numpy().view("uint64")
    for i in differ:
        v = _to_int(c_h[i])
        assert v >= R_MOD, f"cell {i}: canonical value {hex(v)} is below r and its Montgomery form differs from the conversion"
        assert _to_int(m_h[i]) % R_MOD == (v << 256) % R_MOD, f"cell {i}: not congruent to the canonical value times 2^256"
    plan.close()


def test_full_size_config3(h2w, h2w_api, oracle, consts):
    """cfg 3 (2^20 rows, 28 queries) with PoseidonBN254 caps, both fuse flags, one proof: whole-stream equality on the device."""
    plan, d_proofs = _plans(h2w, h2w_api, oracle, consts, 1, 11, [0xF1B00013], d=20, q=28, rb=1)
    assert plan.trace_info_bn()["fused"] > 0
    _flat_pair(plan, d_proofs, 1, "cfg 3, PoseidonBN254 caps, flags 8|3")
    plan.close()
