"""H2W_TRACE_SPLIT_SELECTS on the device: a wide select_by_indicator on 52 to 64 entries replayed as consecutive parts (csrc/replay_lane.h under
H2W_REPLAY_PARTS, the kernel k_replay_parts) writes the stream of the select as one op.

Hand-driven programs (tests/replay_prog.py; those h2w_plan_from_trace refuses without the flag): per proof the whole stream equals the oracle's
bytes, the status word is the integer model's, the cells at the program's handles hold the integer model's values.  Proof i selects entry i mod n
among pairwise distinct entries, so every entry - on either side of every cut, wherever the lowering makes it - is the selected one in some proof.

The PoseidonBN254 verifier at cap_height 6 (64 wide cap entries imported into verify_proof_to_cap_with_cap_index: the shape the flag is for) through
every call that works on a traced plan: flat, Montgomery form, sharded, columns, the keygen lists, verdicts.  The yardsticks are the CPU oracle's
stream, h2w_advice_to_montgomery of it, h2w_layout_columns of it, and the compiled plan's h2w_fri_verdict_batch.  A proof is 830 MB of advice: the
oracle's streams are computed once for the module and compared on the device."""
import ctypes as C

import numpy as np
import pytest

import replay_prog as rp
import verdict_ref as VR
from test_trace_split_selects import IND_PROGRAM, SPLIT, SPLIT_PROGRAMS, VERIFIER_SCOPES, lower, plan_ex

pytestmark = pytest.mark.gpu

MONTGOMERY = 1
NO = 0xFFFFFFFF


# ---------------------------------------------------------------- hand-driven programs
def distinct_entries(i, n):
    """n wide entries of proof i, pairwise distinct: the edges of the field (0, 1, 2^64 +- 1, 2^128 +- 1, 2^253, r - 1) moved apart by the entry's number"""
    v = [(rp.pick(rp.FR_EDGES, i, k) + (k << 96) + (i << 160)) % rp.R for k in range(n)]
    assert len(set(v)) == n
    return v


def make_batch(prog, n_proofs):
    far = prog.fn.__qualname__.startswith("prog_far_operands")
    n = (prog.nwords - 1) // 4 if far else (prog.nwords - 8) // 5
    base = rp.make_far_operands(n) if far else rp.make_lists(n, prog.lookup_bits, True)
    idx_word, first = (4 * n, 0) if far else (0, 8 + n)
    proofs = []
    for i in range(n_proofs):
        p = base(i)
        for k, v in enumerate(distinct_entries(i, n)):
            rp._put_fr(p, first + 4 * k, v)
        p[idx_word] = i % n
        assert len(p) == prog.nwords
        proofs.append(p)
    return proofs


def check_on_device(h2w, api, oracle, prog, proofs, flags=SPLIT):
    """rp.check_on_device on a plan lowered with `flags`"""
    import torch
    lw = lower(h2w, api, prog.fn, prog.proof_a(), flags, prog.lookup_bits, prog.scopes)
    plan, n, W = lw.plan, len(proofs), prog.nwords
    assert plan.trace_op_counts()[rp.tape_enums()["DOP_FR_SELIND"]] >= 2
    d_proofs = torch.from_numpy(np.array(proofs, dtype=np.uint64).reshape(n * W).view(np.int64)).cuda()
    advice = torch.zeros(n * plan.num_cells * 32, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    plan.run(d_proofs.data_ptr(), n, advice.data_ptr(), ws.data_ptr(), st)
    torch.cuda.synchronize()
    status = plan.status(ws.data_ptr(), n, st)
    got = advice.cpu().numpy().view(np.uint64).reshape(n, plan.num_cells, 4)
    plan.close()
    for i, p in enumerate(proofs):
        want_vals, ib = rp.int_run(prog.fn, p)
        assert not ib.unspecified
        stream, cells, vals, entries = rp.oracle_run(oracle, prog.fn, p, prog.lookup_bits, entries=True)
        assert cells == lw.offsets and len(stream) == lw.num_cells * 32
        assert vals == want_vals, f"proof {i}: the oracle's values differ from the integer model"
        rp.compare_on_device(i, got[i], status[i], ib.status(), ib, stream, entries, lw.offsets, want_vals)
    return status


@pytest.mark.parametrize("case", SPLIT_PROGRAMS, ids=lambda c: c[0].name)
def test_a_program_with_a_split_select_replays_to_the_oracles_stream(h2w, h2w_api, oracle, case):
    prog = case[0]
    for n in (1, 70):      # one proof; a batch with a partial second wavefront in which every entry (n <= 64) is selected once
        check_on_device(h2w, h2w_api, oracle, prog, make_batch(prog, n))


def test_an_indicator_that_is_no_bit_in_any_part_of_a_split_select_is_status_5(h2w, h2w_api, oracle):
    """The select on 64 wide entries with its indicators read from the proof (tests/test_trace_split_selects.py IND_PROGRAM: two parts - 64 entries
    are never more).  Proof i with i % 4 != 0 has one entry set and one indicator of 2, 2^32 or p - 1, at position 0, 1, .. 63 in turn: in the first
    part, on either side of the cut wherever the lowering makes it, in the last part.  Status 5, and the cells in front of the select - the loads of
    the entries and of the indicators - are the oracle's.  Its neighbours (i % 4 == 0: one entry set, or three) have status 0 and the whole stream."""
    prog = IND_PROGRAM; n = 64; proofs = []; positions = set()
    for i in range(87):
        p = [0] * prog.nwords
        for k, v in enumerate(distinct_entries(i, n)):
            rp._put_fr(p, 4 * k, v)
        p[4 * n + (7 * i) % n] = 1
        if i % 4 == 0 and i % 8:
            p[4 * n + (7 * i + 20) % n] = p[4 * n + n - 1] = 1      # several entries set: the sum is the field's
        if i % 4:
            pos = (i - i // 4 - 1) % n; positions.add(pos)
            p[4 * n + pos] = rp.OFF_POOL[i % 3]
        proofs.append(p)
    assert positions == set(range(n))
    status = check_on_device(h2w, h2w_api, oracle, prog, proofs)
    assert status == [5 if i % 4 else 0 for i in range(len(proofs))]


# ---------------------------------------------------------------- the PoseidonBN254 verifier at cap_height 6
def _upload(proofs):
    import torch
    return torch.from_numpy(np.concatenate([np.frombuffer(bytes(p), dtype=np.int64) for p in proofs])).cuda()


def _dev(stream_bytes):
    import torch
    return torch.frombuffer(bytearray(stream_bytes), dtype=torch.int64).cuda()


@pytest.fixture(scope="module")
def cap6(h2w, h2w_api, oracle, consts):
    """The shape, the context that recorded the verifier on the proof of seed 61 (witness_gen_only = 0: the keygen lists too), the proofs of seeds
    61 and 62 on the device, the oracle's stream of each and the traced run's own - on the device, [cells x 4] int64."""
    import torch
    ko, kh = consts
    sh = h2w.fibonacci_shape(7, 2, rate_bits=1, hash_mode=1, cap_height=6); osh = oracle.fibonacci_shape(7, 2, rate_bits=1, hash_mode=1, cap_height=6)
    proofs = [oracle.synth_proof(osh, s) for s in (61, 62)]
    ctx = h2w_api.Context(21, False, 0); ctx.trace_begin()
    h2w_api.verify_stark(ctx, sh, kh, np.frombuffer(bytes(proofs[0]), dtype=np.uint64))
    want = []
    for p in proofs:
        o = oracle.Ctx(21, track_scopes=False)
        assert oracle.verify_stark(o, osh, ko, p) == 0
        want.append(_dev(o.advice_bytes()).reshape(-1, 4)); o.close()
    env = dict(sh=sh, osh=osh, ctx=ctx, nwords=len(proofs[0]), d_proofs=_upload(proofs), want=want, traced=_dev(ctx.advice_bytes()).reshape(-1, 4), kh=kh, ko=ko)
    assert want[0].shape[0] == ctx.num_cells()
    yield env
    ctx.close(); env.clear(); torch.cuda.empty_cache()


def _plan(h2w, h2w_api, cap6, flags):
    plan = plan_ex(h2w, h2w_api, cap6["ctx"], cap6["nwords"], VERIFIER_SCOPES, flags, cap6["kh"] if flags & 3 else None)
    assert plan.num_cells == cap6["ctx"].num_cells() and plan.trace_op_counts()[rp.tape_enums()["DOP_FR_SELIND"]] >= 2
    return plan


def _run(plan, d_proofs, n, fill=-1):
    import torch
    adv = torch.full((n, plan.num_cells, 4), fill, dtype=torch.int64, device="cuda"); ws = torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    plan.run(d_proofs.data_ptr(), n, adv.data_ptr(), ws.data_ptr(), st); torch.cuda.synchronize()
    assert plan.status(ws.data_ptr(), n, st) == [0] * n
    return adv


def _assert_stream(got, want, what):
    import torch
    if not torch.equal(got, want):
        bad = torch.nonzero((got != want).any(dim=1)).flatten()
        raise AssertionError(f"{what}: {bad.numel()} cells differ, first at {bad[:8].tolist()}: got {got[bad[0]].tolist()} want {want[bad[0]].tolist()}")


@pytest.mark.parametrize("flags", [SPLIT, SPLIT | 1 | 2], ids=["split", "split+fused"])
def test_the_verifier_with_64_bn254_cap_entries_replays_to_the_oracles_stream(h2w, h2w_api, cap6, flags):
    plan = _plan(h2w, h2w_api, cap6, flags)
    if flags & 2:
        assert plan.trace_info_bn()["fused"] > 0
    adv = _run(plan, cap6["d_proofs"], 2)
    _assert_stream(adv[0], cap6["traced"], "the replay of the traced proof against the traced run itself")
    for i in range(2):
        _assert_stream(adv[i], cap6["want"][i], f"proof {i} against the oracle")
    plan.close()


@pytest.mark.parametrize("flags", [SPLIT | 8, SPLIT | 1 | 2 | 8], ids=["split+forms", "split+fused+forms"])
def test_montgomery_form_is_the_converted_canonical_stream(h2w, h2w_api, cap6, flags):
    import torch
    plan = _plan(h2w, h2w_api, cap6, flags)
    plan.set_output_form(MONTGOMERY)
    got = _run(plan, cap6["d_proofs"], 1)[0]
    want = cap6["want"][0].clone()
    assert plan.L.h2w_advice_to_montgomery(want.data_ptr(), want.shape[0], torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert not torch.equal(want, cap6["want"][0])
    _assert_stream(got, want, "Montgomery form against h2w_advice_to_montgomery of the oracle's stream")
    plan.close()


def test_sharded_calls_columns_and_the_keygen_lists(h2w, h2w_api, cap6):
    """Ranks 0 and 1 of world 2 write disjoint blocks that together are the unsharded stream; the column call equals h2w_layout_columns of the flat
    stream at the plan's own break points, which are the compiled plan's; the gates hold on the stream."""
    import torch
    plan = _plan(h2w, h2w_api, cap6, SPLIT); n = 2; st = torch.cuda.current_stream().cuda_stream
    SENT = -0x0123456789ABCDEF
    want = torch.stack(cap6["want"])
    seen = torch.zeros((n, plan.num_cells), dtype=torch.bool, device="cuda")
    for rank in (0, 1):
        adv = torch.full((n, plan.num_cells, 4), SENT, dtype=torch.int64, device="cuda")
        ws = torch.zeros(plan.shard_workspace_bytes(n, rank, 2), dtype=torch.uint8, device="cuda")
        plan.run_shard(cap6["d_proofs"].data_ptr(), n, adv.data_ptr(), ws.data_ptr(), rank, 2, st); torch.cuda.synchronize()
        assert plan.status(ws.data_ptr(), n, st) == [0] * n
        mine = (adv != SENT).any(dim=2)
        assert not bool((mine & seen).any()), f"rank {rank} wrote cells rank 0 wrote"
        assert torch.equal(adv[mine], want[mine]), f"rank {rank}: its blocks are not the unsharded stream's"
        seen |= mine; del adv
    assert bool(seen.all()), "the two ranks together do not cover the stream"
    del seen
    compiled = h2w_api.Plan(cap6["sh"], cap6["kh"])
    k = 20; bp = plan.break_points(k); ncol = len(bp) + 1
    assert bp == compiled.break_points(k) and plan.selectors() == compiled.selectors() and plan.lookup_cells() == compiled.lookup_cells()
    compiled.close()
    assert plan.check_constraints(want.data_ptr(), n)[0] == 0
    cols = torch.full((((n * ncol) << k), 4), 0x5A5A5A5A, dtype=torch.int64, device="cuda"); ref = torch.full_like(cols, 0x3C3C3C3C)
    ws = torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    plan.run_columns(cap6["d_proofs"].data_ptr(), n, bp, k, cols.data_ptr(), ws.data_ptr(), st)
    plan.layout_columns(want.data_ptr(), n, bp, k, ref.data_ptr(), st)
    torch.cuda.synchronize()
    assert plan.status(ws.data_ptr(), n, st) == [0] * n
    _assert_stream(cols, ref, f"columns of 2^{k} rows against h2w_layout_columns of the flat stream")
    plan.close()


def test_verdicts_are_the_compiled_plans(h2w, h2w_api, oracle, cap6):
    """Valid proofs, copies with one leaf word of the trace tree changed, copies with the PoW witness changed: the four words of every verdict equal
    h2w_fri_verdict_batch on the compiled plan of the shape; the valid proofs are accepted."""
    import torch
    ko, kh, osh = cap6["ko"], cap6["kh"], cap6["osh"]
    compiled = h2w_api.Plan(cap6["sh"], kh); L = compiled.proof_layout()
    valid = [np.frombuffer(bytes(oracle.prove_fri(osh, ko, s)), dtype=np.uint64) for s in (77, 78)]
    leaf = lambda q: L["queries"] + q * L["query_words"] + L["oracles"][0]["off"]
    words = [valid[0], VR.bump(valid[0], leaf(0)), VR.bump(valid[0], L["pow_witness"]), valid[1], VR.bump(valid[1], leaf(1) + 1), VR.bump(valid[1], L["pow_witness"]), valid[0]]
    n = len(words)
    d = torch.from_numpy(np.concatenate(words).view(np.int64)).cuda()
    want = compiled.verdict(d.data_ptr(), n); compiled.close()
    plan = _plan(h2w, h2w_api, cap6, SPLIT)
    assert plan.trace_verdict_info()["available"] == 1
    ws = torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    got = plan.trace_verdict(d.data_ptr(), n, ws.data_ptr())
    plan.close()
    print(want, got)
    assert got == want
    assert got[0] == got[3] == got[6] == (0, 0, NO, 0)
    assert all(g[0] != 0 and g[1] > 0 for g in (got[1], got[2], got[4], got[5])) and got[1][2] == 0 and got[4][2] == 1
