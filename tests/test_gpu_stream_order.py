"""Every stream-taking call held to the stream order its header promises (include/h2w.h), by the protocol of tests/stream_order.py: the inputs hold a
second valid set B except between a delayed copy of A and a copy back, all on a non-blocking stream S, and the outputs are snapshotted on S right behind
the call.  A launch that escapes to stream 0, a side stream that starts without waiting for S or that S never waits for, shows as the words of B or as
sentinels; a host wait inside a call that promises none shows as `blocked`.  Every comparison is of exact integers against the oracle's words for A,
which differ from its words for B in every compared output.

First the harness on stand-ins of torch ops (it reports each fault class under this machine's queue setting), then the library's calls:
   h2w_merkle_build; build -> h2w_merkle_open -> h2w_chipbatch_values          in, out, no sync
   h2w_chipbatch_values                                                        in, out, no sync
   h2w_chipbatch_run (field op, hash op with three internal launches)          in, out; blocked printed (the header is silent)
   h2w_fri_witness_batch / _batch2 under the scheduling options                in, out (advice, status words), no sync ("returns after enqueueing")
   h2w_fri_witness_batch_shard, one rank of two                                in, out (its blocks; sentinels elsewhere), no sync
   h2w_fri_verdict_batch / _ex in every form, forked and not                   in, out, no sync
   a traced plan's witness call, then h2w_trace_verdict_batch                  in, out; the verdict call: no sync
   witness -> h2w_advice_digest -> h2w_advice_to_montgomery                    in, out
   h2w_prove_fri_batch                                                         in, out (its header says it synchronises)
Warm-up: every call runs once with the same n on the null stream, followed by torch.cuda.synchronize(), before the protocol - what a first use
uploads, allocates or loads (a plan's first call, the traced lane table, the prover's buffers, the first stream-ordered allocation of a size, the
kernels' code) is documented to wait."""
import ctypes as C
import random

import numpy as np
import pytest

import chipbatch_hash_ref as ref
import chipbatch_values_ref as vref
import merkle_tree_ref as mref
import stream_order as SO
import verdict_ref as R
from chipbatch_hash_ref import BN_PERMUTE, HASH_NO_PAD, MERKLE_VERIFY, TWO_TO_ONE, P

pytestmark = pytest.mark.gpu

SENT64 = 0xA5A5A5A5A5A5A5A5
SENT32 = 0xA5A5A5A5


def _dev_u64(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(words, dtype=np.uint64)).view(np.int64).reshape(-1).copy()).cuda()


def _out(n, dtype):
    import torch
    return torch.zeros((n,), dtype=getattr(torch, dtype), device="cuda")


def _same(got, want, what):
    got = np.asarray(got).reshape(-1); want = np.asarray(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} words differ, first at {int(bad[0])}: got {got[bad[0]]:#x} want {want[bad[0]]:#x}"


def _differ(a, b, what):
    assert (np.asarray(a).reshape(-1) != np.asarray(b).reshape(-1)).any(), what + ": the reference of A equals the reference of B (the run would prove nothing)"


def _report(what, info):
    print(f"{what}: enqueue {info['enqueue_s'] * 1e3:.3f} ms (the call {info['call_s'] * 1e3:.3f} ms), delay {info['delay_ms']:.1f} ms, blocked {info['blocked']}")


# ---------------------------------------------------------------- the harness on stand-ins (torch ops only)
def _standin():
    import torch
    a = torch.arange(1, 4097, dtype=torch.int64, device="cuda")
    b = a + 1000003
    x, y = torch.empty_like(a), torch.empty_like(a)
    f = lambda t: t.cpu().numpy() * 3 + 1
    return a, b, x, y, f


def _f_on(stream, x, y):
    import torch
    with torch.cuda.stream(stream):
        torch.mul(x, 3, out=y)
        y.add_(1)


def _faulty(call, expect):
    """Runs a faulty stand-in; the snapshot must not be f(A).  expect: 'b' (it is f(B)) or 'sentinel'."""
    a, b, x, y, f = call.io
    (snap,), blocked = SO.run_ordered(call, [(x, a, b)], [y])
    if (snap == f(a)).all():
        pytest.fail("inconclusive on this machine: a faulty stand-in came back clean")
    if expect == "b":
        assert (snap == f(b)).all()
    else:
        assert (snap.view(np.uint64) == SENT64).all()


def test_harness_passes_a_correct_call():
    import torch
    a, b, x, y, f = _standin()
    call = lambda s: _f_on(torch.cuda.ExternalStream(s), x, y)
    info = {}
    (snap,), blocked = SO.run_ordered(call, [(x, a, b)], [y], expect_no_sync=True, info=info)
    _report("stand-in", info)
    assert not blocked and (snap == f(a)).all() and not (f(a) == f(b)).any()
    assert info["delay_ms"] >= 0.5 * SO.DELAY_MS


def test_harness_reports_an_escaped_launch():
    import torch
    io = _standin()
    call = lambda s: _f_on(torch.cuda.default_stream(), io[2], io[3])      # the null stream instead of the caller's
    call.io = io
    _faulty(call, "b")


def test_harness_reports_a_missing_join():
    import torch
    io = _standin()
    side = torch.cuda.Stream()

    def call(s):
        ev = torch.cuda.Event()
        ev.record(torch.cuda.ExternalStream(s)); side.wait_event(ev)      # a proper wait-in
        SO.enqueue_delay(side, 20)
        _f_on(side, io[2], io[3])                                         # and no join: the caller's stream never waits for `side`
    call.io = io
    _faulty(call, "sentinel")


def test_harness_reports_a_missing_wait_in():
    import torch
    io = _standin()
    side = torch.cuda.Stream()

    def call(s):
        _f_on(side, io[2], io[3])                                         # `side` does not wait for the caller's stream
        ev = torch.cuda.Event()
        ev.record(side); torch.cuda.ExternalStream(s).wait_event(ev)      # a proper join
    call.io = io
    _faulty(call, "b")


def test_harness_reports_a_stray_synchronisation():
    import torch
    a, b, x, y, f = _standin()

    def call(s):
        st = torch.cuda.ExternalStream(s)
        _f_on(st, x, y)
        st.synchronize()
    try:
        SO.run_ordered(call, [(x, a, b)], [y], expect_no_sync=True)
    except AssertionError as e:
        assert "does not synchronise" in str(e)
    else:
        pytest.fail("inconclusive on this machine: a faulty stand-in came back clean")
    (snap,), blocked = SO.run_ordered(call, [(x, a, b)], [y])
    assert blocked and (snap == f(a)).all()


# ---------------------------------------------------------------- h2w_merkle_build, and build -> open -> values
def _flat_leaves(leaves):
    return [w for tree in leaves for leaf in tree for w in leaf]


def _stores(levels_of_trees):
    return np.array([mref.tree_store(lv) for lv in levels_of_trees], dtype=np.uint64)


@pytest.mark.parametrize("crown", [mref.CROWN_NONE, 4])
@pytest.mark.parametrize("mode", [0, 1])
def test_merkle_build(h2w_api, oracle, consts, mode, crown):
    """(5, 7, 3), three trees: the leaf kernel, every level one lane per node (NONE) or the crown's launches (4).  B has one word = p in tree 1: its
    status words are [0, 4, 0], A's [0, 0, 0]."""
    ko, kh = consts
    n_in, depth, cap, nt = 5, 7, 3, 3
    la, wa = mref.reference_trees(oracle, ko, "consts", mode, n_in, depth, cap, nt, seed=0xB1D + 17 * n_in + depth)
    lb, wb = mref.reference_trees(oracle, ko, "consts", mode, n_in, depth, cap, nt, seed=0x0B0B)
    flat_b = _flat_leaves(lb); flat_b[(1 << depth) * n_in + 3 * n_in + 2] = P      # tree 1, leaf 3, word 2
    want, want_b = _stores(wa), _stores(wb)
    for t in (0, 2):
        _differ(want[t], want_b[t], f"tree {t}")
    m = h2w_api.MerkleTree.new(kh, hash_mode=mode, n_in=n_in, depth=depth, cap_height=cap)
    m.configure(mref.OPT_CROWN_BITS, crown)
    tw = m.tree_words()
    d_a, d_b = _dev_u64(_flat_leaves(la)), _dev_u64(flat_b)
    d_leaves = d_b.clone()
    trees, status = _out(nt * tw, "int64"), _out(nt, "int32")
    call = lambda s: m.build(d_leaves.data_ptr(), nt, trees.data_ptr(), status.data_ptr(), s)
    SO.timed_warm_up(call)
    assert status.cpu().tolist() == [0, 4, 0]      # (the warm-up ran on B)
    info = {}
    (g_trees, g_status), _ = SO.run_ordered(call, [(d_leaves, d_a, d_b)], [trees, status], expect_no_sync=True, info=info)
    _report(f"h2w_merkle_build mode {mode} crown {crown}", info)
    _same(g_status, [0, 0, 0], "status words")
    _same(g_trees.view(np.uint64), want, "trees")
    m.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_build_open_values_without_a_host_step(h2w_api, oracle, consts, mode):
    """(5, 5, 1), three trees, twelve queries: h2w_merkle_build, h2w_merkle_open on its trees, h2w_chipbatch_values on its rows in every form the mode
    admits, all enqueued back to back.  B: other leaves (one word = p in tree 1: build status [0, 4, 0]), other queries, one of them with tree = n_trees
    (open status 4, the row is not written and keeps the sentinel, whose index word the chip refuses: verdict status 4)."""
    ko, kh = consts
    n_in, depth, cap, nt, nq = 5, 5, 1, 3, 12
    la, wa = mref.reference_trees(oracle, ko, "consts", mode, n_in, depth, cap, nt, seed=0x09E4)
    lb, wb = mref.reference_trees(oracle, ko, "consts", mode, n_in, depth, cap, nt, seed=0x09E5)
    flat_b = _flat_leaves(lb); flat_b[(1 << depth) * n_in + 3 * n_in + 2] = P
    rnd = random.Random(70 + mode)
    qa = [(2, 9)] + [(rnd.randrange(nt), rnd.randrange(1 << depth)) for _ in range(nq - 1)]
    qb = [((t + 1) % nt, i ^ 5) for t, i in qa]; qb[5] = (nt, 1)
    rows_a = np.array([mref.opening_row(la[t], wa[t], depth, cap, i) for t, i in qa], dtype=np.uint64)
    rows_b0 = np.array(mref.opening_row(lb[0], wb[0], depth, cap, qb[0][1]), dtype=np.uint64)      # (qb[0] opens tree 0, which B builds)
    assert qb[0][0] == 0
    _differ(_stores(wa)[0], _stores(wb)[0], "tree 0"); _differ(rows_a[0], rows_b0, "row 0")
    m = h2w_api.MerkleTree.new(kh, hash_mode=mode, n_in=n_in, depth=depth, cap_height=cap)
    b = h2w_api.ChipBatch.new_hash(MERKLE_VERIFY, kh, hash_mode=mode, n_in=n_in, depth=depth, cap_height=cap)
    tw, nw = m.tree_words(), m.layout()["num_operands"]
    assert nw == b.num_operands() == rows_a.shape[1]
    forms = vref.forms_of(MERKLE_VERIFY, mode) + (vref.FORM_AUTO,)
    l_a, l_b, q_a, q_b = _dev_u64(_flat_leaves(la)), _dev_u64(flat_b), _dev_u64([w for q in qa for w in q]), _dev_u64([w for q in qb for w in q])
    d_leaves, d_q = l_b.clone(), q_b.clone()
    trees, bst, rows, ost = _out(nt * tw, "int64"), _out(nt, "int32"), _out(nq * nw, "int64"), _out(nq, "int32")
    vers = [_out(nq * 2, "int32") for _ in forms]

    def call(s):
        m.build(d_leaves.data_ptr(), nt, trees.data_ptr(), bst.data_ptr(), s)
        m.open(d_leaves.data_ptr(), trees.data_ptr(), nt, d_q.data_ptr(), nq, rows.data_ptr(), ost.data_ptr(), s)
        for form, ver in zip(forms, vers):
            b.values(rows.data_ptr(), nq, 0, ver.data_ptr(), form=form, stream=s)
    SO.as_bytes(rows).fill_(SO.SENTINEL)
    SO.timed_warm_up(call)      # on B: what the chain stores for it is the other reference
    assert bst.cpu().tolist() == [0, 4, 0] and [i for i, x in enumerate(ost.cpu().tolist()) if x] == [5]
    for ver in vers:
        assert ver.cpu().tolist()[10] == 4
    info = {}
    got, _ = SO.run_ordered(call, [(d_leaves, l_a, l_b), (d_q, q_a, q_b)], [trees, bst, rows, ost] + vers, expect_no_sync=True, info=info)
    _report(f"build -> open -> values mode {mode}", info)
    _same(got[0].view(np.uint64), _stores(wa), "trees")
    _same(got[1], [0] * nt, "build status")
    _same(got[2].view(np.uint64), rows_a, "opening rows")
    _same(got[3], [0] * nq, "open status")
    for form, g in zip(forms, got[4:]):
        _same(g, [0, 0] * nq, f"verdicts in form {form}")
    m.close(); b.close()


# ---------------------------------------------------------------- h2w_chipbatch_values
def _expect_rows(oracle, ko, params, rows):
    from concurrent.futures import ThreadPoolExecutor
    one = lambda r: vref.expected(oracle, ko, 21, params, r)
    head = [one(rows[0])]
    with ThreadPoolExecutor(max_workers=8) as ex:
        return head + list(ex.map(one, rows[1:]))


def _op_words(params, rows):
    return np.array([ref.words_of(*params, r) for r in rows], dtype=np.uint64)


VALUES_CASES = [((HASH_NO_PAD, 0, 9, 0, 0), 17, None), ((HASH_NO_PAD, 1, 10, 0, 0), 17, None), ((BN_PERMUTE, 0, 0, 0, 0), 5, (vref.FORM_ROW,))]


@pytest.mark.parametrize("params,n,forms", VALUES_CASES, ids=lambda v: str(v))
def test_chipbatch_values(h2w_api, oracle, consts, params, n, forms):
    """B: other operands, the last row with a word outside its field (verdict status 4 there; A's verdicts are all (0, 0))."""
    ko, kh = consts
    forms = forms or vref.forms_of(params[0], params[1])
    rnd_a, rnd_b = ref.case_seed(*params, extra=500), ref.case_seed(*params, extra=501)
    rows_a = [ref.random_items(rnd_a, *params) for _ in range(n)]
    rows_b = [ref.random_items(rnd_b, *params) for _ in range(n)]
    want_a, want_b = _expect_rows(oracle, ko, params, rows_a), _expect_rows(oracle, ko, params, rows_b[:-1])
    rows_b[-1] = vref.invalid_row(params, rows_b[-1])
    for i in range(n - 1):
        assert want_a[i][0] != want_b[i][0] and want_a[i][1] == 0
    b = h2w_api.ChipBatch.new_hash(params[0], kh, hash_mode=params[1], n_in=params[2], depth=params[3], cap_height=params[4])
    nres = b.num_results()
    o_a, o_b = _dev_u64(_op_words(params, rows_a)), _dev_u64(_op_words(params, rows_b))
    d_ops = o_b.clone()
    res = [_out(n * nres, "int64") for _ in forms]; ver = [_out(n * 2, "int32") for _ in forms]

    def call(s):
        for form, r, v in zip(forms, res, ver):
            b.values(d_ops.data_ptr(), n, r.data_ptr(), v.data_ptr(), form=form, stream=s)
    SO.timed_warm_up(call)
    for v in ver:
        assert v.cpu().tolist()[2 * (n - 1)] == 4      # (the warm-up ran on B: its last row is refused)
    info = {}
    got, _ = SO.run_ordered(call, [(d_ops, o_a, o_b)], res + ver, expect_no_sync=True, info=info)
    _report(f"h2w_chipbatch_values {params}", info)
    for k, form in enumerate(forms):
        _same(got[k].view(np.uint64), np.array([w for w, _ in want_a], dtype=np.uint64), f"results in form {form}")
        _same(got[len(forms) + k], [0, 0] * n, f"verdicts in form {form}")
    b.close()


# ---------------------------------------------------------------- h2w_chipbatch_run
def test_chipbatch_run_field_op(h2w, oracle):
    """GL_DIV, n = 200.  Row 0 is all zero in B only: its status word is 1 there, 0 in A."""
    import torch
    from test_gpu_chips import OPS, oracle_chip_instance
    L = h2w.lib()
    n, lookup_bits = 200, 21
    h = L.h2w_chipbatch_new(OPS["div"], lookup_bits, 0)
    assert h, h2w.last_error()
    nw, nc = int(L.h2w_chipbatch_num_operands(h)), int(L.h2w_chipbatch_num_cells(h))
    rnd = random.Random(0xD17)
    ops_a = [[rnd.randrange(1, P) for _ in range(nw)] for _ in range(n)]
    ops_b = [[rnd.randrange(1, P) for _ in range(nw)] for _ in range(n)]; ops_b[0] = [0] * nw
    ref_a = [oracle_chip_instance(oracle, "div", lookup_bits, w) for w in ops_a]
    ref_b = [oracle_chip_instance(oracle, "div", lookup_bits, w) for w in ops_b]
    assert [s for _, s in ref_a] == [0] * n and [s for _, s in ref_b] == [1] + [0] * (n - 1)
    assert all(ca != cb for (ca, _), (cb, _) in zip(ref_a, ref_b))
    o_a, o_b = _dev_u64(ops_a), _dev_u64(ops_b)
    d_ops = o_b.clone()
    advice, status = _out(n * nc * 32, "uint8"), _out(n, "int32")
    call = lambda s: L.h2w_chipbatch_run(h, d_ops.data_ptr(), n, advice.data_ptr(), status.data_ptr(), s) == 0 or pytest.fail(h2w.last_error())
    idle_s = SO.timed_warm_up(call)
    assert status.cpu().tolist() == [1] + [0] * (n - 1)
    info = {}
    (adv, st), blocked = SO.run_ordered(call, [(d_ops, o_a, o_b)], [advice, status], delay_ms=SO.delay_for(idle_s), info=info)
    _report(f"h2w_chipbatch_run GL_DIV (idle call {idle_s * 1e3:.3f} ms)", info)
    SO.assert_delay_covers(info, idle_s, "h2w_chipbatch_run")
    _same(st, [0] * n, "status words")
    _same(adv, np.frombuffer(b"".join(c for c, _ in ref_a), dtype=np.uint8), "advice bytes")
    L.h2w_chipbatch_free(h)


@pytest.mark.parametrize("mode", [0, 1])
def test_chipbatch_run_hash_op_in_three_launches(h2w_api, oracle, consts, mode):
    """TWO_TO_ONE, n = 5 with H2W_CHIPBATCH_OPT_CHUNK 2: three internal launches on a stream-ordered allocation.  B: other operands, the last row with a
    word outside its field (status 4; A's status words are all 0)."""
    ko, kh = consts
    params, n = (TWO_TO_ONE, mode, 0, 0, 0), 5
    rnd_a, rnd_b = ref.case_seed(*params, extra=600), ref.case_seed(*params, extra=601)
    rows_a = [ref.random_items(rnd_a, *params) for _ in range(n)]
    rows_b = [ref.random_items(rnd_b, *params) for _ in range(n)]

    def cells(r):
        ctx, _ = ref.oracle_instance(oracle, ko, 21, *params, r)
        assert not ctx.error(), ctx.error()
        c = ctx.advice_bytes(); ctx.close()
        return c
    want_a, want_b = [cells(r) for r in rows_a], [cells(r) for r in rows_b]
    assert all(x != y for x, y in zip(want_a, want_b))
    rows_b[-1] = vref.invalid_row(params, rows_b[-1])
    b = h2w_api.ChipBatch.new_hash(TWO_TO_ONE, kh, hash_mode=mode)
    b.set_chunk(2)
    nc = b.num_cells()
    o_a, o_b = _dev_u64(_op_words(params, rows_a)), _dev_u64(_op_words(params, rows_b))
    d_ops = o_b.clone()
    advice, status = _out(n * nc * 32, "uint8"), _out(n, "int32")
    call = lambda s: b.run(d_ops.data_ptr(), n, advice.data_ptr(), status.data_ptr(), s)
    idle_s = SO.timed_warm_up(call)
    assert status.cpu().tolist() == [0] * (n - 1) + [4]
    info = {}
    (adv, st), blocked = SO.run_ordered(call, [(d_ops, o_a, o_b)], [advice, status], delay_ms=SO.delay_for(idle_s), info=info)
    _report(f"h2w_chipbatch_run TWO_TO_ONE mode {mode} chunk 2 (idle call {idle_s * 1e3:.3f} ms)", info)
    SO.assert_delay_covers(info, idle_s, "h2w_chipbatch_run")
    _same(st, [0] * n, "status words")
    _same(adv, np.frombuffer(b"".join(want_a), dtype=np.uint8), "advice bytes")
    b.close()


# ---------------------------------------------------------------- h2w_fri_witness_batch / _batch2
def _proof_words(p):
    return np.frombuffer(bytes(p), dtype=np.uint64).copy()


def _oracle_stream(oracle, osh, ko, words):
    ctx = oracle.Ctx(osh.lookup_bits)
    assert oracle.verify_stark(ctx, osh, ko, (C.c_uint64 * len(words))(*[int(x) for x in words])) == 0
    out = np.frombuffer(ctx.advice_bytes(), dtype=np.uint64).copy(); ctx.close()
    return out


_WITNESS = {}


def _witness_case(h2w, oracle, consts, mode, n):
    """The witness shape and its proofs, once per (mode, n): A, B (its last proof holds a word = p: status 4 there, 0 everywhere in A), the oracle's
    streams of A and of B's first proof."""
    if (mode, n) not in _WITNESS:
        ko, kh = consts
        sh = h2w.fibonacci_shape(8, 3, rate_bits=1, cap_height=2, hash_mode=mode); osh = oracle.fibonacci_shape(8, 3, rate_bits=1, cap_height=2, hash_mode=mode)
        pa = [_proof_words(oracle.synth_proof(osh, 810 + i)) for i in range(n)]
        pb = [_proof_words(oracle.synth_proof(osh, 820 + i)) for i in range(n)]
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=4) as ex:      # (the oracle holds no state between contexts)
            streams = list(ex.map(lambda p: _oracle_stream(oracle, osh, ko, p), pa + pb[:1]))
        want, want_b0 = np.concatenate(streams[:n]), streams[n]
        _differ(want[:want_b0.size], want_b0, "advice of proof 0")
        pb[-1][len(pb[-1]) // 2] = P
        _WITNESS[(mode, n)] = (sh, osh, np.concatenate(pa), np.concatenate(pb), want, [0] * (n - 1) + [4])
    return _WITNESS[(mode, n)]


def _status_of(plan, ws_snapshot, n):
    """h2w_plan_status on a snapshot of the workspace."""
    import torch
    d = torch.from_numpy(ws_snapshot).cuda()
    return plan.status(d.data_ptr(), n)


def _montgomery_of(h2w, stream_words):
    """The canonical stream through h2w_advice_to_montgomery on the null stream (tests/test_gpu_batch.py pins it to Python integers; a sample is
    checked here as well)."""
    import torch
    d = torch.from_numpy(stream_words.view(np.int64)).cuda()
    assert h2w.lib().h2w_advice_to_montgomery(d.data_ptr(), stream_words.size // 4, 0) == 0
    torch.cuda.synchronize()
    out = d.cpu().numpy().view(np.uint64)
    c, m = stream_words.reshape(-1, 4), out.reshape(-1, 4)
    to_int = lambda row: sum(int(x) << (64 * j) for j, x in enumerate(row))
    rnd = random.Random(c.shape[0])
    for i in list(range(500)) + list(range(c.shape[0] - 500, c.shape[0])) + [rnd.randrange(c.shape[0]) for _ in range(1000)]:
        assert to_int(m[i]) == (to_int(c[i]) << 256) % ref.R, i
    return out


# (fork chains, an emit stream, Montgomery form, chain passes and values form - PoseidonBN254 options; 0: the library's choice, two passes and one wavefront
# per path for a launch this small).  Montgomery form without an emit stream: the direct cells run on the caller's stream (fork 0) or on the side stream,
# and with Goldilocks caps and fork 1 the fork is closed behind the glue strands and opened again for them.
WITNESS_CONFIGS = [(0, False, False, 0), (1, False, False, 0), (0, True, False, 0), (1, True, False, 0), (1, True, True, 0)]
WITNESS_CASES = [(m,) + c + (0,) for m in (0, 1) for c in WITNESS_CONFIGS] + [(1, 1, False, False, 1, 0), (1, 1, False, False, 2, 0)]
WITNESS_CASES += [(m, fork, False, True, 0, 0) for m in (0, 1) for fork in (1, 0)] + [(1, 1, False, False, 2, 1), (1, 1, False, False, 2, 2)]


def _witness_id(case):
    return "-".join(str(x) for x in case[:5]) + (f"-form{case[5]}" if case[5] else "")


@pytest.mark.parametrize("mode,fork,emit,mont,passes,form", WITNESS_CASES, ids=[_witness_id(c) for c in WITNESS_CASES])
def test_witness_batch(h2w, h2w_api, oracle, consts, mode, fork, emit, mont, passes, form):
    """fibonacci_shape(8, 3, rate_bits=1, cap_height=2), two proofs: every launch of the call - prologue, load, permutation records, Merkle chains or
    strands (forked to the plan's side stream or not), glue, expansion (on an emit stream or not), the direct cells' conversion."""
    import torch
    n = 2
    sh, osh, pa, pb, want, status_b = _witness_case(h2w, oracle, consts, mode, n)
    plan = h2w_api.Plan(sh, consts[1])
    plan.configure(h2w_api.OPT_FORK_CHAINS, fork)
    if passes:
        plan.configure(h2w_api.OPT_CHAIN_PASSES, passes)
    if form:
        plan.configure(h2w_api.OPT_VALUES_FORM, form)
    if mont:
        plan.set_output_form(h2w_api.FORM_MONTGOMERY)
        want = _montgomery_of(h2w, want)
    e = torch.cuda.Stream() if emit else None
    p_a, p_b = _dev_u64(pa), _dev_u64(pb)
    d_proofs = p_b.clone()
    advice = _out(n * plan.num_cells * 32, "uint8"); ws = _out(plan.workspace_bytes(n), "uint8")
    call = lambda s: plan.run(d_proofs.data_ptr(), n, advice.data_ptr(), ws.data_ptr(), s, e.cuda_stream if emit else None)
    SO.timed_warm_up(call)
    assert plan.status(ws.data_ptr(), n) == status_b
    info = {}
    (adv, wsn), blocked = SO.run_ordered(call, [(d_proofs, p_a, p_b)], [advice, (ws, 0)], expect_no_sync=True, info=info)
    _report(f"h2w_fri_witness_batch{'2' if emit else ''} mode {mode} fork {fork} montgomery {mont} passes {passes} values form {form}", info)
    assert _status_of(plan, wsn, n) == [0] * n
    _same(adv.view(np.uint64), want, "advice")
    plan.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_witness_batch_shard(h2w, h2w_api, oracle, consts, mode):
    """h2w_fri_witness_batch_shard as rank 1 of 2 with FORK_CHAINS 1, the same shape and proofs: the rank launches three of the six (proof, query) units
    and proof 1's prologue.  Its blocks hold the oracle's words for A; every other word of the buffer is still the sentinel."""
    n, rank, world = 2, 1, 2
    sh, osh, pa, pb, want, status_b = _witness_case(h2w, oracle, consts, mode, n)
    plan = h2w_api.Plan(sh, consts[1])
    plan.configure(h2w_api.OPT_FORK_CHAINS, 1)
    blocks = [(p_, plan.shard_block(rank, world, p_, q)) for p_ in range(n) for q in range(-1, sh.num_queries)]
    own = [(p_, b) for p_, b in blocks if b is not None]
    assert len(own) == 4 and [p_ for p_, b in own if b[2] == 0] == [1]      # (three units of proofs x queries = 6, and the prologue of proof 1)
    expect = np.full(n * plan.num_cells * 4, SENT64, dtype=np.uint64)
    for p_, (_, cnt, g) in own:
        lo = 4 * (p_ * plan.num_cells + g)
        expect[lo:lo + 4 * cnt] = want[lo:lo + 4 * cnt]
    p_a, p_b = _dev_u64(pa), _dev_u64(pb)
    d_proofs = p_b.clone()
    advice = _out(n * plan.num_cells * 32, "uint8"); ws = _out(plan.shard_workspace_bytes(n, rank, world), "uint8")
    call = lambda s: plan.run_shard(d_proofs.data_ptr(), n, advice.data_ptr(), ws.data_ptr(), rank, world, s)
    SO.timed_warm_up(call)
    assert plan.status(ws.data_ptr(), n) == status_b      # (every rank checks every proof's words)
    info = {}
    (adv, wsn), blocked = SO.run_ordered(call, [(d_proofs, p_a, p_b)], [advice, (ws, 0)], expect_no_sync=True, info=info)
    _report(f"h2w_fri_witness_batch_shard mode {mode} rank {rank} of {world}", info)
    assert _status_of(plan, wsn, n) == [0] * n
    _same(adv.view(np.uint64), expect, "advice: this rank's blocks, sentinels elsewhere")
    plan.close()


def test_witness_then_digest_then_montgomery(h2w, h2w_api, oracle, consts):
    """h2w_fri_witness_batch, h2w_advice_digest of its stream, h2w_advice_to_montgomery of it in place, chained on S (PoseidonBN254 caps, one proof)."""
    mode, n = 1, 1
    sh, osh, pa, pb, want, _ = _witness_case(h2w, oracle, consts, mode, n)
    ko = consts[0]
    pb = pb.copy(); pb[len(pb) // 2] = 7      # (B in its field: its digest and its converted cells are the oracle's too)
    want_b = _oracle_stream(oracle, osh, ko, pb)
    dg_a, dg_b = h2w_api.advice_digest_reference(want.reshape(-1, 4)), h2w_api.advice_digest_reference(want_b.reshape(-1, 4))
    assert all(x != y for x, y in zip(dg_a, dg_b))
    cells = _montgomery_of(h2w, want)
    _differ(cells, _montgomery_of(h2w, want_b), "converted cells")
    plan = h2w_api.Plan(sh, consts[1])
    p_a, p_b = _dev_u64(pa), _dev_u64(pb)
    d_proofs = p_b.clone()
    advice = _out(plan.num_cells * 32, "uint8"); ws = _out(plan.workspace_bytes(n), "uint8"); dg = _out(4, "int64")

    def call(s):
        plan.run(d_proofs.data_ptr(), n, advice.data_ptr(), ws.data_ptr(), s)
        plan.advice_digest(advice.data_ptr(), plan.num_cells, dg.data_ptr(), s)
        assert plan.L.h2w_advice_to_montgomery(advice.data_ptr(), plan.num_cells, s) == 0
    idle_s = SO.timed_warm_up(call)
    info = {}
    (adv, wsn, g_dg), blocked = SO.run_ordered(call, [(d_proofs, p_a, p_b)], [advice, (ws, 0), dg], delay_ms=SO.delay_for(idle_s), info=info)
    _report(f"witness -> digest -> montgomery (idle calls {idle_s * 1e3:.3f} ms)", info)
    SO.assert_delay_covers(info, idle_s, "the chain")
    assert _status_of(plan, wsn, n) == [0]
    _same(g_dg.view(np.uint64), np.array(dg_a, dtype=np.uint64), "digest")
    _same(adv.view(np.uint64), cells, "converted cells")
    plan.close()


# ---------------------------------------------------------------- h2w_fri_verdict_batch / _ex
AUTO, QUAD, ROW, FORK = 0, 1, 2, 0x100
_VERDICT = {}


def _verdict_case(h2w, h2w_api, oracle, consts, mode):
    """The small batch of tests/test_gpu_verdict_forms.py as A; B fails other checks (the final polynomial, a step tree's sibling) at other places.
    The oracle's verdict words of both, once per mode."""
    if mode not in _VERDICT:
        from test_gpu_verdict_forms import _small_batch
        ko, kh = consts
        sh, osh, words_a = _small_batch(h2w, oracle, consts, mode)
        plan = h2w_api.Plan(sh, kh); L = plan.proof_layout(); plan.close()
        valid, rand = words_a[0], words_a[1]
        words_b = [R.bump(valid, L["final_poly"] + 1), valid, _proof_words(oracle.synth_proof(osh, 6)), R.bump(valid, R.sibling_word(L, 1, L["steps"][0], 0))]
        run_rand = R.oracle_run(osh, ko, rand)
        smap = R.semantic_map(osh, *run_rand)
        want = R.expected_many(osh, ko, [valid, words_a[2]] + words_b, smap)      # (words_b[1] is the valid proof: run once)
        want_a, want_b = [want[0], R.verdict_of(smap, *run_rand), want[1], want[0]], want[2:]
        assert want_a[0] == (0, 0, R.NO_QUERY) and all(x != y for x, y in zip(want_a, want_b)), (want_a, want_b)
        _VERDICT[mode] = (sh, np.concatenate(words_a), np.concatenate(words_b), [w + (0,) for w in want_a])
    return _VERDICT[mode]


@pytest.mark.parametrize("mode,flags", [(1, None), (1, QUAD), (1, ROW), (1, ROW | FORK), (1, QUAD | FORK), (0, None), (0, QUAD | FORK)])
def test_verdict_batch(h2w, h2w_api, oracle, consts, mode, flags):
    """flags None: h2w_fri_verdict_batch; else h2w_fri_verdict_batch_ex.  Forked, the glue kernel runs on the plan's side stream between a wait-in and a join."""
    n = 4
    sh, wa, wb, want = _verdict_case(h2w, h2w_api, oracle, consts, mode)
    plan = h2w_api.Plan(sh, consts[1])
    p_a, p_b = _dev_u64(wa), _dev_u64(wb)
    d_proofs = p_b.clone()
    out = _out(4 * n, "int32")
    call = lambda s: plan.verdict(d_proofs.data_ptr(), n, s, verdict_ptr=out.data_ptr(), flags=flags)
    SO.timed_warm_up(call)
    info = {}
    (got,), _ = SO.run_ordered(call, [(d_proofs, p_a, p_b)], [out], expect_no_sync=True, info=info)
    _report(f"h2w_fri_verdict_batch mode {mode} flags {flags}", info)
    _same(got.view(np.uint32), np.array(want, dtype=np.uint32), "verdict words")
    plan.close()


# ---------------------------------------------------------------- a traced plan: the replay, then h2w_trace_verdict_batch
@pytest.mark.parametrize("mode", [1, 0])
def test_traced_witness_then_trace_verdict(h2w, h2w_api, oracle, consts, mode):
    """The smallest shape of tests/test_gpu_replay.py (2^6 rows, 2 queries, no fold step), traced on one proof, replayed on two others: the witness
    call and the verdict call chained on S, then the verdict call alone, which after its warm-up (the lane table) synchronises nothing."""
    ko, kh = consts
    n = 2
    sh, osh = R.shape_pair(h2w, oracle, mode, 6, 2, 1, 4)
    ctx = h2w_api.Context(21, True, 0); ctx.trace_begin()
    h2w_api.verify_stark(ctx, sh, kh, _proof_words(oracle.synth_proof(osh, 1)))
    plan = h2w_api.Plan.from_trace(ctx, len(oracle.synth_proof(osh, 1))); ctx.close()
    assert plan.trace_verdict_info()["available"] == 1
    valid_a, valid_b = _proof_words(oracle.prove_fri(osh, ko, 33)), _proof_words(oracle.prove_fri(osh, ko, 34))
    rand_a, rand_b = _proof_words(oracle.synth_proof(osh, 2)), _proof_words(oracle.synth_proof(osh, 3))
    wa, wb = [valid_a, rand_a], [rand_b, valid_b]
    run_rand = R.oracle_run(osh, ko, rand_a)
    smap = R.semantic_map(osh, *run_rand)
    v = R.expected_many(osh, ko, [valid_a, rand_b, valid_b], smap)
    v = [v[0], R.verdict_of(smap, *run_rand), v[1], v[2]]
    want_v = [x + (0,) for x in v[:2]]
    assert v[0] == (0, 0, R.NO_QUERY) == v[3] and v[1][1] > 0 and v[2][1] > 0
    want = np.concatenate([_oracle_stream(oracle, osh, ko, p) for p in wa])
    _differ(want[:want.size // 2], _oracle_stream(oracle, osh, ko, rand_b), "advice of proof 0")
    p_a, p_b = _dev_u64(np.concatenate(wa)), _dev_u64(np.concatenate(wb))
    d_proofs = p_b.clone()
    advice = _out(n * plan.num_cells * 32, "uint8"); ws = _out(plan.workspace_bytes(n), "uint8"); out = _out(4 * n, "int32")
    witness = lambda s: plan.run(d_proofs.data_ptr(), n, advice.data_ptr(), ws.data_ptr(), s)
    verdict = lambda s: plan.trace_verdict(d_proofs.data_ptr(), n, ws.data_ptr(), s, verdict_ptr=out.data_ptr())
    both = lambda s: (witness(s), verdict(s))
    idle_s = SO.timed_warm_up(both)
    info = {}
    (adv, wsn, got), blocked = SO.run_ordered(both, [(d_proofs, p_a, p_b)], [advice, (ws, 0), out], delay_ms=SO.delay_for(idle_s), info=info)
    _report(f"traced witness -> trace verdict mode {mode} (idle calls {idle_s * 1e3:.3f} ms)", info)
    SO.assert_delay_covers(info, idle_s, "the traced chain")
    assert _status_of(plan, wsn, n) == [0] * n
    _same(adv.view(np.uint64), want, "advice")
    _same(got.view(np.uint32), np.array(want_v, dtype=np.uint32), "verdict words")
    info = {}
    (wsn, got), _ = SO.run_ordered(verdict, [(d_proofs, p_a, p_b)], [(ws, 0), out], expect_no_sync=True, info=info)
    _report(f"h2w_trace_verdict_batch mode {mode}", info)
    _same(got.view(np.uint32), np.array(want_v, dtype=np.uint32), "verdict words of the call alone")
    plan.close()


# ---------------------------------------------------------------- h2w_prove_fri_batch
@pytest.mark.parametrize("mode", [1, 0])
def test_prove_fri_batch(h2w, h2w_api, oracle, consts, mode):
    """custom_shape(d=6, q=2), two proofs.  The call synchronises its stream (the transcript runs on the host), so `blocked` is expected; the delay
    is sized by the call's time on an idle stream: every launch in front of its first wait was enqueued behind the delay, the copy of A with it."""
    from prover_util import custom_shape
    ko, kh = consts
    n = 2
    sh, osh = custom_shape(h2w, oracle, d=6, q=2, mode=mode)
    ins_a = [oracle.prove_fri_inputs(osh, 700 + i) for i in range(n)]
    ins_b = [oracle.prove_fri_inputs(osh, 710 + i) for i in range(n)]
    pis = [int(x) for _, p_ in ins_a for x in list(p_)[:sh.n_pis]]      # host memory: the same in both sets
    proof = lambda c, i: np.frombuffer(oracle.prove_fri_coef(osh, ko, c, (C.c_uint64 * max(sh.n_pis, 1))(*pis[i * sh.n_pis:(i + 1) * sh.n_pis])), dtype=np.uint64).copy()
    want = np.concatenate([proof(c, i) for i, (c, _) in enumerate(ins_a)])
    want_b = np.concatenate([proof(c, i) for i, (c, _) in enumerate(ins_b)])
    _differ(want[:want.size // 2], want_b[:want.size // 2], "proof 0"); _differ(want[want.size // 2:], want_b[want.size // 2:], "proof 1")
    pr = h2w_api.Prover(sh, kh)
    c_a = _dev_u64(np.concatenate([np.frombuffer(c, dtype=np.uint64) for c, _ in ins_a]))
    c_b = _dev_u64(np.concatenate([np.frombuffer(c, dtype=np.uint64) for c, _ in ins_b]))
    d_coefs = c_b.clone()
    proofs = _out(n * pr.proof_words, "int64")
    call = lambda s: pr.prove_batch(d_coefs.data_ptr(), pis, proofs.data_ptr(), n, s)
    idle_s = SO.timed_warm_up(call)
    _same(proofs.cpu().numpy().view(np.uint64), want_b, "the warm-up's proofs (of B)")
    info = {}
    (got,), blocked = SO.run_ordered(call, [(d_coefs, c_a, c_b)], [proofs], delay_ms=SO.delay_for(idle_s), info=info)
    _report(f"h2w_prove_fri_batch mode {mode} (idle call {idle_s * 1e3:.3f} ms)", info)
    SO.assert_delay_covers(info, idle_s, "h2w_prove_fri_batch")
    _same(got.view(np.uint64), want, "proof words")
    pr.close()
