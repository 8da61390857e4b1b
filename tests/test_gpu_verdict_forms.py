"""h2w_fri_verdict_batch_ex on the device (include/h2w.h 3b, csrc/verdict.hip): under every accepted `flags` value the verdict words are the ones the
CPU oracle gives (tests/verdict_ref.py, exactly as tests/test_gpu_verdict.py takes them) - the wavefront-per-path Merkle kernel
(k_verdict_merkle_row, rowperm.h bn_permute_rows<false>), the glue kernel forked to the plan's side stream beside either Merkle kernel, and what
FORM_AUTO picks.  The batch of a shape and the oracle's expectation are built once per shape; the forms are looped over it.

Shapes (degree_bits, queries, rate_bits, cap_height): one fold step; none (the cap as high as the tree); a longer path; a one-entry cap (one unit);
three steps of arity 4; no permutation Zs (oracle 1 is the quotient tree).  Edges of the row kernel's grid: 65 units (whatever the number of
wavefronts of a block, the last block is partly filled; the changed sibling is in the last unit), one unit.  Streams: two caller streams forking at
once, one more caller stream than the plan has side streams (the last runs unforked), a witness call and a forked verdict call sharing a side stream."""
import ctypes as C

import numpy as np
import pytest

import verdict_ref as R

pytestmark = pytest.mark.gpu

AUTO, QUAD, ROW, FORK = 0, 1, 2, 0x100
N_SIDE = 16      # include/h2w.h: a plan serves at most 16 caller streams with side streams
SHAPES = {
    "one_fold_step": ((6, 2, 1, 2), {}),
    "no_fold_step": ((6, 2, 1, 4), {}),
    "degree_9": ((9, 2, 1, 2), {}),
    "one_entry_cap": ((6, 1, 1, 0), {}),
    "three_steps": ((8, 2, 2, 2), dict(arity_bits=2, final_poly_bits=3)),
    "no_perm_z": ((6, 2, 1, 2), dict(n_perm_z=0)),
}
FORMS = {1: (ROW, ROW | FORK, QUAD | FORK, AUTO), 0: (QUAD | FORK, AUTO)}
CASES = [(1, name) for name in SHAPES] + [(0, name) for name in list(SHAPES)[:2]]


def _shapes(h2w, oracle, mode, name):
    (db, nq, rb, ch), over = SHAPES[name]
    return R.shape_pair(h2w, oracle, mode, db, nq, rb, ch, **over)


def _upload(plan, words):
    import torch
    host = np.concatenate([np.asarray(w, dtype=np.uint64) for w in words])
    assert len(host) == len(words) * plan.proof_words
    return torch.from_numpy(host.view(np.int64)).cuda()


def _tuples(t, n):
    w = [int(x) & 0xFFFFFFFF for x in t.cpu().tolist()]
    return [tuple(w[4 * i:4 * i + 4]) for i in range(n)]


def _witness_status(plan, d_proofs, n):
    import torch
    advice = torch.empty(n * plan.num_cells * 32, dtype=torch.uint8, device="cuda:0")
    ws = torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda:0")
    plan.run(d_proofs.data_ptr(), n, advice.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return plan.status(ws.data_ptr(), n)


@pytest.mark.parametrize("mode,name", CASES)
def test_every_field_is_the_oracles_under_every_form(h2w, h2w_api, oracle, consts, mode, name):
    ko, kh = consts
    sh, osh = _shapes(h2w, oracle, mode, name)
    plan = h2w_api.Plan(sh, kh)
    names, words, want, noncanonical, siblings = R.build_batch(osh, ko, plan.proof_layout())
    n = len(words)
    d = _upload(plan, words)
    status = _witness_status(plan, d, n)
    root = 4 if mode == 0 else 1
    for i, (flag, q) in siblings.items():      # by construction: exactly its tree's flag, its root's words, its query
        assert want[i] == (flag, root, q), (names[i], want[i])
    assert want[0] == want[-1] == (0, 0, R.NO_QUERY)
    for i in noncanonical:
        assert status[i] == 4, (names[i], status[i])
    for flags in FORMS[mode]:
        got = plan.verdict(d.data_ptr(), n, flags=flags)
        for i, nm in enumerate(names):
            if got[i] != want[i] + (status[i],):
                print(f"flags {flags:#x} {i:2d} {nm:45s} oracle {want[i]} device {got[i]} witness status {status[i]}")
        assert [g[:3] for g in got] == want, hex(flags)
        assert [g[3] for g in got] == status, hex(flags)
    if mode == 1:      # what AUTO resolved to, for the record: these batches are far below any crossover
        assert plan.verdict_form(n) == ROW
    plan.close()


def test_65_units_fill_the_row_kernels_last_block_partly(h2w, h2w_api, oracle, consts):
    """5 proofs x 13 queries: 65 wavefronts of work - 64 is a multiple of every block size, so the last block holds one real wavefront and the others
    leave after the barrier.  The last proof has a sibling of its LAST query changed (the last unit); no other proof's verdict moves with it."""
    ko, kh = consts
    sh, osh = R.shape_pair(h2w, oracle, 1, 6, 13, 1, 2)
    plan = h2w_api.Plan(sh, kh)
    L = plan.proof_layout()
    valid = np.frombuffer(bytes(oracle.prove_fri(osh, ko, 77)), dtype=np.uint64)
    rand = np.frombuffer(bytes(oracle.synth_proof(osh, 5)), dtype=np.uint64)
    smap = R.semantic_map(osh, *R.oracle_run(osh, ko, rand))
    changed = R.bump(valid, R.sibling_word(L, 12, L["steps"][0], 0) + 2)
    words = [valid, R.bump(valid, R.sibling_word(L, 7, L["oracles"][1], 2)), rand, valid, changed]
    want = R.expected_many(osh, ko, words, smap)
    assert want[1] == (R.MERKLE_PERM_Z, 1, 7) and want[4] == (R.MERKLE_STEP, 1, 12) and want[0] == want[3] == (0, 0, R.NO_QUERY)
    d, d0 = _upload(plan, words), _upload(plan, words[:4] + [valid])
    status = _witness_status(plan, d, 5)
    for flags in (ROW, ROW | FORK, AUTO):
        got = plan.verdict(d.data_ptr(), 5, flags=flags)
        print(hex(flags), want, got)
        assert [g[:3] for g in got] == want and [g[3] for g in got] == status
        before = plan.verdict(d0.data_ptr(), 5, flags=flags)
        assert before[:4] == got[:4] and before[4] == before[0] and got[4] != before[4]
    plan.close()


def test_one_proof_of_one_query(h2w, h2w_api, oracle, consts):
    ko, kh = consts
    sh, osh = _shapes(h2w, oracle, 1, "one_entry_cap")
    plan = h2w_api.Plan(sh, kh)
    L = plan.proof_layout()
    valid = np.frombuffer(bytes(oracle.prove_fri(osh, ko, 77)), dtype=np.uint64)
    smap = R.semantic_map(osh, *R.oracle_run(osh, ko, oracle.synth_proof(osh, 5)))
    for words in ([valid], [R.bump(valid, R.sibling_word(L, 0, L["oracles"][0], L["oracles"][0]["sibs"] - 1))]):
        want = R.expected_many(osh, ko, words, smap)
        d = _upload(plan, words)
        status = _witness_status(plan, d, 1)
        for flags in (ROW, ROW | FORK):
            got = plan.verdict(d.data_ptr(), 1, flags=flags)
            assert [g[:3] for g in got] == want and [g[3] for g in got] == status, (hex(flags), want, got)
    plan.close()


def _small_batch(h2w, oracle, consts, mode):
    ko, kh = consts
    sh, osh = _shapes(h2w, oracle, mode, "one_fold_step")
    valid = np.frombuffer(bytes(oracle.prove_fri(osh, ko, 77)), dtype=np.uint64)
    rand = np.frombuffer(bytes(oracle.synth_proof(osh, 5)), dtype=np.uint64)
    return sh, osh, [valid, rand, R.bump(valid, 3), valid]


@pytest.mark.parametrize("mode", [1, 0])
def test_form_quad_is_the_plain_call_word_for_word(h2w, h2w_api, oracle, consts, mode):
    sh, osh, words = _small_batch(h2w, oracle, consts, mode)
    plan = h2w_api.Plan(sh, consts[1])
    d = _upload(plan, words)
    plain = plan.verdict(d.data_ptr(), len(words))
    assert plain[0][:2] == (0, 0) and plain[3] == plain[0] and plain[1][1] > 0 and plain[2][1] > 0
    assert plan.verdict(d.data_ptr(), len(words), flags=QUAD) == plain
    for flags in FORMS[mode]:
        assert plan.verdict(d.data_ptr(), len(words), flags=flags) == plain, hex(flags)
    plan.close()


def test_no_proof_writes_nothing(h2w, h2w_api, consts):
    import torch
    plan = h2w_api.Plan(h2w.fibonacci_shape(6, 2, rate_bits=1, cap_height=2), consts[1])
    for flags in (AUTO, QUAD, ROW, ROW | FORK):
        assert plan.verdict(0, 0, flags=flags) == []
        out = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        assert plan.verdict(0, 0, verdict_ptr=out.data_ptr(), flags=flags) is None      # (nothing is read or written)
        torch.cuda.synchronize()
        assert out.cpu().tolist() == [0x5A5A5A5A] * 4
    plan.close()


def _hip_current_device():
    """hipGetDevice of the one HIP runtime this process holds (the one libh2w.so is bound to)."""
    paths = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    assert len(paths) == 1, paths
    dev = C.c_int(-1)
    assert C.CDLL(paths[0]).hipGetDevice(C.byref(dev)) == 0
    return dev.value


def test_the_callers_device_stays_current_under_row_fork(h2w, h2w_api, oracle, consts):
    import torch
    sh, osh, words = _small_batch(h2w, oracle, consts, 1)
    plan = h2w_api.Plan(sh, consts[1], 0)
    d = _upload(plan, words).to("cuda:0")
    out = torch.zeros(4 * len(words), dtype=torch.int32, device="cuda:0")
    cur = torch.cuda.device_count() - 1
    torch.cuda.set_device(cur)
    try:
        assert _hip_current_device() == cur
        plan.verdict(d.data_ptr(), len(words), 0, verdict_ptr=out.data_ptr(), flags=ROW | FORK)
        assert _hip_current_device() == cur
        torch.cuda.synchronize(0)
        w = out.cpu().tolist()
        assert w[0:2] == [0, 0] and w[12:16] == w[0:4] and w[5] > 0
    finally:
        torch.cuda.set_device(0)
    plan.close()


@pytest.mark.parametrize("n_streams", [2, N_SIDE + 1])
def test_caller_streams_forking_at_once_give_the_serial_words(h2w, h2w_api, oracle, consts, n_streams):
    """Every caller stream enqueues a ROW | FORK call; results are read after all have completed.  With one more caller stream than the plan has side
    streams the last call finds none left and runs unforked: the same words."""
    import torch
    sh, osh, words = _small_batch(h2w, oracle, consts, 1)
    plan = h2w_api.Plan(sh, consts[1])
    n = len(words)
    d = _upload(plan, words)
    serial = plan.verdict(d.data_ptr(), n)
    assert serial[0][:2] == (0, 0) and serial[1][1] > 0
    streams = [torch.cuda.Stream() for _ in range(n_streams)]
    outs = [torch.zeros(4 * n, dtype=torch.int32, device="cuda:0") for _ in streams]
    torch.cuda.synchronize()
    for s, o in zip(streams, outs):
        plan.verdict(d.data_ptr(), n, s.cuda_stream, verdict_ptr=o.data_ptr(), flags=ROW | FORK)
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        assert _tuples(o, n) == serial, i
    for s, o in zip(streams, outs):      # the side streams exist now: once more, two calls per stream back to back
        o.zero_()
    torch.cuda.synchronize()
    for s, o in zip(streams, outs):
        plan.verdict(d.data_ptr(), n, s.cuda_stream, verdict_ptr=o.data_ptr(), flags=QUAD | FORK)
        plan.verdict(d.data_ptr(), n, s.cuda_stream, verdict_ptr=o.data_ptr(), flags=ROW | FORK)
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        assert _tuples(o, n) == serial, i
    plan.close()


def test_a_witness_call_and_a_forked_verdict_share_a_side_stream(h2w, h2w_api, oracle, consts):
    """H2W_OPT_FORK_CHAINS 1, two-pass chains: the witness call's chain kernels and the verdict call's glue kernel are enqueued on the same side stream,
    back to back, with no synchronisation between the calls.  Digests of the advice and the verdicts equal those of the two calls run apart."""
    import torch
    sh, osh, words = _small_batch(h2w, oracle, consts, 1)
    plan = h2w_api.Plan(sh, consts[1])
    plan.configure(h2w_api.OPT_FORK_CHAINS, 1); plan.configure(h2w_api.OPT_CHAIN_PASSES, 2)
    n = len(words)
    d = _upload(plan, words)
    s = torch.cuda.Stream()

    def witness(advice, ws):
        plan.run(d.data_ptr(), n, advice.data_ptr(), ws.data_ptr(), s.cuda_stream)

    def digest(advice):
        dg = torch.zeros(4, dtype=torch.int64, device="cuda:0")
        plan.advice_digest(advice.data_ptr(), n * plan.num_cells, dg.data_ptr(), s.cuda_stream)
        torch.cuda.synchronize()
        return dg.cpu().tolist()

    new = lambda: (torch.zeros(n * plan.num_cells * 32, dtype=torch.uint8, device="cuda:0"), torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda:0"))
    # apart
    a0, w0 = new()
    torch.cuda.synchronize()
    witness(a0, w0); torch.cuda.synchronize()
    st0, dg0 = plan.status(w0.data_ptr(), n), digest(a0)
    v0 = plan.verdict(d.data_ptr(), n, s.cuda_stream, flags=ROW | FORK)
    assert [v[3] for v in v0] == st0 and v0 == plan.verdict(d.data_ptr(), n)
    # together, either order
    for verdict_first in (False, True):
        a1, w1 = new()
        out = torch.zeros(4 * n, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        if verdict_first:
            plan.verdict(d.data_ptr(), n, s.cuda_stream, verdict_ptr=out.data_ptr(), flags=ROW | FORK)
        witness(a1, w1)
        if not verdict_first:
            plan.verdict(d.data_ptr(), n, s.cuda_stream, verdict_ptr=out.data_ptr(), flags=ROW | FORK)
        torch.cuda.synchronize()
        assert _tuples(out, n) == v0, verdict_first
        assert plan.status(w1.data_ptr(), n) == st0 and digest(a1) == dg0 and torch.equal(a1, a0), verdict_first
    plan.close()
