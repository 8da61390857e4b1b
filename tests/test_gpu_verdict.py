"""h2w_fri_verdict_batch on the device (include/h2w.h 3b, csrc/verdict.hip): every field of every proof's verdict equals what the CPU oracle
says about that proof (tests/verdict_ref.py: n_failed = the oracle's failing semantic pairs, the PoW bit = a failing lookup, flags and first_query
from the place of every failing pair in the oracle's stream), and `status` equals h2w_plan_status after a witness call on the same buffer.

One batch per shape holds the valid proof; +1 mod p on one word of it - a sibling of each tree, an initial leaf word, a step evaluation at the
selected index and one off it, a final-polynomial coefficient, the PoW witness, a word of each cap -; a uniformly random proof; a proof with a
Goldilocks word >= p (status 4; the oracle's one broken constraint of the gadget's own wiring, the range check of that word's load, is not a
check on the proof and is left out of n_failed: verdict_ref.oracle_run); and the valid proof again, last: no verdict leaks between proofs.
No expectation is reasoned: a corrupted cap word moves every challenge, and a query may keep its index.

Shapes (degree_bits, queries, rate_bits, cap_height): the smallest at which the kernels differ - one fold step, none, a longer path, a one-entry
cap, three steps of arity 4, no permutation Zs (oracle 1 is the quotient tree), other widths / PoW bits / challenges, pow_bits 0, the published tables.
Edges: 65 (proof, query) units with PoseidonBN254 caps (a second wavefront of glue lanes, a second block of quads whose last wavefront holds one real
quad), one unit, no proof."""
import ctypes as C

import numpy as np
import pytest

import verdict_ref as R

pytestmark = pytest.mark.gpu

SHAPES = {
    "one_fold_step": ((6, 2, 1, 2), {}),
    "no_fold_step": ((6, 2, 1, 4), {}),
    "degree_9": ((9, 2, 1, 2), {}),
    "one_entry_cap": ((6, 1, 1, 0), {}),
    "three_steps": ((8, 2, 2, 2), dict(arity_bits=2, final_poly_bits=3)),
    "no_perm_z": ((6, 2, 1, 2), dict(n_perm_z=0)),
    "widths": ((6, 2, 1, 2), dict(n_cols=6, n_quotient=4, pow_bits=10, num_challenges=3)),
    "pow_bits_0": ((6, 2, 1, 2), dict(pow_bits=0)),
}


def _shapes(h2w, oracle, mode, name):
    (db, nq, rb, ch), over = SHAPES[name]
    return R.shape_pair(h2w, oracle, mode, db, nq, rb, ch, **over)


def _device_verdicts(h2w_api, plan, words, stream=0):
    """(verdicts of the batch, the device buffer of its proofs)"""
    import torch
    n = len(words)
    host = np.concatenate([np.asarray(w, dtype=np.uint64) for w in words])
    assert len(host) == n * plan.proof_words
    d = torch.from_numpy(host.view(np.int64)).cuda()
    return plan.verdict(d.data_ptr(), n, stream), d


def _witness_status(plan, d_proofs, n):
    import torch
    advice = torch.empty(n * plan.num_cells * 32, dtype=torch.uint8, device="cuda:0")
    ws = torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda:0")
    plan.run(d_proofs.data_ptr(), n, advice.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return plan.status(ws.data_ptr(), n)


def _check_batch(h2w_api, plan, osh, ko):
    names, words, want, noncanonical, siblings = R.build_batch(osh, ko, plan.proof_layout())
    got, d = _device_verdicts(h2w_api, plan, words)
    status = _witness_status(plan, d, len(words))
    for i, name in enumerate(names):
        print(f"{i:2d} {name:45s} oracle {want[i]} device {got[i]} witness status {status[i]}")
    root = 4 if osh.hash_mode == 0 else 1
    for i, (flag, q) in siblings.items():      # by construction: exactly its tree's flag, its root's words, its query
        assert want[i] == (flag, root, q), (names[i], want[i])
    assert want[0] == want[-1] == (0, 0, R.NO_QUERY)
    for i in noncanonical:
        assert status[i] == 4, (names[i], status[i])
    assert [g[:3] for g in got] == want
    assert [g[3] for g in got] == status
    return got


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_verdict_field_is_the_oracles(h2w, h2w_api, oracle, consts, mode, name):
    ko, kh = consts
    sh, osh = _shapes(h2w, oracle, mode, name)
    plan = h2w_api.Plan(sh, kh)
    _check_batch(h2w_api, plan, osh, ko)
    plan.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_published_tables(h2w, h2w_api, oracle, published, mode):
    ko, kh = published
    sh, osh = _shapes(h2w, oracle, mode, "one_fold_step")
    plan = h2w_api.Plan(sh, kh)
    _check_batch(h2w_api, plan, osh, ko)
    plan.close()


def test_65_units_cross_a_wavefront_of_glue_lanes_and_a_block_of_quads(h2w, h2w_api, oracle, consts):
    """5 proofs x 13 queries, PoseidonBN254 caps: unit 64 is the first lane of the glue kernel's second block and the one real quad of the Merkle
    kernel's second block (63 tail quads beside it redo it and must not count); its proof, the last, has a sibling of its LAST query changed."""
    ko, kh = consts
    sh, osh = R.shape_pair(h2w, oracle, 1, 6, 13, 1, 2)
    plan = h2w_api.Plan(sh, kh)
    L = plan.proof_layout()
    valid = np.frombuffer(bytes(oracle.prove_fri(osh, ko, 77)), dtype=np.uint64)
    rand = np.frombuffer(bytes(oracle.synth_proof(osh, 5)), dtype=np.uint64)
    smap = R.semantic_map(osh, *R.oracle_run(osh, ko, rand))
    words = [valid, R.bump(valid, R.sibling_word(L, 7, L["oracles"][1], 2)), rand, valid, R.bump(valid, R.sibling_word(L, 12, L["steps"][0], 0) + 2)]
    want = R.expected_many(osh, ko, words, smap)
    assert want[1] == (R.MERKLE_PERM_Z, 1, 7) and want[4] == (R.MERKLE_STEP, 1, 12) and want[2][1] >= 13 * len(R.site_flags(osh))
    got, d = _device_verdicts(h2w_api, plan, words)
    print(want, got)
    assert [g[:3] for g in got] == want
    assert [g[3] for g in got] == _witness_status(plan, d, 5)
    plan.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_one_proof_of_one_query(h2w, h2w_api, oracle, consts, mode):
    ko, kh = consts
    sh, osh = _shapes(h2w, oracle, mode, "one_entry_cap")
    plan = h2w_api.Plan(sh, kh)
    L = plan.proof_layout()
    valid = np.frombuffer(bytes(oracle.prove_fri(osh, ko, 77)), dtype=np.uint64)
    smap = R.semantic_map(osh, *R.oracle_run(osh, ko, oracle.synth_proof(osh, 5)))
    for words in ([valid], [R.bump(valid, R.sibling_word(L, 0, L["oracles"][0], L["oracles"][0]["sibs"] - 1))]):
        want = R.expected_many(osh, ko, words, smap)
        got, d = _device_verdicts(h2w_api, plan, words)
        assert [g[:3] for g in got] == want and [g[3] for g in got] == _witness_status(plan, d, 1), (want, got)
    plan.close()


BN_R = 21888242871839275222246405745257275088548364400416034343698204186575808495617      # the BN254 scalar field's modulus


def _with(valid, at, values):
    """A copy of the proof with the words from `at` on replaced by `values`."""
    c = valid.copy()
    c[at:at + len(values)] = np.array(values, dtype=np.uint64)
    return c


@pytest.mark.parametrize("mode", [1, 0])
def test_status_4_at_the_field_boundaries_is_the_witness_calls(h2w, h2w_api, oracle, consts, mode):
    """Status 4 (a proof word outside its field) is one predicate (csrc/batchargs.h load_item_out_of_field) that the witness call's k_prologue_load and
    the verdict call's k_verdict_check both ask: the verdict's status word is the witness call's for every proof.  A `>=` that became `>` there would
    move both alike, so the batch holds the boundary itself: every proof is the valid one with one place at the modulus (status 4) or one below it
    (not 4) - an openings word and a final-polynomial word against p = 2^64 - 2^32 + 1; entry 0 of the trace cap and sibling 0 of query 1's first
    tree against p in their limb 2 (Goldilocks caps: four Goldilocks words) or, as the four words of one BN254 element, against r (PoseidonBN254 caps)."""
    ko, kh = consts
    sh, osh = _shapes(h2w, oracle, mode, "one_fold_step")
    plan = h2w_api.Plan(sh, kh)
    L = plan.proof_layout()
    valid = np.frombuffer(bytes(oracle.prove_fri(osh, ko, 77)), dtype=np.uint64)
    limbs = lambda x: [(x >> (64 * i)) & (2**64 - 1) for i in range(4)]
    hashes = {"trace cap entry 0": L["trace_cap"], "sibling 0 of query 1's first tree": R.sibling_word(L, 1, L["oracles"][0], 0)}
    cases = [("valid", valid, False),
             ("openings word = p", _with(valid, L["openings"] + 1, [R.GL_P]), True),
             ("openings word = p - 1", _with(valid, L["openings"] + 1, [R.GL_P - 1]), False),
             ("final-polynomial word = 2^64 - 1", _with(valid, L["final_poly"] + 1, [2**64 - 1]), True)]
    for name, at in hashes.items():
        if mode == 0:
            cases += [(name + ": limb 2 = p", _with(valid, at + 2, [R.GL_P]), True), (name + ": limb 2 = p - 1", _with(valid, at + 2, [R.GL_P - 1]), False)]
        else:
            cases += [(name + " = r", _with(valid, at, limbs(BN_R)), True), (name + " = r - 1", _with(valid, at, limbs(BN_R - 1)), False)]
    got, d = _device_verdicts(h2w_api, plan, [w for _, w, _ in cases])
    status = _witness_status(plan, d, len(cases))
    for (name, _, outside), g, s in zip(cases, got, status):
        print(f"{name:50s} outside its field: {outside!s:5s} verdict status {g[3]} witness status {s}")
    assert [g[3] for g in got] == status
    for (name, _, outside), s in zip(cases, status):
        assert (s == 4) == outside, (name, s)
    plan.close()


def test_no_proof(h2w, h2w_api, consts):
    import torch
    plan = h2w_api.Plan(h2w.fibonacci_shape(6, 2, rate_bits=1, cap_height=2), consts[1])
    assert plan.verdict(0, 0) == []
    out = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    assert plan.verdict(0, 0, verdict_ptr=out.data_ptr()) is None      # (nothing is read or written)
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [0x5A5A5A5A] * 4
    plan.close()


def _small_batch(h2w, oracle, consts, mode):
    ko, kh = consts
    sh, osh = _shapes(h2w, oracle, mode, "one_fold_step")
    valid = np.frombuffer(bytes(oracle.prove_fri(osh, ko, 77)), dtype=np.uint64)
    rand = np.frombuffer(bytes(oracle.synth_proof(osh, 5)), dtype=np.uint64)
    return sh, osh, [valid, rand, R.bump(valid, 3), valid]


@pytest.mark.parametrize("mode", [1, 0])
def test_two_streams_and_every_plan_option_give_the_same_words(h2w, h2w_api, oracle, consts, mode):
    """The call is stream-ordered (two calls on two streams, results read after both), and no h2w_plan_configure option changes a verdict:
    the Montgomery output form, one-pass and two-pass chains."""
    import torch
    ko, kh = consts
    sh, osh, words = _small_batch(h2w, oracle, consts, mode)
    plan = h2w_api.Plan(sh, kh)
    n = len(words)
    d = torch.from_numpy(np.concatenate(words).view(np.int64)).cuda()
    first, _ = _device_verdicts(h2w_api, plan, words)
    assert first[0][:2] == (0, 0) and first[3] == first[0] and first[1][1] > 0 and first[2][1] > 0
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    o1 = torch.zeros(4 * n, dtype=torch.int32, device="cuda:0"); o2 = torch.zeros(4 * n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    plan.verdict(d.data_ptr(), n, s1.cuda_stream, verdict_ptr=o1.data_ptr())
    plan.verdict(d.data_ptr(), n, s2.cuda_stream, verdict_ptr=o2.data_ptr())
    torch.cuda.synchronize()
    as_tuples = lambda t: [tuple(int(x) & 0xFFFFFFFF for x in t.cpu().tolist()[4 * i:4 * i + 4]) for i in range(n)]
    assert as_tuples(o1) == first and as_tuples(o2) == first
    plan.set_output_form(h2w_api.FORM_MONTGOMERY)
    assert plan.verdict(d.data_ptr(), n) == first
    plan.set_output_form(h2w_api.FORM_CANONICAL)
    for passes in (1, 2):
        plan.configure(h2w_api.OPT_CHAIN_PASSES, passes)
        assert plan.verdict(d.data_ptr(), n) == first
        assert [g[3] for g in first] == _witness_status(plan, d, n)      # (the witness call itself under the option)
    plan.close()


def test_a_traced_plan_is_refused(h2w, h2w_api, oracle, consts):
    import torch
    ko, kh = consts
    sh, osh = _shapes(h2w, oracle, 1, "one_fold_step")
    proof = oracle.synth_proof(osh, 43)
    tctx = h2w_api.Context(21, True, 0); tctx.trace_begin()
    h2w_api.verify_stark(tctx, sh, kh, np.frombuffer(bytes(proof), dtype=np.uint64))
    rplan = h2w_api.Plan.from_trace(tctx, len(proof)); tctx.close()
    d = torch.frombuffer(bytearray(bytes(proof)), dtype=torch.int64).cuda()
    out = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    with pytest.raises(h2w_api.H2WError, match="traced plan"):
        rplan.verdict(d.data_ptr(), 1, verdict_ptr=out.data_ptr())
    with pytest.raises(h2w_api.H2WError, match="traced plan"):
        rplan.proof_layout()
    rplan.close()


def _hip_current_device():
    """hipGetDevice of the one HIP runtime this process holds (the one libh2w.so is bound to)."""
    paths = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    assert len(paths) == 1, paths
    dev = C.c_int(-1)
    assert C.CDLL(paths[0]).hipGetDevice(C.byref(dev)) == 0
    return dev.value


def test_the_callers_device_stays_current(h2w, h2w_api, oracle, consts):
    """The plan's device is current for the duration of the call only: with another device current where there is one (the last), a plan on
    device 0 judges proofs on cuda:0 and the thread's device is what it was."""
    import torch
    ko, kh = consts
    sh, osh, words = _small_batch(h2w, oracle, consts, 1)
    plan = h2w_api.Plan(sh, kh, 0)
    d = torch.from_numpy(np.concatenate(words).view(np.int64)).to("cuda:0")
    out = torch.zeros(4 * len(words), dtype=torch.int32, device="cuda:0")
    cur = torch.cuda.device_count() - 1
    torch.cuda.set_device(cur)
    try:
        assert _hip_current_device() == cur
        plan.verdict(d.data_ptr(), len(words), 0, verdict_ptr=out.data_ptr())
        assert _hip_current_device() == cur
        torch.cuda.synchronize(0)
        w = out.cpu().tolist()
        assert w[0:2] == [0, 0] and w[12:16] == w[0:4] and w[5] > 0
    finally:
        torch.cuda.set_device(0)
    plan.close()
