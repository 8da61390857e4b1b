"""The host side of the verdict call (include/h2w.h 3b): h2w_plan_proof_layout names the words of a flat proof, and what it names is what the
CPU oracle takes them for - +1 on "sibling j of tree t of query q" makes exactly that tree's root of that query differ from its cap entry
(tests/verdict_ref.py: 4 failing pairs with Goldilocks caps, 1 with PoseidonBN254 caps), for the first and last sibling of every tree of the first
and last query.  Without a device h2w_fri_verdict_batch refuses."""
import ctypes as C

import numpy as np
import pytest

import verdict_ref as R

SHAPES = {"one_fold_step": {}, "no_perm_z": dict(n_perm_z=0)}


def _plan(h2w, h2w_api, oracle, consts, mode, over):
    ko, kh = consts
    sh, osh = R.shape_pair(h2w, oracle, mode, **over)
    return h2w_api.Plan(sh, kh), sh, osh, ko


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_proof_layout_partitions_the_proof(h2w, h2w_api, oracle, consts, mode, shape):
    plan, sh, osh, ko = _plan(h2w, h2w_api, oracle, consts, mode, SHAPES[shape])
    L = plan.proof_layout()
    assert L["total"] == plan.proof_words == oracle.lib().orc_proof_words(C.byref(osh))
    assert len(L["oracles"]) == (3 if sh.n_perm_z > 0 else 2) and len(L["steps"]) == R.fold_steps(osh) and L["cap_size"] == 1 << sh.cap_height
    cap = 4 * L["cap_size"]
    seg = [(L["trace_cap"], cap), (L["quotient_cap"], cap), (L["openings"], 2 * (2 * sh.n_cols + 2 * sh.n_perm_z + sh.n_quotient)),
           (L["perm_cap"], cap if sh.n_perm_z > 0 else 0), (L["pow_witness"], 1), (L["final_poly"], L["commit_caps"] - L["final_poly"]),
           (L["commit_caps"], len(L["steps"]) * cap), (L["pis"], sh.n_pis)]
    for q in range(sh.num_queries):
        seg += [(L["queries"] + q * L["query_words"] + t["off"], t["leaf"] + 4 * t["sibs"]) for t in L["oracles"] + L["steps"]]
    assert [t["leaf"] for t in L["oracles"]] == ([sh.n_cols, sh.n_perm_z, sh.n_quotient] if sh.n_perm_z > 0 else [sh.n_cols, sh.n_quotient])
    assert all(t["leaf"] == 2 << sh.arity_bits for t in L["steps"])
    at = 0
    for start, n in sorted(s for s in seg if s[1] > 0):
        assert start == at, (start, at)
        at += n
    assert at == L["total"]
    # the raw call: the size query, a buffer too small
    n = h2w.lib().h2w_plan_proof_layout(plan.p, None, 0)
    assert n == 14 + 3 * len(L["oracles"]) + 3 * len(L["steps"])
    assert h2w.lib().h2w_plan_proof_layout(plan.p, (C.c_uint64 * (n - 1))(), n - 1) == -1 and "words needed" in h2w.last_error()
    plan.close()


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_a_sibling_named_by_the_layout_breaks_its_root_in_the_oracle(h2w, h2w_api, oracle, consts, mode, shape):
    plan, sh, osh, ko = _plan(h2w, h2w_api, oracle, consts, mode, SHAPES[shape])
    L = plan.proof_layout()
    plan.close()
    smap = R.semantic_map(osh, *R.oracle_run(osh, ko, oracle.synth_proof(osh, 5)))
    valid = np.frombuffer(bytes(oracle.prove_fri(osh, ko, 77)), dtype=np.uint64)
    flags = ([R.MERKLE_TRACE, R.MERKLE_PERM_Z, R.MERKLE_QUOTIENT] if sh.n_perm_z > 0 else [R.MERKLE_TRACE, R.MERKLE_QUOTIENT]) + [R.MERKLE_STEP] * len(L["steps"])
    cases = [(q, f, R.sibling_word(L, q, t, j)) for q in (0, sh.num_queries - 1) for t, f in zip(L["oracles"] + L["steps"], flags) for j in sorted({0, t["sibs"] - 1})]
    got = R.expected_many(osh, ko, [valid] + [R.bump(valid, at) for _, _, at in cases], smap)
    assert got[0] == (0, 0, R.NO_QUERY)
    root = 4 if mode == 0 else 1
    assert got[1:] == [(f, root, q) for q, f, _ in cases]


def test_without_a_device_the_verdict_call_refuses(h2w, h2w_api, consts):
    if h2w.lib().h2w_device_count() > 0:
        pytest.skip("GPU present")
    plan = h2w_api.Plan(h2w.fibonacci_shape(6, 2, rate_bits=1, cap_height=2), consts[1])
    words = (C.c_uint64 * plan.proof_words)(); out = (C.c_uint32 * 4)()
    with pytest.raises(h2w_api.H2WError, match="no HIP device"):
        plan.verdict(C.addressof(words), 1, verdict_ptr=C.addressof(out))
    plan.close()
