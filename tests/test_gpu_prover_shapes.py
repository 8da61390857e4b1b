"""The device prover (csrc/prover.hip) at the shape edges the witness generator is held to (test_gpu_batch.test_shape_edge_cases) and at
the edges of its own kernels, word for word against the oracle's prover (oracle/prover.inc) on the same committed polynomials, both hash
modes.  tests/test_gpu_prover.py stays on the Fibonacci defaults (arity 16, 4 + 2 + 2 polynomials, 16 PoW bits, a fresh handle per proof).

  * no permutation oracle (two oracles, batch 1 = the trace alone); cap_height 0 (trees to the root) and cap_height = lde_bits (the cap is
    the leaf level: no tree level, no sibling);
  * arity 2, 4, 8 (a commit-phase leaf of 4 words is not hashed under Goldilocks caps and is under PoseidonBN254 caps); exactly MAX_STEPS
    fold steps;
  * polynomials per oracle 2, 3, 4, 5, 6, 8, 9, 10, 13 (the no-op thresholds 4 / 3 and the 8- / 9-word sponge blocks of the leaf
    hasher) and 16 in all;
  * an NTT of exactly one LDS tile (lde_bits 11) and of one global stage before it (lde_bits 12, by degree and by rate);
  * pow_bits 0 and 3 (a round of 2^8 candidates), at 16 bits a witness found in the second search round; 0 and 64 public inputs;
  * the field's edge values as coefficients, all-zero and constant polynomials (a zero quotient), an all-zero instance;
  * one handle over calls of different batch sizes.
The cases marked chain also go through the device witness generator and the oracle's verifier and MockProver, which tell a prover fault
from a fault of the oracle's prover.  The oracle proves every other case (MockProver clean) in 0.01 - 4.6 s on one CPU core.
pow_bits 23 (rounds of 2^22 candidates, the witness in the second) is held to a recorded digest of the oracle's proof and to the chain:
the oracle needs 88 s and 99 s for these two proofs."""
import pytest

from prover_util import assert_chain, assert_words_equal, custom_shape, gpu_prove, prove_coefs

pytestmark = pytest.mark.gpu

P = 2**64 - 2**32 + 1

# id: (shape as custom_shape takes it, through the witness generator too)
CASES = {
    "noperm": (dict(d=6, q=2, n_perm_z=0), True),
    "cap0": (dict(d=6, q=1, cap=0), True),
    "capfull": (dict(d=3, q=2, cap=4), False),
    "arity4": (dict(d=8, q=2, rb=2, cap=2, arity_bits=2, final_poly_bits=3), True),
    "arity8": (dict(d=9, q=2, rb=3, cap=1, arity_bits=3), False),
    "arity2": (dict(d=5, q=2, cap=1, arity_bits=1, final_poly_bits=2), True),
    "steps8": (dict(d=10, q=2, cap=1, arity_bits=1, final_poly_bits=2), True),
    "cols": (dict(d=6, q=2, pow_bits=10, n_cols=6, n_quotient=4, n_pis=1, num_challenges=3), False),
    "blocks": (dict(d=6, q=2, n_cols=8, n_perm_z=4, n_quotient=3), False),
    "full16": (dict(d=6, q=2, n_cols=9, n_perm_z=3, n_quotient=4), False),
    "wide2": (dict(d=6, q=2, n_cols=5, n_perm_z=0, n_quotient=10), False),
    "wide13": (dict(d=6, q=2, n_cols=13, n_perm_z=0, n_quotient=3), False),
    "lde11": (dict(d=10, q=2, cap=2), False),
    "lde12_degree": (dict(d=11, q=2, cap=2), False),
    "lde12_rate": (dict(d=10, q=2, rb=2, cap=2), False),
    "pow0": (dict(d=6, q=2, pow_bits=0), False),
    "pow3": (dict(d=6, q=2, pow_bits=3), False),
    "pis0": (dict(d=6, q=2, n_pis=0), False),
    "pis64": (dict(d=6, q=2, n_pis=64), False),
}
SEED = 0x5AFE0000


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("case", list(CASES))
def test_shape_edges_equal_the_oracle_prover(h2w, h2w_api, oracle, published, case, mode):
    ko, kh = published
    kw, chain = CASES[case]
    sh, osh = custom_shape(h2w, oracle, mode=mode, **kw)
    coefs, pis, d_proof, _ = gpu_prove(h2w, h2w_api, oracle, kh, sh, osh, SEED + list(CASES).index(case))
    assert_words_equal(d_proof.cpu().numpy(), oracle.prove_fri_coef(osh, ko, coefs, pis), case)
    if chain:
        assert_chain(h2w_api, oracle, ko, kh, sh, osh, d_proof)


# pow_bits 16 searches 2^16 candidates per device round.  The seeds are chosen (on the CPU, with the oracle) so that the smallest witness
# lies in the second round - blocks of a finished proof's later rounds return at once, an unfinished one goes on: mode -> (seed, witness)
POW_SECOND_ROUND = {1: (0x5AFE0309, 96326), 0: (0x5AFE0300, 92085)}


@pytest.mark.parametrize("mode", [1, 0])
def test_witness_found_in_the_second_search_round(h2w, h2w_api, oracle, published, mode):
    import numpy as np
    ko, kh = published
    sh, osh = custom_shape(h2w, oracle, mode=mode, d=6, q=2)
    seed, witness = POW_SECOND_ROUND[mode]
    coefs, pis, d_proof, _ = gpu_prove(h2w, h2w_api, oracle, kh, sh, osh, seed)
    want = oracle.prove_fri_coef(osh, ko, coefs, pis)
    cs = 1 << sh.cap_height
    at = 8 * cs + 2 * (2 * sh.n_cols + 2 * sh.n_perm_z + sh.n_quotient) + 4 * cs      # ProofLayout::pow_witness
    assert 1 << 16 <= np.frombuffer(want, dtype=np.uint64)[at] == witness < 1 << 17
    assert_words_equal(d_proof.cpu().numpy(), want, "second round")


# pow_bits 23 is above the clamp of a search round at 2^22 candidates.  The oracle grinds one candidate after the other, 18 us each, so
# its proofs (88 s and 99 s) are recorded as digests (tools/make_golden_prover.py -> tests/golden/prover_digests.json).  The seeds are
# the first of 0x5AFE1000.. whose smallest witness lies beyond the first round of 2^22:
#   powhi_gl    (Goldilocks caps)    seed 0x5AFE1001, witness 4681752 (second round)
#   powhi_bn254 (PoseidonBN254 caps) seed 0x5AFE1000, witness 5582216 (second round)
@pytest.mark.parametrize("case", ["powhi_bn254", "powhi_gl"])
def test_pow_bits_above_the_round_clamp(h2w, h2w_api, oracle, published, case):
    import hashlib, json, os
    import numpy as np
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prover_digests.json")))[case]
    ko, kh = published
    assert gold["pow_bits"] == 23 and gold["pow_witness"] == {"powhi_gl": 4681752, "powhi_bn254": 5582216}[case] >= 1 << 22
    sh, osh = custom_shape(h2w, oracle, mode=gold["hash_mode"], d=gold["degree_bits"], q=gold["queries"], rb=gold["rate_bits"], pow_bits=gold["pow_bits"])
    _, _, d_proof, _ = gpu_prove(h2w, h2w_api, oracle, kh, sh, osh, gold["seed"])
    words = d_proof.cpu().numpy().view(np.uint64)
    assert len(words) == gold["proof_words"]
    assert int(words[gold["pow_witness_word_index"]]) == gold["pow_witness"]
    assert hashlib.sha256(words.tobytes()).hexdigest() == gold["sha256"]
    assert_chain(h2w_api, oracle, ko, kh, sh, osh, d_proof)      # (the verifier's range check of the PoW response among the rest)


def _edge_coefs(oracle, osh, variant):
    """The oracle's seeded inputs with the coefficients overwritten: "edges" = polynomial 0 all zero, 1 a constant (both have a zero
    quotient by X - zeta), 2 cycling through the values at which 64-bit modular arithmetic goes wrong, the others all p - 1;
    "zero" = every polynomial zero (F = 0: every leaf of a tree equal, a zero final polynomial)."""
    coefs, pis = oracle.prove_fri_inputs(osh, SEED + 100)
    n = 1 << osh.degree_bits; npoly = len(coefs) // n
    cycle = [0, 1, P - 1, P - 2, 2**32 - 1, 2**32, 2**63, P - 2**32]
    for p_ in range(npoly):
        for i in range(n):
            if variant == "zero" or p_ == 0:
                v = 0
            elif p_ == 1:
                v = 0x123456789ABCDEF if i == 0 else 0
            elif p_ == 2:
                v = cycle[i % len(cycle)]
            else:
                v = P - 1
            coefs[p_ * n + i] = v
    return coefs, pis


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("variant", ["edges", "zero"])
def test_field_edges_in_the_committed_polynomials(h2w, h2w_api, oracle, published, variant, mode):
    ko, kh = published
    sh, osh = custom_shape(h2w, oracle, mode=mode, d=9, q=2, cap=2)          # one fold step
    coefs, pis = _edge_coefs(oracle, osh, variant)
    d_proof, _ = prove_coefs(h2w_api, sh, kh, coefs, pis)
    assert_words_equal(d_proof.cpu().numpy(), oracle.prove_fri_coef(osh, ko, coefs, pis), variant)
    if variant == "edges":
        assert_chain(h2w_api, oracle, ko, kh, sh, osh, d_proof)


def test_one_handle_over_calls_of_different_sizes(h2w, h2w_api, oracle, published):
    """ensure_capacity keeps the buffers of the largest batch: 1, 3, 1, 2 proofs through one handle, every stride following the call's
    own n; the first proof again, into a poisoned buffer, is the first proof; n = 0 writes nothing, n = 2049 is refused."""
    import numpy as np
    import torch
    ko, kh = published
    sh, osh = custom_shape(h2w, oracle, mode=1, d=9, q=2, cap=2)
    st = torch.cuda.current_stream().cuda_stream
    pr = h2w_api.Prover(sh, kh)
    POISON = 0x5A5A5A5A5A5A5A5A

    def batch(seeds):
        ins = [oracle.prove_fri_inputs(osh, sd) for sd in seeds]
        coefs = torch.from_numpy(np.concatenate([np.frombuffer(c, dtype=np.int64) for c, _ in ins])).cuda()
        pis = [int(x) for _, p_ in ins for x in list(p_)[:sh.n_pis]]
        proofs = torch.full((len(seeds) * pr.proof_words,), POISON, dtype=torch.int64, device="cuda")
        if len(seeds) == 1:
            pr.prove(coefs.data_ptr(), pis, proofs.data_ptr(), st)
        else:
            pr.prove_batch(coefs.data_ptr(), pis, proofs.data_ptr(), len(seeds), st)
        torch.cuda.synchronize()
        got = proofs.cpu().numpy().reshape(len(seeds), pr.proof_words)
        for i, (c, p_) in enumerate(ins):
            assert_words_equal(got[i], oracle.prove_fri_coef(osh, ko, c, p_), f"seeds {seeds}, proof {i}")
        return got, coefs, pis

    A = SEED + 200
    first, coefs, pis = batch([A])
    batch([A + 1, A + 2, A + 3])
    again, _, _ = batch([A])
    assert (first == again).all()
    batch([A + 4, A + 5])
    out = torch.full((pr.proof_words,), POISON, dtype=torch.int64, device="cuda")
    pr.prove_batch(coefs.data_ptr(), pis, out.data_ptr(), 0, st)
    torch.cuda.synchronize()
    assert (out == POISON).all()
    with pytest.raises(h2w_api.H2WError, match="at most 2048 proofs per call"):
        pr.prove_batch(coefs.data_ptr(), pis, out.data_ptr(), 2049, st)
    assert (out == POISON).all()
    pr.close()
