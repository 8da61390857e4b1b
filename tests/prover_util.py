"""Shared by the GPU tests that take shapes and proofs (tests/test_gpu_prover.py, tests/test_gpu_prover_shapes.py, tests/test_gpu_batch.py):
a shape off the Fibonacci defaults on both sides, one proof from the device prover, the word-for-word comparison with the oracle's
prover, and the chain prover -> witness generator -> oracle."""
import ctypes as C


def custom_shape(h2w, oracle, **kw):
    """A shape on both sides: d, q, rb, cap, mode, then any field of the shape by name; the rest are the Fibonacci defaults."""
    sh = h2w.fibonacci_shape(kw.pop("d"), kw.pop("q"), rate_bits=kw.pop("rb", 1), cap_height=kw.pop("cap", 4), hash_mode=kw.pop("mode", 1))
    osh = oracle.fibonacci_shape(sh.degree_bits, sh.num_queries, rate_bits=sh.rate_bits, cap_height=sh.cap_height, hash_mode=sh.hash_mode)
    for k, v in kw.items():
        setattr(sh, k, v); setattr(osh, k, v)
    return sh, osh


def prove_coefs(h2w_api, sh, kh, coefs, pis):
    """One proof of a fresh device prover for the given coefficients (a ctypes array, as the oracle's prover takes it), into a buffer
    in which an unwritten word would show; a shape without public inputs passes the null pointer h2w_prove_fri documents."""
    import numpy as np
    import torch
    pr = h2w_api.Prover(sh, kh)
    d_coefs = torch.from_numpy(np.frombuffer(coefs, dtype=np.int64).copy()).cuda()
    assert d_coefs.numel() == pr.num_polys << sh.degree_bits
    d_proof = torch.full((pr.proof_words,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    if sh.n_pis > 0:
        pr.prove(d_coefs.data_ptr(), list(pis)[:sh.n_pis], d_proof.data_ptr(), st)
    else:
        assert pr.L.h2w_prove_fri(pr.p, d_coefs.data_ptr(), None, d_proof.data_ptr(), st) == 0
    torch.cuda.synchronize()
    t = pr.timing(); pr.close()
    return d_proof, t


def gpu_prove(h2w, h2w_api, oracle, kh, sh, osh, seed):
    coefs, pis = oracle.prove_fri_inputs(osh, seed)
    d_proof, t = prove_coefs(h2w_api, sh, kh, coefs, pis)
    return coefs, pis, d_proof, t


def assert_words_equal(got, want, what="proof"):
    """got, want: the proof words (numpy uint64 / a ctypes array); the count and the first indices of the words that differ."""
    import numpy as np
    got = np.asarray(got).view(np.uint64); want = np.frombuffer(want, dtype=np.uint64)
    assert got.shape == want.shape, f"{what}: {got.shape} words, the oracle's has {want.shape}"
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(want)} proof words differ, first at {bad[:8]}"


def assert_chain(h2w_api, oracle, ko, kh, sh, osh, d_proof):
    """A device proof through the device witness generator: accepted (status 0), every gate and lookup holds on the device, the restated
    verifier and MockProver accept it (Merkle roots, fold consistency, final polynomial, PoW), and the advice equals the oracle's."""
    import torch
    plan = h2w_api.Plan(sh, kh)
    assert plan.proof_words == d_proof.numel()
    advice = torch.zeros(plan.num_cells * 32, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(plan.workspace_bytes(1), dtype=torch.uint8, device="cuda")
    plan.run(d_proof.data_ptr(), 1, advice.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert plan.status(ws.data_ptr(), 1) == [0]
    assert plan.check_constraints(advice.data_ptr(), 1) == (0, 0)
    ctx = oracle.Ctx(sh.lookup_bits, witness_gen_only=False)
    words = (C.c_uint64 * plan.proof_words).from_buffer_copy(d_proof.cpu().numpy().tobytes())
    assert oracle.verify_stark(ctx, osh, ko, words) == 0, ctx.error()
    mp = ctx.mock_prover()
    assert mp["bad"] == 0 and mp["semantic_failed"] == 0, mp
    assert advice.cpu().numpy().tobytes() == ctx.advice_bytes()
    ctx.close(); plan.close()
