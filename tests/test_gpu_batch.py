"""GPU parity, API level 3: h2w_fri_witness_batch (value kernels + expansion kernel on the MI355X) against the CPU
oracle's advice stream, byte for byte, on the same seeded synthetic proofs.  Small shapes compare every cell of
every proof; BASELINE.json's configs 1 and 3 (BN254 caps) are compared in full as well (the oracle needs seconds)."""
import ctypes as C

import pytest

from prover_util import custom_shape

pytestmark = pytest.mark.gpu


def run_batch(h2w, h2w_api, oracle, consts, shape_args, seeds, lookup_bits=21, wlrc=1, split_streams=False, valid=False, cap_height=4, passes=0, values_form=0):
    import torch
    ko, kh = consts
    sh = h2w.fibonacci_shape(*shape_args[:2], rate_bits=shape_args[2], hash_mode=shape_args[3], lookup_bits=lookup_bits, witness_load_range_check=wlrc, cap_height=cap_height)
    osh = oracle.fibonacci_shape(*shape_args[:2], rate_bits=shape_args[2], hash_mode=shape_args[3], lookup_bits=lookup_bits, witness_load_range_check=wlrc, cap_height=cap_height)
    plan = h2w_api.Plan(sh, kh)
    if passes:
        plan.configure(3, passes)          # H2W_OPT_CHAIN_PASSES
    if values_form:
        plan.configure(4, values_form)     # H2W_OPT_VALUES_FORM
    n = len(seeds)
    proofs = [oracle.prove_fri(osh, ko, s) if valid else oracle.synth_proof(osh, s) for s in seeds]   # valid: oracle/prover.inc
    host = torch.empty(n * plan.proof_words, dtype=torch.int64)
    for i, p in enumerate(proofs):
        host[i * plan.proof_words:(i + 1) * plan.proof_words] = torch.frombuffer(bytearray(bytes(p)), dtype=torch.int64)
    d_proofs = host.cuda()
    advice = torch.zeros(n * plan.num_cells * 32, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if split_streams:      # h2w_fri_witness_batch2: expansion kernel on its own stream, ordered by events
        emit = torch.cuda.Stream()
        plan.run(d_proofs.data_ptr(), n, advice.data_ptr(), ws.data_ptr(), stream, emit.cuda_stream)
    else:
        plan.run(d_proofs.data_ptr(), n, advice.data_ptr(), ws.data_ptr(), stream)
    torch.cuda.synchronize()
    assert plan.status(ws.data_ptr(), n, stream) == [0] * n
    got = advice.cpu().numpy().tobytes()
    for i, p in enumerate(proofs):
        ctx = oracle.Ctx(lookup_bits)
        assert oracle.verify_stark(ctx, osh, ko, p) == 0
        assert ctx.num_cells() == plan.num_cells
        want = ctx.advice_bytes()
        g = got[i * plan.num_cells * 32:(i + 1) * plan.num_cells * 32]
        if g != want:
            import numpy as np
            a = np.frombuffer(g, dtype=np.uint64).reshape(-1, 4); b = np.frombuffer(want, dtype=np.uint64).reshape(-1, 4)
            bad = np.nonzero((a != b).any(axis=1))[0]
            raise AssertionError(f"proof {i}: {len(bad)} cells differ, first at {bad[:8]}: got {a[bad[0]]} want {b[bad[0]]}")
        ctx.close()
    plan.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_small_shapes_every_cell(h2w, h2w_api, oracle, consts, mode):
    run_batch(h2w, h2w_api, oracle, consts, (6, 2, 1, mode), [1, 2, 3])          # no fold step, 2 queries
    run_batch(h2w, h2w_api, oracle, consts, (7, 3, 2, mode), [4])                # one fold step (the path no reference test exercises)
    run_batch(h2w, h2w_api, oracle, consts, (5, 1, 1, mode), [5, 6], wlrc=0)     # single query; SVG-era loader


@pytest.mark.parametrize("passes,form", [(1, 0), (2, 1), (2, 2)])
def test_merkle_paths_in_one_pass_and_in_two(h2w, h2w_api, oracle, consts, passes, form):
    """H2W_OPT_CHAIN_PASSES: the PoseidonBN254 Merkle paths as one kernel that walks and emits (1) or as a values pass plus one quad per
    permutation (2: every level of every path side by side) - the values pass in both of its forms (H2W_OPT_VALUES_FORM: four lanes per path, a
    Montgomery product on one lane | one wavefront per path, one 29-bit limb per lane: rowfr.h).  Same cells; the defaults pick by the size of the launch."""
    run_batch(h2w, h2w_api, oracle, consts, (8, 3, 2, 1), [61, 62, 63], passes=passes, values_form=form)          # one fold step, rate_bits 2
    run_batch(h2w, h2w_api, oracle, consts, (10, 4, 1, 1), [0xF1B00001], passes=passes, values_form=form)         # BASELINE configs[0]
    run_batch(h2w, h2w_api, oracle, consts, (4, 2, 1, 1), [64], passes=passes, cap_height=4, values_form=form)    # lde_bits 5: one-level paths, unit-less oracle strands


@pytest.mark.parametrize("form", [1, 2])
def test_values_pass_forms_on_the_published_tables_and_on_valid_proofs(h2w, h2w_api, oracle, consts, published, form):
    """Both forms of the values pass under the published circomlib tables and under the seeded full-width ones, on a valid FRI instance (every
    Merkle root then matches) and on random words; the last shape leaves the last block of four wavefronts partly filled."""
    run_batch(h2w, h2w_api, oracle, published, (9, 2, 1, 1), [43], valid=True, cap_height=2, passes=2, values_form=form)
    run_batch(h2w, h2w_api, oracle, published, (10, 4, 1, 1), [0xF1B00001, 0xF1B00002], passes=2, values_form=form)
    run_batch(h2w, h2w_api, oracle, consts, (7, 5, 2, 1), [71, 72, 73, 74, 75, 76, 77], passes=2, values_form=form)      # 35 units: partly filled blocks of four wavefronts


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("table", ["full_width", "largest_small", "just_beyond_small"])
def test_goldilocks_mds_tables_of_every_width(h2w, h2w_api, oracle, consts, mode, table):
    """The values phase walks a small-entry Goldilocks MDS matrix as two 64-bit sums and one reduction (csrc/glperm.h glq_mds_small: entries below 2^26,
    glcoop.h glp_small_mds) and any other with one multiply-add per entry: both paths, and the bound between them, against the oracle - the synthetic and
    the published tables are all tiny-entry ones.  Challenger permutations in both hash modes, Merkle permutations too with Goldilocks caps."""
    ko0, _ = consts
    ko = oracle.Consts.from_buffer_copy(bytes(ko0))
    p = 2**64 - 2**32 + 1
    for i in range(12):
        if table == "full_width":
            ko.mds_circ[i] = (0x9E3779B97F4A7C15 * (i + 1)) % p; ko.mds_diag[i] = (0xD1B54A32D192ED03 * (i + 3)) % p
        else:
            ko.mds_circ[i] = 2**26 - 1 - (i % 3); ko.mds_diag[i] = 2**26 - 1 if i in (0, 5) else 0
    if table == "just_beyond_small":
        ko.mds_circ[7] = 2**26
    kh = h2w.PoseidonConsts.from_buffer_copy(bytes(ko))
    run_batch(h2w, h2w_api, oracle, (ko, kh), (7, 3, 2, mode), [91, 92])          # one fold step
    run_batch(h2w, h2w_api, oracle, (ko, kh), (6, 2, 1, mode), [93], valid=True, cap_height=2)


@pytest.mark.parametrize("lookup_bits", [13, 8, 17])
def test_other_lookup_bits(h2w, h2w_api, oracle, consts, lookup_bits):
    run_batch(h2w, h2w_api, oracle, consts, (7, 2, 1, 1), [7], lookup_bits=lookup_bits)
    run_batch(h2w, h2w_api, oracle, consts, (6, 1, 1, 0), [8], lookup_bits=lookup_bits)


@pytest.mark.parametrize("mode", [1, 0])
def test_config1_full(h2w, h2w_api, oracle, consts, mode):
    """BASELINE.json configs[0]: 2^10 rows, 4 queries."""
    run_batch(h2w, h2w_api, oracle, consts, (10, 4, 1, mode), [0xF1B00001, 0xF1B00011])


@pytest.mark.parametrize("mode", [1, 0])
def test_separate_emit_stream(h2w, h2w_api, oracle, consts, mode):
    run_batch(h2w, h2w_api, oracle, consts, (8, 3, 1, mode), [21, 22, 23], split_streams=True)


@pytest.mark.parametrize("mode", [1, 0])
def test_valid_fri_proofs(h2w, h2w_api, oracle, consts, mode):
    """Same byte-for-byte parity on VALID FRI instances (every value then sits on the accepting path: Merkle roots match,
    fold steps agree, PoW response has its leading zeros) — the oracle's MockProver is all-green on these inputs
    (tests/test_oracle_valid_proof.py)."""
    run_batch(h2w, h2w_api, oracle, consts, (6, 3, 1, mode), [31, 32], valid=True, cap_height=2)
    run_batch(h2w, h2w_api, oracle, consts, (9, 2, 1, mode), [33], valid=True, cap_height=2)     # one fold step


@pytest.mark.parametrize("mode", [1, 0])
def test_published_poseidon_tables(h2w, h2w_api, oracle, published, mode):
    """The batched path under the published parameter sets (plonky2 Goldilocks / circomlib BN254 tables, pinned to published
    known-answer vectors in tests/test_poseidon_published.py): valid FRI instances with and without a fold step, and BASELINE
    configs[0]'s shape (2^10 rows, 4 queries) on random words, byte for byte."""
    run_batch(h2w, h2w_api, oracle, published, (6, 3, 1, mode), [41, 42], valid=True, cap_height=2)
    run_batch(h2w, h2w_api, oracle, published, (9, 2, 1, mode), [43], valid=True, cap_height=2)
    run_batch(h2w, h2w_api, oracle, published, (10, 4, 1, mode), [0xF1B00001])


def test_config3_bn254_full(h2w, h2w_api, oracle, consts):
    """BASELINE.json configs[2]: 2^20 rows, 28 queries, cap_height 4, PoseidonBN254 Merkle — 28.58 M cells, every byte."""
    run_batch(h2w, h2w_api, oracle, consts, (20, 28, 1, 1), [0xF1B00003])


def test_config2_bn254_full(h2w, h2w_api, oracle, consts):
    """BASELINE.json configs[1]: 2^16 rows, 28 queries, rate_bits 2."""
    run_batch(h2w, h2w_api, oracle, consts, (16, 28, 2, 1), [0xF1B00002])


def run_custom(h2w, h2w_api, oracle, consts, seeds, valid=False, **kw):
    import torch
    ko, kh = consts
    sh, osh = custom_shape(h2w, oracle, **kw)
    plan = h2w_api.Plan(sh, kh)
    n = len(seeds)
    proofs = [oracle.prove_fri(osh, ko, s) if valid else oracle.synth_proof(osh, s) for s in seeds]   # valid: oracle/prover.inc
    host = torch.empty(n * plan.proof_words, dtype=torch.int64)
    for i, p in enumerate(proofs):
        host[i * plan.proof_words:(i + 1) * plan.proof_words] = torch.frombuffer(bytearray(bytes(p)), dtype=torch.int64)
    d_proofs = host.cuda()
    advice = torch.zeros(n * plan.num_cells * 32, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    plan.run(d_proofs.data_ptr(), n, advice.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    status = plan.status(ws.data_ptr(), n)
    got = advice.cpu().numpy().tobytes()
    outs = []
    for i, p in enumerate(proofs):
        ctx = oracle.Ctx(sh.lookup_bits)
        rc = oracle.verify_stark(ctx, osh, ko, p)
        outs.append((rc, ctx.error(), ctx.num_cells(), ctx.advice_bytes() == got[i * plan.num_cells * 32:(i + 1) * plan.num_cells * 32]))
        ctx.close()
    nc = plan.num_cells
    plan.close()
    return status, outs, nc


@pytest.mark.parametrize("mode", [1, 0])
def test_shape_edge_cases(h2w, h2w_api, oracle, consts, mode):
    """Shapes the reference supports but never tests: no permutation argument (2 oracles), cap_height 0 (verify_proof,
    merkle/mod.rs:104-115), other pow bits / arity / column counts, one query."""
    cases = [dict(d=6, q=2, n_perm_z=0), dict(d=6, q=1, cap=0), dict(d=8, q=2, rb=2, cap=2, arity_bits=2, final_poly_bits=3),
             dict(d=6, q=2, pow_bits=10, n_cols=6, n_quotient=4, n_pis=1, num_challenges=3), dict(d=9, q=2, rb=3, cap=1, arity_bits=3),
             dict(d=5, q=2, cap=1, arity_bits=1, final_poly_bits=2),      # (arity 2: every size of the tabulated FRI constants, chips.h FriTab, is walked by some case)
             dict(d=10, q=2, cap=1, arity_bits=1, final_poly_bits=2)]     # exactly MAX_STEPS = 8 fold steps: every slot of the per-step arrays
    for kw in cases:
        status, outs, nc = run_custom(h2w, h2w_api, oracle, consts, [11, 12], mode=mode, **kw)
        assert status == [0, 0], (kw, status)
        for rc, err, n, same in outs:
            assert rc == 0 and n == nc and same, (kw, rc, err, n, nc, same)
    # and one of them on a valid instance (two fold steps of arity 4)
    status, outs, nc = run_custom(h2w, h2w_api, oracle, consts, [13], valid=True, mode=mode, **cases[2])
    assert status == [0] and all(rc == 0 and n == nc and same for rc, err, n, same in outs)
    # and the eight fold steps on a valid instance
    status, outs, nc = run_custom(h2w, h2w_api, oracle, consts, [14], valid=True, mode=mode, **cases[6])
    assert status == [0] and all(rc == 0 and n == nc and same for rc, err, n, same in outs)


@pytest.mark.parametrize("mode", [1, 0])
def test_noncanonical_proof_words_are_flagged(h2w, h2w_api, oracle, consts, mode):
    """Words the reference's types cannot hold (a Goldilocks word >= p, a BN254 hash >= r): status 4.  Goldilocks words still give
    the oracle's cells (both sides compute on the raw 64-bit value); in-range proofs keep status 0."""
    import random
    import torch
    ko, kh = consts
    P = 2**64 - 2**32 + 1
    sh = h2w.fibonacci_shape(6, 2, hash_mode=mode); osh = oracle.fibonacci_shape(6, 2, hash_mode=mode)
    plan = h2w_api.Plan(sh, kh)
    rnd = random.Random(3)
    for trial in range(3):
        pr = oracle.synth_proof(osh, 100 + trial)
        if trial:                         # trial 0: untouched
            for _ in range(10):
                i = rnd.randrange(len(pr))
                pr[i] = rnd.choice([P, P + 1, 2**64 - 1])
        d_proofs = torch.frombuffer(bytearray(bytes(pr)), dtype=torch.int64).cuda()
        advice = torch.zeros(plan.num_cells * 32, dtype=torch.uint8, device="cuda")
        ws = torch.zeros(plan.workspace_bytes(1), dtype=torch.uint8, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        plan.run(d_proofs.data_ptr(), 1, advice.data_ptr(), ws.data_ptr(), st)
        torch.cuda.synchronize()
        assert plan.status(ws.data_ptr(), 1, st) == [4 if trial else 0]
        if mode == 0 or trial == 0:
            ctx = oracle.Ctx(21)
            assert oracle.verify_stark(ctx, osh, ko, pr) == 0
            assert ctx.advice_bytes() == advice.cpu().numpy().tobytes()
            ctx.close()
    plan.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_cap_height_five(h2w, h2w_api, oracle, consts, mode):
    """A 32-entry Merkle cap (cap_height 5; the reference's standard_fast_config has 4, nothing in it bounds the height): the cap's
    select_from_idx is 8 + 12 * 31 + 1 + 3 * 32 cells per hash element."""
    run_batch(h2w, h2w_api, oracle, consts, (7, 2, 1, mode), [91, 92], cap_height=5)
    run_batch(h2w, h2w_api, oracle, consts, (8, 2, 2, mode), [93], cap_height=6)          # 64 entries, one fold step


@pytest.mark.parametrize("mode", [1, 0])
def test_packed_shard_layout(h2w, h2w_api, oracle, consts, mode):
    """h2w_fri_witness_batch_shard_compact: a rank's buffer holds only its own blocks, back to back (1 / world of the stream).  Every block
    of every rank equals the oracle's cells of that block, the ranks' blocks cover every proof exactly once, and nothing is written
    outside them."""
    import numpy as np
    import torch
    ko, kh = consts
    sh = h2w.fibonacci_shape(7, 5, rate_bits=2, hash_mode=mode); osh = oracle.fibonacci_shape(7, 5, rate_bits=2, hash_mode=mode)
    plan = h2w_api.Plan(sh, kh)
    n, world = 5, 3
    proofs = [oracle.synth_proof(osh, 140 + i) for i in range(n)]
    host = torch.empty(n * plan.proof_words, dtype=torch.int64)
    for i, p in enumerate(proofs):
        host[i * plan.proof_words:(i + 1) * plan.proof_words] = torch.frombuffer(bytearray(bytes(p)), dtype=torch.int64)
    d_proofs = host.cuda()
    st = torch.cuda.current_stream().cuda_stream
    want = []
    for p in proofs:
        ctx = oracle.Ctx(21, track_scopes=False)
        assert oracle.verify_stark(ctx, osh, ko, p) == 0
        want.append(np.frombuffer(ctx.advice_bytes(), dtype=np.int64).reshape(plan.num_cells, 4)); ctx.close()
    covered = np.zeros((n, plan.num_cells), dtype=np.int32)
    total = 0
    for rank in range(world):
        cells = plan.shard_cells(n, rank, world); total += cells
        buf = torch.full((cells + 8, 4), -1, dtype=torch.int64, device="cuda")          # 8 guard cells behind the buffer
        ws = torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda")
        plan.run_shard_compact(d_proofs.data_ptr(), n, buf.data_ptr(), ws.data_ptr(), rank, world, st)
        torch.cuda.synchronize()
        assert plan.status(ws.data_ptr(), n, st) == [0] * n
        got = buf.cpu().numpy()
        assert (got[cells:] == -1).all()
        used = np.zeros(cells, dtype=bool)
        for p_ in range(n):
            for q in range(-1, sh.num_queries):
                blk = plan.shard_block(rank, world, p_, q)
                owner = (p_ % world) if q < 0 else (p_ * sh.num_queries + q) % world
                assert (blk is not None) == (owner == rank)
                if blk is None:
                    continue
                lo, cnt, g = blk
                assert (got[lo:lo + cnt] == want[p_][g:g + cnt]).all(), (rank, p_, q)
                assert not used[lo:lo + cnt].any(); used[lo:lo + cnt] = True
                covered[p_, g:g + cnt] += 1
        assert (got[:cells][~used] == -1).all()              # (slack of a query slot: untouched)
    assert (covered == 1).all()
    assert total < n * plan.num_cells + n * sh.num_queries + world          # no more than the stream plus one slack cell per query block
    plan.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_packed_shard_layout_at_the_bench_launch_size(h2w, h2w_api, oracle, consts, mode):
    """The schedule bench.py --shard-queries / --emulate-rank runs (VERDICT r03 task 1): a launch covers batch x world proofs, so that a rank of 8
    has more than 512 (proof, query) units - the size at which the library walks the PoseidonBN254 Merkle paths in ONE pass (k_merkle_bn_fused) -,
    its workspace is h2w_plan_shard_workspace_bytes (unit buffers of its own units only), its advice the packed buffer.  Every block of two ranks
    equals the same block of the unsharded GPU stream of the same proofs, and that stream equals the oracle's for a sample of the proofs."""
    import numpy as np
    import torch
    ko, kh = consts
    nq, world = 5, 8
    sh = h2w.fibonacci_shape(6, nq, rate_bits=2, hash_mode=mode); osh = oracle.fibonacci_shape(6, nq, rate_bits=2, hash_mode=mode)
    plan = h2w_api.Plan(sh, kh)
    n = 824 if mode == 1 else 48                    # 824 x 5 = 4120 units: 515 per rank
    words = plan.proof_words
    prng = np.random.default_rng(77)
    host = torch.from_numpy(prng.integers(0, 1 << 60, n * words, dtype=np.int64))
    d_proofs = host.cuda()
    st = torch.cuda.current_stream().cuda_stream
    full = torch.zeros((n, plan.num_cells, 4), dtype=torch.int64, device="cuda")
    ws = torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    plan.run(d_proofs.data_ptr(), n, full.data_ptr(), ws.data_ptr(), st)
    torch.cuda.synchronize()
    assert plan.status(ws.data_ptr(), n, st) == [0] * n
    if mode == 1:
        assert int(plan.timing_ex(0)[7]) == 1
    for i in (0, 1, n // 2, n - 1):                # the unsharded stream against the oracle
        import ctypes
        ctx = oracle.Ctx(21, track_scopes=False)
        pr = (ctypes.c_uint64 * words).from_buffer_copy(host[i * words:(i + 1) * words].numpy().tobytes())
        assert oracle.verify_stark(ctx, osh, ko, pr) == 0
        assert full[i].cpu().numpy().tobytes() == ctx.advice_bytes(), i
        ctx.close()
    del ws
    for rank in (0, 5):
        cells = plan.shard_cells(n, rank, world)
        wbytes = plan.shard_workspace_bytes(n, rank, world)
        assert wbytes <= plan.workspace_bytes(n)
        if mode == 1:
            assert wbytes < plan.workspace_bytes(n)      # the unit buffers are the rank's own
        buf = torch.full((cells + 8, 4), -1, dtype=torch.int64, device="cuda")
        ws = torch.zeros(wbytes + 256, dtype=torch.uint8, device="cuda"); ws[wbytes:] = 0x5A      # guard bytes behind the workspace
        plan.run_shard_compact(d_proofs.data_ptr(), n, buf.data_ptr(), ws.data_ptr(), rank, world, st)
        torch.cuda.synchronize()
        assert plan.status(ws.data_ptr(), n, st) == [0] * n
        assert (ws[wbytes:] == 0x5A).all()
        if mode == 1:
            assert int(plan.timing_ex(0)[7]) == 1          # more than 512 units of this rank: the one-pass paths
        assert (buf[cells:] == -1).all()
        for p_ in range(n):
            for q in range(-1, nq):
                blk = plan.shard_block(rank, world, p_, q)
                owner = (p_ % world) if q < 0 else (p_ * nq + q) % world
                assert (blk is not None) == (owner == rank)
                if blk is None:
                    continue
                lo, cnt, g = blk
                assert torch.equal(buf[lo:lo + cnt], full[p_, g:g + cnt]), (rank, p_, q)
        del buf, ws
    plan.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_query_sharding_union_is_the_full_stream(h2w, h2w_api, oracle, consts, mode):
    """(proof, query) units dealt round-robin to the ranks, the prologue block of a proof to rank proof mod world (every
    rank still computes every prologue's VALUES: it needs the challenges).  A rank's buffer holds its own blocks only (the rest
    stays as it was: zero here); the blocks of different ranks are disjoint and their union is byte-for-byte the oracle's stream."""
    import numpy as np
    import torch
    D = importlib_distributed()
    ko, kh = consts
    sh = h2w.fibonacci_shape(7, 5, rate_bits=2, hash_mode=mode); osh = oracle.fibonacci_shape(7, 5, rate_bits=2, hash_mode=mode)
    plan = h2w_api.Plan(sh, kh)
    n, world = 3, 4
    proofs = [oracle.synth_proof(osh, 40 + i) for i in range(n)]
    host = torch.empty(n * plan.proof_words, dtype=torch.int64)
    for i, p in enumerate(proofs):
        host[i * plan.proof_words:(i + 1) * plan.proof_words] = torch.frombuffer(bytearray(bytes(p)), dtype=torch.int64)
    d_proofs = host.cuda()
    st = torch.cuda.current_stream().cuda_stream
    parts = []
    for rank in range(world):
        advice = torch.zeros(n * plan.num_cells * 4, dtype=torch.int64, device="cuda")
        ws = torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda")
        plan.run_shard(d_proofs.data_ptr(), n, advice.data_ptr(), ws.data_ptr(), rank, world, st)
        torch.cuda.synchronize()
        assert plan.status(ws.data_ptr(), n, st) == [0] * n
        parts.append(advice.cpu().numpy().reshape(n, plan.num_cells, 4))
    want = []
    for p in proofs:
        ctx = oracle.Ctx(21, track_scopes=False)
        assert oracle.verify_stark(ctx, osh, ko, p) == 0
        want.append(np.frombuffer(ctx.advice_bytes(), dtype=np.int64).reshape(plan.num_cells, 4)); ctx.close()
    want = np.stack(want)
    union = np.zeros_like(want)
    touched = np.zeros((n, plan.num_cells), dtype=np.int32)
    for part in parts:
        touched += (part != 0).any(axis=2)
        union |= part
    assert (union == want).all()
    assert set(np.unique(touched)) <= {0, 1}              # every non-zero cell has exactly one writer: the ranks' blocks are disjoint
    nq = sh.num_queries
    wrote = [((part != 0).any(axis=2)) for part in parts]
    for rank in range(world):
        mine = D.my_units(n, nq, rank, world)
        assert wrote[rank].sum() > 0 and len(mine) in (n * nq // world, n * nq // world + 1)
        for p_ in range(n):      # a rank that owns neither a unit nor the prologue of a proof writes nothing of it
            if not any(pp == p_ for pp, _ in mine) and D.prologue_owner(p_, world) != rank:
                assert wrote[rank][p_].sum() == 0
    # the prologue block (the cells before the first query block) of proof p comes from rank p mod world alone
    first_query_cell = min(int(np.argmax(wrote[r][0])) for r in range(world) if r != D.prologue_owner(0, world) and wrote[r][0].any())
    assert wrote[D.prologue_owner(0, world)][0][:first_query_cell].sum() > 0
    for r in range(world):
        if r != D.prologue_owner(0, world):
            assert wrote[r][0][:first_query_cell].sum() == 0
    plan.close()


def importlib_distributed():
    import importlib
    return importlib.import_module("halo2-plonky2-verifier_amd.distributed")


def test_montgomery_form_output(h2w, h2w_api, oracle, consts):
    """h2w_advice_to_montgomery: every cell becomes v * 2^256 mod r (halo2curves' in-memory Fr); checked against Python integers
    on the whole stream of a small proof, and the conversion is a bijection (distinct digests, status untouched)."""
    import numpy as np
    import torch
    ko, kh = consts
    R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    sh = h2w.fibonacci_shape(5, 1, hash_mode=1); osh = oracle.fibonacci_shape(5, 1, hash_mode=1)
    plan = h2w_api.Plan(sh, kh)
    pr = oracle.synth_proof(osh, 77)
    d_proofs = torch.frombuffer(bytearray(bytes(pr)), dtype=torch.int64).cuda()
    advice = torch.zeros(plan.num_cells * 32, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(plan.workspace_bytes(1), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    plan.run(d_proofs.data_ptr(), 1, advice.data_ptr(), ws.data_ptr(), st)
    torch.cuda.synchronize()
    canon = advice.cpu().numpy().tobytes()
    assert h2w.lib().h2w_advice_to_montgomery(advice.data_ptr(), plan.num_cells, st) == 0
    torch.cuda.synchronize()
    mont = advice.cpu().numpy().tobytes()
    rng = np.random.default_rng(1)
    idx = np.concatenate([np.arange(0, 2000), rng.integers(0, plan.num_cells, 20000), np.arange(plan.num_cells - 2000, plan.num_cells)])
    for i in idx:
        v = int.from_bytes(canon[32 * i:32 * i + 32], "little")
        assert int.from_bytes(mont[32 * i:32 * i + 32], "little") == (v << 256) % R, int(i)
    plan.close()


def test_device_status_where_reference_panics(h2w, h2w_api, oracle, consts):
    """GoldilocksChip::div asserts b != 0 (base.rs:379); ext inv of 0 likewise.  A proof crafted to hit it (subgroup_x - zeta
    = 0 cannot be forced without the challenger, so use scalar_div by a zero coset start: not reachable either) -> instead
    check the status word stays 0 on ordinary proofs and the API reports a bad plan / buffers loudly."""
    import torch
    ko, kh = consts
    plan = h2w_api.Plan(h2w.fibonacci_shape(6, 2), kh)
    with pytest.raises(h2w_api.H2WError):
        plan.run(0, 1, 0, 0, 0)                       # null buffers
    bad = h2w.fibonacci_shape(6, 2); bad.lookup_bits = 40
    with pytest.raises(h2w_api.H2WError):
        h2w_api.Plan(bad, kh)
    bad = h2w.fibonacci_shape(6, 200)
    with pytest.raises(h2w_api.H2WError):
        h2w_api.Plan(bad, kh)
    plan.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_expand_records_alone_rewrites_the_same_cells(h2w, h2w_api, oracle, consts, mode):
    """h2w_fri_expand_records (the expansion kernel alone, used by bench.py's roofline leg): wiping every cell and re-expanding the
    records left in the workspace restores exactly the cells that come from block records; the cells the value kernels write
    directly stay wiped, and their number is num_cells - num_record_cells."""
    import numpy as np
    import torch
    ko, kh = consts
    sh = h2w.fibonacci_shape(8, 3, rate_bits=1, hash_mode=mode); osh = oracle.fibonacci_shape(8, 3, rate_bits=1, hash_mode=mode)
    plan = h2w_api.Plan(sh, kh)
    proofs = [oracle.synth_proof(osh, s) for s in (5, 6)]
    host = torch.cat([torch.frombuffer(bytearray(bytes(p)), dtype=torch.int64) for p in proofs]).cuda()
    advice = torch.zeros(2 * plan.num_cells * 32, dtype=torch.uint8, device="cuda"); ws = torch.zeros(plan.workspace_bytes(2), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    plan.run(host.data_ptr(), 2, advice.data_ptr(), ws.data_ptr(), st); torch.cuda.synchronize()
    full = advice.cpu().numpy().reshape(2 * plan.num_cells, 32).copy()
    advice.fill_(0xEE)
    plan.expand_records(2, advice.data_ptr(), ws.data_ptr(), st); torch.cuda.synchronize()
    again = advice.cpu().numpy().reshape(2 * plan.num_cells, 32)
    wiped = (again == 0xEE).all(axis=1)
    assert int(wiped.sum()) == 2 * (plan.num_cells - plan.num_record_cells)
    assert (again[~wiped] == full[~wiped]).all()
    plan.close()


def test_two_plans_with_different_tables_interleaved_on_two_streams(h2w, h2w_api, oracle, consts, published):
    """Distinct handles are independent (include/h2w.h): two PoseidonBN254 plans of the same shape with DIFFERENT Poseidon tables (the
    seeded synthetic set and the published one) run concurrently, interleaved over two streams, each launch into its own buffers;
    every launch's stream equals the oracle's for its own tables.  (The tables are per-plan device buffers staged into LDS by the chain
    kernel; round 1 kept them in one process-wide __constant__ symbol, which two such plans would have raced on.)"""
    import torch
    (ko_a, kh_a), (ko_b, kh_b) = consts, published
    sh = h2w.fibonacci_shape(8, 3, rate_bits=1, hash_mode=1, cap_height=2); osh = oracle.fibonacci_shape(8, 3, rate_bits=1, hash_mode=1, cap_height=2)
    plans = [h2w_api.Plan(sh, kh_a), h2w_api.Plan(sh, kh_b)]
    kos = [ko_a, ko_b]
    n, rounds = 2, 3
    proofs = [oracle.synth_proof(osh, 500 + i) for i in range(n)]
    host = torch.empty(n * plans[0].proof_words, dtype=torch.int64)
    for i, p in enumerate(proofs):
        host[i * plans[0].proof_words:(i + 1) * plans[0].proof_words] = torch.frombuffer(bytearray(bytes(p)), dtype=torch.int64)
    d_proofs = host.cuda()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    torch.cuda.synchronize()
    for r in range(rounds):
        for k in (0, 1):
            advice = torch.zeros(n * plans[k].num_cells * 32, dtype=torch.uint8, device="cuda")
            ws = torch.zeros(plans[k].workspace_bytes(n), dtype=torch.uint8, device="cuda")
            outs.append((k, advice, ws))
    torch.cuda.synchronize()
    for j, (k, advice, ws) in enumerate(outs):                       # all launches enqueued before anything is waited for
        plans[k].run(d_proofs.data_ptr(), n, advice.data_ptr(), ws.data_ptr(), streams[(j + k) % 2].cuda_stream)
    torch.cuda.synchronize()
    want = []
    for k in (0, 1):
        w = b""
        for p in proofs:
            ctx = oracle.Ctx(21)
            assert oracle.verify_stark(ctx, osh, kos[k], p) == 0
            w += ctx.advice_bytes(); ctx.close()
        want.append(w)
    assert want[0] != want[1]
    for k, advice, ws in outs:
        assert plans[k].status(ws.data_ptr(), n) == [0] * n
        assert advice.cpu().numpy().tobytes() == want[k]
    for pl in plans:
        pl.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
def test_scheduling_options_do_not_change_the_cells(h2w, h2w_api, oracle, consts, mode):
    """H2W_OPT_FORK_CHAINS / H2W_OPT_SERIAL_EXPAND only move kernels between streams and order them with events: one plan driven on
    three streams with every combination of the two options, all launches enqueued before anything is waited for, each launch into
    its own buffers; every launch's stream is the oracle's."""
    import torch
    ko, kh = consts
    sh = h2w.fibonacci_shape(8, 3, rate_bits=1, hash_mode=mode, cap_height=1); osh = oracle.fibonacci_shape(8, 3, rate_bits=1, hash_mode=mode, cap_height=1)
    plan = h2w_api.Plan(sh, kh)
    n = 3
    proofs = [oracle.synth_proof(osh, 900 + i) for i in range(n)]
    host = torch.empty(n * plan.proof_words, dtype=torch.int64)
    for i, p in enumerate(proofs):
        host[i * plan.proof_words:(i + 1) * plan.proof_words] = torch.frombuffer(bytearray(bytes(p)), dtype=torch.int64)
    d_proofs = host.cuda()
    want = b""
    for p in proofs:
        ctx = oracle.Ctx(21)
        assert oracle.verify_stark(ctx, osh, ko, p) == 0
        want += ctx.advice_bytes(); ctx.close()
    streams = [torch.cuda.Stream() for _ in range(3)]
    outs = []
    for fork in (1, 0):
        for serial in (1, 0, -1):
            for s in range(3):
                outs.append((fork, serial, s, torch.zeros(n * plan.num_cells * 32, dtype=torch.uint8, device="cuda"),
                             torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda")))
    torch.cuda.synchronize()
    for fork, serial, s, advice, ws in outs:
        plan.configure(1, fork); plan.configure(2, serial)         # include/h2w.h: H2W_OPT_FORK_CHAINS = 1, H2W_OPT_SERIAL_EXPAND = 2
        plan.run(d_proofs.data_ptr(), n, advice.data_ptr(), ws.data_ptr(), streams[s].cuda_stream)
    torch.cuda.synchronize()
    for fork, serial, s, advice, ws in outs:
        assert plan.status(ws.data_ptr(), n) == [0] * n
        assert advice.cpu().numpy().tobytes() == want, (fork, serial, s)
    with pytest.raises(Exception):
        plan.configure(99, 0)
    # the library's event accessor (H2W_EV_*: 6 / 7 = expansion start / end, 0 / 8 = call start / end): with the expansion kernels serialised the
    # next one never starts before the previous one ended, whatever stream it is on
    plan.configure(1, 1); plan.configure(2, 1)
    for _, _, s, advice, ws in outs[:6]:
        plan.run(d_proofs.data_ptr(), n, advice.data_ptr(), ws.data_ptr(), streams[s].cuda_stream)
    torch.cuda.synchronize()
    for back in range(5):
        assert plan.event_gap(back, 6, back, 7) > 0 and plan.event_gap(back, 0, back, 8) > 0
        assert plan.event_gap(back + 1, 7, back, 6) >= 0
    with pytest.raises(Exception):
        plan.event_gap(0, 0, 0, 99)
    plan.close()


@pytest.mark.gpu
def test_comm_world_of_one(h2w, h2w_api):
    """h2w_comm_* on the one GPU of the test box: a world of one rank (RCCL refuses two ranks on one device) - id, init, the in-place
    proof broadcast and the digest all-gather run through RCCL and leave the data as it was."""
    import importlib
    import torch
    D = importlib.import_module("halo2-plonky2-verifier_amd.distributed")
    L = h2w.lib()
    ident = D.Comm.unique_id(L)
    assert len(ident) == 128
    comm = D.Comm(L, ident, 0, 1, 0)
    assert L.h2w_comm_rank(comm.p) == 0 and L.h2w_comm_world(comm.p) == 1
    proofs = torch.arange(1, 4097, dtype=torch.int64, device="cuda")
    want = proofs.clone()
    comm.broadcast_proofs(proofs)
    dig = torch.tensor([11, 22, 33, 44], dtype=torch.int64, device="cuda"); out = torch.zeros(4, dtype=torch.int64, device="cuda")
    comm.allgather_digests(dig, out)
    torch.cuda.synchronize()
    assert torch.equal(proofs, want) and torch.equal(out, dig)
    with pytest.raises(RuntimeError):
        comm.broadcast_proofs(proofs, root=1)
    comm.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_two_ranks_over_rccl(h2w, h2w_api, oracle, consts, mode, tmp_path):
    """The multi-rank path on real hardware (needs two GPUs: skipped on the one-GPU test box, where RCCL refuses two ranks on one device): two fresh
    processes, one per GPU - h2w_comm_init over RCCL, ONE broadcast of the proof block from rank 0, h2w_fri_witness_batch_shard_compact on each
    rank, all-gather of the digests of the ranks' packed buffers - every rank ends with both digests, and each equals the checksum of that rank's
    blocks of the oracle's streams."""
    import json
    import os
    import subprocess
    import sys
    import numpy as np
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    ko, kh = consts
    n, world = 3, 2
    here = os.path.dirname(os.path.abspath(__file__))
    idf = str(tmp_path / "comm.id")
    procs = [subprocess.Popen([sys.executable, os.path.join(here, "_comm_rank.py"), str(r), str(world), idf, str(mode), str(n)], stdout=subprocess.PIPE, text=True) for r in range(world)]
    outs = [json.loads(p.communicate(timeout=600)[0].strip().splitlines()[-1]) for p in procs]
    assert all(p.returncode == 0 for p in procs)
    assert outs[0]["digests"] == outs[1]["digests"] and outs[0]["proof_checksum"] == outs[1]["proof_checksum"]
    assert all(o["status"] == [0] * n for o in outs)
    sh = h2w.fibonacci_shape(7, 5, rate_bits=2, hash_mode=mode); osh = oracle.fibonacci_shape(7, 5, rate_bits=2, hash_mode=mode)
    plan = h2w_api.Plan(sh, kh)
    streams = []
    for i in range(n):
        ctx = oracle.Ctx(21, track_scopes=False)
        assert oracle.verify_stark(ctx, osh, ko, oracle.synth_proof(osh, 900 + i)) == 0
        streams.append(np.frombuffer(ctx.advice_bytes(), dtype=np.uint64).reshape(-1, 4).copy()); ctx.close()
    for rank in range(world):
        packed = np.zeros((plan.shard_cells(n, rank, world), 4), dtype=np.uint64)
        for p_ in range(n):
            for q in range(-1, sh.num_queries):
                blk = plan.shard_block(rank, world, p_, q)
                if blk is not None:
                    packed[blk[0]:blk[0] + blk[1]] = streams[p_][blk[2]:blk[2] + blk[1]]
        assert outs[0]["digests"][4 * rank:4 * rank + 4] == h2w_api.advice_digest_reference(packed), rank
    plan.close()
