"""Traced plans with H2W_TRACE_FUSE_GL_PERMUTE (include/h2w.h 2d, Plan.from_trace(fuse_consts=...)): every stretch of the tape that the lowering
verifies to be a Goldilocks-Poseidon permutation on the given tables runs as ONE device op (values on the lane, records by a wavefront per listed
permutation); everything else - other tables, a value that escapes - stays interpreted.  The stream is the oracle's / the unfused plan's / an eager
run's byte for byte either way; trace_info() says what was fused."""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GL_P = 2**64 - 2**32 + 1


# ---------------------------------------------------------------------------------------------------------------- whole verifier
def _oracle_perm_count(oracle, osh, ko, proof, lookup_bits):
    """Goldilocks-Poseidon permutations of the shape, from the oracle's scope tree: every one opens exactly one "mds_partial_layer_init" scope
    (hash/poseidon/permutation.rs:108-132; PoseidonBN254 has none) of a fixed size, measured on a single permutation."""
    L = oracle.lib()
    one = oracle.Ctx(lookup_bits, track_scopes=True)
    ins = (oracle.AV * 12)(*[L.orc_gl_load_constant(one.p, i) for i in range(12)]); outs = (oracle.AV * 12)()
    L.orc_gl_poseidon_permute(one.p, C.byref(ko), ins, outs)
    unit = sum(v for k, v in one.scopes().items() if k.split(";")[-1] == "mds_partial_layer_init"); one.close()
    assert unit > 0
    o = oracle.Ctx(lookup_bits, track_scopes=True)
    assert oracle.verify_stark(o, osh, ko, proof) == 0
    total = sum(v for k, v in o.scopes().items() if k.split(";")[-1] == "mds_partial_layer_init"); o.close()
    assert total % unit == 0
    return total // unit


def _upload(proofs, words):
    import torch
    host = torch.empty(len(proofs) * words, dtype=torch.int64)
    for i, p in enumerate(proofs):
        host[i * words:(i + 1) * words] = torch.frombuffer(bytearray(bytes(p)), dtype=torch.int64)
    return host.cuda()


def trace_and_replay_fused(h2w, h2w_api, oracle, consts, shape_args, seed_a, seeds, cap_height=4, valid=False, lookup_bits=21):
    """The pattern of tests/test_gpu_replay.py trace_and_replay, on a fused plan; also: what was fused, and the unfused plan's size."""
    import torch
    ko, kh = consts
    sh = h2w.fibonacci_shape(*shape_args[:2], rate_bits=shape_args[2], hash_mode=shape_args[3], cap_height=cap_height, lookup_bits=lookup_bits)
    osh = oracle.fibonacci_shape(*shape_args[:2], rate_bits=shape_args[2], hash_mode=shape_args[3], cap_height=cap_height, lookup_bits=lookup_bits)
    mk = (lambda s: oracle.prove_fri(osh, ko, s)) if valid else (lambda s: oracle.synth_proof(osh, s))
    proof_a = mk(seed_a)
    ctx = h2w_api.Context(lookup_bits, True, 0)
    ctx.trace_begin()
    h2w_api.verify_stark(ctx, sh, kh, np.frombuffer(bytes(proof_a), dtype=np.uint64))
    unfused = h2w_api.Plan.from_trace(ctx, len(proof_a))
    plan = h2w_api.Plan.from_trace(ctx, len(proof_a), fuse_consts=kh)
    assert plan.num_cells == ctx.num_cells() == unfused.num_cells and plan.proof_words == len(proof_a)
    ctx.close()
    info = plan.trace_info(); info0 = unfused.trace_info()
    assert info0["fused"] == 0 and info0["candidates_left"] == 0 and info0["list_entries"] == 0
    assert info["fused"] == _oracle_perm_count(oracle, osh, ko, proof_a, lookup_bits) and info["candidates_left"] == 0 and info["list_entries"] == info["fused"]
    assert info["ops"] == info0["ops"] and info["segments"] == info0["segments"]
    unfused.close()
    proofs = [proof_a] + [mk(s) for s in seeds]
    n = len(proofs)
    d_proofs = _upload(proofs, plan.proof_words)
    advice = torch.zeros(n * plan.num_cells * 32, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    plan.run(d_proofs.data_ptr(), n, advice.data_ptr(), ws.data_ptr(), st)
    torch.cuda.synchronize()
    assert plan.status(ws.data_ptr(), n, st) == [0] * n
    got = advice.cpu().numpy().tobytes()
    nb = plan.num_cells * 32
    for i, p in enumerate(proofs):
        o = oracle.Ctx(lookup_bits, track_scopes=False)
        assert oracle.verify_stark(o, osh, ko, p) == 0
        want = o.advice_bytes(); o.close()
        g = got[i * nb:(i + 1) * nb]
        if g != want:
            a = np.frombuffer(g, dtype=np.uint64).reshape(-1, 4); b = np.frombuffer(want, dtype=np.uint64).reshape(-1, 4)
            bad = np.nonzero((a != b).any(axis=1))[0]
            raise AssertionError(f"proof {i}: {len(bad)} cells differ, first at {bad[:8]}: got {a[bad[0]]} want {b[bad[0]]}")
    plan.close()
    return info


@pytest.mark.parametrize("mode", [1, 0])
def test_fused_replay_small_shapes(h2w, h2w_api, oracle, consts, mode):
    trace_and_replay_fused(h2w, h2w_api, oracle, consts, (6, 2, 1, mode), 1, [2, 3])
    trace_and_replay_fused(h2w, h2w_api, oracle, consts, (7, 3, 2, mode), 4, [5])
    trace_and_replay_fused(h2w, h2w_api, oracle, consts, (9, 2, 1, mode), 33, [34], cap_height=2, valid=True)


@pytest.mark.parametrize("mode", [1, 0])
def test_fused_replay_config1(h2w, h2w_api, oracle, published, mode):
    info = trace_and_replay_fused(h2w, h2w_api, oracle, published, (10, 4, 1, mode), 0xF1B00001, [0xF1B00002, 0xF1B00003, 0xF1B00004])
    assert info["fused"] > 0


def test_fused_replay_config3_bn254(h2w, h2w_api, oracle, published):
    """BASELINE.json configs[2] (2^20 rows, 28 queries, PoseidonBN254 caps): the root's Fiat-Shamir sponge fused; the traced proof and one other."""
    trace_and_replay_fused(h2w, h2w_api, oracle, published, (20, 28, 1, 1), 0xF1B00003, [0xF1B00013])


def test_other_tables_leave_every_stretch_interpreted(h2w, h2w_api, oracle, consts):
    """Traced on tables A, fused with tables B = A with one round constant changed: nothing equals B's canonical tape, every permutation-shaped stretch
    stays interpreted, and the stream is still the oracle's on A."""
    import torch
    ko, kh = consts
    kb = h2w.PoseidonConsts.from_buffer_copy(bytes(kh)); kb.all_round_constants[5] ^= 1
    sh = h2w.fibonacci_shape(6, 2, hash_mode=0); osh = oracle.fibonacci_shape(6, 2, hash_mode=0)
    proofs = [oracle.synth_proof(osh, s) for s in (11, 12)]
    ctx = h2w_api.Context(21, True, 0); ctx.trace_begin()
    h2w_api.verify_stark(ctx, sh, kh, np.frombuffer(bytes(proofs[0]), dtype=np.uint64))
    good = h2w_api.Plan.from_trace(ctx, len(proofs[0]), fuse_consts=kh)
    plan = h2w_api.Plan.from_trace(ctx, len(proofs[0]), fuse_consts=kb); ctx.close()
    info = plan.trace_info(); nperm = good.trace_info()["fused"]; good.close()
    assert info["fused"] == 0 and info["list_entries"] == 0 and info["candidates_left"] == nperm > 0
    d_proofs = _upload(proofs, plan.proof_words); st = torch.cuda.current_stream().cuda_stream
    adv = torch.zeros(2 * plan.num_cells * 32, dtype=torch.uint8, device="cuda"); ws = torch.zeros(plan.workspace_bytes(2), dtype=torch.uint8, device="cuda")
    plan.run(d_proofs.data_ptr(), 2, adv.data_ptr(), ws.data_ptr(), st); torch.cuda.synchronize()
    assert plan.status(ws.data_ptr(), 2, st) == [0, 0]
    got = adv.cpu().numpy().tobytes(); nb = plan.num_cells * 32
    for i, p in enumerate(proofs):
        o = oracle.Ctx(21, track_scopes=False); assert oracle.verify_stark(o, osh, ko, p) == 0
        assert got[i * nb:(i + 1) * nb] == o.advice_bytes(); o.close()
    plan.close()


# ---------------------------------------------------------------------------------------------------------------- unit traces
def _unit_run(h2w, h2w_api, body, words, trace):
    """words: one tagged Goldilocks input each; body(ctx, native, chip, inputs) drives the calls.  Returns the context."""
    L = h2w.lib()
    ctx = h2w_api.Context(21, True, 0)
    if trace:
        ctx.trace_begin()
    native = h2w_api.NativeChip(ctx); chip = h2w_api.GoldilocksChip(native)
    ins = []
    for w, v in enumerate(words):
        assert L.h2w_trace_input(ctx.p, w, 1) == 0
        ins.append(chip.load_witness(int(v)))
    body(ctx, native, chip, ins)
    return ctx


def _chip_permute(h2w, ctx, k, st):
    out = (h2w.Assigned * 12)()
    assert h2w.lib().h2w_chip_gl_poseidon_permute(ctx.p, C.byref(k), (h2w.Assigned * 12)(*st), out) == 0
    return list(out)


def _replay_unit(h2w, h2w_api, plan, body, word_sets):
    """The plan on every word set; returns the status words.  A status-0 stream must equal an eager run of `body` on those words."""
    import torch
    n = len(word_sets); words = len(word_sets[0])
    host = torch.tensor(np.array(word_sets, dtype=np.uint64).astype(np.int64).reshape(-1))
    d = host.cuda(); st = torch.cuda.current_stream().cuda_stream
    adv = torch.zeros(n * plan.num_cells * 32, dtype=torch.uint8, device="cuda"); ws = torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    plan.run(d.data_ptr(), n, adv.data_ptr(), ws.data_ptr(), st); torch.cuda.synchronize()
    status = plan.status(ws.data_ptr(), n, st)
    got = adv.cpu().numpy().tobytes(); nb = plan.num_cells * 32
    for i, w in enumerate(word_sets):
        if status[i] == 0:
            e = _unit_run(h2w, h2w_api, body, w, False)
            assert e.num_cells() == plan.num_cells and got[i * nb:(i + 1) * nb] == e.advice_bytes(), f"input set {i}"
            e.close()
    assert words == plan.proof_words
    return status


def test_mixed_tables_fuse_only_the_matching_permutation(h2w, h2w_api, consts):
    """One trace, h2w_chip_gl_poseidon_permute twice on tagged inputs: on tables A, then on B.  Fused with A: one op, one stretch left interpreted."""
    ko, kh = consts
    kb = h2w.PoseidonConsts.from_buffer_copy(bytes(kh)); kb.fast_partial_round_constants[3] ^= 5

    def body(ctx, native, chip, ins):
        a = _chip_permute(h2w, ctx, kh, ins[:12])
        b = _chip_permute(h2w, ctx, kb, a[:4] + ins[12:20])
        chip.mul(a[11], b[0])
    rng = np.random.default_rng(17)
    sets = [[int(x) for x in rng.integers(0, GL_P, 20, dtype=np.uint64)] for _ in range(3)]
    ctx = _unit_run(h2w, h2w_api, body, sets[0], True)
    plan = h2w_api.Plan.from_trace(ctx, 20, parallel_scopes=(), fuse_consts=kh); ctx.close()
    info = plan.trace_info()
    assert info["fused"] == 1 and info["candidates_left"] == 1 and info["list_entries"] == 1
    assert _replay_unit(h2w, h2w_api, plan, body, sets) == [0, 0, 0]
    plan.close()


def _hand_permute(chip, k, st):
    """PoseidonChip::permute driven call by call through the level-2 ABI, as csrc/chips.h PoseidonPermutationChip drives it through csrc/abi_backend.cpp
    (a constant operand: h2w_gl_load_constant right in front of the op).  Returns the output state and the outputs of the first constant layer."""
    M = (1 << 64) - 1
    lc = chip.load_constant
    st = list(st); rc = 0; first_layer = None

    def sbox(x):
        x2 = chip.mul(x, x); x4 = chip.mul(x2, x2); x6 = chip.mul(x4, x2); return chip.mul(x6, x)

    def full_rounds(st, rc):
        nonlocal first_layer
        for _ in range(4):
            st = [chip.add(st[i], lc(k.all_round_constants[i + 12 * rc])) for i in range(12)]
            if first_layer is None:
                first_layer = list(st)
            st = [sbox(x) for x in st]
            for _z in range(12):
                lc(0)
            res = []
            for r in range(12):
                acc = lc(0)
                for i in range(12):
                    acc = chip.mul_add(lc(k.mds_circ[i]), st[(i + r) % 12], acc)
                res.append(chip.mul_add(lc(k.mds_diag[r]), st[r], acc))
            st = res; rc += 1
        return st, rc
    st, rc = full_rounds(st, rc)
    st = [chip.add(st[i], lc(k.fast_partial_first_round_constant[i])) for i in range(12)]
    res = [lc(0) for _ in range(12)]; res[0] = st[0]
    for r in range(1, 12):
        for c in range(1, 12):
            res[c] = chip.mul_add(lc(k.fast_partial_round_initial_matrix[r - 1][c - 1]), st[r], res[c])
    st = res
    for r in range(22):
        s0 = chip.add(sbox(st[0]), lc(k.fast_partial_round_constants[r]))
        d = chip.mul(lc((k.mds_circ[0] + k.mds_diag[0]) & M), s0)
        for i in range(1, 12):
            d = chip.mul_add(lc(k.fast_partial_round_w_hats[r][i - 1]), st[i], d)
        for _z in range(12):
            lc(0)
        st = [d] + [chip.mul_add(lc(k.fast_partial_round_vs[r][i - 1]), s0, st[i]) for i in range(1, 12)]
    rc += 22
    st, rc = full_rounds(st, rc)
    return st, first_layer


def test_a_stretch_whose_interior_value_escapes_stays_interpreted(h2w, h2w_api, consts):
    """h2w_chip_gl_poseidon_permute hands out no interior handle, so the permutation is driven BY HAND through the level-2 calls, call for call what the
    chip does: such a stretch equals the canonical tape (scope names and the caller play no part) and fuses.  With one h2w_add that reads an interior
    value - an output of the first constant layer - it must not; the stream is an eager run's either way."""
    ko, kh = consts

    def make(escape):
        def body(ctx, native, chip, ins):
            out, first_layer = _hand_permute(chip, kh, ins[:12])
            native.add(first_layer[3] if escape else out[3], out[0])
        return body
    rng = np.random.default_rng(23)
    sets = [[int(x) for x in rng.integers(0, GL_P, 12, dtype=np.uint64)] for _ in range(2)]
    for escape in (False, True):
        body = make(escape)
        ctx = _unit_run(h2w, h2w_api, body, sets[0], True)
        plan = h2w_api.Plan.from_trace(ctx, 12, parallel_scopes=(), fuse_consts=kh); ctx.close()
        info = plan.trace_info()
        assert (info["fused"], info["candidates_left"]) == ((0, 1) if escape else (1, 0)), (escape, info)
        assert _replay_unit(h2w, h2w_api, plan, body, sets) == [0, 0]
        plan.close()


def test_status_words_on_a_fused_plan(h2w, h2w_api, consts):
    """A non-canonical proof word is still status 4, a zero divisor (GoldilocksChip::div, base.rs:379) still status 1, on a plan with a fused permutation."""
    ko, kh = consts

    def body(ctx, native, chip, ins):
        out = _chip_permute(h2w, ctx, kh, ins[:12])
        chip.div(out[0], ins[12])
    rng = np.random.default_rng(29)
    sets = [[int(x) for x in rng.integers(1, GL_P, 13, dtype=np.uint64)] for _ in range(4)]
    sets[1][12] = 0                 # the divisor
    sets[2][5] = GL_P + 1           # a word outside the field
    ctx = _unit_run(h2w, h2w_api, body, sets[0], True)
    plan = h2w_api.Plan.from_trace(ctx, 13, parallel_scopes=(), fuse_consts=kh); ctx.close()
    assert plan.trace_info()["fused"] == 1
    assert _replay_unit(h2w, h2w_api, plan, body, sets) == [0, 1, 4, 0]
    plan.close()


# ---------------------------------------------------------------------------------------------------------------- sharded and column forms
@pytest.mark.parametrize("mode", [1, 0])
def test_fused_plan_shards_and_columns_equal_the_unfused_plan(h2w, h2w_api, oracle, consts, mode):
    """World 2, both ranks, flat (h2w_fri_witness_batch_shard) and packed (_shard_compact): every block of the fused plan is the unfused plan's; so are
    the FlexGate columns (h2w_fri_witness_batch_columns)."""
    import torch
    ko, kh = consts
    args = (7, 5, 2, mode)
    sh = h2w.fibonacci_shape(*args[:2], rate_bits=args[2], hash_mode=mode); osh = oracle.fibonacci_shape(*args[:2], rate_bits=args[2], hash_mode=mode)
    n, world = 3, 2
    proofs = [oracle.synth_proof(osh, 60 + i) for i in range(n)]
    ctx = h2w_api.Context(21, False, 0); ctx.trace_begin()
    h2w_api.verify_stark(ctx, sh, kh, np.frombuffer(bytes(oracle.synth_proof(osh, 59)), dtype=np.uint64))
    unfused = h2w_api.Plan.from_trace(ctx, len(proofs[0])); fused = h2w_api.Plan.from_trace(ctx, len(proofs[0]), fuse_consts=kh); ctx.close()
    assert fused.trace_info()["fused"] > 0 and fused.num_cells == unfused.num_cells
    d_proofs = _upload(proofs, fused.proof_words); st = torch.cuda.current_stream().cuda_stream
    for rank in range(world):
        assert fused.shard_cells(n, rank, world) == unfused.shard_cells(n, rank, world)
        flat, packed = [], []
        for pl in (unfused, fused):
            adv = torch.zeros(n * pl.num_cells * 4, dtype=torch.int64, device="cuda"); ws = torch.zeros(pl.shard_workspace_bytes(n, rank, world), dtype=torch.uint8, device="cuda")
            pl.run_shard(d_proofs.data_ptr(), n, adv.data_ptr(), ws.data_ptr(), rank, world, st); torch.cuda.synchronize()
            assert pl.status(ws.data_ptr(), n, st) == [0] * n
            flat.append(adv)
            cells = pl.shard_cells(n, rank, world)
            buf = torch.full((cells + 8, 4), -1, dtype=torch.int64, device="cuda"); ws = torch.zeros(pl.shard_workspace_bytes(n, rank, world), dtype=torch.uint8, device="cuda")
            pl.run_shard_compact(d_proofs.data_ptr(), n, buf.data_ptr(), ws.data_ptr(), rank, world, st); torch.cuda.synchronize()
            assert pl.status(ws.data_ptr(), n, st) == [0] * n
            packed.append(buf)
        assert torch.equal(flat[0], flat[1]), f"flat shard, rank {rank}"
        assert torch.equal(packed[0], packed[1]), f"packed shard, rank {rank}"
        assert bool((flat[1] != 0).any())
        for p_ in range(n):
            for q in range(-1, sh.num_queries):
                assert fused.shard_block(rank, world, p_, q) == unfused.shard_block(rank, world, p_, q)
    k = 14
    bp = unfused.break_points(k); ncol = len(bp) + 1
    assert fused.break_points(k) == bp
    cols = []
    for pl, fill in ((unfused, 0x5A), (fused, 0xA5)):
        out = torch.full((((n * ncol) << k) * 32,), fill, dtype=torch.uint8, device="cuda"); ws = torch.zeros(pl.workspace_bytes(n), dtype=torch.uint8, device="cuda")
        pl.run_columns(d_proofs.data_ptr(), n, bp, k, out.data_ptr(), ws.data_ptr(), st); torch.cuda.synchronize()
        assert pl.status(ws.data_ptr(), n, st) == [0] * n
        cols.append(out)
    assert torch.equal(cols[0], cols[1])
    unfused.close(); fused.close()
