"""Traced plans with H2W_TRACE_FUSE_BN_PERMUTE (include/h2w.h 2d, Plan.from_trace(fuse_consts=..., fuse_bn=True)): every stretch of the tape that
the lowering verifies to be a PoseidonBN254 permutation on the given tables runs as ONE device op (values on the lane, its 4,032 cells by a quad of
k_bn_emit_traced); everything else - other tables, a value that escapes, the permutation with the Context's load_zero cell - stays interpreted.  The
stream is the oracle's / the unfused plan's / an eager run's byte for byte either way; trace_info_bn() says what was fused."""
import ctypes as C

import numpy as np
import pytest

from test_trace_lowering_bn import oracle_bn_perm_count

pytestmark = pytest.mark.gpu
FR_R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
EDGES = [[0] * 4, [FR_R - 1] * 4, [0, 1, FR_R - 1, 1 << 253]]


def _upload(proofs, words):
    import torch
    host = torch.empty(len(proofs) * words, dtype=torch.int64)
    for i, p in enumerate(proofs):
        host[i * words:(i + 1) * words] = torch.frombuffer(bytearray(bytes(p)), dtype=torch.int64)
    return host.cuda()


def _run(plan, d_proofs, n):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    adv = torch.zeros(n * plan.num_cells * 32, dtype=torch.uint8, device="cuda"); ws = torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    plan.run(d_proofs.data_ptr(), n, adv.data_ptr(), ws.data_ptr(), st); torch.cuda.synchronize()
    return plan.status(ws.data_ptr(), n, st), adv.cpu().numpy().tobytes()


def _assert_stream(got, want, what):
    if got != want:
        a = np.frombuffer(got, dtype=np.uint64).reshape(-1, 4); b = np.frombuffer(want, dtype=np.uint64).reshape(-1, 4)
        bad = np.nonzero((a != b).any(axis=1))[0]
        raise AssertionError(f"{what}: {len(bad)} cells differ, first at {bad[:8]}: got {a[bad[0]]} want {b[bad[0]]}")


# ---------------------------------------------------------------------------------------------------------------- whole verifier
_ORACLE = {}


def _oracle_streams(oracle, key, osh, ko, make_proofs):
    """The proofs of a case, the oracle's streams of them and its count of PoseidonBN254 permutations: computed once, shared by the tests that need them."""
    if key not in _ORACLE:
        out = []; proofs = make_proofs()
        for p in proofs:
            o = oracle.Ctx(21, track_scopes=False)
            assert oracle.verify_stark(o, osh, ko, p) == 0
            out.append(o.advice_bytes()); o.close()
        _ORACLE[key] = (proofs, out, oracle_bn_perm_count(oracle, osh, ko, proofs[0]))
    return _ORACLE[key]


CASES = {"6-2": ((6, 2, 1, 1), 1, [2, 3], 4, False), "7-3": ((7, 3, 2, 1), 4, [5, 6], 4, False), "9-2-cap2-valid": ((9, 2, 1, 1), 33, [34, 35], 2, True)}


def _whole_verifier(h2w, h2w_api, oracle, consts, key, shape_args, seed_a, seeds, cap_height, valid, fuse_gl):
    ko, kh = consts
    sh = h2w.fibonacci_shape(*shape_args[:2], rate_bits=shape_args[2], hash_mode=1, cap_height=cap_height)
    osh = oracle.fibonacci_shape(*shape_args[:2], rate_bits=shape_args[2], hash_mode=1, cap_height=cap_height)
    mk = (lambda s: oracle.prove_fri(osh, ko, s)) if valid else (lambda s: oracle.synth_proof(osh, s))
    proofs, want, nperm = _oracle_streams(oracle, key, osh, ko, lambda: [mk(seed_a)] + [mk(s) for s in seeds])
    ctx = h2w_api.Context(21, True, 0); ctx.trace_begin()
    h2w_api.verify_stark(ctx, sh, kh, np.frombuffer(bytes(proofs[0]), dtype=np.uint64))
    plan = h2w_api.Plan.from_trace(ctx, len(proofs[0]), fuse_consts=kh, fuse_bn=True, fuse_gl=fuse_gl)
    assert plan.num_cells == ctx.num_cells() and plan.proof_words == len(proofs[0]); ctx.close()
    info = plan.trace_info_bn()
    assert nperm > 0 and info["fused"] + info["left"] == nperm and info["left"] <= 1 and info["list_entries"] == info["fused"], (info, nperm)
    assert (plan.trace_info()["fused"] > 0) == fuse_gl
    status, got = _run(plan, _upload(proofs, plan.proof_words), len(proofs))
    assert status == [0] * len(proofs)
    nb = plan.num_cells * 32
    for i in range(len(proofs)):
        _assert_stream(got[i * nb:(i + 1) * nb], want[i], f"proof {i}")
    plan.close()


@pytest.mark.parametrize("fuse_gl", [False, True], ids=["flags2", "flags3"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_bn_replay_small_shapes(h2w, h2w_api, oracle, consts, case, fuse_gl):
    _whole_verifier(h2w, h2w_api, oracle, consts, case, *CASES[case], fuse_gl)


@pytest.mark.parametrize("fuse_gl", [False, True], ids=["flags2", "flags3"])
def test_fused_bn_replay_config1(h2w, h2w_api, oracle, published, fuse_gl):
    _whole_verifier(h2w, h2w_api, oracle, published, "cfg1", (10, 4, 1, 1), 0xF1B00001, [0xF1B00002, 0xF1B00003], 4, False, fuse_gl)


def test_other_tables_leave_every_bn_stretch_interpreted(h2w, h2w_api, oracle, consts):
    """Traced on tables A, fused with tables B = A with one bit of bn_c[5] changed: nothing equals B's canonical tape, every PoseidonBN254-shaped
    stretch stays interpreted, and the stream is still the oracle's on A."""
    ko, kh = consts
    kb = h2w.PoseidonConsts.from_buffer_copy(bytes(kh)); kb.bn_c[5].l[0] ^= 1
    sh = h2w.fibonacci_shape(6, 2, hash_mode=1); osh = oracle.fibonacci_shape(6, 2, hash_mode=1)
    proofs, want, nperm = _oracle_streams(oracle, "6-2", osh, ko, lambda: [oracle.synth_proof(osh, s) for s in (1, 2, 3)])
    ctx = h2w_api.Context(21, True, 0); ctx.trace_begin()
    h2w_api.verify_stark(ctx, sh, kh, np.frombuffer(bytes(proofs[0]), dtype=np.uint64))
    plan = h2w_api.Plan.from_trace(ctx, len(proofs[0]), fuse_consts=kb, fuse_bn=True, fuse_gl=False); ctx.close()
    assert plan.trace_info_bn() == {"fused": 0, "left": nperm, "list_entries": 0}
    status, got = _run(plan, _upload(proofs, plan.proof_words), 3)
    assert status == [0, 0, 0]
    nb = plan.num_cells * 32
    for i in range(3):
        _assert_stream(got[i * nb:(i + 1) * nb], want[i], f"proof {i}")
    plan.close()


def test_noncanonical_hash_is_status_4_as_on_the_unfused_plan(h2w, h2w_api, oracle, consts):
    """The first hash of the proof (trace_cap[0], words 0..3) set to r + 1 in one proof of three: status 4 for that proof on the unfused and on the
    fused plan; the other proofs' streams are the oracle's (the flagged proof's cells are "unreduced", include/h2w.h: not compared)."""
    ko, kh = consts
    sh = h2w.fibonacci_shape(6, 2, hash_mode=1); osh = oracle.fibonacci_shape(6, 2, hash_mode=1)
    proofs, want, _ = _oracle_streams(oracle, "6-2", osh, ko, lambda: [oracle.synth_proof(osh, s) for s in (1, 2, 3)])
    bad = oracle.synth_proof(osh, 2)
    for j in range(4):
        bad[j] = ((FR_R + 1) >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    batch = [proofs[0], bad, proofs[2]]
    ctx = h2w_api.Context(21, True, 0); ctx.trace_begin()
    h2w_api.verify_stark(ctx, sh, kh, np.frombuffer(bytes(proofs[0]), dtype=np.uint64))
    unfused = h2w_api.Plan.from_trace(ctx, len(proofs[0])); fused = h2w_api.Plan.from_trace(ctx, len(proofs[0]), fuse_consts=kh, fuse_bn=True); ctx.close()
    assert fused.trace_info_bn()["fused"] > 0
    d = _upload(batch, fused.proof_words); nb = fused.num_cells * 32
    s0, _g0 = _run(unfused, d, 3); s1, g1 = _run(fused, d, 3)
    assert s0 == [0, 4, 0] and s1 == s0
    for i in (0, 2):
        _assert_stream(g1[i * nb:(i + 1) * nb], want[i], f"proof {i}")
    unfused.close(); fused.close()


# ---------------------------------------------------------------------------------------------------------------- unit traces
def _fr_int(f):
    return int.from_bytes(bytes(f), "little")


def _unit_run(h2w, h2w_api, body, state, trace):
    """state: four field elements, each one tagged 4-word input; body(ctx, native, inputs) drives the calls.  The zero cell is loaded first, as the
    verifier's run loads it (stark/mod.rs:483-508), so that no permutation of the body holds it.  Returns the context."""
    L = h2w.lib()
    ctx = h2w_api.Context(21, True, 0)
    if trace:
        ctx.trace_begin()
    native = h2w_api.NativeChip(ctx)
    native.load_zero()
    ins = []
    for i, v in enumerate(state):
        assert L.h2w_trace_input(ctx.p, 4 * i, 4) == 0
        ins.append(native.load_witness(int(v)))
    body(ctx, native, ins)
    return ctx


def _words(state):
    return [(int(v) >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for v in state for j in range(4)]


def _chip_permute(h2w, ctx, k, st):
    out = (h2w.Assigned * 4)()
    assert h2w.lib().h2w_chip_bn_poseidon_permute(ctx.p, C.byref(k), (h2w.Assigned * 4)(*st), out) == 0
    return list(out)


def _replay_unit(h2w, h2w_api, plan, body, states):
    """The plan on every state; a status-0 stream must equal an eager run of `body` on that state.  Returns the status words."""
    import torch
    n = len(states)
    host = torch.tensor(np.array([_words(s) for s in states], dtype=np.uint64).astype(np.int64).reshape(-1))
    assert plan.proof_words == 16
    status, got = _run(plan, host.cuda(), n)
    nb = plan.num_cells * 32
    for i, s in enumerate(states):
        if status[i] == 0:
            e = _unit_run(h2w, h2w_api, body, s, False)
            assert e.num_cells() == plan.num_cells
            _assert_stream(got[i * nb:(i + 1) * nb], e.advice_bytes(), f"state {i}")
            e.close()
    return status


def test_unit_permutation_twice_in_a_row_on_70_states(h2w, h2w_api, consts):
    """h2w_chip_bn_poseidon_permute alone on four tagged inputs, then again on its own outputs (the ring hands the first op's outputs to the second):
    two fused ops; 70 states - more than one wavefront of quads with a ragged tail - among them the edge states."""
    ko, kh = consts

    def body(ctx, native, ins):
        a = _chip_permute(h2w, ctx, kh, ins)
        b = _chip_permute(h2w, ctx, kh, a)
        native.add(a[1], b[2])
    rng = np.random.default_rng(41)
    states = EDGES + [[int.from_bytes(rng.bytes(32), "little") % FR_R for _ in range(4)] for _ in range(67)]
    ctx = _unit_run(h2w, h2w_api, body, states[3], True)
    plan = h2w_api.Plan.from_trace(ctx, 16, parallel_scopes=(), fuse_consts=kh, fuse_bn=True, fuse_gl=False); ctx.close()
    assert plan.trace_info_bn() == {"fused": 2, "left": 0, "list_entries": 2}
    assert _replay_unit(h2w, h2w_api, plan, body, states) == [0] * 70
    plan.close()


def test_the_zero_cell_permutation_is_recognised_and_left(h2w, h2w_api, consts):
    """Without the leading load_zero the first permutation of the trace holds the Context's cached zero cell in its first mix (4,033 cells): it is
    counted as left interpreted, the second one is fused, the stream is an eager run's."""
    ko, kh = consts
    L = h2w.lib()

    def run(state, trace):
        ctx = h2w_api.Context(21, True, 0)
        if trace:
            ctx.trace_begin()
        native = h2w_api.NativeChip(ctx); ins = []
        for i, v in enumerate(state):
            assert L.h2w_trace_input(ctx.p, 4 * i, 4) == 0
            ins.append(native.load_witness(int(v)))
        _chip_permute(h2w, ctx, kh, _chip_permute(h2w, ctx, kh, ins))
        return ctx
    rng = np.random.default_rng(43)
    states = [[int.from_bytes(rng.bytes(32), "little") % FR_R for _ in range(4)] for _ in range(3)]
    ctx = run(states[0], True)
    plan = h2w_api.Plan.from_trace(ctx, 16, parallel_scopes=(), fuse_consts=kh, fuse_bn=True); ctx.close()
    assert plan.trace_info_bn() == {"fused": 1, "left": 1, "list_entries": 1}
    import torch
    host = torch.tensor(np.array([_words(s) for s in states], dtype=np.uint64).astype(np.int64).reshape(-1))
    status, got = _run(plan, host.cuda(), 3)
    assert status == [0, 0, 0]
    nb = plan.num_cells * 32
    for i, s in enumerate(states):
        e = run(s, False); _assert_stream(got[i * nb:(i + 1) * nb], e.advice_bytes(), f"state {i}"); e.close()
    plan.close()


def _hand_permute(native, k, st):
    """PoseidonBN254PermutationChip::permute driven call by call through the level-1 ABI, as csrc/chips.h drives it through csrc/abi_backend.cpp.
    Returns the output state and the outputs of the first ark."""
    lc = lambda f: native.load_constant(_fr_int(f))      # noqa: E731
    st = list(st)

    def exp5(x):
        x2 = native.mul(x, x); x4 = native.mul(x2, x2); return native.mul(x4, x)

    def ark(st, it):
        return [native.add(st[i], lc(k.bn_c[it + i])) for i in range(4)]

    def mix(st, m):
        z = native.load_zero(); ns = []
        for i in range(4):
            acc = z
            for j in range(4):
                acc = native.mul_add(m[j * 4 + i], st[j], acc)
            ns.append(acc)
        return ns

    def full_rounds(st, first):
        m = [lc(k.bn_m[i][j]) for i in range(4) for j in range(4)]; p = [lc(k.bn_p[i][j]) for i in range(4) for j in range(4)]
        for i in range(3):
            st = [exp5(x) for x in st]
            st = ark(st, (i + 1) * 4 if first else 20 + 56 + i * 4)
            st = mix(st, m)
        st = [exp5(x) for x in st]
        return mix(ark(st, 16), p) if first else mix(st, m)
    st = ark(st, 0); first_layer = list(st)
    st = full_rounds(st, True)
    for r in range(56):
        st[0] = native.add(exp5(st[0]), lc(k.bn_c[20 + r]))
        ns0 = native.load_zero()
        for j in range(4):
            ns0 = native.mul_add(lc(k.bn_s[7 * r + j]), st[j], ns0)
        for kk in range(1, 4):
            st[kk] = native.mul_add(lc(k.bn_s[7 * r + 4 + kk - 1]), st[0], st[kk])
        st[0] = ns0
    return full_rounds(st, False), first_layer


def test_a_bn_stretch_whose_interior_value_escapes_stays_interpreted(h2w, h2w_api, consts):
    """The permutation driven BY HAND through the level-1 calls, call for call what the chip does: such a stretch equals the canonical tape and
    fuses.  With one h2w_add that reads an interior value - an output of the first ark - it must not; the stream is an eager run's either way."""
    ko, kh = consts

    def make(escape):
        def body(ctx, native, ins):
            out, first_layer = _hand_permute(native, kh, ins)
            native.add(first_layer[3] if escape else out[3], out[0])
        return body
    rng = np.random.default_rng(47)
    states = [[int.from_bytes(rng.bytes(32), "little") % FR_R for _ in range(4)] for _ in range(2)]
    for escape in (False, True):
        body = make(escape)
        ctx = _unit_run(h2w, h2w_api, body, states[0], True)
        plan = h2w_api.Plan.from_trace(ctx, 16, parallel_scopes=(), fuse_consts=kh, fuse_bn=True, fuse_gl=False); ctx.close()
        info = plan.trace_info_bn()
        assert (info["fused"], info["left"]) == ((0, 1) if escape else (1, 0)), (escape, info)
        assert _replay_unit(h2w, h2w_api, plan, body, states) == [0, 0]
        plan.close()


# ---------------------------------------------------------------------------------------------------------------- sharded and column forms
def test_fused_bn_plan_shards_and_columns_equal_the_unfused_plan(h2w, h2w_api, oracle, consts):
    """Worlds 2 and 3, every rank, flat (h2w_fri_witness_batch_shard) and packed (_shard_compact): every block of the fused plan is the unfused
    plan's; so are the FlexGate columns at k = 12 (h2w_fri_witness_batch_columns)."""
    import torch
    ko, kh = consts
    sh = h2w.fibonacci_shape(7, 3, rate_bits=2, hash_mode=1); osh = oracle.fibonacci_shape(7, 3, rate_bits=2, hash_mode=1)
    n = 3
    proofs = [oracle.synth_proof(osh, 60 + i) for i in range(n)]
    ctx = h2w_api.Context(21, False, 0); ctx.trace_begin()
    h2w_api.verify_stark(ctx, sh, kh, np.frombuffer(bytes(oracle.synth_proof(osh, 59)), dtype=np.uint64))
    unfused = h2w_api.Plan.from_trace(ctx, len(proofs[0])); fused = h2w_api.Plan.from_trace(ctx, len(proofs[0]), fuse_consts=kh, fuse_bn=True); ctx.close()
    assert fused.trace_info_bn()["fused"] > 0 and fused.num_cells == unfused.num_cells
    d_proofs = _upload(proofs, fused.proof_words); st = torch.cuda.current_stream().cuda_stream
    for world in (2, 3):
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
            assert torch.equal(flat[0], flat[1]), f"flat shard, world {world} rank {rank}"
            assert torch.equal(packed[0], packed[1]), f"packed shard, world {world} rank {rank}"
            assert bool((flat[1] != 0).any())
    k = 12
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
