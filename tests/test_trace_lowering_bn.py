"""H2W_TRACE_FUSE_BN_PERMUTE, the host side (no GPU): the lowering finds every PoseidonBN254 permutation of a traced verifier run - as many as the
oracle's scope tree counts -, fuses all but at most the one that holds the Context's cached load_zero cell, and leaves Goldilocks-only traces and
unflagged plans as they were."""
import ctypes as C

import numpy as np
import pytest


def oracle_bn_perm_count(oracle, osh, ko, proof, lookup_bits=21):
    """PoseidonBN254 permutations of the shape, from the oracle's scope tree.  A PoseidonBN254 permutation opens one "partial_rounds" scope
    (hash/poseidon_bn254/permutation.rs:83-110); a Goldilocks one opens one too, plus one "mds_partial_layer_init" (hash/poseidon/permutation.rs:108-132).
    Both unit sizes are measured on single permutations; the count follows from the totals, and the division must be exact."""
    L = oracle.lib()

    def cells(ctx, name):
        return sum(v for k, v in ctx.scopes().items() if k.split(";")[-1] == name)
    one = oracle.Ctx(lookup_bits, track_scopes=True)
    ins = (oracle.AV * 12)(*[L.orc_gl_load_constant(one.p, i) for i in range(12)]); outs = (oracle.AV * 12)()
    L.orc_gl_poseidon_permute(one.p, C.byref(ko), ins, outs)
    gl_init, gl_pr = cells(one, "mds_partial_layer_init"), cells(one, "partial_rounds"); one.close()
    one = oracle.Ctx(lookup_bits, track_scopes=True)
    L.orc_load_zero(one.p)
    ins = (oracle.AV * 4)(*[L.orc_load_constant(one.p, oracle.Fr.from_int(i + 1)) for i in range(4)]); outs = (oracle.AV * 4)()
    L.orc_bn_poseidon_permute(one.p, C.byref(ko), ins, outs)
    bn_pr = cells(one, "partial_rounds"); assert cells(one, "mds_partial_layer_init") == 0; one.close()
    assert gl_init > 0 and gl_pr > 0 and bn_pr > 0
    o = oracle.Ctx(lookup_bits, track_scopes=True)
    assert oracle.verify_stark(o, osh, ko, proof) == 0
    tot_init, tot_pr = cells(o, "mds_partial_layer_init"), cells(o, "partial_rounds"); o.close()
    assert tot_init % gl_init == 0
    n_gl = tot_init // gl_init
    assert (tot_pr - n_gl * gl_pr) % bn_pr == 0
    return (tot_pr - n_gl * gl_pr) // bn_pr


def _trace(h2w, h2w_api, oracle, consts, shape_args, seed=42):
    ko, kh = consts
    sh = h2w.fibonacci_shape(*shape_args[:2], rate_bits=shape_args[2], hash_mode=shape_args[3]); osh = oracle.fibonacci_shape(*shape_args[:2], rate_bits=shape_args[2], hash_mode=shape_args[3])
    proof = oracle.synth_proof(osh, seed)
    ctx = h2w_api.Context(21, True, 0); ctx.trace_begin()
    h2w_api.verify_stark(ctx, sh, kh, np.frombuffer(bytes(proof), dtype=np.uint64))
    return ctx, proof, osh


@pytest.mark.parametrize("fuse_gl", [False, True])
def test_every_bn_permutation_of_the_verifier_is_found(h2w, h2w_api, oracle, consts, fuse_gl):
    ko, kh = consts
    ctx, proof, osh = _trace(h2w, h2w_api, oracle, consts, (6, 2, 1, 1))
    plain = h2w_api.Plan.from_trace(ctx, len(proof)); glf = h2w_api.Plan.from_trace(ctx, len(proof), fuse_consts=kh)
    plan = h2w_api.Plan.from_trace(ctx, len(proof), fuse_consts=kh, fuse_bn=True, fuse_gl=fuse_gl)
    info = plan.trace_info_bn()
    nperm = oracle_bn_perm_count(oracle, osh, ko, proof)
    assert nperm > 0 and info["fused"] + info["left"] == nperm and info["left"] <= 1 and info["list_entries"] == info["fused"]
    assert plan.num_cells == ctx.num_cells() == plain.num_cells and plan.proof_words == len(proof)
    # the Goldilocks counts keep their meaning and their values; unflagged plans know no PoseidonBN254 op
    assert plan.trace_info() == (glf.trace_info() if fuse_gl else plain.trace_info())
    assert plain.trace_info_bn() == {"fused": 0, "left": 0, "list_entries": 0} == glf.trace_info_bn()
    # the list entry adds 144 bytes per fused permutation and proof (256-byte granules); the value store loses the fused stretches' interior slots
    base = glf if fuse_gl else plain
    for n in (1, 3):
        assert 0 < plan.workspace_bytes(n) <= base.workspace_bytes(n) + n * info["fused"] * 144 + 256
    plain.close(); glf.close(); plan.close(); ctx.close()


def test_goldilocks_caps_have_no_bn_permutation(h2w, h2w_api, oracle, consts):
    ko, kh = consts
    ctx, proof, osh = _trace(h2w, h2w_api, oracle, consts, (6, 2, 1, 0))
    glf = h2w_api.Plan.from_trace(ctx, len(proof), fuse_consts=kh); both = h2w_api.Plan.from_trace(ctx, len(proof), fuse_consts=kh, fuse_bn=True)
    assert both.trace_info_bn() == {"fused": 0, "left": 0, "list_entries": 0}
    assert both.trace_info() == glf.trace_info() and both.num_records == glf.num_records and both.num_cells == glf.num_cells
    assert [both.workspace_bytes(n) for n in (1, 5)] == [glf.workspace_bytes(n) for n in (1, 5)]
    glf.close(); both.close(); ctx.close()


def test_flag_errors(h2w, h2w_api, oracle, consts):
    ko, kh = consts
    ctx, proof, osh = _trace(h2w, h2w_api, oracle, consts, (6, 2, 1, 1))
    L = h2w.lib(); names = (C.c_char_p * 0)()
    assert not L.h2w_plan_from_trace_ex(ctx.p, len(proof), names, 0, 0, None, h2w.H2W_TRACE_FUSE_BN_PERMUTE) and "needs the Poseidon tables" in h2w.last_error()
    assert not L.h2w_plan_from_trace_ex(ctx.p, len(proof), names, 0, 0, C.byref(kh), 4) and "unknown flag" in h2w.last_error()
    ctx.close()
