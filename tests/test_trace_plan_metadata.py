"""A traced plan as a first-class plan, the host side (no GPU: a traced plan lowers without a device): its block structure (the depth-1 parallel
instances, the query rounds, are the shard units) and the keygen metadata a witness_gen_only=False tracing context hands it - both equal to the
compiled plan of the same shape."""
import numpy as np
import pytest


def _trace(h2w, h2w_api, oracle, args, seed=42, witness_gen_only=True, parallel_scopes=None, cap_height=4):
    d, q, rb, mode = args
    sh = h2w.fibonacci_shape(d, q, rate_bits=rb, hash_mode=mode, cap_height=cap_height)
    osh = oracle.fibonacci_shape(d, q, rate_bits=rb, hash_mode=mode, cap_height=cap_height)
    proof = oracle.synth_proof(osh, seed)
    ctx = h2w_api.Context(21, witness_gen_only, 0); ctx.trace_begin()
    h2w_api.verify_stark(ctx, sh, h2w.published_consts(), np.frombuffer(bytes(proof), dtype=np.uint64))
    kw = {} if parallel_scopes is None else {"parallel_scopes": parallel_scopes}
    plan = h2w_api.Plan.from_trace(ctx, len(proof), **kw)
    ctx.close()
    return plan, h2w_api.Plan(sh, h2w.published_consts()), osh


@pytest.mark.parametrize("mode", [1, 0])
def test_traced_plan_has_the_compiled_block_structure(h2w, h2w_api, oracle, mode):
    traced, compiled, _ = _trace(h2w, h2w_api, oracle, (7, 5, 2, mode))
    assert traced.strand_layout() == compiled.strand_layout()
    pro, q0, q1, total = traced.strand_layout()
    assert 0 < pro < total and q0 > 0 and q1 > 0 and pro + q0 + 4 * q1 == total
    for n in (5, 17):
        for world in (1, 3, 8):
            for rank in range(world):
                assert traced.shard_cells(n, rank, world) == compiled.shard_cells(n, rank, world), (n, world, rank)
                assert 0 < traced.shard_workspace_bytes(n, rank, world) <= traced.workspace_bytes(n)
                for p in range(n):
                    for q in range(-1, 5):
                        assert traced.shard_block(rank, world, p, q) == compiled.shard_block(rank, world, p, q), (n, world, rank, p, q)
    traced.close(); compiled.close()


def _norm_eq(pairs):
    return sorted((min(a, b), max(a, b)) for a, b in pairs)


@pytest.mark.parametrize("mode", [1, 0])
def test_traced_plan_carries_the_keygen_metadata(h2w, h2w_api, oracle, mode):
    """Traced on proof A with witness_gen_only=False: the selectors, lookup cells, copy constraints and constant equalities (filled in from a
    DIFFERENT proof B) equal the compiled plan's, which tests/test_keygen_metadata.py pins to the oracle."""
    traced, compiled, osh = _trace(h2w, h2w_api, oracle, (6, 2, 1, mode), seed=11, witness_gen_only=False, cap_height=2)
    proof_b = oracle.synth_proof(osh, 12)
    assert traced.num_cells == compiled.num_cells
    assert traced.selectors() == compiled.selectors()
    assert traced.lookup_cells() == compiled.lookup_cells()
    assert _norm_eq(traced.equalities()) == _norm_eq(compiled.equalities())
    assert sorted(traced.const_equalities(proof_b)) == sorted(compiled.const_equalities(proof_b))
    assert traced.break_points(14) == compiled.break_points(14)
    if mode == 1:
        assert sorted(traced.const_equalities()) == sorted(compiled.const_equalities())
    else:      # the Goldilocks-Poseidon hash wires are constants of the circuit: the proof is needed
        with pytest.raises(h2w.H2WError):
            traced.const_equalities()
    traced.close(); compiled.close()


def test_a_witness_only_trace_has_no_keygen_metadata(h2w, h2w_api, oracle):
    traced, compiled, _ = _trace(h2w, h2w_api, oracle, (6, 2, 1, 1))
    with pytest.raises(h2w.H2WError, match="witness_gen_only"):
        traced.selectors()
    with pytest.raises(h2w.H2WError, match="witness_gen_only"):
        traced.equalities()
    traced.close(); compiled.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_a_plan_without_query_units_refuses_to_shard(h2w, h2w_api, oracle, mode):
    """Only the Merkle scope parallel: its instances do not tile the stream behind the root's block, so there are no shard units."""
    traced, compiled, _ = _trace(h2w, h2w_api, oracle, (7, 5, 2, mode), parallel_scopes=("verify_proof_to_cap_with_cap_index",))
    with pytest.raises(h2w.H2WError, match="not shardable"):
        traced.shard_cells(5, 0, 3)
    with pytest.raises(h2w.H2WError, match="not shardable"):
        traced.shard_block(0, 3, 0, -1)
    with pytest.raises(h2w.H2WError, match="not shardable"):
        traced.run_shard(0, 5, 0, 0, 0, 3)
    with pytest.raises(h2w.H2WError, match="not shardable"):
        traced.run_shard_compact(0, 5, 0, 0, 0, 3)
    assert traced.shard_workspace_bytes(5, 0, 3) == 0
    assert traced.strand_layout()[0] == traced.num_cells          # one block
    traced.close(); compiled.close()
