"""The batched hash / Merkle chip ops on the device (h2w_chipbatch_new_hash, include/h2w.h 2c, csrc/chiphash.hip): every instance's cells
equal, byte for byte, the oracle's advice for a fresh context that loaded the same operands and ran the same op - the reference's chip tests
(hash/poseidon/permutation.rs:325-347, hash/poseidon_bn254/permutation.rs:266-301, hash/*/hash.rs test_hash_no_pad / test_hash_two_to_one,
merkle/mod.rs:136-265), n at a time.

Shapes: the smallest at which the kernels can go wrong.  Goldilocks-Poseidon ops run one wavefront per instance (n = 1 .. 3: more than one
block, more than one listed permutation per instance); PoseidonBN254 ops one quad per instance, 16 quads a wavefront, 64 a block: n = 1 (one
quad of a wavefront), 17 (a second wavefront with one real quad, 15 tail quads), 65 (a second block).  Every case runs twice: as is, and
with one row made invalid (status 4), which must leave every other instance as it was."""
import json
import os

import pytest

import chipbatch_hash_ref as ref
import devcheck_ref
from chipbatch_hash_ref import BN_PERMUTE, GL_PERMUTE, HASH_NO_PAD, MERKLE_VERIFY, TWO_TO_ONE, P, R

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _rows(params, n, seed_extra=0):
    """n instances: seeded random, with the edge rows all 0 (index 0), all p - 1 / r - 1 (index 2^depth - 1), index 0, index 2^depth - 1 -
    as many of them as fit, starting at a case-dependent one so that cases with n = 2 cover all four between them."""
    op, mode, n_in, depth, cap = params
    rnd = ref.case_seed(*params, extra=seed_extra)
    top = (1 << depth) - 1
    edges = [dict(fill="zero"), dict(fill="max"), dict(index=0), dict(index=top)]
    k = (n_in + depth + cap + mode) % 4
    edges = edges[k:] + edges[:k]
    if n == 1:
        return [ref.random_items(rnd, *params)]
    return [ref.random_items(rnd, *params, **(edges[i] if i < len(edges) else {})) for i in range(n)]


def _invalid(params, items):
    """The row with one operand outside its field: a Goldilocks word = p, an Fr = r, the leaf index = 2^depth."""
    op, mode, n_in, depth, cap = params
    bad = list(items)
    if op in (GL_PERMUTE, HASH_NO_PAD):
        bad[len(bad) // 2] = P
    elif op == BN_PERMUTE or (op == TWO_TO_ONE and mode == 1):
        bad[-1] = R
    elif op == TWO_TO_ONE:
        bad[0] = [1, 2, P, 3]
    else:
        bad[n_in] = 1 << depth
    return bad


def _device_run(h2w, h2w_api, kh, params, lookup_bits, rows, chunk=None):
    import numpy as np
    import torch
    b = h2w_api.ChipBatch.new_hash(params[0], kh, hash_mode=params[1], n_in=params[2], depth=params[3], cap_height=params[4], lookup_bits=lookup_bits)
    nw, nc, n = b.num_operands(), b.num_cells(), len(rows)
    assert nw == ref.num_operands(*params)
    if chunk:
        b.set_chunk(chunk)
    words = np.array([ref.words_of(*params, r) for r in rows], dtype=np.uint64)
    assert words.shape == (n, nw)
    d_ops = torch.tensor(words.view(np.int64).reshape(-1), dtype=torch.int64, device="cuda")
    advice = torch.full(((n + 1) * nc * 32,), SENTINEL, dtype=torch.uint8, device="cuda")      # one spare instance behind the batch
    status = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
    b.run(d_ops.data_ptr(), n, advice.data_ptr(), status.data_ptr(), 0)
    torch.cuda.synchronize()
    got = advice.cpu().numpy().tobytes(); st = status.cpu().tolist()
    b.close()
    assert got[n * nc * 32:] == bytes([SENTINEL]) * (nc * 32), "the spare instance behind the batch was written"
    assert st[n] == -1
    return nc, got, st[:n]


def _check(h2w, h2w_api, oracle, tables, params, lookup_bits, n, golden=None, seed_extra=0, first=()):
    """The case as is, then with its last row invalid.  golden: (inputs, outputs) of published known answers for the first rows; first: rows to put in
    front instead of the generated ones."""
    ko, kh = tables
    rows = _rows(params, n, seed_extra)
    for i, r in enumerate(first):
        rows[i] = list(r)
    if golden:
        for i, (gin, _) in enumerate(golden[:n]):
            rows[i] = list(gin)
    want = []
    for i, r in enumerate(rows):      # the reference, once per row: both runs are held to it
        ctx, out = ref.oracle_instance(oracle, ko, lookup_bits, *params, r)
        assert not ctx.error(), ctx.error()
        want.append(ctx.advice_bytes())
        if golden and i < len(golden):
            assert [o.v.to_int() for o in out] == list(golden[i][1])
            for o in out:         # the output-state cells carry the published vector
                assert want[i][o.cell * 32:(o.cell + 1) * 32] == o.v.to_int().to_bytes(32, "little")
        ctx.close()
    nc, got, st = _device_run(h2w, h2w_api, kh, params, lookup_bits, rows)
    assert all(len(w) == nc * 32 for w in want)
    print(f"case {params} L={lookup_bits} n={n}: statuses {st}, rows with all {nc} cells equal: {[got[i * nc * 32:(i + 1) * nc * 32] == want[i] for i in range(n)].count(True)}")
    for i in range(n):
        assert st[i] == 0, (params, i, st[i])
        assert got[i * nc * 32:(i + 1) * nc * 32] == want[i], (params, i, _first_diff(got[i * nc * 32:(i + 1) * nc * 32], want[i]))
    bad_at = n - 1
    rows2 = list(rows); rows2[bad_at] = _invalid(params, rows[bad_at])
    nc2, got2, st2 = _device_run(h2w, h2w_api, kh, params, lookup_bits, rows2)
    print(f"case {params} L={lookup_bits} n={n}: statuses with row {bad_at} invalid: {st2}")
    assert st2 == [4 if i == bad_at else 0 for i in range(n)]
    assert got2[:bad_at * nc * 32] == got[:bad_at * nc * 32], "a status-4 row changed another instance"
    return rows, nc, got


def _first_diff(a, b):
    for c in range(min(len(a), len(b)) // 32):
        if a[c * 32:(c + 1) * 32] != b[c * 32:(c + 1) * 32]:
            return f"cell {c} of {len(b) // 32} differs"
    return "lengths differ"


def _golden(which):
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_published.json")))
    return [([int(x, 16) for x in v["in"]], [int(x, 16) for x in v["out"]]) for v in g[which]["permutation_vectors"]]


@pytest.mark.parametrize("n", [1, 3])
def test_gl_permute(h2w, h2w_api, oracle, consts, n):
    _check(h2w, h2w_api, oracle, consts, (GL_PERMUTE, 0, 0, 0, 0), 21, n)


def test_gl_permute_published_known_answers(h2w, h2w_api, oracle, published):
    """plonky2's tables (the small-MDS path of the values phase): the output-state cells carry its published permutation vectors."""
    _check(h2w, h2w_api, oracle, published, (GL_PERMUTE, 0, 0, 0, 0), 21, 3, golden=_golden("goldilocks_w12"))


@pytest.mark.parametrize("n", [1, 17, 65])
def test_bn_permute(h2w, h2w_api, oracle, consts, n):
    _check(h2w, h2w_api, oracle, consts, (BN_PERMUTE, 0, 0, 0, 0), 21, n)


def test_bn_permute_published_known_answers(h2w, h2w_api, oracle, published):
    """circomlib's tables: the output-state cells of the first rows carry its vectors (poseidon([1, 2, 3]) among them)."""
    _check(h2w, h2w_api, oracle, published, (BN_PERMUTE, 0, 0, 0, 0), 21, 17, golden=_golden("bn254_t4"))


@pytest.mark.parametrize("mode,n_in", [(m, k) for m in (0, 1) for k in ref.HASH_N_IN[m]])
def test_hash_no_pad(h2w, h2w_api, oracle, consts, mode, n_in):
    _check(h2w, h2w_api, oracle, consts, (HASH_NO_PAD, mode, n_in, 0, 0), 21, 3 if mode == 0 else 17)


@pytest.mark.parametrize("mode", [0, 1])
def test_two_to_one(h2w, h2w_api, oracle, consts, mode):
    _check(h2w, h2w_api, oracle, consts, (TWO_TO_ONE, mode, 0, 0, 0), 21, 2 if mode == 0 else 17)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", ref.MERKLE_SHAPES, ids=lambda s: "leaf%d-depth%d-cap%d" % s)
def test_merkle_verify(h2w, h2w_api, oracle, consts, mode, shape):
    """(20, 3, 1): the reference's test; (3, 3, 0): verify_proof, the leaf a no-op hash in both modes; (4, 2, 2): no siblings, the leaf a no-op with
    Goldilocks hashes and hashed with BN254; (5, 1, 0); (20, 3, 2)."""
    _check(h2w, h2w_api, oracle, consts, (MERKLE_VERIFY, mode) + shape, 21, 2 if mode == 0 else 17)


def test_merkle_verify_second_block(h2w, h2w_api, oracle, consts):
    _check(h2w, h2w_api, oracle, consts, (MERKLE_VERIFY, 1, 20, 3, 1), 21, 65, seed_extra=2)


@pytest.mark.parametrize("mode", [0, 1])
def test_published_tables_hash_and_merkle(h2w, h2w_api, oracle, published, mode):
    _check(h2w, h2w_api, oracle, published, (HASH_NO_PAD, mode, 9, 0, 0), 21, 3 if mode == 0 else 17, seed_extra=3)
    _check(h2w, h2w_api, oracle, published, (MERKLE_VERIFY, mode, 5, 1, 0), 21, 2 if mode == 0 else 17, seed_extra=3)


@pytest.mark.parametrize("mode", [0, 1])
def test_lookup_bits_13(h2w, h2w_api, oracle, consts, mode):
    _check(h2w, h2w_api, oracle, consts, (HASH_NO_PAD, mode, 9, 0, 0), 13, 3 if mode == 0 else 17, seed_extra=4)
    _check(h2w, h2w_api, oracle, consts, (MERKLE_VERIFY, mode, 20, 3, 1), 13, 2 if mode == 0 else 17, seed_extra=4)


@pytest.mark.parametrize("mode", [0, 1])
def test_chunked_run_equals_unchunked(h2w, h2w_api, oracle, consts, mode):
    """H2W_CHIPBATCH_OPT_CHUNK = 2 with n = 5: launches of 2, 2 and 1 instances."""
    params = (MERKLE_VERIFY, mode, 20, 3, 1)
    rows, nc, got = _check(h2w, h2w_api, oracle, consts, params, 21, 5, seed_extra=5)
    nc2, got2, st2 = _device_run(h2w, h2w_api, consts[1], params, 21, rows, chunk=2)
    assert st2 == [0] * 5 and nc2 == nc
    assert got2 == got


@pytest.mark.parametrize("name", devcheck_ref.ADVERSARIAL)
def test_emitter_on_degenerate_and_greedy_tables(h2w, h2w_api, oracle, name):
    """bn_emit_cells on the table blocks the lazy value walks are held to (devcheck_ref.lazy_sets: entries of 0, 1, r - 1, r - 1 times 2^-261, and the two
    greedy sets), the oracle on the same bytes: its arithmetic is canonical, and a table block is data.  The first rows are the fixed states of those
    checks and the state a greedy set was built for."""
    import numpy as np
    block, own = devcheck_ref.lazy_sets()[name]
    raw = np.array(block, dtype="<u8").tobytes()
    ko, kh = oracle.Consts.from_buffer_copy(raw), h2w.PoseidonConsts.from_buffer_copy(raw)
    assert bytes(ko) == raw and bytes(kh) == raw
    states = [st for _, st in devcheck_ref.FIXED_STATES] + ([own] if own else [])
    _check(h2w, h2w_api, oracle, (ko, kh), (BN_PERMUTE, 0, 0, 0, 0), 21, 17, seed_extra=6, first=states)
    _check(h2w, h2w_api, oracle, (ko, kh), (TWO_TO_ONE, 1, 0, 0, 0), 21, 17, seed_extra=6)
