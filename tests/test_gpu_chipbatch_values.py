"""h2w_chipbatch_values on the device (include/h2w.h 2c, csrc/chipvalues.hip): every instance's result words are the oracle's output wires of a
fresh context that loaded the same operands and ran the same op, its n_failed the number of failing pairs among that context's copy constraints,
its status the word h2w_chipbatch_run stores - exact integers, no tolerance (tests/chipbatch_values_ref.py derives them).

Shapes: the launch geometry's edges.  Goldilocks-Poseidon ops run one wavefront per instance (n = 1, 3); the four-lane PoseidonBN254 form runs 16
instances a wavefront, 64 a block: n = 1, 17 (a second wavefront with live tail quads), 65 (a second block); the wavefront-per-instance form four
instances a block: n = 1, 5.  One set of oracle runs per case; every form and count is held to it.  The result and verdict buffers are
sentinel-filled with one spare instance behind the batch, which must stay untouched."""
import json
import os

import pytest

import chipbatch_hash_ref as ref
import chipbatch_values_ref as vref
import devcheck_ref
from chipbatch_hash_ref import BN_PERMUTE, GL_PERMUTE, HASH_NO_PAD, MERKLE_VERIFY, TWO_TO_ONE
from chipbatch_values_ref import FORM_AUTO, FORM_QUAD, FORM_ROW

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
QUAD_BLOCK, QUAD_WAVES = 256, 4      # bnquad.h
COUNTS = {(0, FORM_QUAD): (1, 3), (1, FORM_QUAD): (1, 17, QUAD_BLOCK // 4 + 1), (1, FORM_ROW): (1, QUAD_WAVES + 1)}


def _handle(h2w_api, kh, params, lookup_bits=21):
    return h2w_api.ChipBatch.new_hash(params[0], kh, hash_mode=params[1], n_in=params[2], depth=params[3], cap_height=params[4], lookup_bits=lookup_bits)


def _upload(params, rows):
    import numpy as np
    import torch
    words = np.array([ref.words_of(*params, r) for r in rows], dtype=np.uint64)
    assert words.shape == (len(rows), ref.num_operands(*params))
    return torch.tensor(words.view(np.int64).reshape(-1), dtype=torch.int64, device="cuda")


def _values(b, params, rows, form, d_ops=None):
    """One call on handle b: ([result words of row i], [(status, n_failed) of row i]).  The spare instance behind the batch must keep the sentinel."""
    import numpy as np
    import torch
    n, nres = len(rows), b.num_results()
    assert nres == vref.NUM_RESULTS[params[0]]
    d_ops = _upload(params, rows) if d_ops is None else d_ops
    res = torch.full(((n + 1) * max(nres, 1) * 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    ver = torch.full(((n + 1) * 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    b.values(d_ops.data_ptr(), n, res.data_ptr() if nres else 0, ver.data_ptr(), form=form)
    torch.cuda.synchronize()
    rb, vb = res.cpu().numpy().tobytes(), ver.cpu().numpy().tobytes()
    assert rb[n * nres * 8:] == bytes([SENTINEL]) * (len(rb) - n * nres * 8), "result words behind the batch were written"
    assert vb[n * 8:] == bytes([SENTINEL]) * 8, "the verdict behind the batch was written"
    rw = np.frombuffer(rb[:n * nres * 8], dtype="<u8").reshape(n, nres).tolist() if nres else [[] for _ in range(n)]
    vw = np.frombuffer(vb[:n * 8], dtype="<u4").reshape(n, 2).tolist()
    return rw, [tuple(v) for v in vw]


def _rows(params, n, seed_extra=0):
    """n instances: the first random, then all 0 (index 0), all p - 1 / r - 1 (index 2^depth - 1), index 0, index 2^depth - 1, the rest random."""
    rnd = ref.case_seed(*params, extra=100 + seed_extra)
    top = (1 << params[3]) - 1
    edges = [{}, dict(fill="zero"), dict(fill="max"), dict(index=0), dict(index=top)]
    return [ref.random_items(rnd, *params, **(edges[i] if i < len(edges) else {})) for i in range(n)]


def _expect_all(oracle, ko, lookup_bits, params, rows):
    from concurrent.futures import ThreadPoolExecutor
    one = lambda r: vref.expected(oracle, ko, lookup_bits, params, r)
    head = [one(rows[0])]      # (the oracle holds no state between contexts once it has run once)
    with ThreadPoolExecutor(max_workers=8) as ex:
        return head + list(ex.map(one, rows[1:]))


def _hold(params, form, got, want, rows_desc=""):
    rw, vw = got
    for i, (words, n_failed) in enumerate(want):
        assert vw[i] == (0, n_failed), (params, form, rows_desc, i, vw[i], n_failed)
        assert rw[i] == words, (params, form, rows_desc, i)


def _check_case(h2w_api, oracle, tables, params, lookup_bits=21, seed_extra=0, first=(), counts=None):
    """Every form the op's hash admits at every count of its geometry against one set of oracle runs; then, at the form's middle count, the last row
    made invalid: status 4 there, every other row's words byte-equal."""
    ko, kh = tables
    fam = ref.family(params[0], params[1])
    counts = counts or COUNTS
    nmax = max(max(counts[(fam, f)]) for f in vref.forms_of(params[0], params[1]))
    rows = _rows(params, nmax, seed_extra)
    for i, r in enumerate(first):
        rows[i] = list(r)
    want = _expect_all(oracle, ko, lookup_bits, params, rows)
    b = _handle(h2w_api, kh, params, lookup_bits)
    for form in vref.forms_of(params[0], params[1]):
        for n in counts[(fam, form)]:
            got = _values(b, params, rows[:n], form)
            print(f"case {params} L={lookup_bits} form={form} n={n}: verdicts {sorted(set(got[1]))}, rows with every result word equal: {[got[0][i] == want[i][0] for i in range(n)].count(True)}")
            _hold(params, form, got, want[:n], f"n={n}")
        n = sorted(counts[(fam, form)])[-2] if len(counts[(fam, form)]) > 2 else max(counts[(fam, form)])
        good = _values(b, params, rows[:n], form)
        bad_rows = rows[:n - 1] + [vref.invalid_row(params, rows[n - 1])]
        bad = _values(b, params, bad_rows, form)
        assert [s for s, _ in bad[1]] == [0] * (n - 1) + [4], (params, form, bad[1])
        assert bad[0][:n - 1] == good[0][:n - 1] and bad[1][:n - 1] == good[1][:n - 1], "a status-4 row changed another instance"
    auto = _values(b, params, rows[:3], FORM_AUTO)
    _hold(params, FORM_AUTO, auto, want[:3], "auto")
    b.close()
    return rows, want


@pytest.mark.parametrize("params", ref.PARAMS, ids=str)
def test_every_case_in_every_form(h2w_api, oracle, consts, params):
    _check_case(h2w_api, oracle, consts, params)


def _golden(which):
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_published.json")))
    return [([int(x, 16) for x in v["in"]], [int(x, 16) for x in v["out"]]) for v in g[which]["permutation_vectors"]]


@pytest.mark.parametrize("op,which", [(GL_PERMUTE, "goldilocks_w12"), (BN_PERMUTE, "bn254_t4")])
def test_published_known_answers(h2w_api, oracle, published, op, which):
    """plonky2's and circomlib's tables: the result words of the published inputs are the published vectors (poseidon([1, 2, 3]) among them)."""
    params = (op, 0, 0, 0, 0)
    golden = _golden(which)
    assert golden
    rows = [list(gin) for gin, _ in golden]
    b = _handle(h2w_api, published[1], params)
    for form in vref.forms_of(op, 0):
        rw, vw = _values(b, params, rows, form)
        for i, (_, gout) in enumerate(golden):
            assert vw[i] == (0, 0)
            assert rw[i] == vref.result_words(op, 0, [_Wire(v) for v in gout]), (which, form, i)
    b.close()
    _check_case(h2w_api, oracle, published, params, seed_extra=1, first=rows[:3], counts={(0, FORM_QUAD): (3,), (1, FORM_QUAD): (17,), (1, FORM_ROW): (5,)})


class _Wire:
    """An output wire by its value alone (vref.result_words reads o.v.to_int())."""

    def __init__(self, v):
        self.v = self
        self._v = v

    def to_int(self):
        return self._v


def _merkle_batch(oracle, ko, params, seed_extra=0):
    """One batch of openings: [(what, items, n_failed the row must have or None)].  Every n_failed is also the oracle's."""
    op, mode, n_in, depth, cap = params
    rnd = ref.case_seed(*params, extra=200 + seed_extra)
    root = 4 if mode == 0 else 1
    top = (1 << depth) - 1
    valid = vref.valid_merkle(oracle, ko, 21, params, rnd, index=top)
    slot = vref.cap_slot(params, valid)
    bare_leaf = mode == 0 and depth == cap and n_in <= 4      # the node is the leaf itself: one word of it is one comparison
    batch = [("valid, index 2^depth - 1", valid, 0),
             ("valid, index 0", vref.valid_merkle(oracle, ko, 21, params, rnd, index=0), 0),
             ("valid, random index", vref.valid_merkle(oracle, ko, 21, params, rnd), 0),
             ("leaf word", vref.bump_item(params, valid, n_in - 1), 1 if bare_leaf else root),
             ("cap entry", vref.bump_item(params, valid, slot, word=1), 1)]
    if depth > cap:
        batch.append(("first sibling", vref.bump_item(params, valid, n_in + 1 + (1 << cap), word=0), root))
        batch.append(("last sibling", vref.bump_item(params, valid, len(valid) - 1, word=3), root))
    if mode == 0:
        three = vref.bump_item(params, valid, slot, word=3)
        batch.append(("cap entry equal to the node in three words of four", three, 1))
        batch.append(("random operands", ref.random_items(rnd, *params), 4))
    else:
        batch.append(("random operands", ref.random_items(rnd, *params), 1))
    batch.append(("valid again", valid, 0))
    return batch


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", ref.MERKLE_SHAPES + ((1, 32, 0),), ids=lambda s: "leaf%d-depth%d-cap%d" % s)
def test_merkle_verdicts(h2w_api, oracle, consts, mode, shape):
    """Valid openings, corrupted ones and random ones in one batch; (1, 32, 0): the deepest path, its first valid row at index 2^32 - 1."""
    params = (MERKLE_VERIFY, mode) + shape
    ko, kh = consts
    batch = _merkle_batch(oracle, ko, params)
    rows = [items for _, items, _ in batch]
    want = _expect_all(oracle, ko, 21, params, rows)
    for (what, _, nf), (words, n_failed) in zip(batch, want):
        assert words == [] and (nf is None or nf == n_failed), (what, nf, n_failed)
    assert rows[0][shape[0]] == (1 << shape[1]) - 1
    b = _handle(h2w_api, kh, params)
    assert b.num_results() == 0
    for form in vref.forms_of(MERKLE_VERIFY, mode):
        got = _values(b, params, rows, form)
        print(f"merkle {params} form={form}:", [(what, v) for (what, _, _), v in zip(batch, got[1])])
        _hold(params, form, got, want, "merkle batch")
    b.close()


AGREEMENT = [(GL_PERMUTE, 0, 0, 0, 0), (BN_PERMUTE, 0, 0, 0, 0), (HASH_NO_PAD, 0, 9, 0, 0), (HASH_NO_PAD, 1, 10, 0, 0), (TWO_TO_ONE, 0, 0, 0, 0),
             (TWO_TO_ONE, 1, 0, 0, 0), (MERKLE_VERIFY, 0, 20, 3, 1), (MERKLE_VERIFY, 1, 20, 3, 1)]


@pytest.mark.parametrize("params", AGREEMENT, ids=str)
def test_agreement_with_the_witness_call(h2w_api, oracle, consts, params):
    """The same handle, the same operands (one row invalid): the status words of h2w_chipbatch_run are the verdicts' status words, and the cells of its
    advice at the oracle's output-wire offsets carry the result words."""
    import torch
    ko, kh = consts
    fam = ref.family(params[0], params[1])
    n = 3 if fam == 0 else 5
    rows = _rows(params, n, seed_extra=3)
    rows[1] = vref.invalid_row(params, rows[1])
    b = _handle(h2w_api, kh, params)
    nc, nres = b.num_cells(), b.num_results()
    d_ops = _upload(params, rows)
    advice = torch.empty((n * nc * 32,), dtype=torch.uint8, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    b.run(d_ops.data_ptr(), n, advice.data_ptr(), status.data_ptr(), 0)
    torch.cuda.synchronize()
    st = status.cpu().tolist(); adv = advice.cpu().numpy().tobytes()
    assert st == [0, 4] + [0] * (n - 2)
    for form in vref.forms_of(params[0], params[1]):
        rw, vw = _values(b, params, rows, form, d_ops=d_ops)
        assert [s for s, _ in vw] == st, (params, form, vw, st)
        for i in range(n):
            if st[i]:
                continue
            words, failing, cells, oadv = vref.oracle_values(oracle, ko, 21, params, rows[i], want_cells=True)
            assert adv[i * nc * 32:(i + 1) * nc * 32] == oadv and len(oadv) == nc * 32
            per = 1 if fam == 0 else 4
            from_cells = []
            for c in cells:
                v = int.from_bytes(adv[(i * nc + c) * 32:(i * nc + c + 1) * 32], "little")
                assert v >> (64 * per) == 0
                from_cells += [(v >> (64 * k)) & vref.MASK64 for k in range(per)]
            assert len(from_cells) == nres and rw[i] == from_cells == words, (params, form, i)
            assert vw[i] == (0, len(failing))
    b.close()


@pytest.mark.parametrize("name", devcheck_ref.ADVERSARIAL)
def test_lazy_value_reach(h2w, h2w_api, oracle, name):
    """The table blocks the lazy value walks are held to (devcheck_ref.lazy_sets: entries of 0, 1, r - 1, r - 1 times 2^-261, and the two greedy sets):
    there the walks reach their stated bounds, and a result that left without its final reduction would not be the oracle's canonical value.  The first
    rows are the fixed states of those checks and the state a greedy set was built for; both PoseidonBN254 forms."""
    import numpy as np
    block, own = devcheck_ref.lazy_sets()[name]
    raw = np.array(block, dtype="<u8").tobytes()
    ko, kh = oracle.Consts.from_buffer_copy(raw), h2w.PoseidonConsts.from_buffer_copy(raw)
    assert bytes(ko) == raw and bytes(kh) == raw
    states = [st for _, st in devcheck_ref.FIXED_STATES] + ([own] if own else [])
    small = {(1, FORM_QUAD): (17,), (1, FORM_ROW): (5,)}
    _check_case(h2w_api, oracle, (ko, kh), (BN_PERMUTE, 0, 0, 0, 0), seed_extra=6, first=states, counts=small)
    params = (MERKLE_VERIFY, 1, 20, 3, 1)
    batch = _merkle_batch(oracle, ko, params, seed_extra=6)
    rows = [items for _, items, _ in batch]
    want = _expect_all(oracle, ko, 21, params, rows)
    assert want[0] == ([], 0) and want[-1] == ([], 0)      # (what a corruption costs is the oracle's word alone here: a degenerate table may hash everything to one node)
    b = _handle(h2w_api, kh, params)
    for form in (FORM_QUAD, FORM_ROW):
        _hold(params, form, _values(b, params, rows, form), want, name)
    b.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_lookup_bits_13_and_the_chunk_option_change_nothing(h2w_api, oracle, consts, mode):
    """The values do not depend on lookup_bits; the call runs its instances as one launch and does not look at H2W_CHIPBATCH_OPT_CHUNK."""
    for params in ((HASH_NO_PAD, mode, 9, 0, 0), (MERKLE_VERIFY, mode, 20, 3, 1)):
        rows, want13 = _check_case(h2w_api, oracle, consts, params, lookup_bits=13, seed_extra=4, counts={(0, FORM_QUAD): (3,), (1, FORM_QUAD): (5,), (1, FORM_ROW): (5,)})
        n = len(rows)
        b21, b13 = _handle(h2w_api, consts[1], params, 21), _handle(h2w_api, consts[1], params, 13)
        b13.set_chunk(2)
        for form in vref.forms_of(params[0], mode):
            assert _values(b21, params, rows, form) == _values(b13, params, rows, form)
            _hold(params, form, _values(b13, params, rows, form), want13, "chunk 2")
        b21.close(); b13.close()
