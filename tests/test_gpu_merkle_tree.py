"""h2w_merkle_build and h2w_merkle_open on the device (include/h2w.h 2e, csrc/merkletree.hip): every word of every tree is the reference tree's
(tests/merkle_tree_ref.py: the oracle's value functions alone; tests/test_merkle_tree_host.py pins that reference to the chip), whichever levels the
crown builds; an opening row is the row assembled from the reference tree and goes, without visiting the host, into the batched Merkle chip, which
accepts it.  Exact integers, no tolerance.  Every buffer the calls write lies between sentinel guard words, which must stay untouched.

Shapes: the smallest at which a path of the code can go wrong - the no-op boundary of the leaf hasher, the absorb boundaries of both sponges, an Fr filled
with one, two and three words, trees without any two_to_one, every cap height against a short tree, every crown boundary of a depth-7 tree, a crown of
three launches, and one call over many workgroups with two trees."""
import random

import pytest

import chipbatch_values_ref as vref
import merkle_tree_ref as mref
from chipbatch_hash_ref import MERKLE_VERIFY, P

pytestmark = pytest.mark.gpu

GUARD = 64                       # sentinel words in front of and behind a buffer
SENT = 0x5A5A5A5A5A5A5A5A
NONE, AUTO, OPT = mref.CROWN_NONE, mref.CROWN_AUTO, mref.OPT_CROWN_BITS


def _tables(request, name):
    return request.getfixturevalue(name)


def _dev_u64(words):
    import numpy as np
    import torch
    return torch.from_numpy(np.array(words, dtype=np.uint64).view(np.int64).copy()).cuda()


def _guarded(n_words):
    """A device buffer of n_words u64 between two guards: (tensor, pointer of word 0)."""
    import torch
    t = torch.full((n_words + 2 * GUARD,), SENT, dtype=torch.int64, device="cuda")
    return t, t.data_ptr() + 8 * GUARD


def _read_guarded(t, n_words, what):
    import numpy as np
    a = t.cpu().numpy().view(np.uint64)
    assert (a[:GUARD] == SENT).all() and (a[GUARD + n_words:] == SENT).all(), what + ": a guard word was written"
    return a[GUARD:GUARD + n_words]


def _flat_leaves(leaves):
    return [w for tree in leaves for leaf in tree for w in leaf]


def _build(m, d_leaves, n_trees, tw):
    """One build: (the words of trees_dev as [n_trees][tw], the status words, the trees tensor and its pointer)."""
    import torch
    trees, p_trees = _guarded(n_trees * tw)
    status = torch.full((n_trees + 2,), 0x77, dtype=torch.int32, device="cuda")
    m.build(d_leaves.data_ptr(), n_trees, p_trees, status.data_ptr() + 4)
    torch.cuda.synchronize()
    st = status.cpu().tolist()
    assert st[0] == 0x77 and st[-1] == 0x77, "a status word outside [n_trees] was written"
    return _read_guarded(trees, n_trees * tw, "trees_dev").reshape(n_trees, tw), st[1:-1], trees, p_trees


def _hold_trees(got, want_trees, what):
    import numpy as np
    for t, levels in enumerate(want_trees):
        want = np.array(mref.tree_store(levels), dtype=np.uint64)
        diff = np.nonzero(got[t] != want)[0]
        assert diff.size == 0, (what, "tree", t, "first differing word", int(diff[0]), "of", want.size, "differing", int(diff.size))


def _case(request, h2w_api, oracle, tables, mode, n_in, depth, cap, n_trees, crowns=(AUTO,)):
    ko, kh = _tables(request, tables)
    leaves, want = mref.reference_trees(oracle, ko, tables, mode, n_in, depth, cap, n_trees, seed=0xB1D + 17 * n_in + depth)
    flat = _flat_leaves(leaves)
    assert 0 in flat and P - 1 in flat
    d_leaves = _dev_u64(flat)
    m = h2w_api.MerkleTree.new(kh, hash_mode=mode, n_in=n_in, depth=depth, cap_height=cap)
    tw = m.tree_words()
    for crown in crowns:
        m.configure(OPT, crown)
        got, st, _, _ = _build(m, d_leaves, n_trees, tw)
        assert st == [0] * n_trees, (crown, st)
        _hold_trees(got, want, (tables, mode, n_in, depth, cap, "crown", crown))
    m.close()


N_IN = {0: (4, 5, 8, 9, 16, 17, 20), 1: (3, 4, 9, 10, 11, 12, 18, 19, 20)}      # the no-op boundary, the absorb boundaries, the reference's own leaf width
SMALL = [(m, s) for m in (0, 1) for s in ((1, 1, 1), (4, 2, 2), (1, 1, 0))] + [(m, (n, 3, 1)) for m in (0, 1) for n in N_IN[m]]


@pytest.mark.parametrize("tables", ["consts", "published"])
@pytest.mark.parametrize("mode,shape", SMALL, ids=lambda v: str(v))
def test_every_word_of_small_trees(request, h2w_api, oracle, tables, mode, shape):
    """Trees without any two_to_one, the smallest tree with one node, and every leaf length at which the hasher takes another path; two trees a call."""
    _case(request, h2w_api, oracle, tables, mode, *shape, n_trees=2, crowns=(NONE, AUTO))


@pytest.mark.parametrize("tables", ["consts", "published"])
@pytest.mark.parametrize("mode", [0, 1])
def test_every_word_over_many_workgroups(request, h2w_api, oracle, tables, mode):
    """(5, 12, 0) with two trees: 8,192 leaves over 128 workgroups of the wide kernels (every level one lane per node under NONE), the second tree a
    stride behind the first; and what AUTO makes of the same call."""
    _case(request, h2w_api, oracle, tables, mode, 5, 12, 0, n_trees=2, crowns=(NONE, AUTO))


@pytest.mark.parametrize("tables", ["consts", "published"])
@pytest.mark.parametrize("mode", [0, 1])
def test_every_cap_height_against_a_short_tree(request, h2w_api, oracle, tables, mode):
    for cap in range(7):
        _case(request, h2w_api, oracle, tables, mode, 3, 7, cap, n_trees=3, crowns=(NONE, AUTO))


@pytest.mark.parametrize("tables", ["consts", "published"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cap", [0, 3])
def test_every_crown_boundary(request, h2w_api, oracle, tables, mode, cap):
    """(5, 7, cap) with three trees under NONE, 0 .. 7 and AUTO: the stored words do not depend on which levels one wavefront per node builds."""
    _case(request, h2w_api, oracle, tables, mode, 5, 7, cap, n_trees=3, crowns=(NONE, 0, 1, 2, 3, 4, 5, 6, 7, AUTO))


@pytest.mark.parametrize("tables", ["consts", "published"])
@pytest.mark.parametrize("mode", [0, 1])
def test_a_crown_of_several_launches(request, h2w_api, oracle, tables, mode):
    """(5, 12, 2) with one tree under NONE, 4, 10 and 12: a crown of one, three and three launches (levels hand over at kernel boundaries as well as in
    LDS), the last of them starting at the leaf digests."""
    _case(request, h2w_api, oracle, tables, mode, 5, 12, 2, n_trees=1, crowns=(NONE, 4, 10, 12))


def _open(m, d_leaves, p_trees, n_trees, queries, nw):
    """One open: (rows as [n][nw], status words, the operands tensor and its pointer)."""
    import torch
    n = len(queries)
    d_q = _dev_u64([w for q in queries for w in q])
    ops, p_ops = _guarded(n * nw)
    status = torch.full((n + 2,), 0x77, dtype=torch.int32, device="cuda")
    m.open(d_leaves.data_ptr(), p_trees, n_trees, d_q.data_ptr(), n, p_ops, status.data_ptr() + 4)
    torch.cuda.synchronize()
    st = status.cpu().tolist()
    assert st[0] == 0x77 and st[-1] == 0x77, "a status word outside [n] was written"
    return _read_guarded(ops, n * nw, "operands_dev").reshape(n, nw), st[1:-1], ops, p_ops


def _verdicts(b, p_ops, n, form):
    import numpy as np
    import torch
    ver = torch.full((n * 2,), -1, dtype=torch.int32, device="cuda")
    b.values(p_ops, n, 0, ver.data_ptr(), form=form)
    torch.cuda.synchronize()
    return [tuple(v) for v in ver.cpu().numpy().view(np.uint32).reshape(n, 2).tolist()]


@pytest.mark.parametrize("mode", [0, 1])
def test_openings_are_the_chip_s_operands(h2w_api, oracle, consts, mode):
    """Every index of a depth-5 tree over three trees, shuffled, one query twice: the rows are the reference's; the same device buffer is accepted by
    h2w_chipbatch_values in every form; a word of a leaf, of a sibling and of the selected cap entry changed on the device fails exactly those rows; one
    row's advice stream from h2w_chipbatch_run is the oracle's for those operands."""
    import numpy as np
    import torch
    ko, kh = consts
    n_in, depth, cap, n_trees = 5, 5, 1, 3
    params = (MERKLE_VERIFY, mode, n_in, depth, cap)
    leaves, want = mref.reference_trees(oracle, ko, "consts", mode, n_in, depth, cap, n_trees, seed=0x09E4)
    m = h2w_api.MerkleTree.new(kh, hash_mode=mode, n_in=n_in, depth=depth, cap_height=cap)
    tw, nw = m.tree_words(), m.layout()["num_operands"]
    d_leaves = _dev_u64(_flat_leaves(leaves))
    got, st, trees, p_trees = _build(m, d_leaves, n_trees, tw)
    _hold_trees(got, want, "openings")
    queries = [(t, i) for t in range(n_trees) for i in range(1 << depth)] + [(1, 7)]
    random.Random(5).shuffle(queries)
    n = len(queries)
    rows, st, ops, p_ops = _open(m, d_leaves, p_trees, n_trees, queries, nw)
    assert st == [0] * n
    want_rows = [mref.opening_row(leaves[t], want[t], depth, cap, i) for t, i in queries]
    assert rows.tolist() == want_rows
    b = h2w_api.ChipBatch.new_hash(MERKLE_VERIFY, kh, hash_mode=mode, n_in=n_in, depth=depth, cap_height=cap)
    assert b.num_operands() == nw
    forms = vref.forms_of(MERKLE_VERIFY, mode)
    for form in forms + (vref.FORM_AUTO,):
        assert _verdicts(b, p_ops, n, form) == [(0, 0)] * n, form
    # one row through the witness call: its cells are the oracle's for those operands
    nc = b.num_cells()
    advice = torch.empty((nc * 32,), dtype=torch.uint8, device="cuda")
    rst = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    b.run(p_ops + 8 * nw * 3, 1, advice.data_ptr(), rst.data_ptr(), 0)
    torch.cuda.synchronize()
    _, failing, _, oadv = vref.oracle_values(oracle, ko, 21, params, mref.items_of(mode, n_in, depth, cap, want_rows[3]), want_cells=True)
    assert rst.cpu().tolist() == [0] and failing == [] and advice.cpu().numpy().tobytes() == oadv
    # corruptions on the device: row a a leaf word, row b its last sibling, row c the cap entry its index selects
    a, bb, c = 2, 11, 40
    at = lambda r, w: GUARD + r * nw + w
    cap_word = n_in + 1 + 4 * (queries[c][1] >> (depth - cap)) + 1
    for r, w in ((a, n_in - 1), (bb, nw - 1), (c, cap_word)):
        ops[at(r, w)] = int(np.array([(want_rows[r][w] + 1) % P], dtype=np.uint64).view(np.int64)[0])
    # what the chip makes of each: the oracle's count of failing equalities (a leaf or a sibling moves the whole node: every comparison of the root
    # check - four Goldilocks words, one Fr; a cap entry that differs from the node in ONE word fails the one comparison of that word in either mode)
    expect = {}
    for r, w in ((a, n_in - 1), (bb, nw - 1), (c, cap_word)):
        bad = list(want_rows[r]); bad[w] = (bad[w] + 1) % P
        expect[r] = vref.expected(oracle, ko, 21, params, mref.items_of(mode, n_in, depth, cap, bad))[1]
    assert expect[a] == expect[bb] == (4 if mode == 0 else 1) and expect[c] == 1, expect
    for form in forms:
        v = _verdicts(b, p_ops, n, form)
        assert v == [(0, expect.get(i, 0)) for i in range(n)], (form, [(i, x) for i, x in enumerate(v) if x != (0, 0)])
    b.close(); m.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_status_words(h2w_api, oracle, consts, mode):
    """A leaf word = p in tree 1 of 3: build status [0, 4, 0], trees 0 and 2 the reference's.  Queries with tree = n_trees and with index = 2^depth: status 4
    on those rows alone, which are not written; the other rows are the reference's.  Empty calls return 0 and write nothing."""
    import numpy as np
    import torch
    ko, kh = consts
    n_in, depth, cap, n_trees = 5, 4, 1, 3
    leaves, want = mref.reference_trees(oracle, ko, "consts", mode, n_in, depth, cap, n_trees, seed=0x57A7)
    m = h2w_api.MerkleTree.new(kh, hash_mode=mode, n_in=n_in, depth=depth, cap_height=cap)
    tw, nw = m.tree_words(), m.layout()["num_operands"]
    good = _flat_leaves(leaves)
    bad = list(good); bad[(1 << depth) * n_in + 3 * n_in + 2] = P      # tree 1, leaf 3, word 2
    d_bad = _dev_u64(bad)
    got, st, _, _ = _build(m, d_bad, n_trees, tw)
    assert st == [0, 4, 0]
    for t in (0, 2):
        assert got[t].tolist() == mref.tree_store(want[t]), t
    d_leaves = _dev_u64(good)
    got, st, trees, p_trees = _build(m, d_leaves, n_trees, tw)
    assert st == [0, 0, 0]
    _hold_trees(got, want, "status")
    queries = [(0, 0), (n_trees, 1), (2, 15), (1, 1 << depth), (1, 9), (1 << 40, 1 << 40)]
    rows, st, _, _ = _open(m, d_leaves, p_trees, n_trees, queries, nw)
    assert st == [0, 4, 0, 4, 0, 4]
    for i, (t, idx) in enumerate(queries):
        if st[i] == 0:
            assert rows[i].tolist() == mref.opening_row(leaves[t], want[t], depth, cap, idx), i
        else:
            assert (rows[i] == SENT).all(), ("a refused row was written", i)
    # empty calls: 0, nothing written (null buffers are not looked at)
    before = trees.clone()
    m.build(d_leaves.data_ptr(), 0, p_trees, 0)
    m.open(d_leaves.data_ptr(), p_trees, n_trees, 0, 0, 0, 0)
    m.build(0, 0, 0, 0)
    torch.cuda.synchronize()
    assert torch.equal(before, trees)
    m.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_two_handles_on_different_tables(h2w_api, oracle, consts, published, mode):
    """Tables are per-handle buffers: two handles on different tables, called alternately on one stream, each give their own reference trees."""
    import torch
    n_in, depth, cap, n_trees = 5, 7, 3, 3
    hs = []
    for name, (ko, kh) in (("consts", consts), ("published", published)):
        leaves, want = mref.reference_trees(oracle, ko, name, mode, n_in, depth, cap, n_trees, seed=0xB1D + 17 * n_in + depth)
        hs.append((h2w_api.MerkleTree.new(kh, hash_mode=mode, n_in=n_in, depth=depth, cap_height=cap), _dev_u64(_flat_leaves(leaves)), want))
    tw = hs[0][0].tree_words()
    assert mref.tree_store(hs[0][2][0]) != mref.tree_store(hs[1][2][0])
    outs = []
    for rnd, crown in enumerate((NONE, 7, 2)):
        for m, d_leaves, want in hs:
            m.configure(OPT, crown)
            buf, p = _guarded(n_trees * tw)
            status = torch.zeros((n_trees,), dtype=torch.int32, device="cuda")
            m.build(d_leaves.data_ptr(), n_trees, p, status.data_ptr())
            outs.append((buf, status, want, crown))
    torch.cuda.synchronize()
    for buf, status, want, crown in outs:
        assert status.cpu().tolist() == [0] * n_trees
        _hold_trees(_read_guarded(buf, n_trees * tw, "trees_dev").reshape(n_trees, tw), want, ("two handles", crown))
    for m, _, _ in hs:
        m.close()
