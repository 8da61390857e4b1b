"""What h2w_merkle_build and h2w_merkle_open (include/h2w.h 2e, csrc/merkletree.hip) must store, from the CPU oracle's VALUE functions alone - shared
by tests/test_merkle_tree_host.py and tests/test_gpu_merkle_tree.py.

A tree is plonky2's MerkleTree::new(leaves, cap_height): leaf digest = orc_nv_hash_or_noop(leaf); inner node = two_to_one(left, right), which the
oracle does not export and prover.inc's nv_two_to_one states - the first four words of orc_nv_gl_permute on [l, r, 0^4] (hash_mode 0), element 0 of
orc_nv_bn_permute on [0, 0, l, r] (hash_mode 1).  A hash is four words in both modes.  The hash store holds the levels from the leaves upward,
level l at word 4 (2^(depth+1) - 2^(depth-l+1)); nothing above the cap exists.  tests/test_merkle_tree_host.py pins this reference to the chip
(MerkleTreeChip::verify_proof_to_cap on a keygen context of the oracle) independently of the code under test.
"""
import ctypes as C
import random

import chipbatch_hash_ref as ref
from chipbatch_hash_ref import MERKLE_VERIFY, P

MASK64 = 0xFFFFFFFFFFFFFFFF
CROWN_NONE, CROWN_AUTO = 254, 255
OPT_CROWN_BITS = 1


def level_offset(depth, l):
    return 4 * ((1 << (depth + 1)) - (1 << (depth - l + 1)))


def tree_words(depth, cap_height):
    return 4 * ((1 << (depth + 1)) - (1 << cap_height))


def num_operands(n_in, depth, cap_height):
    return n_in + 1 + 4 * ((1 << cap_height) + depth - cap_height)


def leaf_digest(oracle, ko, mode, leaf):
    out = (C.c_uint64 * 4)()
    oracle.lib().orc_nv_hash_or_noop(C.byref(ko), mode, (C.c_uint64 * len(leaf))(*leaf), len(leaf), out)
    return list(out)


def two_to_one(oracle, ko, mode, l, r):
    L = oracle.lib()
    if mode == 0:
        st = (C.c_uint64 * 12)(*(list(l) + list(r) + [0] * 4))
        L.orc_nv_gl_permute(C.byref(ko), st)
        return list(st)[:4]
    as_int = lambda h: sum(w << (64 * i) for i, w in enumerate(h))
    st = (oracle.Fr * 4)(oracle.Fr.from_int(0), oracle.Fr.from_int(0), oracle.Fr.from_int(as_int(l)), oracle.Fr.from_int(as_int(r)))
    L.orc_nv_bn_permute(C.byref(ko), st)
    v = st[0].to_int()
    return [(v >> (64 * i)) & MASK64 for i in range(4)]


def build_tree(oracle, ko, mode, leaves, depth, cap_height):
    """leaves: 2^depth lists of n_in words -> the levels 0 .. depth - cap_height, each a list of hashes (four words)."""
    assert len(leaves) == 1 << depth
    levels = [[leaf_digest(oracle, ko, mode, leaf) for leaf in leaves]]
    for _ in range(depth - cap_height):
        below = levels[-1]
        levels.append([two_to_one(oracle, ko, mode, below[2 * i], below[2 * i + 1]) for i in range(len(below) // 2)])
    return levels


def tree_store(levels):
    """The levels as the words of the tree's hash store."""
    return [w for lv in levels for h in lv for w in h]


def opening_row(leaves, levels, depth, cap_height, index):
    """leaf, index, cap, siblings: the operand words of a MERKLE_VERIFY instance."""
    row = list(leaves[index]) + [index]
    row += [w for h in levels[depth - cap_height] for w in h]
    for j in range(depth - cap_height):
        row += levels[j][(index >> j) ^ 1]
    return row


def items_of(mode, n_in, depth, cap_height, row):
    """An opening row as the items chipbatch_hash_ref's oracle_instance takes (a hash: four words / one Fr as an integer)."""
    items = list(row[:n_in + 1])
    for k in range(n_in + 1, len(row), 4):
        h = row[k:k + 4]
        items.append(sum(w << (64 * i) for i, w in enumerate(h)) if mode == 1 else list(h))
    assert len(items) == len(ref.operand_kinds(MERKLE_VERIFY, mode, n_in, depth, cap_height))
    return items


def seeded_leaves(seed, n_trees, n_in, depth):
    """[tree][leaf][word]: seeded canonical words, with the words 0 and p - 1 planted in every tree."""
    rnd = random.Random(seed)
    trees = [[[rnd.randrange(P) for _ in range(n_in)] for _ in range(1 << depth)] for _ in range(n_trees)]
    for t, tree in enumerate(trees):
        tree[0][0] = 0
        tree[-1][n_in - 1] = P - 1
        tree[(t + 1) % len(tree)][(t * 7) % n_in] = P - 1 if t & 1 else 0
    return trees


_CACHE = {}


def reference_trees(oracle, ko, tables_name, mode, n_in, depth, cap_height, n_trees, seed):
    """(leaves, [levels of tree t]) for seeded leaves - computed once per case and shared (never changed by its users)."""
    key = (tables_name, mode, n_in, depth, n_trees, seed)      # (a tree with a cap is the tree without one, cut off at the cap)
    if key not in _CACHE:
        leaves = seeded_leaves(seed, n_trees, n_in, depth)
        _CACHE[key] = (leaves, [build_tree(oracle, ko, mode, lv, depth, 0) for lv in leaves])
    leaves, full = _CACHE[key]
    return leaves, [levels[:depth - cap_height + 1] for levels in full]
