"""The layout of the batched hash / Merkle chip ops (h2w_chipbatch_new_hash, include/h2w.h 2c) without a device: for every parameter set
the GPU tests run, cells and operand words per instance against an oracle context that ran the same program; and what the two
constructors refuse."""
import ctypes as C

import pytest

import chipbatch_hash_ref as ref


def _new(h2w, kh, op, mode, n_in, depth, cap, lookup_bits=21):
    return h2w.lib().h2w_chipbatch_new_hash(op, C.byref(kh), mode, n_in, depth, cap, lookup_bits, 0)


@pytest.mark.parametrize("lookup_bits", [21, 13])
@pytest.mark.parametrize("params", ref.PARAMS, ids=lambda p: "op%d-m%d-n%d-d%d-c%d" % p)
def test_cells_and_operands_per_instance(h2w, oracle, consts, params, lookup_bits):
    """num_cells equals the oracle's count for the same program on arbitrary operands; num_operands the count of the operand table."""
    ko, kh = consts; L = h2w.lib()
    h = _new(h2w, kh, *params, lookup_bits=lookup_bits)
    assert h, h2w.last_error()
    try:
        assert int(L.h2w_chipbatch_num_operands(h)) == ref.num_operands(*params)
        items = ref.random_items(ref.case_seed(*params), *params)
        ctx, _ = ref.oracle_instance(oracle, ko, lookup_bits, *params, items)
        assert not ctx.error()
        assert int(L.h2w_chipbatch_num_cells(h)) == ctx.num_cells()
        ctx.close()
    finally:
        L.h2w_chipbatch_free(h)


def test_published_tables_give_the_same_layout(h2w, oracle, published):
    """The layout does not depend on the tables' values."""
    ko, kh = published; L = h2w.lib()
    for params in ((ref.GL_PERMUTE, 0, 0, 0, 0), (ref.BN_PERMUTE, 0, 0, 0, 0), (ref.MERKLE_VERIFY, 0, 20, 3, 1), (ref.MERKLE_VERIFY, 1, 20, 3, 1)):
        h = _new(h2w, kh, *params)
        assert h, h2w.last_error()
        ctx, _ = ref.oracle_instance(oracle, ko, 21, *params, ref.random_items(ref.case_seed(*params, extra=1), *params))
        assert int(L.h2w_chipbatch_num_cells(h)) == ctx.num_cells()
        ctx.close(); L.h2w_chipbatch_free(h)


REFUSED = {
    "cap_height > depth": (ref.MERKLE_VERIFY, 0, 4, 2, 3),
    "cap_height > 6": (ref.MERKLE_VERIFY, 1, 4, 8, 7),
    "depth 0": (ref.MERKLE_VERIFY, 0, 4, 0, 0),
    "depth 33": (ref.MERKLE_VERIFY, 1, 4, 33, 0),
    "merkle n_in 0": (ref.MERKLE_VERIFY, 0, 0, 3, 1),
    "hash n_in 0": (ref.HASH_NO_PAD, 1, 0, 0, 0),
    "hash n_in above the limit": (ref.HASH_NO_PAD, 0, ref.MAX_N_IN + 1, 0, 0),
    "merkle n_in above the limit": (ref.MERKLE_VERIFY, 1, ref.MAX_N_IN + 1, 3, 1),
    "permute with n_in": (ref.GL_PERMUTE, 0, 12, 0, 0),
    "bn permute with depth": (ref.BN_PERMUTE, 0, 0, 1, 0),
    "bn permute with hash_mode": (ref.BN_PERMUTE, 1, 0, 0, 0),
    "two_to_one with n_in": (ref.TWO_TO_ONE, 0, 2, 0, 0),
    "two_to_one with cap_height": (ref.TWO_TO_ONE, 1, 0, 0, 1),
    "hash with depth": (ref.HASH_NO_PAD, 0, 8, 3, 0),
    "hash_mode 2": (ref.TWO_TO_ONE, 2, 0, 0, 0),
}


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_constructor_refuses(h2w, consts, why):
    _, kh = consts
    assert not _new(h2w, kh, *REFUSED[why]), why
    assert "h2w_chipbatch_new_hash" in h2w.last_error()


def test_limits_are_accepted(h2w, consts):
    """The largest n_in the header names (at least 512), depth 32, cap_height 6; GL_PERMUTE ignores hash_mode."""
    _, kh = consts; L = h2w.lib()
    assert ref.MAX_N_IN == h2w.H2W_CHIPBATCH_MAX_N_IN >= 512
    for params in ((ref.HASH_NO_PAD, 0, ref.MAX_N_IN, 0, 0), (ref.MERKLE_VERIFY, 0, 1, 32, 6), (ref.GL_PERMUTE, 1, 0, 0, 0)):
        h = _new(h2w, kh, *params)
        assert h, h2w.last_error()
        assert int(L.h2w_chipbatch_num_operands(h)) == ref.num_operands(*params)
        L.h2w_chipbatch_free(h)


@pytest.mark.parametrize("op", range(9))
def test_field_ops_go_through_the_old_constructor_only(h2w, consts, op):
    _, kh = consts
    assert not _new(h2w, kh, op, 0, 0, 0, 0)
    assert h2w.last_error().endswith("use h2w_chipbatch_new")


@pytest.mark.parametrize("op", range(9, 14))
def test_hash_ops_go_through_the_new_constructor_only(h2w, op):
    assert not h2w.lib().h2w_chipbatch_new(op, 21, 0)
    assert h2w.last_error().endswith("use h2w_chipbatch_new_hash")


def test_wrapper_and_configure(h2w, h2w_api, consts):
    """api.ChipBatch: layout queries without a device; the chunk option takes 1 .. 32768 on a hash handle."""
    _, kh = consts
    b = h2w_api.ChipBatch.new_hash(ref.MERKLE_VERIFY, kh, hash_mode=1, n_in=20, depth=3, cap_height=1)
    assert b.num_operands() == ref.num_operands(ref.MERKLE_VERIFY, 1, 20, 3, 1) and b.num_cells() > 3 * 4032
    b.configure(h2w.H2W_CHIPBATCH_OPT_CHUNK, 2)
    for bad in (0, 32769):
        with pytest.raises(h2w.H2WError):
            b.configure(h2w.H2W_CHIPBATCH_OPT_CHUNK, bad)
    with pytest.raises(h2w.H2WError):
        b.configure(99, 1)
    b.close()
    with pytest.raises(h2w.H2WError):
        h2w_api.ChipBatch.new_hash(ref.MERKLE_VERIFY, kh, hash_mode=1, n_in=20, depth=3, cap_height=4)
