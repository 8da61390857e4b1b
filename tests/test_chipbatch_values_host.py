"""The host side of h2w_chipbatch_values / h2w_chipbatch_num_results (include/h2w.h 2c, csrc/chipvalues.hip; no GPU): the symbols are declared,
exported and bound; num_results needs no device; every refusal comes before any device work - so it is the answer on a machine without a device
too - and names its reason; the verdict struct is 8 bytes on both sides of the binding.  And the reference module of the GPU test
(tests/chipbatch_values_ref.py) is held to the oracle here: its builder of valid Merkle openings, its result words, its failing pairs."""
import ctypes as C
import os
import re

import pytest

import chipbatch_hash_ref as ref
import chipbatch_values_ref as vref
from chipbatch_hash_ref import BN_PERMUTE, GL_PERMUTE, HASH_NO_PAD, MERKLE_VERIFY, TWO_TO_ONE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _new(h2w_api, kh, params, lookup_bits=21):
    return h2w_api.ChipBatch.new_hash(params[0], kh, hash_mode=params[1], n_in=params[2], depth=params[3], cap_height=params[4], lookup_bits=lookup_bits)


def test_the_symbols_are_declared_exported_and_bound(h2w, h2w_api):
    header = open(os.path.join(ROOT, "include", "h2w.h")).read()
    assert re.search(r"typedef struct \{ uint32_t status, n_failed; \} h2w_chipbatch_verdict_t;", header)
    assert re.search(r"uint64_t\s+h2w_chipbatch_num_results\(const h2w_chipbatch \*\);", header)
    assert re.search(r"int\s+h2w_chipbatch_values\(h2w_chipbatch \*, const uint64_t \*operands_dev, uint64_t n,\s*uint64_t \*results_dev, "
                     r"h2w_chipbatch_verdict_t \*verdict_dev,\s*unsigned form, void \*stream\);", header)
    for name, value in (("AUTO", 0), ("QUAD", 1), ("ROW", 2)):
        m = re.search(r"#define H2W_CHIPBATCH_FORM_%s\s+(\d+)" % name, header)
        assert m and int(m.group(1)) == value == getattr(h2w, "H2W_CHIPBATCH_FORM_" + name) == getattr(vref, "FORM_" + name)
    assert re.search(r"#define H2W_ABI_VERSION 1\b", header)
    L = h2w.lib()
    nres, values = L.h2w_chipbatch_num_results, L.h2w_chipbatch_values      # (exported: ctypes resolves them)
    assert nres.restype is C.c_uint64 and list(nres.argtypes) == [C.c_void_p]
    assert values.restype is C.c_int and list(values.argtypes) == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p]


def test_the_verdict_is_eight_bytes_on_both_sides_of_the_binding(h2w):
    assert C.sizeof(h2w.ChipBatchVerdict) == 8
    assert [(n, t) for n, t in h2w.ChipBatchVerdict._fields_] == [("status", C.c_uint32), ("n_failed", C.c_uint32)]
    rs = open(os.path.join(ROOT, "rust", "h2w-sys", "src", "lib.rs")).read()
    assert re.search(r"#\[repr\(C\)\][^\n]*pub struct H2wChipBatchVerdict \{ pub status: u32, pub n_failed: u32 \}", rs)
    assert "verdict_dev: *mut H2wChipBatchVerdict, form: c_uint" in rs


@pytest.mark.parametrize("params", ref.PARAMS, ids=str)
def test_num_results_of_every_case_needs_no_device(h2w_api, consts, params):
    b = _new(h2w_api, consts[1], params)
    assert b.num_results() == vref.NUM_RESULTS[params[0]] == {GL_PERMUTE: 12, BN_PERMUTE: 16, HASH_NO_PAD: 4, TWO_TO_ONE: 4, MERKLE_VERIFY: 0}[params[0]]
    b.close()


def test_null_and_field_op_handles_are_refused(h2w, h2w_api):
    L = h2w.lib()
    words = (C.c_uint64 * 64)(); out = (C.c_uint64 * 64)(); ver = (C.c_uint32 * 2)(0x5A5A5A5A, 0x5A5A5A5A)
    assert L.h2w_chipbatch_values(None, C.addressof(words), 1, C.addressof(out), C.addressof(ver), 0, None) == -1
    assert "h2w_chipbatch_values: null handle" in h2w.last_error()
    assert L.h2w_chipbatch_num_results(None) == 0
    b = h2w_api.ChipBatch(2, 21)      # H2W_OP_GL_MUL: a handle of h2w_chipbatch_new
    for form in (0, 1, 2):
        with pytest.raises(h2w_api.H2WError, match=r"h2w_chipbatch_values: a handle of h2w_chipbatch_new \(the field ops, 0-8\) has no values call"):
            b.values(C.addressof(words), 1, C.addressof(out), C.addressof(ver), form=form)
    assert b.num_results() == 0 and "a handle of h2w_chipbatch_new" in h2w.last_error()
    b.close()
    assert list(ver) == [0x5A5A5A5A] * 2


@pytest.mark.parametrize("params", [(GL_PERMUTE, 0, 0, 0, 0), (HASH_NO_PAD, 0, 9, 0, 0), (TWO_TO_ONE, 0, 0, 0, 0), (MERKLE_VERIFY, 0, 20, 3, 1),
                                    (BN_PERMUTE, 0, 0, 0, 0), (HASH_NO_PAD, 1, 9, 0, 0), (MERKLE_VERIFY, 1, 20, 3, 1)], ids=str)
def test_every_refusal_names_its_reason(h2w, h2w_api, consts, params):
    """Before any device work: the answers are the same with and without a device, and the buffers are host memory nobody may touch."""
    b = _new(h2w_api, consts[1], params)
    bn = ref.family(params[0], params[1]) == 1
    words = (C.c_uint64 * b.num_operands())(); out = (C.c_uint64 * 16)(*([0xA5A5] * 16)); ver = (C.c_uint32 * 2)(0x5A5A5A5A, 0x5A5A5A5A)
    call = lambda form, n=1, ops=C.addressof(words), res=C.addressof(out), v=C.addressof(ver): b.values(ops, n, res, v, form=form)
    for form in (3, 4, 0xFF, 0x102, 0xFFFFFFFF):
        with pytest.raises(h2w_api.H2WError, match=r"h2w_chipbatch_values: unknown form %d \(H2W_CHIPBATCH_FORM_AUTO, _QUAD, _ROW\)" % form):
            call(form)
    if not bn:
        for n in (1, 0):      # (a refusal of the form, not of the batch)
            with pytest.raises(h2w_api.H2WError, match="H2W_CHIPBATCH_FORM_ROW is a PoseidonBN254 form and the handle's hash_mode is 0"):
                call(vref.FORM_ROW, n)
    for form in (vref.FORM_AUTO, vref.FORM_QUAD) + ((vref.FORM_ROW,) if bn else ()):
        with pytest.raises(h2w_api.H2WError, match="h2w_chipbatch_values: null buffer"):
            call(form, ops=None)
        with pytest.raises(h2w_api.H2WError, match="h2w_chipbatch_values: null buffer"):
            call(form, v=None)
        if b.num_results():
            with pytest.raises(h2w_api.H2WError, match="h2w_chipbatch_values: null buffer"):
                call(form, res=None)
    assert list(ver) == [0x5A5A5A5A] * 2 and list(out) == [0xA5A5] * 16
    if h2w.lib().h2w_device_count() == 0:      # everything accepted reaches the device check, under the entry point's own name
        for form in (vref.FORM_AUTO, vref.FORM_QUAD) + ((vref.FORM_ROW,) if bn else ()):
            with pytest.raises(h2w_api.H2WError, match="h2w_chipbatch_values: no HIP device"):
                call(form)
        if not b.num_results():
            with pytest.raises(h2w_api.H2WError, match="h2w_chipbatch_values: no HIP device"):
                call(vref.FORM_AUTO, res=None)      # MERKLE_VERIFY: results_dev may be null
        assert list(ver) == [0x5A5A5A5A] * 2
    b.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", ref.MERKLE_SHAPES, ids=lambda s: "leaf%d-depth%d-cap%d" % s)
def test_the_builder_of_valid_openings(oracle, consts, mode, shape):
    """Random operands fail every comparison of the root check (four with Goldilocks hashes, one with PoseidonBN254); with the computed node in the
    selected cap entry nothing fails; a bumped sibling, leaf word or cap entry fails again - all of it, and one word of a Goldilocks entry one."""
    params = (MERKLE_VERIFY, mode) + shape
    n_in, depth, cap = shape
    rnd = ref.case_seed(*params, extra=11)
    ko = consts[0]
    root = 4 if mode == 0 else 1
    assert vref.expected(oracle, ko, 21, params, ref.random_items(rnd, *params)) == ([], root)
    for index in (None, 0, (1 << depth) - 1):
        items = vref.valid_merkle(oracle, ko, 21, params, rnd, index=index)
        assert vref.expected(oracle, ko, 21, params, items) == ([], 0)
    slot = vref.cap_slot(params, items)
    bare_leaf = mode == 0 and depth == cap and n_in <= 4      # (4, 2, 2) with Goldilocks hashes: the node IS the leaf (hash_or_noop, no level): one word differs
    assert vref.expected(oracle, ko, 21, params, vref.bump_item(params, items, 0)) == ([], 1 if bare_leaf else root)      # a leaf word
    assert vref.expected(oracle, ko, 21, params, vref.bump_item(params, items, slot, word=2)) == ([], 1)         # one word of the selected entry
    if cap > 0:      # an entry the index does not select is not compared
        other = n_in + 1 + ((slot - n_in - 1) ^ 1)
        assert vref.expected(oracle, ko, 21, params, vref.bump_item(params, items, other)) == ([], 0)
    if depth > cap:
        assert vref.expected(oracle, ko, 21, params, vref.bump_item(params, items, len(items) - 1, word=3)) == ([], root)      # the last sibling


def test_result_words_are_the_output_wires(oracle, consts):
    """Goldilocks wires one word each, native wires four little-endian words; the published BN254 vector comes out as its words."""
    ko = consts[0]
    rnd = ref.case_seed(GL_PERMUTE, 0, 0, 0, 0, extra=12)
    for params in ((GL_PERMUTE, 0, 0, 0, 0), (BN_PERMUTE, 0, 0, 0, 0), (HASH_NO_PAD, 0, 9, 0, 0), (HASH_NO_PAD, 1, 10, 0, 0), (TWO_TO_ONE, 0, 0, 0, 0), (TWO_TO_ONE, 1, 0, 0, 0)):
        items = ref.random_items(rnd, *params)
        words, failing, cells, adv = vref.oracle_values(oracle, ko, 21, params, items, want_cells=True)
        assert len(words) == vref.NUM_RESULTS[params[0]] and failing == []
        per = 1 if ref.family(params[0], params[1]) == 0 else 4
        assert len(cells) * per == len(words)
        for k, c in enumerate(cells):      # the wires' cells carry the words
            v = int.from_bytes(adv[c * 32:(c + 1) * 32], "little")
            assert [(v >> (64 * i)) & vref.MASK64 for i in range(per)] == words[k * per:(k + 1) * per] and v >> (64 * per) == 0
