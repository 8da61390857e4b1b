"""Code generation of the expansion kernel's two output forms, on the cross-compiled gfx950 assembly (no GPU needed; the model is
test_codegen_invariants.py): the Montgomery instantiation converts in registers - no scratch or flat access anywhere, its flush loop included -
and the canonical instantiations are what they were before the form existed."""
import re

import pytest

from codegen_util import compile_asm, count as _count, loops as _loops

# Instructions of the canonical kernels at the commit before the output form, c4c5383 ("Traced plans: (proof, query) sharding, keygen metadata and
# status 4"): `git archive c4c5383 halo2-plonky2-verifier_amd/csrc include | tar -x -C DIR`, then in DIR/halo2-plonky2-verifier_amd/csrc
# `hipcc <codegen_util.FLAGS> expand.hip -o expand.s`, counted with _function / _count below.  The body now takes its arguments by reference from a one-line
# kernel; the scheduler answers with up to nine instructions fewer here; 16 (under 1 % of the smallest kernel) is allowed.
PARENT = {"_ZN3h2w11expand_fastILi21ELb0ELb0EE": 1722, "_ZN3h2w11expand_fastILi21ELb1ELb0EE": 1908, "_ZN3h2w11expand_fastILi21ELb1ELb1EE": 2210,
          "_ZN3h2w11expand_fastILi13ELb1ELb0EE": 1949, "_ZN3h2w11expand_fastILi8ELb1ELb0EE": 2096, "_ZN3h2w15expand_kernel_tILi32ELi5ELb0EE": 1135}
TOLERANCE = 16


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return compile_asm("expand.hip", tmp_path_factory.mktemp("asm"))


def _function(lines, prefix):
    start = next(i for i, l in enumerate(lines) if re.match("^" + re.escape(prefix) + r"\w*:", l))
    return start, next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])


def test_canonical_instantiations_are_unchanged(asm):
    for name, parent in PARENT.items():
        lo, hi = _function(asm, name)
        n = _count(asm, lo, hi)
        assert abs(n - parent) <= TOLERANCE, f"{name}: {n} instructions, {parent} before the output form"


@pytest.mark.parametrize("name", ["_ZN3h2w16expand_fast_montILi21ELb1ELb0EE", "_ZN3h2w16expand_fast_montILi21ELb0ELb0EE", "_ZN3h2w16expand_fast_montILi21ELb1ELb1EE"])
def test_montgomery_flush_converts_in_registers(asm, name):
    lo, hi = _function(asm, name)
    assert _count(asm, lo, hi, "scratch_") == 0 and _count(asm, lo, hi, "flat_") == 0
    # the flush loop (groups of four records; its steps are unrolled): the innermost loop that holds the conversions (at least 16 + 4 + 15 multiply-adds
    # each) and the cell stores, and the exchange of halves between neighbouring lanes
    flush = [(a, b) for a, b in _loops(asm, lo, hi) if _count(asm, a, b, "v_mad_u64_u32") + _count(asm, a, b, "v_mul_(lo|hi)_u32") >= 45 and _count(asm, a, b, "global_store_dwordx4") >= 2]
    assert flush, "flush loop with the conversion not found"
    a, b = min(flush, key=lambda ab: ab[1] - ab[0])
    assert _count(asm, a, b, "scratch_") == 0 and _count(asm, a, b, "flat_") == 0
    assert _count(asm, a, b, "global_load") == 0, "the flush loop reads memory behind its own stores"
    assert _count(asm, a, b, "ds_read_b128") >= 1
    assert sum(1 for l in asm[a:b + 1] if "quad_perm:[1,0,3,2]" in l) >= 4, "the halves are no longer exchanged with DPP moves"
    assert _count(asm, a, b, "ds_bpermute") == 0
    res = "\n".join(asm[hi:hi + 120])
    assert re.search(r"ScratchSize: 0\b", res) and re.search(r"Occupancy: [2-9]", res), "two blocks per CU no longer fit"
