"""Code-generation invariants of k_verdict_merkle_row (csrc/verdict.hip; rowperm.h bn_permute_rows<false>), on the cross-compiled gfx950 assembly
(no GPU needed; in the manner of tests/test_codegen_invariants.py).

The kernel keeps nothing but comparisons: it writes global memory through the VerdictAcc atomics alone - no global, flat or buffer store anywhere in
it (the S-box stores of the storing form are gone, and nothing else took their place).  Dropping the stores must not have changed the round: its
partial-round loop holds the three lane-cooperative products (3 x 29 multiply-adds) that k_merkle_bn_values_row's loop holds, without a scratch or
flat access, with the table entries read ahead of the first product, and no longer than that loop; the seven-product full-round loops are there too."""
import re

import pytest

from codegen_util import compile_asm, count as _count, loops as _loops


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("asm")
    return {src: compile_asm(src, d) for src in ("verdict.hip", "glue.hip")}


def _kernel(lines, mangled_prefix):
    """(first, last) line of a kernel: its label to its .Lfunc_end (a kernel has several s_endpgm)."""
    start = next(i for i, l in enumerate(lines) if re.match("^" + re.escape(mangled_prefix) + r"\w*:", l))
    end = next(i for i in range(start, len(lines)) if re.match(r"^\.Lfunc_end\d+:", lines[i]))
    return start, end


def _partial_loop(lines, lo, hi):
    loops = list(_loops(lines, lo, hi))
    partial = [(a, b) for a, b in loops if 85 <= _count(lines, a, b, "v_mad_u64_u32") <= 90]
    assert partial, "partial-round loop (three products of 29 multiply-adds) not found"
    return min(partial, key=lambda ab: ab[1] - ab[0]), loops


def test_the_row_verdict_kernel_writes_global_memory_through_atomics_only(asm):
    v = asm["verdict.hip"]
    lo, hi = _kernel(v, "_ZN3h2w20k_verdict_merkle_row")
    for kind in ("global_store", "flat_store", "buffer_store"):
        assert _count(v, lo, hi, kind) == 0, f"{kind} in k_verdict_merkle_row"
    assert _count(v, lo, hi, "global_atomic") >= 4, "the verdict words' atomics (add, or, umin, cmpswap) are gone"
    assert not [l for l in v[lo:hi + 1] if re.match(r"^\s+s_(swappc|call)_b64", l)], "the flattened kernel calls out of line (a callee could store)"


def test_its_partial_round_is_the_storing_forms_without_the_stores(asm):
    v, g = asm["verdict.hip"], asm["glue.hip"]
    (a, b), loops = _partial_loop(v, *_kernel(v, "_ZN3h2w20k_verdict_merkle_row"))
    (c, d), _ = _partial_loop(g, *_kernel(g, "_ZN3h2w22k_merkle_bn_values_row"))
    mads, ref_mads = _count(v, a, b, "v_mad_u64_u32"), _count(g, c, d, "v_mad_u64_u32")
    print(f"multiply-adds per partial round: {mads} (storing form {ref_mads})")
    assert mads == ref_mads, "the store-free round is not the three products of the storing round"
    assert _count(g, c, d, "global_store") == 3 and _count(v, a, b, "global_") == 0      # the only difference that is meant
    assert _count(v, a, b, "scratch_") + _count(v, a, b, "flat_") == 0, "scratch / flat accesses in the store-free partial round"
    assert not [l for l in v[a:b + 1] if re.search(r"s_waitcnt.*vmcnt", l)], "a vector-memory wait in a loop without vector memory traffic"
    n = sum(1 for l in v[a:b + 1] if re.match(r"^\s+[a-z]", l))
    ref_n = sum(1 for l in g[c:d + 1] if re.match(r"^\s+[a-z]", l))
    print(f"instructions per partial round: {n} (storing form {ref_n})")
    assert n <= ref_n, "the round grew although it lost its stores"
    first_mad = next(i for i in range(a, b + 1) if re.match(r"^\s+v_mad_u64_u32", v[i]))
    assert _count(v, a, first_mad, "ds_read") >= 6, "the round's table entries are no longer read ahead of its first product"
    full = [(e, f) for e, f in loops if (f < a or e > b) and 195 <= _count(v, e, f, "v_mad_u64_u32") <= 215]
    assert full, "full-round loop (seven products) not found"
    for e, f in full:
        assert _count(v, e, f, "scratch_") + _count(v, e, f, "flat_") + _count(v, e, f, "global_store") == 0
