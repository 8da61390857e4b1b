"""The expansion kernels ON THE DEVICE, on records written by hand: tests/hip/expandcheck.hip links the product's own csrc/expand.hip and calls launch_expand
once per process on a case file; every cell of the output buffer - record cells, the gaps between records, the slack behind a proof's last cell and 64 guard
cells at both ends - is compared bit for bit with Python integers (tests/expand_ref.py, pinned to the oracle by tests/test_expand_refs.py).  The rest of the
suite reaches these kernels only through plans and eager contexts, i.e. with the records a seeded random proof happens to produce: V = A B + C >= p^2, a
quotient of 65 bits, r = 0 or p - 1, off-domain witnesses, and the tile geometry of expand_fast (short last pass and row, the all-GLOP shortcut next to mixed
groups, a record whose virtual cell list starts in front of flat cell 0, the own-lane templates across a column boundary) are chosen here instead.

Which instantiation a case selects is launch_expand's own choice; expand_ref.Case.kernel() states it and why, and the test asserts the conditions the harness
prints.  One child process per test, under its own time limit; a non-zero status fails the test with the child's output, and nothing is retried."""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import expand_ref as ref

pytestmark = pytest.mark.gpu

FAST = [21, 13, 8]


@pytest.fixture(scope="module")
def expandcheck(tmp_path_factory):
    assert shutil.which("hipcc"), "the device harness needs hipcc"
    exe = str(tmp_path_factory.mktemp("expandcheck") / "expandcheck")
    t0 = time.time()
    r = subprocess.run(ref.harness_command(exe), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    print("expandcheck: harness + expand.hip compiled in %.1f s" % (time.time() - t0))
    return exe


def run_case(exe, cs, tmp_path, kernel):
    assert cs.kernel() == kernel, (cs.name, cs.kernel())      # the instantiation this case is written for
    fin, fout = str(tmp_path / "case.in"), str(tmp_path / "case.out")
    open(fin, "wb").write(ref.pack_case(cs))
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", "120", exe, fin, fout], capture_output=True, text=True)
    dt = time.time() - t0
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):      # a fault, an abort or the time limit: nothing more is started on this device in this session
        pytest.exit("expandcheck %s: exit status %d\n%s%s" % (cs.name, r.returncode, r.stdout, r.stderr), returncode=1)
    assert r.returncode == 0, "expandcheck %s: exit status %d\n%s%s" % (cs.name, r.returncode, r.stdout, r.stderr)
    assert cs.conditions() in r.stdout.splitlines(), r.stdout
    got = np.fromfile(fout, dtype=np.uint8)
    os.remove(fin); os.remove(fout)      # (up to 48 MB a case: not left to the temporary directory's retention)
    t0 = time.time()
    msgs = ref.check(cs, got)
    print("expandcheck %s -> %s: child process %.2f s, comparison %.2f s, %d cells" % (cs.name, kernel, dt, time.time() - t0, cs.total_cells()))
    assert not msgs, "%d cells differ\n%s" % (len(msgs), "\n".join(msgs[:40]))


@pytest.mark.parametrize("nrec", ref.STATIC_NREC)
@pytest.mark.parametrize("L", FAST)
def test_flat_canonical_static_grid(expandcheck, tmp_path, L, nrec):
    run_case(expandcheck, ref.static_case(L, nrec), tmp_path, "expand_fast<%d, false, false>" % L)


@pytest.mark.parametrize("per_cu,nproofs", ref.ROAM_SHAPES)
@pytest.mark.parametrize("L", FAST)
def test_flat_canonical_roaming_grid(expandcheck, tmp_path, L, per_cu, nproofs):
    run_case(expandcheck, ref.roam_case(L, per_cu, nproofs), tmp_path, "expand_fast<%d, true, false>" % L)


@pytest.mark.parametrize("nrec", ref.STATIC_NREC)
@pytest.mark.parametrize("L", FAST)
def test_montgomery_static_grid(expandcheck, tmp_path, L, nrec):
    """the per-step word counts of the flush (L = 8 has two-word steps, L = 21 none) and the exchange of halves between lane pairs"""
    run_case(expandcheck, ref.static_case(L, nrec, mont=True), tmp_path, "expand_fast_mont<%d, false, false>" % L)


@pytest.mark.parametrize("per_cu,nproofs", ref.ROAM_SHAPES)
@pytest.mark.parametrize("L", FAST)
def test_montgomery_roaming_grid(expandcheck, tmp_path, L, per_cu, nproofs):
    run_case(expandcheck, ref.roam_case(L, per_cu, nproofs, mont=True), tmp_path, "expand_fast_mont<%d, true, false>" % L)


@pytest.mark.parametrize("L", FAST)
def test_columns_through_the_fast_kernel_canonical(expandcheck, tmp_path, L):
    """column boundaries on a record's first cell, its last cell, inside, at 8- and 16-cell flush-step edges, inside T_CONST4 and T_REP12, between two records"""
    run_case(expandcheck, ref.column_case(L), tmp_path, "expand_fast<%d, false, true>" % L)


@pytest.mark.parametrize("L", FAST)
def test_columns_through_the_fast_kernel_montgomery(expandcheck, tmp_path, L):
    run_case(expandcheck, ref.column_case(L, mont=True), tmp_path, "expand_fast_mont<%d, false, true>" % L)


@pytest.mark.parametrize("nrec", ref.GENERIC_NREC)
@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("cols", [0, 1])
@pytest.mark.parametrize("counter", [0, 1])
@pytest.mark.parametrize("L", [17, 20])
def test_generic_kernel(expandcheck, tmp_path, L, counter, cols, mont, nrec):
    """lookup_bits the fast kernel is not instantiated for: with and without the work counter, flat and with a few hundred columns, in both forms"""
    run_case(expandcheck, ref.generic_case(L, nrec, counter, cols, bool(mont)), tmp_path,
             "%s<32, 5, %s>" % ("expand_kernel_mont" if mont else "expand_kernel_t", "true" if cols else "false"))


@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("which", [0, 1])
def test_one_layout_through_the_generic_and_the_fast_kernel(expandcheck, tmp_path, which, mont):
    """L = 20 and L = 21 share a cell layout: the same records and offsets, each result compared with Python (not with the other)"""
    cs = ref.shared_layout_cases(bool(mont))[which]
    m = "_mont" if mont else ""
    run_case(expandcheck, cs, tmp_path, ("expand_kernel%s<32, 5, false>" % (m or "_t")) if which == 0 else "expand_fast%s<21, false, false>" % m)
