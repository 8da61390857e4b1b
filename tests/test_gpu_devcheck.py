"""The hand-written wavefront arithmetic ON THE DEVICE, at its edge cases: tests/hip/devcheck.hip runs the product's own __device__ functions
(csrc/glperm.h glq_*, glq_mds_small, glq_dense12, glp_permute_lanes; rowfr.h mont and the ways to build its operands; rowperm.h bn_permute_rows with and
without its stores; bnquad.h QuadSinkT::bn_values as QUAD_VALUES and QUAD_VERDICT; the plain C++ routes of field.h and montform.h) on chosen words, and every result word is compared with Python integers (tests/devcheck_ref.py).  The host checks
under tests/cpp/ pin the algorithms; this pins the instructions: the carry-out of v_mad_u64_u32 into a scalar pair, the vcc chains, the wait states
behind an asm block, the DPP bank masks and bound_ctrl, the lane swaps - with lanes of one wavefront needing different corrections in one instruction.

One child process per group, one device context each, under its own time limit; a non-zero status fails the test with the child's output."""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import devcheck_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def devcheck(tmp_path_factory):
    assert shutil.which("hipcc"), "the device harness needs hipcc"
    exe = str(tmp_path_factory.mktemp("devcheck") / "devcheck")
    r = subprocess.run(ref.harness_command(exe), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def run_group(exe, group, tmp_path):
    cases_of, pack, check = ref.GROUPS[group]
    cases = cases_of()
    fin, fout = str(tmp_path / (group + ".in")), str(tmp_path / (group + ".out"))
    open(fin, "wb").write(pack(cases))
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", "120", exe, group, fin, fout], capture_output=True, text=True)
    dt = time.time() - t0
    assert r.returncode == 0, "devcheck %s: exit status %d\n%s%s" % (group, r.returncode, r.stdout, r.stderr)
    out = np.fromfile(fout, dtype="<u8")
    t0 = time.time()
    msgs = check(cases, out)
    print("devcheck %s: child process %.2f s, comparison %.2f s; %s" % (group, dt, time.time() - t0, r.stdout.strip()))
    assert not msgs, "\n".join(msgs)
    return cases


def test_glq_per_lane_primitives_and_chains(devcheck, tmp_path):
    cases = run_group(devcheck, "glq", tmp_path)
    for op, cls in (("reduce", ref.reduce_class), ("mul", lambda a, b, c: ref.product_class(a, b)), ("muladd", ref.product_class)):
        per, waves = ref.class_counts(cases[op], cls)
        print("  glq_%s: %d cases (%s), %d of %d wavefronts hold all four classes" % (op, len(cases[op]), ", ".join("%s %d" % x for x in zip(ref.CLASSES, per)), waves, len(cases[op]) // 64))
    print("  glq_reduce96: %d cases, glq_add: %d cases" % (len(cases["reduce96"]), len(cases["add"])))


def test_mds_small_and_dense12_blocks(devcheck, tmp_path):
    cases = run_group(devcheck, "mds", tmp_path)
    print("  glq_mds_small: %d wavefronts, glq_dense12: %d wavefronts" % (len(cases["mds"]), len(cases["d12"])))


def test_glp_permute_lanes(devcheck, tmp_path):
    cases = run_group(devcheck, "perm", tmp_path)
    print("  glp_permute_lanes: %d tables, %d cases (one wavefront each)" % (len(cases["tabs"]), len(cases["cases"])))


def test_row_montgomery_product_and_operands(devcheck, tmp_path):
    cases = run_group(devcheck, "mont", tmp_path)
    print("  rf::mont: %d wavefronts, four products each, both ways to build the operand" % len(cases))


def test_bn_permute_rows(devcheck, tmp_path):
    cases = run_group(devcheck, "bn", tmp_path)
    print("  bn_permute_rows, storing and store-free: %d tables (%d of them adversarial: %s), %d cases (one wavefront each)"
          % (len(cases["tabs"]), len(ref.ADVERSARIAL), ", ".join(ref.ADVERSARIAL), len(cases["cases"])))


def test_bn_values_quad_walk_at_its_stated_bounds(devcheck, tmp_path):
    """QuadSinkT::bn_values (QUAD_VALUES, then QUAD_VERDICT on the same pointers) on the tables that take its lazy values to their stated bounds
    (devcheck_ref.lazy_sets): the stored state, the 168 S-box words and both returned states against the limb model and the integer permutation; nothing
    outside a unit's own region written; a case gives the same words in whichever quad it sits, alone in its wavefront or with fifteen others."""
    cases = run_group(devcheck, "quad", tmp_path)
    ls = cases["launches"]
    live = sum(bin(x["live"]).count("1") for x in ls)
    print("  bn_values: %d tables, %d wavefronts (%d with all sixteen quads, %d with one; unit_local 0: %d, 1: %d), %d live quads, each as QUAD_VALUES and QUAD_VERDICT"
          % (len(cases["tabs"]), len(ls), sum(1 for x in ls if x["live"] == 0xFFFF), sum(1 for x in ls if x["live"] != 0xFFFF), sum(1 for x in ls if x["unit"] == 0),
             sum(1 for x in ls if x["unit"] == 1), live))
    assert {x["live"] for x in ls} == {0xFFFF, 1 << 0, 1 << 5, 1 << 15} and {x["unit"] for x in ls} == {0, 1}


def test_plain_routes_as_the_device_compiler_builds_them(devcheck, tmp_path):
    cases = run_group(devcheck, "plain", tmp_path)
    print("  " + ", ".join("%s %d" % (k, len(cases[k])) for k in ref.PLAIN_OPS))
