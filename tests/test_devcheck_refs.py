"""The references, generators and harness of the device checks (tests/test_gpu_devcheck.py), as far as they can be checked without a GPU: the Python
walks of the two Poseidon permutations reproduce the published vectors and the oracle, the generated inputs meet their coverage conditions (computed
from the inputs alone), and tests/hip/devcheck.hip cross-compiles for gfx950."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import devcheck_ref as ref


def test_python_permutations_reproduce_the_published_vectors():
    pub = ref.published()
    assert len(pub["gl_vectors"]) >= 3 and pub["gl_vectors"][0][0] == [0] * 12 and pub["gl_vectors"][0][1][0] == 0x3c18a9786cb0b359
    for st, out in pub["gl_vectors"]:
        assert ref.gl_permute(st, pub["k"]) == out
    assert len(pub["bn_vectors"]) >= 1
    for st, out in pub["bn_vectors"]:
        assert ref.bn_permute(st, pub["k"])[0] == out


def test_python_permutations_equal_the_oracle_on_random_states(oracle):
    L = oracle.lib()
    rng = random.Random(20260101)
    for k in (oracle.published_consts(), oracle.synth_consts(0xC0FFEE)):
        K = [int(w) for w in np.frombuffer(bytes(k), dtype="<u8")]
        assert len(K) == ref.KW
        ctx = oracle.Ctx(21)
        for _ in range(20):
            st = [rng.randrange(ref.P) for _ in range(12)]
            ins = (oracle.AV * 12)(*[L.orc_gl_load_witness(ctx.p, x) for x in st]); outs = (oracle.AV * 12)()
            L.orc_gl_poseidon_permute(ctx.p, C.byref(k), ins, outs)
            assert ref.gl_permute(st, K) == [outs[i].v.to_int() for i in range(12)]
        for _ in range(20):
            st = [rng.randrange(ref.R) for _ in range(4)]
            ins = (oracle.AV * 4)(*[L.orc_load_witness(ctx.p, C.byref(oracle.Fr.from_int(x))) for x in st]); outs = (oracle.AV * 4)()
            L.orc_bn_poseidon_permute(ctx.p, C.byref(k), ins, outs)
            assert ref.bn_permute(st, K)[0] == [outs[i].v.to_int() for i in range(4)]
        ctx.close()
    assert [int(w) for w in np.frombuffer(bytes(oracle.published_consts()), dtype="<u8")] == ref.published()["k"]


def test_device_harness_cross_compiles(tmp_path):
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc")
    exe = os.path.join(str(tmp_path), "devcheck")
    r = subprocess.run(ref.harness_command(exe), capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(exe), r.stdout + r.stderr
    src = open(os.path.join(ref.ROOT, "tests", "hip", "devcheck.hip")).read()
    assert not re.search(r"\basm\s*(volatile\s*)?\(", src)      # results leave through plain stores: the harness has no assembly of its own


def test_glq_reduce_cases_reach_every_correction_in_mixed_wavefronts():
    cases = ref.glq_cases()
    red = cases["reduce"]
    per, waves = ref.class_counts(red, ref.reduce_class)
    assert min(per) >= 1000, dict(zip(ref.CLASSES, per))      # the host check's own threshold, for each of none / carry / borrow / both
    assert waves >= 100, waves
    # nothing the issue lists was dropped on the way: the full cross product of the edge words, 2^16 random triples and 2^16 products
    have = set(red)
    assert all((lo, p2, p3) in have for lo in ref.E64 for p2 in ref.E32 for p3 in ref.E32)
    assert len(red) >= 16 * 7 * 7 + 2 * (1 << 16) + 2 * (1 << 13) and len(red) % 64 == 0
    # the classification is the one the host restatement counts with (tests/cpp/glq_reduce_check.cpp)
    for lo, p2, p3 in red[:4096]:
        m = p2 * ref.EPS + lo
        assert ref.reduce_class(lo, p2, p3) == (1 if m >> 64 else 0) + (2 if ((m & ref.M64) >> 32) == 0 and (m & ref.M32) < p3 else 0)
    for lo, h0, h1 in cases["reduce96"]:
        assert lo + h1 * ref.EPS < 1 << 64
    assert any(lo + h1 * ref.EPS == ref.M64 for lo, h0, h1 in cases["reduce96"])      # the precondition's last admitted sum
    B = 1 << ref.small_mds_bits()
    assert B == 1 << 26
    assert (12 * 2 * (B - 1) * ref.M32 + ref.M32, ) * 2 == tuple((lo, h0 + (h1 << 32)) for lo, h0, h1 in cases["reduce96"] if lo == 12 * 2 * (B - 1) * ref.M32 + ref.M32)[0]
    for op in ("mul", "muladd"):
        ops = [v for x in cases[op] for v in x[:2]]
        assert sum(1 for v in ops if v >= ref.P) >= 1000 and sum(1 for v in ops if v < ref.P) >= 1000 and len(cases[op]) % 64 == 0
    per, waves = ref.class_counts(cases["muladd"], ref.product_class)
    assert min(per) >= 1000 and waves >= 32, (per, waves)
    per, _ = ref.class_counts(cases["mul"], lambda a, b, c: ref.product_class(a, b))
    assert per[0] >= 256 and per[1] >= 256 and per[2] >= 256, per      # (a product of two words with both corrections is a 2^-48 event: glq_muladd and glq_reduce carry that class)
    assert all(a < ref.P or b < ref.P for a, b, c in cases["add"]) and len(cases["add"]) % 64 == 0


def test_block_and_permutation_cases_cover_what_they_are_written_for():
    B = 1 << ref.small_mds_bits()
    m = ref.mds_cases()
    names = [c["name"] for c in m["mds"]]
    assert len(names) == 6 * 5 * 3 and len(set(names)) == len(names)
    assert max(e for c in m["mds"] for row in c["m"] for e in row) == 2 * (B - 1)
    assert any(all(x == ref.M64 for x in c["x"][:12]) and all(e == 2 * (B - 1) for row in c["m"] for e in row) and c["next"][0] == ref.P - 1 for c in m["mds"])
    t1 = ((1 << 22) - 1) * ref.M32
    assert any(c["limb"][:12] == [(1 << 22) - 1] * 12 and c["w"][0] == [ref.M64] * 12 and c["a0"][0] == 24 * t1 + ref.M32 for c in m["d12"])
    assert (36 * t1 + ref.M32) ** 5 < 1 << 296      # 36 terms and a dword: below 2^59.2
    p = ref.perm_cases()
    assert [ref._is_small(K) for K in p["tabs"]] == [True, True, True, True, False, True, False, False]
    assert {(c["small"], c["n"]) for c in p["cases"]} == {(0, 1), (0, 8), (1, 1), (1, 8)} and sum(c["list"] for c in p["cases"]) == 2
    assert all(len(K) == ref.KW and max(K) < 1 << 64 for K in p["tabs"]) and len(ref.perm_expected()) == len(p["cases"])
    assert len(ref.perm_pack(p)) == 8 * (2 + len(p["tabs"]) * ref.KW + 16 * len(p["cases"]))
    mc = ref.mont_cases()
    assert len(mc) == len(ref.MONT_KS) * 3 * 60
    for c in mc:      # no 64-bit column of T = a x b, nor of T + m N behind it (m's limbs below 2^30 + 2^6, N's below 2^29), wraps
        for a, b in zip(c["a"], c["b"]):
            assert max(sum(a[i] * b[k - i] for i in range(9) if 0 <= k - i < 9) for k in range(17)) + 9 * ref.M29 * ((1 << 30) + (1 << 6)) < 1 << 64
            assert ref.limbs_value(a) < 1 << 261 and ref.limbs_value(b) < 1 << 261
    assert any(ref.limbs_value(c["a"][1]) == ref.R - 1 for c in mc) and any(ref.limbs_value(c["a"][0]) == 0 for c in mc)
    assert len(ref.mont_pack(mc)) == 8 * (1 + 68 * len(mc))
    b = ref.bn_cases()
    assert len(b["cases"]) == 12 and len(ref.bn_pack(b)) == 8 * (2 + 2 * ref.KW + 20 * 12)
    pl = ref.plain_cases()
    assert all(len(pl[k]) % 64 == 0 and len(pl[k]) >= 1 << 14 for k in ref.PLAIN_OPS)
    assert all(((1 << 32 * n) - 1,) in pl["mf%d" % n] for n in (2, 3, 4, 8))
    assert len(ref.plain_pack(pl)) == 8 * (8 + sum(len(pl[k]) * w for k, w in zip(ref.PLAIN_OPS, (2, 3, 8, 9, 1, 2, 2, 4))))
    g = ref.glq_cases()
    assert len(ref.glq_pack(g)) == 8 * (8 + 3 * sum(len(g[k]) for k in ref.GLQ_OPS))
    assert len(ref.mds_pack(m)) == 8 * (2 + 512 * len(m["mds"]) + 928 * len(m["d12"]))
