"""The prover's value hashers (csrc/proverhash.h: the two permutations, hash_or_noop and two_to_one as prover.hip's kernels and host transcript
run them), compiled as plain C++ and held to the oracle on the host: orc_nv_gl_permute, orc_nv_bn_permute and orc_nv_hash_or_noop on the published
and on seeded tables, both instantiations of the Goldilocks permutation, every input length of the two leaf hashers in both hash modes."""
import ctypes as C
import json
import os
import random
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GL_P = 0xFFFFFFFF00000001
FR_R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
K_GL, K_BN, K_HASH, K_TWO = range(4)
SEEDS = (0xC0FFEE, 0x5EED0001, 0x5EED0002)


def _limbs(x):
    return [(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def _group(kind, k, cases):
    """One group of the case file: cases are flat lists of u64 words."""
    return struct.pack("<2Q", kind, len(cases)) + bytes(k) + b"".join(struct.pack("<%dQ" % len(c), *c) for c in cases)


def _full_width(oracle, seed):
    """Seeded tables with full-width entries in every Goldilocks table, the MDS rows included (as test_glperm_values.py builds them): gl_mds_is_small is false."""
    k = oracle.synth_consts(seed)
    trng = random.Random(seed)
    for name in ("all_round_constants", "mds_circ", "mds_diag", "fast_partial_first_round_constant", "fast_partial_round_constants"):
        arr = getattr(k, name)
        for i in range(len(arr)):
            arr[i] = trng.randrange(1 << 63, GL_P)
    for name in ("fast_partial_round_initial_matrix", "fast_partial_round_w_hats", "fast_partial_round_vs"):
        arr = getattr(k, name)
        for i in range(len(arr)):
            for j in range(len(arr[i])):
                arr[i][j] = trng.randrange(1 << 63, GL_P)
    # (mds_circ[0] + mds_diag[0] is formed as a 64-bit sum by the gadget, in the field by the value walks: the same element unless the sum wraps 2^64)
    k.mds_circ[0] = trng.randrange(1 << 63, 5 << 61); k.mds_diag[0] = trng.randrange(1 << 62, 3 << 61)
    return k


def _gl_permute(L, k, st):
    buf = (C.c_uint64 * 12)(*st)
    L.orc_nv_gl_permute(C.byref(k), buf)
    return list(buf)


def _bn_permute(oracle, k, st):
    buf = (oracle.Fr * 4)(*[oracle.Fr.from_int(x) for x in st])
    oracle.lib().orc_nv_bn_permute(C.byref(k), buf)
    return [buf[i].to_int() for i in range(4)]


def test_prover_hashers_match_the_oracle_on_the_host(tmp_path, oracle):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    L = oracle.lib()
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "poseidon_published.json")))
    vecs = gold["goldilocks_w12"]["permutation_vectors"]
    assert len(vecs) >= 3 and vecs[0]["in"] == ["0x0"] * 12 and vecs[0]["out"][0] == "0x3c18a9786cb0b359"      # plonky2's three lead the list
    kp = oracle.published_consts()
    full = [_full_width(oracle, seed) for seed in SEEDS]
    rng = random.Random(20241021)
    gl_edges = [[0] * 12, [GL_P - 1] * 12, [1] * 12, list(range(GL_P - 12, GL_P))]
    want = {"gl_small": 0, "gl_full": 0, "bn": 0, "hash16": 0, "hash32": 0, "two": 0}

    # gl_permute: the published vectors, then edge and random states against the oracle; small-MDS tables run both instantiations
    blob = _group(K_GL, kp, [[int(x, 16) for x in v["in"]] + [int(x, 16) for x in v["out"]] for v in vecs]); want["gl_small"] += len(vecs)
    for k, key in [(kp, "gl_small")] + [(kf, "gl_full") for kf in full]:
        states = gl_edges + [[rng.randrange(GL_P) for _ in range(12)] for _ in range(60)]
        blob += _group(K_GL, k, [st + _gl_permute(L, k, st) for st in states]); want[key] += len(states)
    # bn_permute_m between to_mont and from_mont
    for k in [kp] + full:
        states = [[0] * 4, [FR_R - 1] * 4] + [[rng.randrange(FR_R) for _ in range(4)] for _ in range(12)]
        blob += _group(K_BN, k, [sum((_limbs(x) for x in st + _bn_permute(oracle, k, st)), []) for st in states]); want["bn"] += len(states)
    # hash_or_noop: every length of both instantiations in both modes (the no-op edge, partial and exact rate blocks, one or two trailing words of an element)
    for k in (kp, full[0]):
        cases = []
        for maxn in (16, 32):
            for mode in (0, 1):
                for n in range(maxn + 1):
                    vals = [rng.randrange(GL_P) for _ in range(n)]
                    out = (C.c_uint64 * 4)()
                    L.orc_nv_hash_or_noop(C.byref(k), mode, (C.c_uint64 * max(n, 1))(*vals), n, out)
                    cases.append([mode, maxn, n] + vals + [0] * (32 - n) + list(out)); want["hash%d" % maxn] += 1
        blob += _group(K_HASH, k, cases)
    # two_to_one from the oracle's two permutations: Goldilocks = the first four words of the permutation of (l, r, 0); BN254 = slot 0 of that of (0, 0, l, r)
    for k in (kp, full[0]):
        cases = []
        for mode in (0, 1):
            pairs = [([0] * 4, [0] * 4), ([GL_P - 1] * 4, [GL_P - 1] * 4), ([0] * 4, [GL_P - 1] * 4)]
            pairs += [([rng.randrange(GL_P) for _ in range(4)], [rng.randrange(GL_P) for _ in range(4)]) for _ in range(8)] if mode == 0 else \
                     [(_limbs(FR_R - 1), _limbs(FR_R - 1))] + [(_limbs(rng.randrange(FR_R)), _limbs(rng.randrange(FR_R))) for _ in range(8)]
            for l, r in pairs:
                if mode == 0:
                    out = _gl_permute(L, k, l + r + [0] * 4)[:4]
                else:
                    # (four words at p - 1 are above r: no hash of this mode, whose words are a canonical element.  two_to_one's to_mont takes any 256 bits
                    # as the element they denote; the oracle's permutation takes canonical elements only, so it is given that element)
                    out = _limbs(_bn_permute(oracle, k, [0, 0] + [sum(w << (64 * i) for i, w in enumerate(h)) % FR_R for h in (l, r)])[0])
                cases.append([mode] + l + r + out); want["two"] += 1
        blob += _group(K_TWO, k, cases)

    path = os.path.join(str(tmp_path), "cases.bin")
    open(path, "wb").write(blob)
    exe = os.path.join(str(tmp_path), "proverhash_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "halo2-plonky2-verifier_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "proverhash_check.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    assert want["gl_full"] == 3 * 64 and want["hash16"] == 2 * 2 * 17 and want["hash32"] == 2 * 2 * 33
    assert "groups: 13 " + " ".join("%s: %d" % (key, want[key]) for key in ("gl_small", "gl_full", "bn", "hash16", "hash32", "two")) in r.stdout, r.stdout
