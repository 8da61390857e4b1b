"""Python-integer references, input generators and comparisons of the device checks (tests/test_gpu_devcheck.py runs tests/hip/devcheck.hip on a GPU,
tests/test_devcheck_refs.py checks this module without one).  A plain module: no fixtures, no pytest.

Every group has three functions: <group>_cases() builds the inputs (deterministic), <group>_pack(cases) the harness's case file (raw little-endian
words, the layout written at the group's function in devcheck.hip), <group>_check(cases, out) compares the harness's result words and returns a list
of messages (empty: all equal).  Everything is exact; nothing has a tolerance."""
import functools
import json
import os
import random
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2-plonky2-verifier_amd", "csrc")

P = 0xFFFFFFFF00000001            # Goldilocks
EPS = 0xFFFFFFFF
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001      # BN254 Fr
M29 = (1 << 29) - 1
RINV261 = pow(1 << 261, -1, R)
FILL = 0xA5A5A5A5A5A5A5A5         # what the harness leaves in a result word no kernel wrote

# the edge words of tests/cpp/glq_reduce_check.cpp
E64 = [0, 1, 2, EPS - 1, EPS, EPS + 1, P - 1, P, P + 1, M64, M64 - 1, 1 << 32, (1 << 32) - 2, 1 << 63, 0xFFFFFFFF00000000, 0x00000000FFFFFFFE]
E32 = [0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF]
CLASSES = ("none", "carry", "borrow", "both")


def harness_command(out):
    """hipcc with the flags of build.sh and the two include directories."""
    flags = re.search(r'^FLAGS="(.*)"$', open(os.path.join(ROOT, "build.sh")).read(), flags=re.M).group(1).replace("$H2W_EXTRA", "").split()
    return ["hipcc", *flags, "-I", os.path.join(ROOT, "halo2-plonky2-verifier_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
            os.path.join(ROOT, "tests", "hip", "devcheck.hip"), "-o", out]


def words(xs):
    return np.array([int(x) for x in xs], dtype=np.uint64).astype("<u8")


def dwords(xs):
    a = np.array([int(x) for x in xs], dtype=np.uint32).astype("<u4")
    assert a.size % 2 == 0
    return a.view("<u8")


def _first(msgs, n=8):
    return msgs[:n] + (["... %d mismatches in all" % len(msgs)] if len(msgs) > n else [])


# ------------------------------------------------------------------------------------------------ (a) glq_reduce and its kin
def reduce_class(lo, p2, p3):
    """Which correction glq_reduce applies to lo + p2 2^64 + p3 2^96: u = lo + p2 eps carries out of 64 bits, u mod 2^64 - p3 borrows."""
    m = lo + p2 * EPS
    c, u = m >> 64, m & M64
    return (1 if c else 0) + (2 if u < p3 else 0)


def product_class(a, b, c=0):
    n = a * b + c
    return reduce_class(n & M64, (n >> 64) & M32, n >> 96)


def _mix_classes(cases, cls):
    """Deal the cases out class by class, so that the 64 lanes of a wavefront need different corrections in the same instruction; nothing is dropped."""
    pools = [[], [], [], []]
    for x in cases:
        pools[cls(*x)].append(x)
    out, at = [], [0, 0, 0, 0]
    while len(out) < len(cases):
        for k in range(4):
            if at[k] < len(pools[k]):
                out.append(pools[k][at[k]])
                at[k] += 1
    return out


def _pad64(cases, filler):
    return cases + [filler] * (-len(cases) % 64)


def class_counts(cases, cls):
    """(cases per class, wavefronts that hold all four classes)"""
    k = [cls(*x) for x in cases]
    per = [k.count(i) for i in range(4)]
    waves = sum(1 for w in range(0, len(k), 64) if len(set(k[w:w + 64])) == 4)
    return per, waves


@functools.lru_cache(None)
def glq_cases():
    rng = random.Random(0x676C71)
    r64 = lambda: rng.getrandbits(64)
    r32 = lambda: rng.getrandbits(32)
    red = [(lo, p2, p3) for lo in E64 for p2 in E32 for p3 in E32]
    red += [(r64(), r32(), r32()) for _ in range(1 << 16)]
    red += [(r32(), 0, r32()) for _ in range(1 << 13)]                                   # the borrow: u below 2^32 and below p3
    for _ in range(1 << 13):                                                             # carry AND borrow: u just past 2^64
        p2 = r32() or 1
        red.append((((-p2 * EPS) & M64) + (r64() & 0xFFFF), p2, r32()))
    for i in range(1 << 16):                                                             # products, as glq_mul forms them
        a = r64() if i & 1 else E64[rng.randrange(16)]
        b = r64() if i & 2 else E64[rng.randrange(16)]
        n = a * b
        red.append((n & M64, (n >> 64) & M32, n >> 96))
    red = _pad64(_mix_classes(red, reduce_class), (0, 0, 0))

    # glq_reduce96: lo + h0 2^32 + h1 2^64 with lo + h1 eps < 2^64, by construction
    r96 = []
    for h1 in E32 + [0x12345678]:
        top = M64 - h1 * EPS                                                             # the largest lo the precondition admits
        for lo in sorted({0, 1, EPS, 1 << 32, top >> 1, top - 1, top}):
            for h0 in E32:
                r96.append((lo, h0, h1))
    for i in range(1 << 14):                                                             # sums below 2^63
        s = 1 if i % 3 else 5
        hi = r64() >> s
        r96.append((r64() >> s, hi & M32, hi >> 32))
    s_mds = 12 * (2 * ((1 << small_mds_bits()) - 1)) * M32 + M32                         # the largest sums glq_mds_small and glq_dense12 can form
    s_d12 = 36 * ((1 << 22) - 1) * M32 + M32
    for s0 in (s_mds, s_d12):
        for s1 in (s_mds, s_d12, 0):
            r96.append((s0, s1 & M32, s1 >> 32))
    for lo, h0, h1 in r96:
        assert lo + h1 * EPS < 1 << 64 and lo < 1 << 64 and h0 <= M32 and h1 <= M32
    r96 = _pad64(r96, (0, 0, 0))

    any64 = lambda: rng.randrange(P, 1 << 64) if rng.randrange(4) == 0 else rng.randrange(P)      # canonical and not: any representative is an operand
    mul = [(a, b, E64[(i + j) % 16]) for i, a in enumerate(E64) for j, b in enumerate(E64)]
    mul += [(any64(), any64(), any64()) for _ in range(1 << 12)]
    for s in range(0, 24):                                                               # a b = p3 2^96 exactly: u = 0 < p3, the borrow alone
        for _ in range(16):
            p3 = rng.randrange(1, 1 << (31 - s)) if s < 31 else 1
            mul.append((1 << (63 - s), p3 << (33 + s), any64()))
    mul = _pad64(_mix_classes(mul, lambda a, b, c: product_class(a, b)), (0, 0, 0))

    mad = [(a, b, c) for a in E64 for b in E64 for c in (0, P - 1, M64, EPS)]
    mad += [(any64(), any64(), any64()) for _ in range(1 << 12)]
    for _ in range(1 << 11):                                                             # the borrow alone: a b = p3 2^96, c below p3
        p3 = rng.randrange(1 << 16, 1 << 31)
        mad.append((1 << 63, p3 << 33, rng.randrange(1 << 16)))
    made = 0
    while made < 1 << 11:                                                                # carry and borrow: c chosen so that lo + p2 eps lands just past 2^64
        a, b, t = any64(), any64(), r64() & 0xFFFF
        pr = a * b
        for g in (0, 1):
            p2 = ((pr >> 64) + g) & M32
            lo = (t - p2 * EPS) & M64
            c = (lo - pr) & M64
            n = pr + c
            if n & M64 == lo and (n >> 64) & M32 == p2 and product_class(a, b, c) == 3:
                mad.append((a, b, c))
                made += 1
                break
    mad = _pad64(_mix_classes(mad, product_class), (0, 0, 0))

    canon = [x for x in E64 if x < P]
    add = [(a, b, 0) for a in E64 for b in canon] + [(b, a, 0) for a in E64 for b in canon]      # one operand canonical
    add += [(r64(), rng.randrange(P), 0) for _ in range(1 << 11)] + [(rng.randrange(P), r64(), 0) for _ in range(1 << 11)]
    add = _pad64(add, (0, 0, 0))
    return dict(reduce=red, reduce96=r96, mul=mul, muladd=mad, add=add)


GLQ_OPS = ("reduce", "reduce96", "mul", "muladd", "add")


def glq_pack(cases):
    parts = [words([len(cases[k]) for k in GLQ_OPS] + [0, 0, 0])]
    for k in GLQ_OPS:
        for col in range(3):
            parts.append(words([x[col] for x in cases[k]]))
    return np.concatenate(parts).tobytes()


def _cmp_modp(name, got, want, msgs):
    for i, (g, w) in enumerate(zip(got, want)):
        g = int(g)
        if g % P != w:
            msgs.append("%s: case %d (wavefront %d, lane %d): got 0x%x, want 0x%x mod p" % (name, i, i // 64, i % 64, g, w))


def glq_check(cases, out):
    msgs, at = [], 0
    need = sum(len(cases[k]) * w for k, w in zip(GLQ_OPS, (2, 1, 3, 3, 1)))
    if len(out) != need:
        return ["glq: %d result words, expected %d" % (len(out), need)]

    def take(n):
        nonlocal at
        at += n
        return out[at - n:at]
    red = cases["reduce"]
    n = len(red)
    val = [(lo + (p2 << 64) + (p3 << 96)) % P for lo, p2, p3 in red]
    _cmp_modp("glq_reduce", take(n), val, msgs)
    _cmp_modp("glq_reduce of a glq_reduce", take(n), [(v + (p2 << 64) + (p3 << 96)) % P for v, (lo, p2, p3) in zip(val, red)], msgs)
    r96 = cases["reduce96"]
    _cmp_modp("glq_reduce96", take(len(r96)), [(lo + (h0 << 32) + (h1 << 64)) % P for lo, h0, h1 in r96], msgs)
    mul = cases["mul"]
    n = len(mul)
    _cmp_modp("glq_mul", take(n), [a * b % P for a, b, c in mul], msgs)
    _cmp_modp("glq_mul of a glq_mul", take(n), [a * b * c % P for a, b, c in mul], msgs)
    want = []
    for i in range(n):      # x^3 of the even row's lane times x^4 of the odd row's (glq_pair_rows)
        w, l = i // 64 * 64, i % 64
        e, o = w + (l & 0x20) + (l & 15), w + (l & 0x20) + 16 + (l & 15)
        want.append(pow(mul[e][0], 3, P) * pow(mul[o][0], 4, P) % P)
    _cmp_modp("the S-box shape (x^2, x^3 | x^4, lane swap, product)", take(n), want, msgs)
    mad = cases["muladd"]
    n = len(mad)
    _cmp_modp("glq_muladd", take(n), [(a * b + c) % P for a, b, c in mad], msgs)
    want_acc, want_s0 = [], []
    for w in range(0, n, 64):      # acc = y s0 + acc, s0 = lane 16 + k's acc, four times
        acc = [c % P for a, b, c in mad[w:w + 64]]
        s0 = mad[w][0] % P
        for k in range(4):
            acc = [(mad[w + l][1] * s0 + acc[l]) % P for l in range(64)]
            s0 = acc[16 + k]
        want_acc += acc
        want_s0 += [s0] * 64
    _cmp_modp("glq_muladd read through glq_lane_fence + readlane64 (accumulator)", take(n), want_acc, msgs)
    _cmp_modp("glq_muladd read through glq_lane_fence + readlane64 (the value read)", take(n), want_s0, msgs)
    add = cases["add"]
    _cmp_modp("glq_add", take(len(add)), [(a + b) % P for a, b, c in add], msgs)
    if at != len(out):
        msgs.append("glq: %d result words, expected %d" % (len(out), at))
    return _first(msgs)


# ------------------------------------------------------------------------------------------------ (b) glq_mds_small, glq_dense12
@functools.lru_cache(None)
def small_mds_bits():
    """The bound glp_small_mds (glcoop.h) admits: circulant and diagonal entries below 2^bits each."""
    src = open(os.path.join(CSRC, "glcoop.h")).read()
    m = re.search(r"inline bool glp_small_mds\(.*?\{(.*?)\n\}", src, flags=re.S)
    sh = set(re.findall(r">= \(1ull << (\d+)\)", m.group(1)))
    assert len(sh) == 1, sh
    return int(sh.pop())


def _dense_row(circ, diag, r):
    return [(circ[(j - r) % 12] + (diag[r] if j == r else 0)) for j in range(12)]


@functools.lru_cache(None)
def mds_cases():
    rng = random.Random(0x6D6473)
    B = 1 << small_mds_bits()
    pub = published()
    lc = lambda l: min(l & 15, 11)
    rows = {
        "bound": [_dense_row([B - 1] * 12, [B - 1] * 12, lc(l)) for l in range(64)],      # every entry at the bound: B - 1 off the diagonal, 2 (B - 1) on it
        "bound everywhere": [[2 * (B - 1)] * 12 for l in range(64)],
        "zeros": [[0] * 12 for l in range(64)],
        "ones": [[1] * 12 for l in range(64)],
        "plonky2": [_dense_row(pub["gl"]["mds_circ"], pub["gl"]["mds_diag"], lc(l)) for l in range(64)],
        "random": [[rng.randrange(2 * B - 1) for j in range(12)] for l in range(64)],
    }
    xs = {
        "all 2^64-1": [M64] * 64, "all p-1": [P - 1] * 64, "zeros": [0] * 64,
        "one-hot": [(M64 if l == 5 else 0) for l in range(64)],
        "random": [rng.getrandbits(64) for l in range(64)],
    }
    for k in ("all 2^64-1", "all p-1", "one-hot"):      # lanes 12.. are not read: they hold something else
        xs[k] = xs[k][:12] + [rng.getrandbits(64) for l in range(52)]
    nexts = {"0": [0] * 64, "p-1": [P - 1] * 64, "random": [rng.randrange(P) for l in range(64)]}
    mds = [dict(name="rows %s, x %s, next %s" % (a, b, c), m=rows[a], x=xs[b], next=nexts[c]) for a in rows for b in xs for c in nexts]
    L22, t1 = (1 << 22) - 1, ((1 << 22) - 1) * M32
    limbs = {"all 2^22-1": [L22] * 64, "zeros": [0] * 64, "one-hot": [(L22 if l == 11 else 0) for l in range(64)], "random": [rng.getrandbits(22) for l in range(64)]}
    for k in ("all 2^22-1", "one-hot"):
        limbs[k] = limbs[k][:12] + [rng.getrandbits(32) for l in range(52)]
    ws = {"all 2^64-1": [[M64] * 12 for l in range(64)], "zeros": [[0] * 12 for l in range(64)], "random": [[rng.getrandbits(64) for j in range(12)] for l in range(64)]}
    accs = {"0": ([0] * 64, [0] * 64), "24 terms and a dword": ([24 * t1 + M32] * 64, [24 * t1 + M32] * 64),
            "random": ([rng.randrange(24 * t1) for l in range(64)], [rng.randrange(24 * t1) for l in range(64)])}
    d12 = [dict(name="limbs %s, w %s, sums %s" % (a, b, c), limb=limbs[a], w=ws[b], a0=accs[c][0], a1=accs[c][1]) for a in limbs for b in ws for c in accs]
    return dict(mds=mds, d12=d12)


def mds_pack(cases):
    parts = [words([len(cases["mds"]), len(cases["d12"])])]
    for c in cases["mds"]:
        parts += [words(c["x"]), words(c["next"]), dwords([e for row in c["m"] for e in row])]
    for c in cases["d12"]:
        parts += [words(c["a0"]), words(c["a1"]), dwords(c["limb"]), dwords([w & M32 for row in c["w"] for w in row]), dwords([w >> 32 for row in c["w"] for w in row])]
    return np.concatenate(parts).tobytes()


def mds_check(cases, out):
    msgs, at = [], 0
    if len(out) != 64 * len(cases["mds"]) + 128 * len(cases["d12"]):
        return ["mds: %d result words, expected %d" % (len(out), 64 * len(cases["mds"]) + 128 * len(cases["d12"]))]
    for c in cases["mds"]:
        for l in range(64):
            lo = sum(c["m"][l][j] * (c["x"][j] & M32) for j in range(12)) + (c["next"][l] & M32)
            hi = sum(c["m"][l][j] * (c["x"][j] >> 32) for j in range(12)) + (c["next"][l] >> 32)
            assert lo < 1 << 63 and hi < 1 << 63                                        # (inside glq_reduce96's precondition, as the header says)
            want, got = (lo + (hi << 32)) % P, int(out[at + l])
            if got % P != want:
                msgs.append("glq_mds_small, %s: lane %d: got 0x%x, want 0x%x mod p" % (c["name"], l, got, want))
        at += 64
    for c in cases["d12"]:
        for l in range(64):
            a0 = c["a0"][l] + sum((c["w"][l][j] & M32) * c["limb"][j] for j in range(12))
            a1 = c["a1"][l] + sum((c["w"][l][j] >> 32) * c["limb"][j] for j in range(12))
            assert a0 ** 5 < 1 << 296 and a1 ** 5 < 1 << 296                            # 36 terms stay below 2^59.2 (glperm.h)
            g0, g1 = int(out[at + l]), int(out[at + 64 + l])
            if (g0, g1) != (a0, a1):
                msgs.append("glq_dense12, %s: lane %d: got (0x%x, 0x%x), want (0x%x, 0x%x)" % (c["name"], l, g0, g1, a0, a1))
        at += 128
    if at != len(out):
        msgs.append("mds: %d result words, expected %d" % (len(out), at))
    return _first(msgs)


# ------------------------------------------------------------------------------------------------ the constant block (include/h2w.h h2w_poseidon_consts_t) as words
KO = dict(arc=0, circ=360, diag=372, first=384, prc=396, init=418, what=539, vs=781)      # glcoop.h KO_*
GL_WORDS = 1023
BO = dict(c=GL_WORDS, s=GL_WORDS + 88 * 4, m=GL_WORDS + 480 * 4, p=GL_WORDS + 496 * 4)
KW = GL_WORDS + 512 * 4


@functools.lru_cache(None)
def published():
    """tests/golden/poseidon_published.json: gl / bn tables as integers, the known-answer vectors, and the whole block as words."""
    j = json.load(open(os.path.join(ROOT, "tests", "golden", "poseidon_published.json")))
    as_int = lambda x: int(x, 16) if isinstance(x, str) else int(x)
    g, b = j["goldilocks_w12"], j["bn254_t4"]
    flat = lambda name: [as_int(v) for row in g[name] for v in row]
    gl = dict(mds_circ=[as_int(v) for v in g["mds_circ"]], mds_diag=[as_int(v) for v in g["mds_diag"]])
    k = [as_int(v) for v in g["all_round_constants"]] + gl["mds_circ"] + gl["mds_diag"] + [as_int(v) for v in g["fast_partial_first_round_constant"]]
    k += [as_int(v) for v in g["fast_partial_round_constants"]] + flat("fast_partial_round_initial_matrix") + flat("fast_partial_round_w_hats") + flat("fast_partial_round_vs")
    assert len(k) == GL_WORDS
    bn = [as_int(v) for v in b["C"]] + [as_int(v) for v in b["S"]] + [as_int(v) for row in b["M"] for v in row] + [as_int(v) for row in b["P"] for v in row]
    assert len(bn) == 512
    vec = lambda vs: [([as_int(x) for x in v["in"]], [as_int(x) for x in v["out"]]) for v in vs]
    return dict(gl=gl, k=k + fr_words(bn), gl_vectors=vec(g["permutation_vectors"]), bn_vectors=vec(b["permutation_vectors"]))


def fr_words(xs):
    return [(x >> (64 * i)) & M64 for x in xs for i in range(4)]


def fr_ints(ws):
    ws = [int(w) for w in ws]
    return [ws[i] | ws[i + 1] << 64 | ws[i + 2] << 128 | ws[i + 3] << 192 for i in range(0, len(ws), 4)]


# ------------------------------------------------------------------------------------------------ (c) Goldilocks Poseidon, plonky2's fast form over the table words
def gl_permute(s, K):
    """hash/poseidon/permutation.rs:216-284 on the words of a constant block: what tools/ubench/ubench_glperm.hip's host walk does."""
    s = list(s)

    def full(rc):
        nonlocal s
        t = [pow((s[i] + K[KO["arc"] + 12 * rc + i]) % P, 7, P) for i in range(12)]
        s = [(t[r] * K[KO["diag"] + r] + sum(K[KO["circ"] + (j - r) % 12] * t[j] for j in range(12))) % P for r in range(12)]
    for i in range(4):
        full(i)
    s = [(s[i] + K[KO["first"] + i]) % P for i in range(12)]
    s = [s[0]] + [sum(K[KO["init"] + (r - 1) * 11 + (c - 1)] * s[r] for r in range(1, 12)) % P for c in range(1, 12)]
    m00 = ((K[KO["circ"]] + K[KO["diag"]]) & M64) % P      # (a wrapping u64 sum, as the reference forms it)
    for r in range(22):
        s0 = (pow(s[0], 7, P) + K[KO["prc"] + r]) % P
        d = (m00 * s0 + sum(K[KO["what"] + r * 11 + i - 1] * s[i] for i in range(1, 12))) % P
        s = [d] + [(s[i] + K[KO["vs"] + r * 11 + i - 1] * s0) % P for i in range(1, 12)]
    for i in range(4):
        full(4 + 22 + i)
    return s


def _is_small(K):
    B = 1 << small_mds_bits()
    return all(K[KO["circ"] + i] < B and K[KO["diag"] + i] < B for i in range(12))


@functools.lru_cache(None)
def perm_cases():
    rng = random.Random(0x7065726D)
    B = 1 << small_mds_bits()
    r64 = lambda: rng.getrandbits(64)

    def table(kind):
        if kind == "published":
            return list(published()["k"])
        K = [r64() % P for _ in range(GL_WORDS)] + [0] * (KW - GL_WORDS)
        if kind == "extreme words":
            K[:GL_WORDS] = [P - 1 if i % 3 == 0 else P - 1 - (r64() & 0xFFFF) if i % 3 == 1 else r64() % P for i in range(GL_WORDS)]
        for i in range(12):
            if kind == "tiny entries":
                c, d = r64() & 63, 8 if i == 0 else 0
            elif kind in ("entries at the small path's bound", "extreme words"):
                c, d = (B - 1 if i == 0 else B - 1 - (r64() & 3)), (r64() & (B - 1) if i == 0 else 0)
            elif kind == "diagonal at the small path's bound too":
                c, d = (B - 1 if i == 0 else B - 1 - (r64() & 3)), (B - 1 if i == 0 else B - 1 - (r64() & 3))
            elif kind == "64-bit entries":
                c, d = r64() % P, (r64() % P if i == 0 else 0)
            else:      # full-width diagonals
                c, d = r64() % P, r64() % P
            K[KO["circ"] + i], K[KO["diag"] + i] = c, d
        return K
    kinds = ["published", "tiny entries", "entries at the small path's bound", "diagonal at the small path's bound too", "64-bit entries", "extreme words",
             "full-width diagonals", "full-width diagonals (2)"]
    tabs = [table(k) for k in kinds]
    states = {"all 0": [0] * 12, "all p-1": [P - 1] * 12, "p-1-i": [P - 1 - i for i in range(12)], "0..11": list(range(12)), "random": [rng.randrange(P) for _ in range(12)]}
    cases = []
    for t, kind in enumerate(kinds):
        for small in ((1, 0) if _is_small(tabs[t]) else (0,)):
            for sn, st in states.items():
                for n in (1, 8):
                    cases.append(dict(name="%s, %s MDS path, state %s, %d permutation(s)" % (kind, "small" if small else "dense", sn, n), tab=t, small=small, n=n, list=0, st=st))
    for t, small in ((0, 1), (4, 0)):      # once on each path with the permutation listed
        cases.append(dict(name="%s, listed" % kinds[t], tab=t, small=small, n=1, list=1, st=states["random"]))
    return dict(tabs=tabs, kinds=kinds, cases=cases)


def perm_pack(c):
    parts = [words([len(c["tabs"]), len(c["cases"])])] + [words(K) for K in c["tabs"]]
    parts += [words([x["tab"], x["small"], x["n"], x["list"]] + x["st"]) for x in c["cases"]]
    return np.concatenate(parts).tobytes()


@functools.lru_cache(None)
def perm_expected():
    c = perm_cases()
    want = []
    for x in c["cases"]:
        s = x["st"]
        for _ in range(x["n"]):
            s = gl_permute(s, c["tabs"][x["tab"]])
        want.append(s)
    return want


def perm_check(c, out):
    msgs, want = [], perm_expected()
    if len(out) != 80 * len(c["cases"]):
        return ["perm: %d result words, expected %d" % (len(out), 80 * len(c["cases"]))]
    for i, x in enumerate(c["cases"]):
        o = [int(v) for v in out[80 * i:80 * i + 80]]
        for l in range(64):      # canonical, and the four rows alike (lanes 12..15 of a row compute along and are ignored)
            if (l & 15) < 12 and o[l] != want[i][l & 15]:
                msgs.append("glp_permute_lanes, %s: lane %d: got 0x%x, want 0x%x" % (x["name"], l, o[l], want[i][l & 15]))
        listed = [0xC0DE000000000000 + i] + x["st"] if x["list"] else [FILL] * 13
        if o[64:77] != listed or o[77:] != [FILL] * 3:
            msgs.append("glp_permute_lanes, %s: the listed words are %s" % (x["name"], ["0x%x" % v for v in o[64:]]))
    return _first(msgs)


# ------------------------------------------------------------------------------------------------ (d) rf::mont and the ways to build its operands
def limbs9(v):
    """v < 2^261 + ... as tight limbs: eight of 29 bits, the ninth takes the rest."""
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def limbs_value(t):
    return sum(int(x) << (29 * i) for i, x in enumerate(t))


def _loosen(t, slack, rng):
    """The same value with limbs that took up to `slack` units of 2^29 from the limb above (a sum of two has such limbs): rowfr_check.cpp loosen."""
    t = list(t)
    for i in range(8):
        can = min(t[i + 1], rng.randrange(slack + 1))
        t[i + 1] -= can
        t[i] += can << 29
    return t


MONT_KS = [(0, 0), (1, 1), (6, 6), (7, 0), (63, 0), (63, 1), (25, 5), (63, 63)]


@functools.lru_cache(None)
def mont_cases():
    rng = random.Random(0x6D6F6E74)
    cases = []
    for k0, k1 in MONT_KS:
        for slack in range(3):
            for it in range(60):
                a = [rng.randrange(R) for _ in range(4)]
                b = [rng.randrange(R) for _ in range(4)]
                if it == 0:
                    a[0] = 0
                if it == 1:
                    a[1] = b[1] = R - 1
                al = [limbs9(x + k0 * R) for x in a]
                bl = [limbs9(x + k1 * R) for x in b]
                if slack:
                    al = [_loosen(t, slack, rng) for t in al]
                    bl = [_loosen(t, slack, rng) for t in bl]
                # tighten's input: limbs up to 2^32 on lanes 0..7, a value below 2^261 (nothing leaves lane 8), 0 above
                tv = []
                for row in range(4):
                    big = M32 if (it + row) % 7 == 0 else None
                    tv += [big if big else rng.getrandbits(32) for _ in range(8)] + [rng.getrandbits(28)] + [0] * 7
                cases.append(dict(name="a + %d r, b + %d r, slack %d, iteration %d" % (k0, k1, slack, it), a=al, b=bl, tv=tv))
    return cases


def mont_pack(cases):
    parts = [words([len(cases)])]
    for c in cases:
        parts.append(dwords([x for t in c["a"] for x in t] + [x for t in c["b"] for x in t] + c["tv"]))
    return np.concatenate(parts).tobytes()


def mont_check(cases, out):
    msgs = []
    o32 = np.ascontiguousarray(out).view("<u4")
    if o32.size != 1344 * len(cases):
        return ["mont: %d result dwords, expected %d" % (o32.size, 1344 * len(cases))]
    for ci, c in enumerate(cases):
        o = [int(v) for v in o32[1344 * ci:1344 * ci + 1344]]
        for row in range(4):
            for i in range(9):
                for k in range(16):
                    l = 16 * row + k
                    if o[i * 64 + l] != c["a"][row][i]:
                        msgs.append("replicate + put_rows, %s: limb %d on lane %d: got 0x%x, want 0x%x" % (c["name"], i, l, o[i * 64 + l], c["a"][row][i]))
                    if (k >= i or (i == 8 and k == 0)) and o[(9 + i) * 64 + l] != c["a"][row][i]:      # limb i is defined on lanes i..15, limb 8 on lane 0 too
                        msgs.append("replicate_rows, %s: limb %d on lane %d: got 0x%x, want 0x%x" % (c["name"], i, l, o[(9 + i) * 64 + l], c["a"][row][i]))
            a, b = limbs_value(c["a"][row]), limbs_value(c["b"][row])
            for which, base in (("replicate + put_rows", 18 * 64), ("replicate_rows", 19 * 64)):
                t = o[base + 16 * row:base + 16 * row + 16]
                v = limbs_value(t[:9])
                why = None
                if any(t[9:]):
                    why = "lanes 9..15 are not 0"
                elif max(t[:9]) >= (1 << 29) + 8:
                    why = "a limb is not below 2^29 + 8"
                elif v % R != a * b * RINV261 % R:
                    why = "the value is not a b / 2^261 mod r"
                elif 100 * (v << 261) >= 100 * a * b + 101 * (R << 261):
                    why = "the value is not below a b / 2^261 + 1.01 r"
                if why:
                    msgs.append("mont (operand by %s), %s, row %d: %s: limbs %s" % (which, c["name"], row, why, ["0x%x" % x for x in t]))
            for k in range(16):
                l = 16 * row + k
                want = (c["tv"][l] & M29) + (c["tv"][l - 1] >> 29 if k else 0)
                if o[20 * 64 + l] != want:
                    msgs.append("tighten, %s: lane %d: got 0x%x, want 0x%x" % (c["name"], l, o[20 * 64 + l], want))
    return _first(msgs)


# ------------------------------------------------------------------------------------------------ (e) PoseidonBN254, circomlib's optimised t = 4 form
def bn_permute(st, K):
    """hash/poseidon_bn254/permutation.rs:83-203 on the words of a constant block, as tests/cpp/rowfr_check.cpp walks it: ark / 4 full (P on the last) /
    56 partial / 4 full.  Returns the output state and the 56 x 3 S-box values x^2, x^4, x^5 of the partial rounds."""
    tab = fr_ints(K[BO["c"]:KW])
    C, S, M, Pm = tab[:88], tab[88:480], [tab[480 + 4 * i:484 + 4 * i] for i in range(4)], [tab[496 + 4 * i:500 + 4 * i] for i in range(4)]
    s, sbox = [x % R for x in st], []
    ark = lambda at: [(s[i] + C[at + i]) % R for i in range(4)]
    mix = lambda m: [sum(m[j][i] * s[j] for j in range(4)) % R for i in range(4)]
    s = ark(0)
    for i in range(3):
        s = [pow(x, 5, R) for x in s]
        s = ark(4 * (i + 1))
        s = mix(M)
    s = [pow(x, 5, R) for x in s]
    s = ark(16)
    s = mix(Pm)
    for r in range(56):
        x2 = s[0] * s[0] % R
        x4 = x2 * x2 % R
        x5 = x4 * s[0] % R
        sbox += [x2, x4, x5]
        s[0] = (x5 + C[20 + r]) % R
        n0 = sum(S[7 * r + j] * s[j] for j in range(4)) % R
        s = [n0] + [(S[7 * r + 4 + k - 1] * s[0] + s[k]) % R for k in range(1, 4)]
    for i in range(3):
        s = [pow(x, 5, R) for x in s]
        s = ark(76 + 4 * i)
        s = mix(M)
    s = [pow(x, 5, R) for x in s]
    s = mix(M)
    return s, sbox


@functools.lru_cache(None)
def bn_cases():
    rng = random.Random(0x626E)
    wide = list(published()["k"][:GL_WORDS]) + fr_words([rng.randrange(R) for _ in range(512)])      # full-width random tables
    tabs = [list(published()["k"]), wide]
    states = [[0] * 4, [R - 1] * 4] + [[rng.randrange(R) for _ in range(4)] for _ in range(4)]
    cases = [dict(name="%s tables, state %d" % (("published", "full-width random")[t], i), tab=t, st=st) for t in range(2) for i, st in enumerate(states)]
    sets = lazy_sets()      # the tables the lazy walks are held to (below): the row form runs the same algebra
    for name in ADVERSARIAL:
        K, own = sets[name]
        tabs.append(K)
        more = [s for _, s in FIXED_STATES] + ([own] if own else []) + states[2:4]
        cases += [dict(name="%s tables, state %d" % (name, i), tab=len(tabs) - 1, st=st) for i, st in enumerate(more)]
    return dict(tabs=tabs, cases=cases)


def bn_pack(c):
    parts = [words([len(c["tabs"]), len(c["cases"])])] + [words(K) for K in c["tabs"]]
    parts += [words([x["tab"], 0, 0, 0] + fr_words(x["st"])) for x in c["cases"]]
    return np.concatenate(parts).tobytes()


BN_OUT = 16 + 1008 + 16             # words per case: the state, the 168 S-box values (12 dwords each), the state of the no-store form


def bn_check(c, out):
    msgs = []
    if len(out) != BN_OUT * len(c["cases"]):
        return ["bn: %d result words, expected %d" % (len(out), BN_OUT * len(c["cases"]))]
    for i, x in enumerate(c["cases"]):
        want, sbox = bn_permute(x["st"], c["tabs"][x["tab"]])
        o = out[BN_OUT * i:BN_OUT * i + BN_OUT]
        got, bare = fr_ints(o[:16]), fr_ints(o[BN_OUT - 16:])
        for e in range(4):
            if got[e] != want[e]:
                msgs.append("bn_permute_rows, %s: element %d: got 0x%x, want 0x%x" % (x["name"], e, got[e], want[e]))
            if bare[e] != want[e]:
                msgs.append("bn_permute_rows<false>, %s: element %d: got 0x%x, want 0x%x" % (x["name"], e, bare[e], want[e]))
        d = [int(v) for v in np.ascontiguousarray(o[16:16 + 1008]).view("<u4")]
        for v in range(168):      # x R in lazy limbs, 12 dwords each (nine used)
            t = d[12 * v:12 * v + 12]
            if any(t[9:]) or limbs_value(t[:9]) * RINV261 % R != sbox[v]:
                msgs.append("bn_permute_rows, %s: S-box value %d (round %d, %s): limbs %s" % (x["name"], v, v // 3, ("x^2", "x^4", "x^5")[v % 3], ["0x%x" % y for y in t]))
                break
    return _first(msgs)


# ------------------------------------------------------------------------------------------------ (e') the lazy nine-limb routines of field.h, limb for limb
# The fr9_* routines on lists of nine Python integers.  Every routine asserts what the C++ relies on and does not check: no 32-bit limb sum wraps, no
# 64-bit accumulator of fr9_mont reaches 2^64, at most one operand of a product has limbs of 2^29 or more and those stay below 2^30, t[8] fits, every
# result is below 2^261, and what fr9_pack takes is below 2^256.
N29 = limbs9(R)
NINV29 = (-pow(R, -1, 1 << 29)) % (1 << 29)
NINV261 = (-pow(R, -1, 1 << 261)) % (1 << 261)
RM = (1 << 261) % R               # the form the walks read: x RM mod r


class LazyBoundError(AssertionError):
    """A precondition of the lazy arithmetic does not hold."""


def _rely(ok, what):
    if not ok:
        raise LazyBoundError(what)


def fr9_from(x):
    _rely(0 <= x < 1 << 256, "fr9_from: four 64-bit words")
    return limbs9(x)


def fr9_pack(t):
    _rely(max(t[:8]) <= M29, "fr9_pack: a limb is not normalised")
    _rely(t[8] < 1 << 24, "fr9_pack: the value is not below 2^256")
    return limbs_value(t)


def fr9_add(a, b):
    r = [x + y for x, y in zip(a, b)]
    _rely(max(r) <= M32, "fr9_add: a 32-bit limb sum wraps")
    return r


def fr9_add_if(c, a, b):
    return fr9_add(a, b) if c else list(a)


def fr9_sel(c, a, b):
    return list(a if c else b)


def fr9_norm(a):
    r, c = [], 0
    for i in range(8):
        v = a[i] + c
        _rely(v <= M32, "fr9_norm: a 32-bit limb sum wraps")
        r.append(v & M29)
        c = v >> 29
    top = a[8] + c
    _rely(top <= M32, "fr9_norm: t[8] does not fit")
    _rely(top <= M29, "fr9_norm: the value is not below 2^261")
    return r + [top]


def fr9_mont(a, b):
    """field.h fr9_mont with its two 64-bit accumulators as written."""
    _rely(max(a) < 1 << 30 and max(b) < 1 << 30, "fr9_mont: an operand has a limb of 2^30 or more")
    _rely(max(a) <= M29 or max(b) <= M29, "fr9_mont: both operands have limbs of 2^29 or more")
    m, r, acc, top = [0] * 9, [0] * 9, 0, 0
    for k in range(9):
        e = 0
        for i in range(k + 1):
            if i & 1:
                e += a[i] * b[k - i]
            else:
                acc += a[i] * b[k - i]
        for i in range(k):
            if i & 1:
                acc += m[i] * N29[k - i]
            else:
                e += m[i] * N29[k - i]
        top = max(top, acc, e)
        acc += e
        top = max(top, acc)
        m[k] = ((acc & M32) * NINV29) & M29
        acc += m[k] * N29[0]
        top = max(top, acc)
        acc >>= 29
    for k in range(9, 17):
        e = 0
        for i in range(k - 8, 9):
            if i & 1:
                e += a[i] * b[k - i]
                acc += m[i] * N29[k - i]
            else:
                acc += a[i] * b[k - i]
                e += m[i] * N29[k - i]
        top = max(top, acc, e)
        acc += e
        top = max(top, acc)
        r[k - 9] = acc & M29
        acc >>= 29
    _rely(top <= M64, "fr9_mont: an accumulator reaches 2^64")
    _rely(acc <= M32, "fr9_mont: t[8] does not fit")
    _rely(acc <= M29, "fr9_mont: the result is not below 2^261")
    r[8] = acc
    return r


def mont_value(a, b):
    """The representative fr9_mont returns, on integers: (a b + m r) / R with m = -a b / r mod R."""
    ab = a * b
    return (ab + (ab * NINV261 & ((1 << 261) - 1)) * R) >> 261


# ------------------------------------------------------------------------------------------------ (e'') bnquad.h bn_values as scheduled, four lanes
BK_C, BK_S, BK_M, BK_P, BK_ZERO, BK_ONE, BK_T = 0, 88, 480, 496, 512, 513, 514      # bntab.h
# the sizes the comment at bn_values names, in multiples of r
QUAD_BOUNDS = {
    "mix + c": 5.3, "X2 (full rounds)": 1.17, "X2 (behind the partial rounds)": 24.2, "X4 (behind the partial rounds)": 4.5, "X5 (behind the partial rounds)": 2.7,
    "s0'": 2.1, "U_k": 1.02, "W_j": 1.37, "XA": 1.04, "T0": 1.01, "s0": 6.2, "X2 (partial rounds)": 1.23, "s_k": 62.5,
}


class QuadTable:
    """The nine-limb table of a constant block as bn_table_build and bn_table9_build build it: entry i < BK_T is entry i of C | S | M | P | 0 | 1 times R
    (canonical), entry BK_T + r is S_0 c of partial round r times R.  `tr` holds the times-R values; a greedy walk writes entries before it reads them."""

    def __init__(self, K):
        self.tr = [x * RM % R for x in fr_ints(K[BO["c"]:KW])] + [0, RM]
        assert len(self.tr) == BK_T

    def k9(self, i):
        if i < BK_T:
            return limbs9(self.tr[i])
        r = i - BK_T
        return limbs9(self.tr[BK_S + 7 * r] * self.tr[BK_C + 20 + r] * RINV261 % R)

    def block(self):
        """The constant block (published Goldilocks half) that builds this table."""
        return list(published()["k"][:GL_WORDS]) + fr_words([x * RINV261 % R for x in self.tr[:512]])


def quad_walk(st, T, greedy=None):
    """QuadSinkT::bn_values on the four lanes of a quad, limb for limb: the three slots of a partial round, the column update that rides in the next round,
    the butterfly sum.  Returns (the canonical output state, the 168 S-box words as stored, {quantity: its largest value}).
    greedy = (kind, n, rng): before an entry of the kind's part of the table is read for the first time it is replaced by the one of n seeded candidates that
    makes the product it enters largest ("column": S'_k for U_k, and P for the mix products in front of the partial rounds; "row": S_0 for XA, T0 and T0 + S_0 c in turn, S_j for W_j, M and P for the mix products)."""
    peak = {}

    def see(name, *vs):
        peak[name] = max([peak.get(name, 0)] + [limbs_value(v) for v in vs])

    def choose(idx, other):
        kind, n, rng = greedy
        ov = limbs_value(other)
        T.tr[idx] = max((rng.randrange(R) for _ in range(n)), key=lambda c: mont_value(ov, c))
    col, row = (greedy and greedy[0] == "column"), (greedy and greedy[0] == "row")
    chosen = set()
    L4 = range(4)
    lm = [0, 0, 1, 2]
    S = [fr9_mont(fr9_from(x), fr9_from(RM * RM % R)) for x in st]
    S = [fr9_norm(fr9_add(S[l], T.k9(BK_C + l))) for l in L4]
    see("mix + c", *S)
    sbox = []

    def mix(mb):
        nonlocal S
        if (row or (col and mb == BK_P)) and mb not in chosen:
            chosen.add(mb)
            for l in L4:
                for j in L4:
                    choose(mb + 4 * j + l, S[j])
        acc = [fr9_mont(S[0], T.k9(mb + l)) for l in L4]
        for j in (1, 2):
            acc = [fr9_add(fr9_mont(S[j], T.k9(mb + 4 * j + l)), acc[l]) for l in L4]
        S = [fr9_norm(fr9_add(fr9_mont(S[3], T.k9(mb + 12 + l)), acc[l])) for l in L4]
        see("mix + c", *S)
    for half in (0, 1):
        if half == 1:
            s0p = [0] * 9
            for r in range(56):
                ix, ic = BK_S + 7 * r, BK_C + 20 + r
                if col and r:
                    for k in (1, 2, 3):
                        choose(ix - 7 + 4 + k - 1, s0p)
                s0b = S[0]
                X2 = fr9_mont(S[0], S[0])
                A = [X2] + [fr9_mont(s0p, T.k9(ix - 7 + 4 + lm[l])) for l in (1, 2, 3)]
                sbox.append(fr9_pack(A[0]))
                S = [S[0]] + [fr9_add(S[l], A[l]) for l in (1, 2, 3)]                  # lanes k: a sum of two until the end of the round
                see("X2 (partial rounds)", X2)
                if r:
                    see("U_k", *A[1:])
                see("s_k", *S[1:])
                X4 = fr9_mont(X2, X2)
                if row:
                    if r % 3 == 0:
                        choose(ix, s0b)
                    else:                                                               # T0 alone, then the whole of lane 0's summand T0 + S_0 c
                        kind, n, rng = greedy
                        x4v, s0v, cv = limbs_value(X4), limbs_value(s0b), (T.tr[ic] if r % 3 == 2 else 0)
                        T.tr[ix] = max((rng.randrange(R) for _ in range(n)), key=lambda c: mont_value(x4v, mont_value(s0v, c)) + c * cv * RINV261 % R)
                    for j in (1, 2, 3):
                        choose(ix + j, S[j])
                B = [X4, fr9_mont(s0b, T.k9(ix))] + [fr9_mont(S[l], T.k9(ix + l)) for l in (2, 3)]
                sbox.append(fr9_pack(B[0]))
                see("XA", B[1])
                Cc = [fr9_mont(X4, B[1]), fr9_mont(S[1], T.k9(ix + 1))] + [fr9_mont(X4, s0b) for l in (2, 3)]
                sbox.append(fr9_pack(Cc[2]))
                see("T0", Cc[0])
                see("W_j", Cc[1], B[2], B[3])
                s0p = fr9_add(Cc[2], T.k9(ic))                                          # a sum of two: only ever multiplied by a constant
                see("s0'", s0p)
                incl = [fr9_add(Cc[0], T.k9(BK_T + r)), Cc[1], B[2], B[3]]
                incl = [fr9_add(incl[l], incl[l ^ 1]) for l in L4]                     # quad_perm [1, 0, 3, 2]
                incl = [fr9_add(incl[l], incl[l ^ 2]) for l in L4]                     # quad_perm [2, 3, 0, 1]
                assert incl[0] == incl[1] == incl[2] == incl[3]
                S = [fr9_norm(incl[0])] + [fr9_norm(S[l]) for l in (1, 2, 3)]
                see("s0", S[0])
            if col:
                for k in (1, 2, 3):
                    choose(BK_S + 7 * 55 + 4 + k - 1, s0p)
            U = [fr9_mont(s0p, T.k9(BK_S + 7 * 55 + 4 + lm[l])) for l in (1, 2, 3)]
            see("U_k", *U)
            S = [S[0]] + [fr9_norm(fr9_add(S[l], U[l - 1])) for l in (1, 2, 3)]
            see("s_k", *S[1:])
        for r in range(4):
            last = r == 3
            X2 = [fr9_mont(S[l], S[l]) for l in L4]
            X4 = [fr9_mont(X2[l], X2[l]) for l in L4]
            S = [fr9_mont(X4[l], S[l]) for l in L4]
            if half == 1 and r == 0:
                see("X2 (behind the partial rounds)", *X2)
                see("X4 (behind the partial rounds)", *X4)
                see("X5 (behind the partial rounds)", *S)
            else:
                see("X2 (full rounds)", *X2)
            if not (half == 1 and last):
                S = [fr9_add(S[l], T.k9(BK_C + (4 * (r + 1) if half == 0 else 76 + 4 * r) + l)) for l in L4]
            mix(BK_P if half == 0 and last else BK_M)
    one9 = [1] + [0] * 8
    out = []
    for l in L4:
        s = fr9_pack(fr9_mont(S[l], one9))
        if s >= R:
            s -= R
        _rely(s < R, "the output is canonical after one subtraction")
        out.append(s)
    return out, sbox, peak


def peaks_in_r(peak):
    return {k: v / R for k, v in peak.items()}


# ---- the tables that walk is held to: a table block is data, and the walk is defined for any canonical entries
GREEDY_N = 256


def _random_block(rng):
    return list(published()["k"][:GL_WORDS]) + fr_words([rng.randrange(R) for _ in range(512)])


@functools.lru_cache(None)
def lazy_sets():
    """name -> (constant block, the state the set was built for or None).  The greedy sets are built by one walk of their own state over a seeded random
    table; every other state runs on them as an ordinary case."""
    sets = {"published": (list(published()["k"]), None)}
    rng = random.Random(0x6C617A79)
    sets["full-width random"] = (_random_block(rng), None)
    for kind in ("column", "row"):
        T = QuadTable(_random_block(rng))
        if kind == "column":
            for i in range(88):
                T.tr[BK_C + i] = R - 1          # the round constants: r - 1 in the form the walk reads
        st = [rng.randrange(R) for _ in range(4)]
        quad_walk(st, T, greedy=(kind, GREEDY_N, rng))
        sets[kind] = (T.block(), st)
    one = lambda v: list(published()["k"][:GL_WORDS]) + fr_words([v] * 512)
    sets["every entry 0"] = (one(0), None)
    sets["every entry 1"] = (one(1), None)
    sets["every entry r-1"] = (one(R - 1), None)
    sets["every entry r-1 as read"] = (one((R - 1) * RINV261 % R), None)
    return sets


ADVERSARIAL = ("column", "row", "every entry 0", "every entry 1", "every entry r-1", "every entry r-1 as read")
FIXED_STATES = (("all 0", [0] * 4), ("all r-1", [R - 1] * 4), ("0, 1, r-1, 2^253", [0, 1, R - 1, 1 << 253]))


@functools.lru_cache(None)
def _lazy_walk(name, st):
    return quad_walk(list(st), QuadTable(lazy_sets()[name][0]))


def lazy_walk(name, st):
    """The model's walk of state st over the set `name` (cached: the CPU tests and the device checks share it)."""
    return _lazy_walk(name, tuple(st))


def lazy_cases():
    """Every (set, state) the quad group runs, live or not: the cases of the CPU checks of the model."""
    seen, out = set(), []
    for x in quad_cases()["launches"]:
        for st in x["st"]:
            if (x["set"], tuple(st)) not in seen:
                seen.add((x["set"], tuple(st)))
                out.append((x["set"], st))
    return out


def quad_reach():
    """({quantity: largest value in r over the ordinary cases}, the same over the cases of the adversarial sets, the column set's s_k case by case)"""
    plain, adv, col = {}, {}, []
    for name, st in lazy_cases():
        pk = peaks_in_r(lazy_walk(name, st)[2])
        into = adv if name in ADVERSARIAL else plain
        for k, v in pk.items():
            into[k] = max(into.get(k, 0.0), v)
        if name == "column":
            col.append(pk["s_k"])
    return plain, adv, col


# Floors of the adversarial sets' reach, in r.  s_k: 58 r is what a value-level model of the schedule measured for a greedy column set (58.9 r with 64
# candidates per entry); it is no derivation.  Every other figure is the value test_quad_walk_cases_reach_the_stated_bounds printed on its first run with
# GREEDY_N = 256 (the largest over all cases of the adversarial sets), cut behind its third decimal.
QUAD_FLOORS = {
    "mix + c": 4.016, "X2 (full rounds)": 1.083, "X2 (behind the partial rounds)": 22.222, "X4 (behind the partial rounds)": 3.799, "X5 (behind the partial rounds)": 2.001,
    "s0'": 2.016, "U_k": 1.009, "W_j": 1.211, "XA": 1.028, "T0": 1.003, "s0": 5.37, "X2 (partial rounds)": 1.111, "s_k": 58.0,
}


# ------------------------------------------------------------------------------------------------ (e''') QuadSinkT::bn_values on the device, sixteen quads a wavefront
@functools.lru_cache(None)
def quad_cases():
    """Launches of one wavefront: a table, sixteen states (one per quad), the quads that are live, unit_local."""
    rng = random.Random(0x71756164)
    sets = lazy_sets()
    names = list(sets)
    launches = []
    for t, name in enumerate(names):
        own = sets[name][1]
        sts = [s for _, s in FIXED_STATES] + [own or [rng.randrange(R) for _ in range(4)]]
        sts += [[rng.randrange(R) for _ in range(4)] for _ in range(12)]
        assert len({tuple(s) for s in sts}) == 16
        launches.append(dict(name="%s, all sixteen quads" % name, set=name, tab=t, live=0xFFFF, unit=0, st=sts))
        if own or name == "published":
            for q, unit in ((0, 1), (5, 0), (15, 1)):      # the set's own state, wherever its quad sits
                moved = list(sts)
                moved[3], moved[q] = moved[q], moved[3]
                launches.append(dict(name="%s, quad %d alone, unit_local %d" % (name, q, unit), set=name, tab=t, live=1 << q, unit=unit, st=moved))
    full = [x for x in launches if x["name"] == "column, all sixteen quads"][0]
    launches.append(dict(full, name="column, all sixteen quads, unit_local 1", unit=1))
    return dict(names=names, tabs=[sets[n][0] for n in names], launches=launches)


QUAD_UNITS = 2                      # unit slots per quad in the result buffer
QUAD_Q_FR = QUAD_UNITS * 4 + QUAD_UNITS * 168 + 4 + 4      # per quad: ustate [2][4], sbx [2][168], st[] after QUAD_VALUES, st[] after QUAD_VERDICT
QUAD_L_WORDS = 16 * QUAD_Q_FR * 4


def quad_pack(c):
    parts = [words([len(c["tabs"]), len(c["launches"])])] + [words(K) for K in c["tabs"]]
    parts += [words([x["tab"], x["live"], x["unit"], 0] + fr_words([v for s in x["st"] for v in s])) for x in c["launches"]]
    return np.concatenate(parts).tobytes()


def quad_check(c, out):
    msgs = []
    if len(out) != QUAD_L_WORDS * len(c["launches"]):
        return ["quad: %d result words, expected %d" % (len(out), QUAD_L_WORDS * len(c["launches"]))]
    seen = {}
    for i, x in enumerate(c["launches"]):
        for q in range(16):
            o = [int(v) for v in out[i * QUAD_L_WORDS + q * QUAD_Q_FR * 4:i * QUAD_L_WORDS + (q + 1) * QUAD_Q_FR * 4]]
            who = "bn_values, %s, quad %d" % (x["name"], q)
            if not (x["live"] >> q) & 1:
                if o != [FILL] * len(o):
                    msgs.append("%s: a quad that returned before the call wrote" % who)
                continue
            u = x["unit"]
            us, sb = o[:32], o[32:32 + 2 * 168 * 4]
            want, sbox, _ = lazy_walk(x["set"], x["st"][q])
            ref_out, ref_sbox = bn_permute(x["st"][q], c["tabs"][x["tab"]])
            assert want == ref_out
            if us[16 * (1 - u):16 * (2 - u)] != [FILL] * 16 or sb[672 * (1 - u):672 * (2 - u)] != [FILL] * 672:
                msgs.append("%s: words outside the unit's own region were written" % who)
            got, gsb = fr_ints(us[16 * u:16 * u + 16]), fr_ints(sb[672 * u:672 * u + 672])
            st_values, st_verdict = fr_ints(o[-32:-16]), fr_ints(o[-16:])
            if got != want:
                msgs.append("%s: the stored state is %s, want %s" % (who, ["0x%x" % v for v in got], ["0x%x" % v for v in want]))
            if st_values != want:
                msgs.append("%s: st[] after QUAD_VALUES is %s, want %s" % (who, ["0x%x" % v for v in st_values], ["0x%x" % v for v in want]))
            if st_verdict != st_values or st_verdict != want:
                msgs.append("%s: st[] after QUAD_VERDICT is %s, after QUAD_VALUES %s" % (who, ["0x%x" % v for v in st_verdict], ["0x%x" % v for v in st_values]))
            for v in range(168):
                if gsb[v] >= 2 * R or gsb[v] * RINV261 % R != ref_sbox[v] or gsb[v] != sbox[v]:
                    msgs.append("%s: S-box word %d (round %d, %s) is 0x%x, the model's 0x%x" % (who, v, v // 3, ("x^2", "x^4", "x^5")[v % 3], gsb[v], sbox[v]))
                    break
            key = (x["set"], tuple(x["st"][q]))
            if seen.setdefault(key, (got, gsb)) != (got, gsb):
                msgs.append("%s: the same case gave other words in another quad" % who)
    return _first(msgs)


# ------------------------------------------------------------------------------------------------ (f) the plain C++ routes, compiled for the device
PLAIN_OPS = ("reduce128", "divmod", "fr_mont_mul", "fr9", "mf2", "mf3", "mf4", "mf8", "canon9")
PLAIN_HDR = 16
CANON9_TOP = 63                     # canon9 runs on x + k r up to this k: past the largest value either lazy walk holds (bnquad.h: 62.5 r)


def largest_sbox_words(n):
    """The n largest S-box words the model of the quad walk stores, over every case of the quad group."""
    ws = set()
    for x in quad_cases()["launches"]:
        for q in range(16):
            if (x["live"] >> q) & 1:
                ws.update(lazy_walk(x["set"], x["st"][q])[1])
    return sorted(ws)[-n:]


@functools.lru_cache(None)
def plain_cases():
    rng = random.Random(0x706C)
    r64 = lambda: rng.getrandbits(64)
    N = 1 << 14
    canon = [x for x in E64 if x < P]
    frs = [0, 1, R - 1, R - 2, 2, (1 << 253), (1 << 128) - 1, 1 << 64, M64]
    c = {}
    c["reduce128"] = [(lo, hi) for lo in E64 for hi in E64] + [(r64(), r64()) for _ in range(N)]
    c["divmod"] = [(a, b, d) for a in canon for b in canon for d in (0, 1, P - 1)] + [(rng.randrange(P), rng.randrange(P), rng.randrange(P)) for _ in range(N)]      # a b + c of canonical values
    c["fr_mont_mul"] = [(a, b) for a in frs for b in frs] + [(rng.randrange(R), rng.randrange(R)) for _ in range(N)]
    # by one, of the lazy words of [r, 2 r) the quad walk stores: what k_sbox_canon does
    c["fr_mont_mul"] += [(x, 1) for x in [R, R + 1, 2 * R - 1, 2 * R - 2] + largest_sbox_words(48) + [rng.randrange(R, 2 * R) for _ in range(1 << 10)]]
    # canon9: twelve dwords as the row walk leaves them - any representative below 2^261, limbs up to eight units above 2^29
    c9 = []
    for i in range(N):
        k = (0, 1, 2, CANON9_TOP)[i & 3] if i < 256 else rng.randrange(CANON9_TOP + 1)
        x = (0, 1, R - 1, R - 2)[(i >> 2) & 3] if i < 64 else rng.randrange(R)
        t = limbs9(x + k * R)
        if i % 4 == 3:      # as a product comes out of rf::mont: limbs of 2^29 + 0 .. 7
            t = [(1 << 29) + rng.randrange(8) if rng.randrange(3) else rng.getrandbits(29) for _ in range(8)] + [rng.getrandbits(28)]
        else:
            t = _loosen(t, i % 4, rng)
        c9.append((t + [0, 0, 0],))
    c["canon9"] = c9
    fr9 = [(limbs9(a), limbs9(b)) for a in frs for b in frs]
    for i in range(N):      # lazy operands: one normalised, the other a sum of two (field.h)
        a, b = limbs9(rng.randrange(R) + rng.randrange(6) * R), limbs9(rng.randrange(R) + rng.randrange(2) * R)
        if i & 1:
            a = [x + y for x, y in zip(a, limbs9(rng.randrange(R)))]
        fr9.append((a, b))
    c["fr9"] = fr9
    for n in (2, 3, 4, 8):
        edge = [(1 << 32 * n) - 1, 0, 1, R - 1, (1 << 32 * n) - 2, 1 << (32 * n - 1)] + [x for x in E64]
        vals = [x & ((1 << 32 * n) - 1) for x in edge] + [rng.getrandbits(32 * n) for _ in range(N)]
        c["mf%d" % n] = [(v,) for v in vals]
    for k in PLAIN_OPS:
        pad = {"fr9": ([0] * 9, [0] * 9), "reduce128": (0, 0), "divmod": (0, 0, 0), "fr_mont_mul": (0, 0), "canon9": ([0] * 12,)}.get(k, (0,))
        c[k] = _pad64(c[k], pad)
    return c


def plain_pack(c):
    parts = [words([len(c[k]) for k in PLAIN_OPS] + [0] * (PLAIN_HDR - len(PLAIN_OPS)))]
    parts.append(words([w for x in c["reduce128"] for w in x]))
    parts.append(words([w for x in c["divmod"] for w in x]))
    parts.append(words(fr_words([v for x in c["fr_mont_mul"] for v in x])))
    parts.append(dwords([w for a, b in c["fr9"] for w in a + b]))
    for n, pad in ((2, 2), (3, 4), (4, 4), (8, 8)):
        parts.append(dwords([(v >> (32 * i)) & M32 for (v,) in c["mf%d" % n] for i in range(pad)]))
    parts.append(dwords([w for (t,) in c["canon9"] for w in t]))
    return np.concatenate(parts).tobytes()


def plain_check(c, out):
    msgs, at = [], 0
    need = sum(len(c[k]) * w for k, w in zip(PLAIN_OPS, (1, 2, 4, 5, 4, 4, 4, 4, 4)))
    if len(out) != need:
        return ["plain: %d result words, expected %d" % (len(out), need)]

    def take(n):
        nonlocal at
        at += n
        return [int(v) for v in out[at - n:at]]
    for i, ((lo, hi), g) in enumerate(zip(c["reduce128"], take(len(c["reduce128"])))):
        if g != (lo + (hi << 64)) % P:
            msgs.append("gl_reduce128: case %d: got 0x%x, want 0x%x" % (i, g, (lo + (hi << 64)) % P))
    g = take(2 * len(c["divmod"]))
    for i, (a, b, d) in enumerate(c["divmod"]):
        if (g[2 * i], g[2 * i + 1]) != divmod(a * b + d, P):
            msgs.append("gl_divmod128: case %d: got (0x%x, 0x%x), want (0x%x, 0x%x)" % ((i, g[2 * i], g[2 * i + 1]) + divmod(a * b + d, P)))
    g = fr_ints(take(4 * len(c["fr_mont_mul"])))
    for i, (a, b) in enumerate(c["fr_mont_mul"]):
        if g[i] != a * b * RINV261 % R:
            msgs.append("fr_mont_mul: case %d: got 0x%x, want 0x%x" % (i, g[i], a * b * RINV261 % R))
    g = take(5 * len(c["fr9"]))
    ninv = (-pow(R, -1, 1 << 261)) % (1 << 261)
    for i, (a, b) in enumerate(c["fr9"]):
        t = [x for w in g[5 * i:5 * i + 5] for x in (w & M32, w >> 32)]
        ab = limbs_value(a) * limbs_value(b)
        want = limbs9((ab + (ab * ninv % (1 << 261)) * R) >> 261)      # (a b + m r) / R, m = -a b / r mod R: the value the algorithm forms, in normalised limbs
        if t[:9] != want or t[9] != 0:
            msgs.append("fr9_norm(fr9_mont): case %d: got %s, want %s" % (i, ["0x%x" % x for x in t], ["0x%x" % x for x in want]))
    for n in (2, 3, 4, 8):
        cs = c["mf%d" % n]
        g = fr_ints(take(4 * len(cs)))
        for i, (v,) in enumerate(cs):
            if g[i] != (v << 256) % R:
                msgs.append("mf_convert<%d>: case %d (0x%x): got 0x%x, want 0x%x" % (n, i, v, g[i], (v << 256) % R))
    g = fr_ints(take(4 * len(c["canon9"])))
    for i, (t,) in enumerate(c["canon9"]):
        want = limbs_value(t[:9]) * RINV261 % R
        if g[i] != want:
            msgs.append("canon9: case %d (limbs %s): got 0x%x, want 0x%x" % (i, ["0x%x" % x for x in t[:9]], g[i], want))
    if at != len(out):
        msgs.append("plain: %d result words, expected %d" % (len(out), at))
    return _first(msgs)


GROUPS = {
    "glq": (glq_cases, glq_pack, glq_check), "mds": (mds_cases, mds_pack, mds_check), "perm": (perm_cases, perm_pack, perm_check),
    "mont": (mont_cases, mont_pack, mont_check), "bn": (bn_cases, bn_pack, bn_check), "quad": (quad_cases, quad_pack, quad_check), "plain": (plain_cases, plain_pack, plain_check),
}
