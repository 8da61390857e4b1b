"""Hand-driven operator programs for the traced-plan tests (a helper, not a test).

A program is a function prog(b) written once against the small backend interface below and run on three backends:
  TraceBackend   a fresh api.Context in trace mode: every *_in tags the proof word (h2w_trace_input) in front of the load; values from "proof A"
  OracleBackend  oracle.Ctx and the orc_* op drivers of oracle/oracle.h, on the raw words of the proof passed in
  IntBackend     Python integers only, no cells: the value of every handle ((a * b + c) % P, % R, bit lists ...) and the status word
lower() turns the traced run into a plan; check_on_device() replays it on a batch and holds every proof's stream to the oracle's bytes, its
status word and the cells at the returned handles to the Int backend's values (and the oracle's values to the Int backend's: a bug the oracle
and the device share still shows).  The programs themselves (PROGRAMS) are shared by tests/test_replay_programs_lowering.py (no GPU) and
tests/test_gpu_replay_programs.py."""
import contextlib
import ctypes as C
import os
import random
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 2**64 - 2**32 + 1
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
M64 = 2**64 - 1

GL_EDGES = [0, 1, 2, 2**32 - 1, 2**32, 2**32 + 1, 2**63, P - 2, P - 1]
GL_NONCANON = [P, P + 1, 2**64 - 1]                       # status 4; the cells still follow the raw word
FR_EDGES = [0, 1, 2**64 - 1, 2**64, 2**128 - 1, 2**128, 2**253, R - 1]
FR_OUT = [R, 2**256 - 1]                                  # status 4; include/h2w.h leaves those cells unspecified
# 128-bit values around the points where GoldilocksChip::reduce changes shape (tests/test_gpu_eager.py test_reduce_at_the_edges_of_its_range),
# those a 64 x 64 + 64 gate can produce: at most (2^64 - 1)^2 + 2^64 - 1 = 2^128 - 2^64
REDUCE_V = [v for v in [0, 1, P - 1, P, P + 1, 2**64 - 1, 2**64, P * (P - 1) + (P - 1), P * P - 1, P * P, P * P + 1, (P - 2) * 2**64, 2**127, 2**128 - 2**64]]


def gate_operands(v):
    """(A, B, C) below 2^64 with A * B + C == v, canonical Goldilocks words where v allows it"""
    best = None
    for b in (P - 1, P, M64):
        a = min(v // b, M64); c = v - a * b
        if c <= M64 and (best is None or sum(x >= P for x in (a, b, c)) < sum(x >= P for x in best)):
            best = (a, b, c)
    assert best is not None, hex(v)
    return best


def tape_enums():
    """The DOP_* and RK_* numbers, parsed out of csrc/tapefmt.h."""
    src = open(os.path.join(ROOT, "halo2-plonky2-verifier_amd", "csrc", "tapefmt.h")).read()
    out = {}
    for first in ("RK_LOCAL", "DOP_END"):
        m = re.search(r"enum\s*\{\s*(" + first + r"\b.*?)\};", src, flags=re.S)
        body = re.sub(r"//[^\n]*", "", m.group(1))
        nxt = 0
        for item in body.split(","):
            item = item.strip()
            if not item:
                continue
            name, _, val = item.partition("=")
            if val.strip():
                nxt = int(val.strip(), 0)
            out[name.strip()] = nxt; nxt += 1
    return out


def flatten(x):
    if isinstance(x, (list, tuple)):
        return [z for y in x for z in flatten(y)]
    return [x]


def fr_words(v):
    return [(v >> (64 * j)) & M64 for j in range(4)]


class _Base:
    @contextlib.contextmanager
    def scope(self, name):
        self.push(name)
        try:
            yield
        finally:
            self.pop()

    def push(self, name): pass
    def pop(self): pass

    def hash_value(self, word):
        return sum(self.w[word + j] << (64 * j) for j in range(4))


class TraceBackend(_Base):
    def __init__(self, h2w, api, words, lookup_bits):
        self.api, self.lib, self.w = api, h2w.lib(), words
        self.ctx = api.Context(lookup_bits, True, 0); self.ctx.trace_begin()
        self.nat = api.NativeChip(self.ctx); self.gl = api.GoldilocksChip(self.nat)

    def _tag(self, word, n):
        assert self.lib.h2w_trace_input(self.ctx.p, word, n) == 0

    def push(self, name): self.ctx.push_context(name)
    def pop(self): self.ctx.pop_context()
    def gl_in(self, word): self._tag(word, 1); return self.gl.load_witness(self.w[word])
    def nat_in(self, word): self._tag(word, 1); return self.nat.load_witness(self.w[word])
    def hash_in(self, word): self._tag(word, 4); return self.nat.load_witness(self.hash_value(word))
    def const_in(self, word): self._tag(word, 1); return self.gl.load_constant(self.w[word])
    def const(self, v): return self.nat.load_constant(v)
    def gl_const(self, v): return self.gl.load_constant(v)
    def add(self, a, b): return self.nat.add(a, b)
    def mul(self, a, b): return self.nat.mul(a, b)
    def mul_add(self, a, b, c): return self.nat.mul_add(a, b, c)
    def select(self, a, b, s): return self.nat.select(a, b, s)
    def select_from_idx(self, arr, idx): return self.nat.select_from_idx(arr, idx)
    def idx_to_indicator(self, idx, n): return self.nat.idx_to_indicator(idx, n)
    def select_array_by_indicator(self, arr2d, ind): return self.nat.select_array_by_indicator(arr2d, ind)
    def num_to_bits(self, a, n): return self.nat.num_to_bits(a, n)
    def bits_to_num(self, bits): return self.nat.bits_to_num(bits)
    def decompose_le(self, a, limb_bits, n): return self.nat.decompose_le(a, limb_bits, n)
    def limbs_to_num(self, limbs, limb_bits): return self.nat.limbs_to_num(limbs, limb_bits)
    def check_less_than_safe(self, a, bound): self.nat.check_less_than_safe(a, bound)
    def range_check(self, a, bits): self.nat.range_check(a, bits)
    def gl_add(self, a, b): return self.gl.add(a, b)
    def gl_sub(self, a, b): return self.gl.sub(a, b)
    def gl_mul(self, a, b): return self.gl.mul(a, b)
    def gl_mul_add(self, a, b, c): return self.gl.mul_add(a, b, c)
    def gl_mul_sub(self, a, b, c): return self.gl.mul_sub(a, b, c)
    def gl_neg(self, a): return self.gl.neg(a)
    def gl_square(self, a): return self.gl.square(a)
    def gl_exp_power_of_2(self, a, k): return self.gl.exp_power_of_2(a, k)
    def gl_reduce(self, a): return self.gl.reduce(a)
    def gl_div(self, a, b): return self.gl.div(a, b)
    def gl_inv(self, a): return self.gl.inv(a)

    def _ext(self, op, a, b):
        out = (self.api.Assigned * 2)()
        rc = self.lib.h2w_chip_ext_op(self.ctx.p, op, self.api._arr(a), self.api._arr(b) if b is not None else None, None, out)
        if rc != 0:
            raise self.api.H2WError("h2w_chip_ext_op: " + self.api.last_error())
        return list(out)

    def ext_mul(self, a, b): return self._ext(2, a, b)
    def ext_inv(self, a): return self._ext(4, a, None)
    def ext_div(self, a, b): return self._ext(5, a, b)


class OracleBackend(_Base):
    def __init__(self, oracle, words, lookup_bits):
        self.O, self.L, self.w = oracle, oracle.lib(), words
        self.ctx = oracle.Ctx(lookup_bits); self.p = self.ctx.p

    def _arr(self, xs): return (self.O.AV * max(len(xs), 1))(*xs)
    def _fr(self, v): return self.O.Fr.from_int(v)
    def gl_in(self, word): return self.L.orc_gl_load_witness(self.p, self.w[word])
    def nat_in(self, word): return self.L.orc_load_witness(self.p, self._fr(self.w[word]))
    def hash_in(self, word): return self.L.orc_load_witness(self.p, self._fr(self.hash_value(word)))
    def const_in(self, word): return self.L.orc_gl_load_constant(self.p, self.w[word])
    def const(self, v): return self.L.orc_load_constant(self.p, self._fr(v))
    def gl_const(self, v): return self.L.orc_gl_load_constant(self.p, v)
    def add(self, a, b): return self.L.orc_add(self.p, a, b)
    def mul(self, a, b): return self.L.orc_mul(self.p, a, b)
    def mul_add(self, a, b, c): return self.L.orc_mul_add(self.p, a, b, c)
    def select(self, a, b, s): return self.L.orc_select(self.p, a, b, s)
    def select_from_idx(self, arr, idx): return self.L.orc_select_from_idx(self.p, self._arr(arr), len(arr), idx)

    def idx_to_indicator(self, idx, n):
        out = (self.O.AV * n)(); self.L.orc_idx_to_indicator(self.p, idx, n, out); return list(out)

    def select_array_by_indicator(self, arr2d, ind):
        ln, w = len(arr2d), len(arr2d[0]); out = (self.O.AV * w)()
        self.L.orc_select_array_by_indicator(self.p, self._arr([x for row in arr2d for x in row]), ln, w, self._arr(ind), out); return list(out)

    def num_to_bits(self, a, n):
        out = (self.O.AV * n)(); self.L.orc_num_to_bits(self.p, a, n, out); return list(out)

    def bits_to_num(self, bits): return self.L.orc_bits_to_num(self.p, self._arr(bits), len(bits))

    def decompose_le(self, a, limb_bits, n):
        out = (self.O.AV * n)(); self.L.orc_decompose_le(self.p, a, limb_bits, n, out); return list(out)

    def limbs_to_num(self, limbs, limb_bits): return self.L.orc_limbs_to_num(self.p, self._arr(limbs), len(limbs), limb_bits)
    def check_less_than_safe(self, a, bound): self.L.orc_check_less_than_safe(self.p, a, bound)
    def range_check(self, a, bits): self.L.orc_range_check(self.p, a, bits)
    def gl_add(self, a, b): return self.L.orc_gl_add(self.p, a, b)
    def gl_sub(self, a, b): return self.L.orc_gl_sub(self.p, a, b)
    def gl_mul(self, a, b): return self.L.orc_gl_mul(self.p, a, b)
    def gl_mul_add(self, a, b, c): return self.L.orc_gl_mul_add(self.p, a, b, c)
    def gl_mul_sub(self, a, b, c): return self.L.orc_gl_mul_sub(self.p, a, b, c)
    def gl_neg(self, a): k = self.L.orc_gl_load_constant(self.p, P - 1); return self.L.orc_gl_mul(self.p, a, k)      # load_neg_one, mul (base.rs:234-238)
    def gl_square(self, a): return self.L.orc_gl_mul(self.p, a, a)
    def gl_exp_power_of_2(self, a, k): return self.L.orc_gl_exp_power_of_2(self.p, a, k)
    def gl_reduce(self, a): return self.L.orc_gl_reduce(self.p, a)
    def gl_div(self, a, b): return self.L.orc_gl_div(self.p, a, b)
    def gl_inv(self, a): return self.L.orc_gl_inv(self.p, a)

    def ext_mul(self, a, b):
        out = (self.O.AV * 2)(); self.L.orc_ext_mul(self.p, self._arr(a), self._arr(b), out); return list(out)

    def ext_inv(self, a):
        out = (self.O.AV * 2)(); self.L.orc_ext_inv(self.p, self._arr(a), out); return list(out)

    def ext_div(self, a, b):
        out = (self.O.AV * 2)(); self.L.orc_ext_div(self.p, self._arr(a), self._arr(b), out); return list(out)


def _ext_mul(a, b):      # F_p[X] / (X^2 - 7)
    return [(a[0] * b[0] + 7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P]


class IntBackend(_Base):
    """Values only.  chip: the status of the first op of the run the reference would panic in (1: a zero divisor, 2: a zero extension element);
    flagged: a proof word outside its field (one word >= p, four words >= r); unspecified: a four-word one, whose cells h2w.h leaves open."""

    def __init__(self, words):
        self.w, self.chip, self.flagged, self.unspecified = words, 0, False, False

    def status(self):
        return self.chip or (4 if self.flagged else 0)

    def _word(self, word):
        if self.w[word] >= P:
            self.flagged = True
        return self.w[word]

    def gl_in(self, word): return self._word(word)
    def nat_in(self, word): return self._word(word)
    def const_in(self, word): return self._word(word)

    def hash_in(self, word):
        v = self.hash_value(word)
        if v >= R:
            self.flagged = self.unspecified = True
        return v

    def const(self, v): return v
    def gl_const(self, v): return v
    def add(self, a, b): return (a + b) % R
    def mul(self, a, b): return a * b % R
    def mul_add(self, a, b, c): return (a * b + c) % R
    def select(self, a, b, s): return a if s else b
    def select_from_idx(self, arr, idx): return arr[idx] if idx < len(arr) else 0
    def idx_to_indicator(self, idx, n): return [1 if i == idx else 0 for i in range(n)]
    def select_array_by_indicator(self, arr2d, ind): return [sum(row[j] * s for row, s in zip(arr2d, ind)) % R for j in range(len(arr2d[0]))]
    def num_to_bits(self, a, n): return [(a >> i) & 1 for i in range(n)]
    def bits_to_num(self, bits): return sum(x << i for i, x in enumerate(bits)) % R
    def decompose_le(self, a, limb_bits, n): return [(a >> (limb_bits * i)) & ((1 << limb_bits) - 1) for i in range(n)]
    def limbs_to_num(self, limbs, limb_bits): return sum(x << (limb_bits * i) for i, x in enumerate(limbs)) % R
    def check_less_than_safe(self, a, bound): pass
    def range_check(self, a, bits): pass
    def gl_add(self, a, b): return (a + b) % P
    def gl_sub(self, a, b): return (a - b) % P
    def gl_mul(self, a, b): return a * b % P
    def gl_mul_add(self, a, b, c): return (a * b + c) % P
    def gl_mul_sub(self, a, b, c): return (a * b - c) % P
    def gl_neg(self, a): return -a % P
    def gl_square(self, a): return a * a % P
    def gl_exp_power_of_2(self, a, k): return pow(a, 2**k, P)
    def gl_reduce(self, a): return a % P

    def gl_div(self, a, b):
        if b % P == 0:
            self.chip = self.chip or 1; b = 1      # the cells of the op on 1
        return a * pow(b, P - 2, P) % P

    def gl_inv(self, a): return self.gl_div(1, a)
    def ext_mul(self, a, b): return _ext_mul(a, b)

    def ext_inv(self, a):
        if a[0] % P == 0 and a[1] % P == 0:
            self.chip = self.chip or 2; a = [1, 0]
        d = pow((a[0] * a[0] - 7 * a[1] * a[1]) % P, P - 2, P)
        return [a[0] * d % P, -a[1] * d % P]

    def ext_div(self, a, b): return _ext_mul(a, self.ext_inv(b))


# ---------------------------------------------------------------- the runner
class Lowered:
    def __init__(self, plan, offsets, num_cells):
        self.plan, self.offsets, self.num_cells = plan, offsets, num_cells


def lower(h2w, api, prog, proof_a, lookup_bits=21, parallel_scopes=()):
    """prog traced on proof A and lowered; raises H2WError where h2w_plan_from_trace refuses."""
    tb = TraceBackend(h2w, api, proof_a, lookup_bits)
    try:
        hs = flatten(prog(tb))
        assert all(h.has_cell for h in hs)
        plan = api.Plan.from_trace(tb.ctx, len(proof_a), parallel_scopes=tuple(parallel_scopes))
        assert plan.num_cells == tb.ctx.num_cells() and plan.proof_words == len(proof_a)
        return Lowered(plan, [int(h.offset) for h in hs], tb.ctx.num_cells())
    finally:
        tb.ctx.close()


def oracle_run(oracle, prog, proof, lookup_bits=21):
    """(stream bytes, cells of the returned handles, their values) of prog on the oracle"""
    ob = OracleBackend(oracle, proof, lookup_bits)
    hs = flatten(prog(ob))
    out = ob.ctx.advice_bytes(), [int(h.cell) for h in hs], [h.v.to_int() for h in hs]
    ob.ctx.close()
    return out


def int_run(prog, proof):
    ib = IntBackend(proof)
    return flatten(prog(ib)), ib


def check_on_device(h2w, api, oracle, prog, proof_a, proofs, lookup_bits=21, parallel_scopes=()):
    """Traces prog on proof A, replays the plan on `proofs` in one batch, and holds every proof to the oracle and to the Int backend.  -> the status words"""
    import numpy as np
    import torch
    lw = lower(h2w, api, prog, proof_a, lookup_bits, parallel_scopes)
    plan, n, W = lw.plan, len(proofs), len(proof_a)
    assert all(len(p) == W for p in proofs)
    host = np.array(proofs, dtype=np.uint64).reshape(n * W)
    d_proofs = torch.from_numpy(host.view(np.int64)).cuda()
    advice = torch.zeros(n * plan.num_cells * 32, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(plan.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    plan.run(d_proofs.data_ptr(), n, advice.data_ptr(), ws.data_ptr(), st)
    torch.cuda.synchronize()
    status = plan.status(ws.data_ptr(), n, st)
    got = advice.cpu().numpy().view(np.uint64).reshape(n, plan.num_cells, 4)
    plan.close()
    for i, p in enumerate(proofs):
        want_vals, ib = int_run(prog, p)
        assert status[i] == ib.status(), f"proof {i}: status {status[i]}, expected {ib.status()}"
        if ib.unspecified:
            continue
        stream, cells, vals = oracle_run(oracle, prog, p, lookup_bits)
        assert cells == lw.offsets and len(stream) == plan.num_cells * 32
        assert vals == want_vals, f"proof {i}: the oracle's values differ from the integer model at handles {[k for k in range(len(vals)) if vals[k] != want_vals[k]][:8]}"
        want = np.frombuffer(stream, dtype=np.uint64).reshape(-1, 4)
        if not np.array_equal(got[i], want):
            bad = np.nonzero((got[i] != want).any(axis=1))[0]
            raise AssertionError(f"proof {i}: {len(bad)} cells differ, first at {bad[:8]}: got {got[i][bad[0]]} want {want[bad[0]]}")
        for k, (c, v) in enumerate(zip(lw.offsets, want_vals)):
            assert [int(x) for x in got[i][c]] == fr_words(v), f"proof {i}: handle {k} (cell {c}) is not the integer model's value {v:#x}"
    return status


# ---------------------------------------------------------------- proofs: lists of u64 words
def pick(pool, i, j, off=0):
    """Word j of proof i out of a pool of edges: neighbouring proofs (the lanes of a wavefront) get neighbouring - different - entries, and the
    combination with the other words shifts from one stretch of len(pool) proofs to the next."""
    return pool[(i + (i // len(pool)) * (j + 1) + 5 * j + off) % len(pool)]


def safe_proof(nwords, seed=1):
    """Proof A: canonical, non-zero, small enough for every op of every program (words below 2^62)."""
    rnd = random.Random(seed)
    return [rnd.randrange(3, 2**62) for _ in range(nwords)]


class Program:
    """name; fn(b); words of a proof; lookup_bits; parallel_scopes; make(i) -> proof i of a batch; sizes: the batch sizes of the device test;
    expect(counts, E): what the op counts of the lowered plan must show (E: tape_enums())"""

    def __init__(self, name, fn, nwords, make, lookup_bits=21, scopes=(), sizes=(1, 130), expect=None):
        self.name, self.fn, self.nwords, self.make, self.lookup_bits, self.scopes, self.sizes, self.expect = name, fn, nwords, make, lookup_bits, tuple(scopes), sizes, expect

    def proof_a(self):
        return safe_proof(self.nwords)

    def batch(self, n):
        return [self.make(i) for i in range(n)]


def _put_fr(p, word, v):
    p[word:word + 4] = fr_words(v)


# ---- 1. Goldilocks ops.  words: 0 a, 1 b, 2 c (any 64-bit word), 3 x, 4 y (mul_sub), 5 6 7 the gate in front of reduce, 8 divisor, 9 10 / 11 12 extension elements
GL_ANY = GL_EDGES + GL_NONCANON


def prog_gl_ops(b):
    a, bb, c, x, y = b.gl_in(0), b.gl_in(1), b.gl_in(2), b.gl_in(3), b.gl_in(4)
    m = b.gl_mul(a, bb); s = b.gl_add(m, c); d = b.gl_sub(s, a); ma = b.gl_mul_add(d, bb, m)
    ms = b.gl_mul_sub(x, y, y); ng = b.gl_neg(a); sq = b.gl_square(c); e8 = b.gl_exp_power_of_2(ma, 3)
    g = b.mul_add(b.nat_in(5), b.nat_in(6), b.nat_in(7)); rd = b.gl_reduce(g)
    dv = b.gl_in(8); q = b.gl_div(m, dv); iv = b.gl_inv(dv)
    e, f = [b.gl_in(9), b.gl_in(10)], [b.gl_in(11), b.gl_in(12)]
    em = b.ext_mul(e, f); ei = b.ext_inv(f); ed = b.ext_div(e, f)
    kc = b.const_in(1); kk = b.gl_mul_add(kc, m, kc)      # a proof word loaded as a constant (what PoseidonChip::load_witness does, hash.rs:86-96)
    return [a, bb, c, m, s, d, ma, ms, ng, sq, e8, g, rd, q, iv, em, ei, ed, kc, kk]


def make_gl_ops(i):
    p = [pick(GL_EDGES if (i % 4) else GL_ANY, i, j) for j in range(3)]
    x, y = pick(GL_ANY, i, 3), pick(GL_EDGES, i, 4)
    if x * y + y * (P - 1) >= 2**128:      # beyond that GoldilocksChip::reduce is out of its range (base.rs:345); the eager call refuses
        y = 2**63
    p += [x, y] + list(gate_operands(REDUCE_V[i % len(REDUCE_V)]))
    p += [pick(GL_EDGES[1:], i, 8)] + [pick(GL_EDGES, i, j) for j in (9, 10, 11)] + [pick(GL_EDGES[1:], i, 12)]
    if i % 16 == 5:
        p[8] = 0                           # a zero divisor: status 1 ...
        if i % 32 == 5:
            p[2] = P + 1                   # ... which wins over a non-canonical word
    if i % 16 == 11:
        p[11] = p[12] = 0                  # a zero extension element: status 2
    return p


# ---- 2. native ops.  words: 0 n0, 1 n1, 2.. h0, 6.. h1, 10.. h2, 14 selector, 15..18 limbs, 19 a canonical word
N_POOL = GL_EDGES + [2**64 - 1]


def prog_native(b):
    n0, n1, h0, h1, h2, s = b.nat_in(0), b.nat_in(1), b.hash_in(2), b.hash_in(6), b.hash_in(10), b.nat_in(14)
    g = b.mul_add(n0, n1, n0); out = [n0, n1, h0, h1, h2, g, b.add(n0, n1), b.mul(n0, n1)]                  # 64 . 64: the gate record
    out += [b.add(g, n0), b.mul(g, n1), b.mul_add(g, g, n0), b.add(g, g)]                                     # a gate output (128 bits) as an operand
    out += [b.add(h0, h1), b.mul(h0, h1), b.mul_add(h0, h1, h2)]                                              # wide
    out += [b.add(h0, n0), b.mul(n1, h1), b.mul_add(h0, n0, n1), b.mul_add(n0, n1, h2)]                       # wide . 64
    out += [b.add(g, h0), b.mul(h1, g), b.mul_add(h2, g, g)]                                                  # wide . 128
    zero, one = b.const(0), b.const(1)
    for sel in (s, zero, one):
        out += [b.select(n0, n1, sel), b.select(h0, h1, sel), b.select(h2, n0, sel), b.select(g, n1, sel)]
    limbs = [b.nat_in(15 + k) for k in range(4)]
    out += [b.limbs_to_num(limbs[:k], 64) for k in (1, 2, 3, 4)]
    for h in (h0, h1, h2):
        out += b.decompose_le(h, 56, 5)
    k = b.nat_in(19); b.check_less_than_safe(k, P); b.check_less_than_safe(limbs[0], P)
    return out


def make_native(i):
    p = [0] * 20
    p[0], p[1] = pick(N_POOL, i, 0), pick(N_POOL, i, 1)
    for k, w in enumerate((2, 6, 10)):
        _put_fr(p, w, pick(FR_EDGES, i, 2 + k))
    if i % 32 == 17:
        _put_fr(p, 6, FR_OUT[0])
    if i % 32 == 29:
        _put_fr(p, 10, FR_OUT[1])
    p[14] = (i // 3) & 1
    p[15] = pick(GL_EDGES, i, 15)
    for k in (16, 17, 18):
        p[k] = pick(N_POOL, i, k)
    p[19] = pick(GL_EDGES, i, 19)
    return p


# ---- 3. lists of n entries.  words: 0 idx, 1 the number to decompose, 2..7 range-checked words, 8.. n one-word entries, then n four-word entries
def rc_bits(L):
    return [1, L - 1, L, L + 1, 2 * L, 64]


def prog_lists(n, L, wide, empty_bits):
    def prog(b):
        idx, v = b.nat_in(0), b.nat_in(1)
        for k, bits in enumerate(rc_bits(L)):
            b.range_check(b.nat_in(2 + k), bits)
        narrow = [b.nat_in(8 + k) for k in range(n)]
        ind = b.idx_to_indicator(idx, n)
        out = [ind, b.select_from_idx(narrow, idx), b.select_array_by_indicator([[x] for x in narrow], ind)]
        if wide:
            arr = [b.hash_in(8 + n + 4 * k) for k in range(n)]
            out += [b.select_array_by_indicator([[x, narrow[k]] for k, x in enumerate(arr)], ind), b.select_from_idx(arr, idx)]
        bits = b.num_to_bits(v, n)
        out += [bits, b.bits_to_num(bits)]
        if empty_bits:
            out.append(b.bits_to_num([]))
        return out
    return prog


def make_lists(n, L, wide):
    def make(i):
        p = [0] * (8 + n + (4 * n if wide else 0))
        p[0] = (0, n - 1, n)[i % 3]
        p[1] = 0 if (i // 3) % 2 else 2**n - 1                   # all-one / all-zero bits
        for k, bits in enumerate(rc_bits(L)):
            p[2 + k] = 0 if (i + k) % 2 else 2**bits - 1
        for k in range(n):
            p[8 + k] = pick(N_POOL, i, k)
            if wide:
                _put_fr(p, 8 + n + 4 * k, pick(FR_EDGES, i, k, off=3))
        return p
    return make


# ---- 4. ring distance.  A value of one, two and four slots consumed exactly `dist` slots after it was produced: dist = the segment's slot count behind
# the consumer's result minus the value's first slot, which is what the lowering compares with the ring's 256 slots.  Slots: a load takes its result's
# and as many for the proof words fetched in front of it; a select one.  words: 0 x, 1 a bit (the padding), 2 n, 3.. h
RING_USED = {1: 2, 2: 2, 4: 8}      # slots from the value's first to the padding: the value (and the proof words fetched for it)
RING_RES = {1: 2, 2: 1, 4: 4}       # slots of the consumer's result: add of two one-word values (a gate), reduce, add of two wide values


def prog_ring(dist):
    def prog(b):
        out = []
        for width in (1, 2, 4):
            if width == 2:
                m1, m2 = b.nat_in(0), b.nat_in(2)
            v = b.nat_in(0) if width == 1 else b.mul(m1, m2) if width == 2 else b.hash_in(3)
            pad = dist - RING_USED[width] - RING_RES[width]
            for _ in range(pad // 2):
                bit = b.nat_in(1)                    # two slots, one cell
            if pad % 2:
                bit = b.select(bit, bit, bit)        # one slot
            use = b.gl_reduce(v) if width == 2 else b.add(v, v)
            out += [v, bit, use]
        return out
    return prog


def make_ring(i):
    p = [pick(N_POOL, i, 0), (i // 2) & 1, pick(N_POOL, i, 2)] + [0] * 4
    _put_fr(p, 3, pick(FR_EDGES, i, 3))
    return p


# ---- 5. far constants: more distinct constants than the part of the two pools kept in LDS.  A fresh plan's pools fill in the order of first use, so
# the k-th constant loaded here is pool entry k.  words: 0 x (Goldilocks), 1 n, 2.. h
N_LIT64, N_LITFR, POOL64_CAP, POOLFR_CAP = 2060, 480, 2048, 472
LIT64 = [0x1000000000 + 3 * k for k in range(N_LIT64)]
LITFR = [2**200 + 2**64 * 7 + k for k in range(N_LITFR)]


def prog_far_consts(b):
    c64 = [b.const(v) for v in LIT64]
    cfr = [b.const(v) for v in LITFR]
    x, n, h = b.gl_in(0), b.nat_in(1), b.hash_in(2)
    out = [x, n, h]
    for k in (POOL64_CAP - 1, POOL64_CAP, POOL64_CAP + 1):
        out += [c64[k], b.gl_mul_add(x, c64[k], x), b.mul_add(n, c64[k], n), b.mul(h, c64[k])]
    for k in (POOLFR_CAP - 1, POOLFR_CAP, POOLFR_CAP + 1):
        out += [cfr[k], b.mul(n, cfr[k]), b.mul_add(h, cfr[k], cfr[k])]
    return out


def make_far_consts(i):
    p = [pick(GL_ANY, i, 0), pick(N_POOL, i, 1)] + [0] * 4
    _put_fr(p, 2, pick(FR_EDGES, i, 2))
    return p


# ---- 6. runs of consecutive Goldilocks ops (DOP_GLOPRUN holds at most 255).  words: 0 x, 1 y, 2 a separator
RUN_LENGTHS = (1, 2, 255, 256, 257)
RUN_K = 0x123456789


def prog_runs(fuse_const=True):
    def prog(b):
        x, y = b.gl_in(0), b.gl_in(1)
        k_early = None if fuse_const else b.gl_const(RUN_K)
        out = [x, y]; v = [x, y, x]      # the ops take the last three values: an operand further back than the ring is fetched, and the fetch ends the run
        for ln in RUN_LENGTHS:
            out.append(b.nat_in(2))      # not a Goldilocks op: the run ends here
            for j in range(ln):
                if ln == 255 and j == 100:      # a constant loaded just in front of the op that takes it: one record (T_KA_GLOP), in the middle of a run
                    k = b.gl_const(RUN_K) if fuse_const else k_early
                    r = b.gl_mul(k, v[-1])
                else:
                    r = (b.gl_mul_add, b.gl_add, b.gl_sub, b.gl_mul)[j % 4](*((v[-1], v[-2], v[-3]) if j % 4 == 0 else (v[-1], v[-3]) if j % 4 == 2 else (v[-1], v[-2])))
                v = v[-2:] + [r]
            out.append(v[-1])
        return out
    return prog


def make_runs(i):
    return [pick(GL_ANY, i, 0), pick(GL_ANY, i, 1), pick(GL_EDGES, i, 2)]


# ---- 7. scopes.  words: 0 x, 1 n0, 2.. h, 6 o1, 7 o2's factor, 8.. o4, 12 .. the instances' own words
SCOPE_NAMES = ("inst", "other", "outer", "inner")


def prog_scopes(ninst):
    def prog(b):
        x, n0, h = b.gl_in(0), b.nat_in(1), b.hash_in(2)
        g = b.mul(n0, n0)                                   # two slots
        out = [x, n0, h, g]
        for k in range(ninst):                               # isomorphic instances: one template, ninst lanes per proof
            with b.scope("inst"):
                a = b.gl_in(12 + k); out += [a, b.gl_mul_add(a, x, a), b.add(g, a)]
        with b.scope("inst"):                                # an instance with no op in it
            pass
        for k in range(2):                                   # another shape at the same depth: a second template in the same launch
            with b.scope("other"):
                a = b.nat_in(12 + k); out += [b.mul_add(h, a, g), b.gl_reduce(g)]
        for k in range(2):
            with b.scope("outer"):
                o1 = b.gl_in(6); o2 = b.mul(b.nat_in(7), n0); o4 = b.hash_in(8)
                out += [o1, o2, o4]
                for j in range(2):
                    with b.scope("inner"):                   # depth 2: a one-, a two- and a four-word value from depth 0 and from depth 1
                        out += [b.gl_mul(x, o1), b.add(g, o2), b.add(h, o4), b.gl_reduce(o2), b.mul_add(o4, g, o1)]
        out += [b.gl_add(x, x), b.add(h, g)]                # the root goes on behind the scopes
        return out
    return prog


def make_scopes(ninst):
    def make(i):
        p = [0] * (12 + max(ninst, 2))
        p[0], p[1], p[6], p[7] = pick(GL_ANY, i, 0), pick(N_POOL, i, 1), pick(GL_EDGES, i, 6), pick(N_POOL, i, 7)
        _put_fr(p, 2, pick(FR_EDGES, i, 2)); _put_fr(p, 8, pick(FR_EDGES, i, 8))
        for k in range(max(ninst, 2)):
            p[12 + k] = pick(GL_EDGES, i, 12 + k)
        return p
    return make


# ---- 8. many far operands in one op: a wide select_array_by_indicator whose array was loaded in the root.  words: 4 k .. entry k, 4 n: idx
def prog_far_operands(n, scoped):
    def prog(b):
        arr = [b.hash_in(4 * k) for k in range(n)]
        with (b.scope("sel") if scoped else contextlib.nullcontext()):
            idx = b.nat_in(4 * n); ind = b.idx_to_indicator(idx, n)
            r = b.select_array_by_indicator([[x] for x in arr], ind)
        return [arr, ind, r]
    return prog


def make_far_operands(n):
    def make(i):
        p = [0] * (4 * n + 1)
        for k in range(n):
            _put_fr(p, 4 * k, pick(FR_EDGES, i, k) if (i + k) % 5 else (R - 1 - k - 64 * i) % R)      # distinct entries among the edges: a wrong a_i shows
        p[4 * n] = (i % 16, n - 1)[(i // 16) % 2]
        return p
    return make


def _need(counts, E, ops=(), fetch=()):
    for name in ops:
        assert counts[E[name]] > 0, f"no {name} in the lowered program"
    for name in fetch:
        assert counts[E["DOP_COUNT"] + E[name]] > 0, f"no DOP_FETCH of {name} in the lowered program"


def fetches(counts, E, kind):
    return counts[E["DOP_COUNT"] + E[kind]]


def longest_run(counts, E):
    return counts[E["DOP_COUNT"] + E["RK_RING"]]


def _expect_gl(c, E): _need(c, E, ("DOP_LOADW", "DOP_LOADW_DIV", "DOP_LOADW_EXTINV", "DOP_GLOP", "DOP_GLOPRUN", "DOP_GATE", "DOP_REDUCE", "DOP_CONST1"), ("RK_INPUT",))
def _expect_native(c, E): _need(c, E, ("DOP_FRCELL", "DOP_GATE", "DOP_FR_ADD", "DOP_FR_MUL", "DOP_FR_MULADD", "DOP_SELECT", "DOP_FR_SELECT", "DOP_LIMBS2NUM", "DOP_DECOMP565", "DOP_CLT"))
def _expect_lists(c, E): _need(c, E, ("DOP_IDX2IND", "DOP_SELIND", "DOP_NUM2BITS", "DOP_BITS2NUM", "DOP_RANGE"))
def _expect_lists_wide(c, E): _expect_lists(c, E); _need(c, E, ("DOP_FR_SELIND",))


def _expect_ring(dist):
    def expect(c, E):
        assert fetches(c, E, "RK_LOCAL") == (5 if dist > 256 else 0), (dist, fetches(c, E, "RK_LOCAL"))      # add(v, v) fetches v twice, reduce(v) once
    return expect


def _expect_far_consts(c, E):
    # the loads of the entries beyond the LDS part fetch them, and so does every use of entries CAP and CAP + 1 (three each); entry CAP - 1 is at hand
    assert fetches(c, E, "RK_LIT64") == N_LIT64 - POOL64_CAP + 6 and fetches(c, E, "RK_LITFR") == N_LITFR - POOLFR_CAP + 6, (fetches(c, E, "RK_LIT64"), fetches(c, E, "RK_LITFR"))


def _expect_runs(c, E):
    assert longest_run(c, E) == 255 and c[E["DOP_GLOPRUN"]] == 5 and c[E["DOP_GLOP"]] == 2, (longest_run(c, E), c[E["DOP_GLOPRUN"]], c[E["DOP_GLOP"]])


def _expect_scopes(c, E):
    _need(c, E, ("DOP_SKIP",), ("RK_IMPORT",))
    assert c[E["DOP_END"]] == 6, c[E["DOP_END"]]      # templates: the root, "inst", the empty "inst", "other", "outer", "inner"


def _expect_far_operands(n, scoped):
    def expect(c, E):
        _need(c, E, ("DOP_FR_SELIND",))
        if scoped:
            assert fetches(c, E, "RK_IMPORT") == n, fetches(c, E, "RK_IMPORT")
    return expect


LIST_CASES = [(1, 21, True), (2, 13, True), (63, 8, False), (64, 21, False)]      # (n, lookup_bits, with the wide array: from 52 wide entries on the op is refused)


def programs(empty_bits=True):
    ps = []
    for L in (21, 13, 8):
        ps.append(Program(f"gl_ops-L{L}", prog_gl_ops, 13, make_gl_ops, L, expect=_expect_gl))
        ps.append(Program(f"native-L{L}", prog_native, 20, make_native, L, expect=_expect_native))
    for n, L, wide in LIST_CASES:
        ps.append(Program(f"lists-n{n}", prog_lists(n, L, wide, empty_bits), 8 + n + (4 * n if wide else 0), make_lists(n, L, wide), L, expect=_expect_lists_wide if wide else _expect_lists))
    for dist in (255, 256, 257):
        ps.append(Program(f"ring-{dist}", prog_ring(dist), 7, make_ring, expect=_expect_ring(dist)))
    ps.append(Program("far_consts", prog_far_consts, 6, make_far_consts, expect=_expect_far_consts))
    ps.append(Program("runs", prog_runs(), 3, make_runs, sizes=(1, 70), expect=_expect_runs))
    for ninst in (1, 63, 64, 65):
        ps.append(Program(f"scopes-{ninst}", prog_scopes(ninst), 12 + max(ninst, 2), make_scopes(ninst), 13, SCOPE_NAMES, sizes=(1, 70) if ninst == 1 else (1, 5), expect=_expect_scopes))
    for scoped in (True, False):
        ps.append(Program(f"far_operands-51-{'scoped' if scoped else 'flat'}", prog_far_operands(51, scoped), 205, make_far_operands(51), 21, ("sel",) if scoped else (), sizes=(1, 70), expect=_expect_far_operands(51, scoped)))
    return ps


PROGRAMS = programs()
