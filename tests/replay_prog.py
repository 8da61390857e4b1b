"""Hand-driven operator programs for the traced-plan tests (a helper, not a test).

A program is a function prog(b) written once against the small backend interface below and run on three backends:
  TraceBackend   a fresh api.Context in trace mode: every *_in tags the proof word (h2w_trace_input) in front of the load; values from "proof A"
  OracleBackend  oracle.Ctx and the orc_* op drivers of oracle/oracle.h, on the raw words of the proof passed in
  IntBackend     Python integers only, no cells: the value of every handle ((a * b + c) % P, % R, bit lists ...) and the status word
lower() turns the traced run into a plan; check_on_device() replays it on a batch and holds every proof's stream to the oracle's bytes, its
status word and the cells at the returned handles to the Int backend's values (and the oracle's values to the Int backend's: a bug the oracle
and the device share still shows); a proof the Int backend gives status 5 (include/h2w.h 2d) is held to the cells in front of the offending op.  The programs themselves (PROGRAMS) are shared by tests/test_replay_programs_lowering.py (no GPU) and
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
        self.entries = []      # the cell count at the entry of every op that can raise status 5, in program order (IntBackend.off indexes it)

    def _enter(self): self.entries.append(self.ctx.num_cells())
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
    def select(self, a, b, s): self._enter(); return self.L.orc_select(self.p, a, b, s)
    def select_from_idx(self, arr, idx): return self.L.orc_select_from_idx(self.p, self._arr(arr), len(arr), idx)

    def idx_to_indicator(self, idx, n):
        out = (self.O.AV * n)(); self.L.orc_idx_to_indicator(self.p, idx, n, out); return list(out)

    def select_array_by_indicator(self, arr2d, ind):
        self._enter(); ln, w = len(arr2d), len(arr2d[0]); out = (self.O.AV * w)()
        self.L.orc_select_array_by_indicator(self.p, self._arr([x for row in arr2d for x in row]), ln, w, self._arr(ind), out); return list(out)

    def num_to_bits(self, a, n):
        out = (self.O.AV * n)(); self.L.orc_num_to_bits(self.p, a, n, out); return list(out)

    def bits_to_num(self, bits): self._enter(); return self.L.orc_bits_to_num(self.p, self._arr(bits), len(bits))

    def decompose_le(self, a, limb_bits, n):
        out = (self.O.AV * n)(); self.L.orc_decompose_le(self.p, a, limb_bits, n, out); return list(out)

    def limbs_to_num(self, limbs, limb_bits): return self.L.orc_limbs_to_num(self.p, self._arr(limbs), len(limbs), limb_bits)
    def check_less_than_safe(self, a, bound): self.L.orc_check_less_than_safe(self.p, a, bound)
    def range_check(self, a, bits): self.L.orc_range_check(self.p, a, bits)
    def gl_add(self, a, b): return self.L.orc_gl_add(self.p, a, b)
    def gl_sub(self, a, b): return self.L.orc_gl_sub(self.p, a, b)
    def gl_mul(self, a, b): return self.L.orc_gl_mul(self.p, a, b)
    def gl_mul_add(self, a, b, c): return self.L.orc_gl_mul_add(self.p, a, b, c)
    def gl_mul_sub(self, a, b, c): self._enter(); return self.L.orc_gl_mul_sub(self.p, a, b, c)
    def gl_neg(self, a): k = self.L.orc_gl_load_constant(self.p, P - 1); return self.L.orc_gl_mul(self.p, a, k)      # load_neg_one, mul (base.rs:234-238)
    def gl_square(self, a): return self.L.orc_gl_mul(self.p, a, a)
    def gl_exp_power_of_2(self, a, k): return self.L.orc_gl_exp_power_of_2(self.p, a, k)
    def gl_reduce(self, a): self._enter(); return self.L.orc_gl_reduce(self.p, a)
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
    """Values only, exact in the field.  chip: the status of the first op of the run that raises one (1: a zero divisor, 2: a zero extension element -
    the reference would panic; 5: an operand outside the domain its op is lowered for, include/h2w.h 2d: a selector, an indicator or a bit above 1,
    more than one indicator set in a select_by_indicator on one-word entries, GoldilocksChip::reduce of 2^128 or more); off: which of the ops that can
    raise 5 - select, select_array_by_indicator, bits_to_num, gl_mul_sub, gl_reduce, counted in program order as OracleBackend.entries lists them - was
    the first to, n_off: how many did; flagged: a proof word outside its field (one word >= p, four words >= r); unspecified: a four-word one, whose
    cells h2w.h leaves open."""

    def __init__(self, words):
        self.w, self.chip, self.flagged, self.unspecified = words, 0, False, False
        self.k, self.off, self.n_off = 0, None, 0

    def _domain(self, left):
        """the entry of an op that can raise 5; left: its operands are outside the domain"""
        if left:
            self.chip = self.chip or 5; self.n_off += 1
            if self.off is None:
                self.off = self.k
        self.k += 1

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
    def select(self, a, b, s): self._domain(s > 1); return ((a - b) * s + b) % R
    def select_from_idx(self, arr, idx): return arr[idx] if idx < len(arr) else 0
    def idx_to_indicator(self, idx, n): return [1 if i == idx else 0 for i in range(n)]
    def select_array_by_indicator(self, arr2d, ind):
        # a column of one-word entries is one narrow op.  (The lowering goes by the static width and the model sees values: the programs that set more
        # than one indicator keep an entry of 2^64 or more in every four-word column.)
        narrow = any(all(row[j] < 2**64 for row in arr2d) for j in range(len(arr2d[0])))
        self._domain(any(s > 1 for s in ind) or (narrow and sum(1 for s in ind if s) > 1))
        return [sum(row[j] * s for row, s in zip(arr2d, ind)) % R for j in range(len(arr2d[0]))]
    def num_to_bits(self, a, n): return [(a >> i) & 1 for i in range(n)]
    def bits_to_num(self, bits): self._domain(any(x > 1 for x in bits)); return sum(x << i for i, x in enumerate(bits)) % R
    def decompose_le(self, a, limb_bits, n): return [(a >> (limb_bits * i)) & ((1 << limb_bits) - 1) for i in range(n)]
    def limbs_to_num(self, limbs, limb_bits): return sum(x << (limb_bits * i) for i, x in enumerate(limbs)) % R
    def check_less_than_safe(self, a, bound): pass
    def range_check(self, a, bits): pass
    def gl_add(self, a, b): return (a + b) % P
    def gl_sub(self, a, b): return (a - b) % P
    def gl_mul(self, a, b): return a * b % P
    def gl_mul_add(self, a, b, c): return (a * b + c) % P
    def gl_mul_sub(self, a, b, c): v = a * b + c * (P - 1); self._domain(v >= 2**128); return v % P      # mul_no_reduce, sub_no_reduce (a + b (p - 1), base.rs:262-272), reduce
    def gl_neg(self, a): return -a % P
    def gl_square(self, a): return a * a % P
    def gl_exp_power_of_2(self, a, k): return pow(a, 2**k, P)
    def gl_reduce(self, a): self._domain(a >= 2**128); return a % P

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


def oracle_run(oracle, prog, proof, lookup_bits=21, entries=False):
    """(stream bytes, cells of the returned handles, their values) of prog on the oracle; entries: and OracleBackend.entries"""
    ob = OracleBackend(oracle, proof, lookup_bits)
    hs = flatten(prog(ob))
    out = ob.ctx.advice_bytes(), [int(h.cell) for h in hs], [h.v.to_int() for h in hs]
    ob.ctx.close()
    return out + (ob.entries,) if entries else out


def held_cells(ib, entries, num_cells):
    """How many cells of a proof's stream are the oracle's (include/h2w.h 2d): all of them, or - an op of the run raised 5 - those in front of the
    first cell of the first such op.  ib: the proof's IntBackend after the run; entries: its OracleBackend's."""
    assert len(entries) == ib.k
    return num_cells if ib.off is None else entries[ib.off]


def compare_on_device(i, got, status, want_status, ib, stream, entries, offsets, want_vals):
    """Proof i of a replayed batch against the oracle's stream and the integer model (check_on_device; tests/test_gpu_replay_split_selects.py).
    got: its cells, [num_cells, 4] u64"""
    import numpy as np
    assert status == want_status, f"proof {i}: status {status}, expected {want_status}"
    want = np.frombuffer(stream, dtype=np.uint64).reshape(-1, 4)
    cut = held_cells(ib, entries, len(want))
    if not np.array_equal(got[:cut], want[:cut]):
        bad = np.nonzero((got[:cut] != want[:cut]).any(axis=1))[0]
        raise AssertionError(f"proof {i} (status {status}, {cut} of {len(want)} cells held): {len(bad)} cells differ, first at {bad[:8]}: got {got[bad[0]]} want {want[bad[0]]}")
    for k, (c, v) in enumerate(zip(offsets, want_vals)):
        if c < cut:
            assert [int(x) for x in got[c]] == fr_words(v), f"proof {i}: handle {k} (cell {c}) is not the integer model's value {v:#x}"


def int_run(prog, proof):
    ib = IntBackend(proof)
    return flatten(prog(ib)), ib


def check_on_device(h2w, api, oracle, prog, proof_a, proofs, lookup_bits=21, parallel_scopes=()):
    """Traces prog on proof A, replays the plan on `proofs` in one batch, and holds every proof to the oracle and to the Int backend: the status word
    is the model's; the whole stream and every handle where no op raised 5, else the cells in front of the first op that did.  -> the status words"""
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
        stream, cells, vals, entries = oracle_run(oracle, prog, p, lookup_bits, entries=True)
        assert cells == lw.offsets and len(stream) == plan.num_cells * 32
        assert vals == want_vals, f"proof {i}: the oracle's values differ from the integer model at handles {[k for k in range(len(vals)) if vals[k] != want_vals[k]][:8]}"
        compare_on_device(i, got[i], status[i], ib.status(), ib, stream, entries, lw.offsets, want_vals)
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

    def __init__(self, name, fn, nwords, make, lookup_bits=21, scopes=(), sizes=(1, 130), expect=None, off=None, fix_a=None):
        self.name, self.fn, self.nwords, self.make, self.lookup_bits, self.scopes, self.sizes, self.expect = name, fn, nwords, make, lookup_bits, tuple(scopes), sizes, expect
        self.off, self.fix_a = off, fix_a      # off: the OffDomain of a program whose batch leaves proof A's domain; fix_a(p): what the eager calls need of proof A

    def proof_a(self):
        p = safe_proof(self.nwords)
        if self.fix_a:
            self.fix_a(p)
        return p

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


# ---- 9. proofs that leave proof A's value domain (include/h2w.h 2d, status 5).  Proof A's eager calls validated what proof A holds; the interpreter
# works at the widths the lowering assigned and has no host call that could refuse: a selector, an indicator or a bit above 1, a second indicator set
# where the entries are one word, a value of 2^128 or more in front of GoldilocksChip::reduce.  Every program starts and ends with a division
# (words 0 1 and 2 3: x, divisor), so that a zero divisor can stand in front of and behind the offence.
OFF_POOL = [2, 2**32, P - 1]


class OffDomain:
    """The batch of such a program.  base(i): proof i, in domain (canonical words: status 0); kinds: [(name, put(p))] - put writes ONE offence into a proof.
    Proof i is in domain where i % 4 == 0; the others take the kinds in turn.  i % 16 == 5: the last divisor is zero as well (the 5 comes first and
    wins), i % 16 == 11: the first one is (status 1; the cells in front of the offending op are still the oracle's)."""

    def __init__(self, base, kinds):
        self.base, self.kinds = base, kinds

    def kind(self, i):
        j = i - i // 4 - 1      # the off-domain proofs in front of proof i; every run of len(kinds) of them holds every kind, rotated by one from run to run, so
        return None if i % 4 == 0 else self.kinds[(j + j // len(self.kinds)) % len(self.kinds)]      # that a kind meets the zero divisors of i % 16 in some proofs only

    def expected_status(self, i):
        return 0 if i % 4 == 0 else 1 if i % 16 == 11 else 5

    def make(self, i):
        p = self.base(i); k = self.kind(i)
        if k:
            k[1](p)
        if i % 16 == 5:
            p[3] = 0
        if i % 16 == 11:
            p[1] = 0
        return p


def _put(word, v):
    return lambda p: p.__setitem__(word, v)


def _div(b, w):
    x, d = b.gl_in(w), b.gl_in(w + 1)
    return [x, d, b.gl_div(x, d)]


def _div_words(i):
    return [pick(GL_EDGES, i, 0), pick(GL_EDGES[1:], i, 1), pick(GL_EDGES, i, 2), pick(GL_EDGES[1:], i, 3)]


# 9a. select.  words: 4 n0, 5 n1, 6.. h0, 10.. h1, 14 .. 17 the selectors of the narrow, the wide, the wide-and-narrow select and of select(n0, n0, .)
def prog_off_select(b):
    out = _div(b, 0)
    n0, n1, h0, h1 = b.nat_in(4), b.nat_in(5), b.hash_in(6), b.hash_in(10)
    sels = [b.nat_in(14 + k) for k in range(4)]
    for (x, y), s in zip(((n0, n1), (h0, h1), (h0, n1), (n0, n0)), sels):      # (a == b: the result would come out right, the selector is still no bit)
        r = b.select(x, y, s); out += [r, b.add(r, n1)]
    return out + _div(b, 2) + [n0, n1, h0, h1] + sels


def base_off_select(i):
    p = _div_words(i) + [pick(GL_EDGES, i, 4), pick(GL_EDGES, i, 5)] + [0] * 8 + [(i >> k) & 1 for k in (2, 3, 4, 5)]
    _put_fr(p, 6, pick(FR_EDGES, i, 6)); _put_fr(p, 10, pick(FR_EDGES, i, 7))
    return p


OFF_SELECT = OffDomain(base_off_select, [(f"{name}-{v:#x}", _put(14 + k, v)) for k, name in enumerate(("narrow", "wide", "mixed", "equal")) for v in OFF_POOL])


# 9b. bits.  words: 4 5 the bits of bits_to_num at n = 2, 6 .. 69 at n = 64; 70, 71 the numbers of num_to_bits at 2 and 8 bits; 72 .. 77 range-checked
# words; 78 check_less_than_safe.  The words from 70 on are beyond their ranges in most proofs of the batch, in-domain ones included: those values fit,
# the stream is the oracle's and the status stays 0.
def prog_off_bits(L):
    def prog(b):
        out = _div(b, 0)
        for bits in ([b.nat_in(4 + k) for k in range(2)], [b.nat_in(6 + k) for k in range(64)]):
            r = b.bits_to_num(bits); out += [r, b.add(r, r)]
        out += [b.num_to_bits(b.nat_in(70), 2), b.num_to_bits(b.nat_in(71), 8)]
        for k, bits in enumerate(rc_bits(L)):
            b.range_check(b.nat_in(72 + k), bits)
        b.check_less_than_safe(b.nat_in(78), P)
        return out + _div(b, 2)
    return prog


def base_off_bits(L):
    def base(i):
        rnd = random.Random(1000 + i)
        p = _div_words(i) + [rnd.randrange(2) for _ in range(66)] + [pick([3, 4, 2**32, P - 1, 1], i, 70), pick([255, 256, 2**63, P - 1, 2**8 + 1], i, 71)]
        if i % 8 == 0:
            p[6:70] = [1] * 64                                          # 2^64 - 1: the largest sum of bits
        for k, bits in enumerate(rc_bits(L)):
            n = (bits + L - 1) // L
            p.append(pick([v for v in (2**bits - 1, 2**bits, 2**bits + 1, 2**(n * L) - 1, 2**(n * L), 2**63, P - 1) if v < P], i, 72 + k))
        return p + [pick([P - 1, P - 2, 0, 2**32], i, 78)]
    return base


def _two_high_bits(p):
    p[4] = p[5] = 2**63      # 2^63 + 2^64: wraps to 2^63 in 64 bits


OFF_BITS_KINDS = [(f"n2-bit{k}-{v:#x}", _put(4 + k, v)) for k in (0, 1) for v in OFF_POOL] + [(f"n64-bit{k}-{v:#x}", _put(6 + k, v)) for k in (0, 1, 63) for v in OFF_POOL] + [("n2-both-2^63", _two_high_bits)]


# 9c. select_by_indicator.  words: 4 5 / 6 7 two one-word entries and their indicators; 8.. 12.. / 16 17 two four-word entries; 18 .. 81 / 82 .. 145 64 one-word
# entries; 146 .. 177 / 178 .. 241 eight four-word entries, in front of 56 four-word constants (64 four-word values loaded by the program would have
# to be fetched into more slots than a lane has, h2w.h 2d).  An indicator list in domain is all zero or has one entry set; where the entries are four
# words it may have several set: the sum is the field's.
SI = {"narrow2": (4, 6, 2), "wide2": (8, 16, 2), "narrow64": (18, 82, 64), "wide64": (146, 178, 64)}      # name -> (first entry word, first indicator word, n)
SI_CONSTS = [2**200 + 2**64 * 7 + k for k in range(56)]
SI_BIG = [2**64, 2**128 - 1, 2**128, 2**253, R - 1]


def prog_off_selind(b):
    out = _div(b, 0)
    ks = [b.const(v) for v in SI_CONSTS]
    use = b.nat_in(4)
    for name, (e0, i0, n) in SI.items():
        wide = name.startswith("wide")
        arr = [b.hash_in(e0 + 4 * k) for k in range(min(n, 8))] + (ks if n == 64 else []) if wide else [b.nat_in(e0 + k) for k in range(n)]
        ind = [b.nat_in(i0 + k) for k in range(n)]
        r = b.select_array_by_indicator([[x] for x in arr], ind); out += [r, b.add(r[0], use)]      # (the result is used: a sum cut to 64 bits would show)
    return out + _div(b, 2)


def base_off_selind(i):
    p = _div_words(i) + [0] * 238
    j = i // 4
    for name, (e0, i0, n) in SI.items():
        wide = name.startswith("wide")
        for k in range(min(n, 8) if wide else n):
            if wide:
                _put_fr(p, e0 + 4 * k, pick(SI_BIG, i, k) if k == 0 else pick(FR_EDGES, i, k, off=2))      # (entry 0: two words or more, IntBackend.select_array_by_indicator)
            else:
                p[e0 + k] = pick(GL_EDGES, i, e0 + k)
        if j % 5 != 4:
            p[i0 + (j * 7 + 3) % n] = 1
        if wide and j % 3 == 1:
            p[i0 + (j * 5) % n] = 1; p[i0 + n - 1] = 1
    return p


def _several_set(e0, i0, n):
    def put(p):
        p[i0:i0 + n] = [0] * n; p[i0] = p[i0 + n - 1] = 1
        p[e0], p[e0 + n - 1] = 2**63, P - 1      # their sum is more than one word
    return put


def _the_issues_case(p):
    p[4:8] = [5, 9, 2, P - 1]      # 5 * 2 + 9 * (p - 1) = 0x8fffffff70000000a


OFF_SELIND_KINDS = [(f"{name}-ind{k}-{v:#x}", _put(i0 + k, v)) for name, (e0, i0, n) in SI.items() for k in sorted({0, n // 2 - 1, n - 1}) for v in OFF_POOL]
OFF_SELIND_KINDS += [(f"{name}-two-set", _several_set(*SI[name])) for name in ("narrow2", "narrow64")] + [("narrow2-5-9-by-2-p-1", _the_issues_case)]


# 9d. GoldilocksChip::reduce.  words: 4 x, 5 y, 6 c of mul_sub (x y + c (p - 1) in front of its reduce); 7.. h0, 11.. h1, 15.. h2 of reduce(h0 h1 + h2)
def prog_off_reduce(b):
    out = _div(b, 0)
    x, y, c = b.gl_in(4), b.gl_in(5), b.gl_in(6)
    ms = b.gl_mul_sub(x, y, c); out += [x, y, c, ms, b.gl_add(ms, x)]
    h = [b.hash_in(7 + 4 * k) for k in range(3)]
    g = b.mul_add(h[0], h[1], h[2]); rd = b.gl_reduce(g); out += h + [g, rd, b.gl_mul(rd, y)]
    return out + _div(b, 2)


def fix_a_off_reduce(p):
    for k in range(3):
        p[8 + 4 * k:11 + 4 * k] = [0, 0, 0]      # h0 h1 + h2 below 2^128 on proof A: the eager reduce takes it; the lowering goes by the static width


MS_X = -(-2**128 // (P - 1)) - (P - 1)      # the least x with (x + p - 1) (p - 1) >= 2^128
_MS = [(P - 1, P - 1, P - 1), (MS_X, P - 1, P - 1), (MS_X - 1, P - 1, P - 1), (P - 1, P - 1, 0), (P - 1, P - 1, 2**33), (2**63, 2**63, P - 1), (0, 0, P - 1), (2**32 + 1, P - 2, P - 1),
       (P - 1, 2**32, P - 1), (0, 0, 0), (1, P - 1, 2**63), (P - 2, P - 1, 2**32 + 1), (P - 1, P - 1, MS_X), (P - 1, P - 1, MS_X - 1), (P - 1, P - 2, P - 1), (2**63, P - 1, 2**63)]
MS_IN = [t for t in _MS if t[0] * t[1] + t[2] * (P - 1) < 2**128]
MS_OFF = [t for t in _MS if t not in MS_IN]
# (A, B, C) with A B + C in the field: 2^128 - 1 and 2^128 exactly, 1 by way of (r - 1)^2, values with only word 2 or only word 3 set
_RD = [(2**64, 2**64 - 1, 2**64 - 1), (2**64, 2**64, 0), (R - 1, R - 1, 0), (0, 0, 0), (2**127, 1, 2**127 - 1), (2**127, 2, 0), (2**200, 1, 0), (2**128, 1, 2**64), (R - 1, 1, 0), (2**253, 3, 5),
       (P, P, 0), (R - 1, 2**128, 2**128 - 1), (2**64 - 1, 2**64 - 1, 2**65 - 2), (2**192, 1, 7)]
RD_IN = [t for t in _RD if (t[0] * t[1] + t[2]) % R < 2**128]
RD_OFF = [t for t in _RD if t not in RD_IN]
assert (2**64, 2**64, 0) in RD_OFF and (2**64, 2**64 - 1, 2**64 - 1) in RD_IN and (P - 1, P - 1, P - 1) in MS_OFF and (MS_X - 1, P - 1, P - 1) in MS_IN and len(MS_OFF) >= 4 and len(RD_IN) >= 5


def _put_rd(p, t):
    for k in range(3):
        _put_fr(p, 7 + 4 * k, t[k])


def base_off_reduce(i):
    p = _div_words(i) + list(pick(MS_IN, i, 4)) + [0] * 12
    _put_rd(p, pick(RD_IN, i, 7))
    return p


OFF_REDUCE_KINDS = [(f"mul_sub-{t[0]:#x}-{t[1]:#x}-{t[2]:#x}", lambda p, t=t: p.__setitem__(slice(4, 7), list(t))) for t in MS_OFF]
OFF_REDUCE_KINDS += [(f"reduce-{t[0]:#x}-{t[1]:#x}-{t[2]:#x}", lambda p, t=t: _put_rd(p, t)) for t in RD_OFF]


# 9e. a wide select on n far entries, as 8., with the indicators proof words: at 64 entries refused without H2W_TRACE_SPLIT_SELECTS, replayed in parts
# with it (tests/test_trace_split_selects.py).  words: 4 k .. entry k, 4 n + k: indicator k
def prog_ind_words_select(n, scoped):
    def prog(b):
        arr = [b.hash_in(4 * k) for k in range(n)]
        with (b.scope("sel") if scoped else contextlib.nullcontext()):
            ind = [b.nat_in(4 * n + k) for k in range(n)]
            r = b.select_array_by_indicator([[x] for x in arr], ind)
            use = b.add(r[0], arr[0])
        return [arr, ind, r, use]
    return prog


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


def _expect_off_select(c, E): _need(c, E, ("DOP_SELECT", "DOP_FR_SELECT", "DOP_LOADW_DIV"))
def _expect_off_bits(c, E): _need(c, E, ("DOP_BITS2NUM", "DOP_NUM2BITS", "DOP_RANGE", "DOP_CLT", "DOP_LOADW_DIV"))
def _expect_off_selind(c, E): _need(c, E, ("DOP_SELIND", "DOP_FR_SELIND", "DOP_LOADW_DIV"))
def _expect_off_reduce(c, E): _need(c, E, ("DOP_GATE", "DOP_FR_MULADD", "DOP_REDUCE", "DOP_LOADW_DIV"))


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
    off = [("off_select", prog_off_select, 18, OFF_SELECT, 21, _expect_off_select, None), ("off_selind", prog_off_selind, 242, OffDomain(base_off_selind, OFF_SELIND_KINDS), 21, _expect_off_selind, None),
           ("off_reduce", prog_off_reduce, 19, OffDomain(base_off_reduce, OFF_REDUCE_KINDS), 21, _expect_off_reduce, fix_a_off_reduce)]
    off += [(f"off_bits-L{L}", prog_off_bits(L), 79, OffDomain(base_off_bits(L), OFF_BITS_KINDS), L, _expect_off_bits, None) for L in (21, 13, 8)]
    for name, fn, nwords, od, L, expect, fix_a in off:
        ps.append(Program(name, fn, nwords, od.make, L, expect=expect, off=od, fix_a=fix_a))
    return ps


PROGRAMS = programs()
OFF_PROGRAMS = [p for p in PROGRAMS if p.off]
