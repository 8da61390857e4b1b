"""Python-integer reference, case generators, packer and checker of the record-level expansion tests (tests/test_gpu_expandcheck.py runs the cases on the
device through tests/hip/expandcheck.hip; tests/test_expand_refs.py pins this file to the oracle without a GPU).

The reference expands a record into its cells from the GADGET DEFINITIONS (halo2-base range_check / check_less_than_safe / the vertical gate, and
GoldilocksChip::load_witness / reduce, as the comments of csrc/records.h cite them) - not from the slot tables of records.h and not from the virtual
cell list of expand_fast.  Cells are integers below r; quotient and remainder come from divmod."""
import bisect
import os
import random
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
P = 2**64 - 2**32 + 1
M64 = 2**64 - 1

# ---------------------------------------------------------------------------------------------- layout constants (mirrors of tests/hip/expandcheck.hip, records.h)
MAGIC = int.from_bytes(b"EXPCHK01", "little")
HEADER = 16
GUARD = 64                       # cells in front of cell 0 and behind the last cell
SENTINEL = 0xA5
SENT_CELL = bytes([SENTINEL]) * 32
(T_CONST1, T_CONST4, T_REP12, T_GATE, T_KB_GATE, T_REDUCE, T_GLOP, T_KA_GLOP, T_KB_GLOP, T_LOADW, T_LOADW2, T_CLT_SAFE) = range(12)
TNAMES = ["T_CONST1", "T_CONST4", "T_REP12", "T_GATE", "T_KB_GATE", "T_REDUCE", "T_GLOP", "T_KA_GLOP", "T_KB_GLOP", "T_LOADW", "T_LOADW2", "T_CLT_SAFE"]
GLOPS = (T_GLOP, T_KA_GLOP, T_KB_GLOP)
FAST_BITS = (21, 13, 8)          # the lookup_bits expand_fast is instantiated for
FAST_T, ROW_RECS, UNIT_RECS = 16, 64, 256      # records per pass / per fetched row / per work unit of expand_fast
FAST_MAX_COLS = 64
GENERIC_TILE = 32                # records per tile of expand_kernel_t<32, 5>


def harness_command(out):
    """hipcc with the flags of build.sh and the two include directories: the harness and the product's own expand.hip, two translation units."""
    flags = re.search(r'^FLAGS="(.*)"$', open(os.path.join(ROOT, "build.sh")).read(), flags=re.M).group(1).replace("$H2W_EXTRA", "").split()
    return ["hipcc", *flags, "-I", os.path.join(ROOT, "halo2-plonky2-verifier_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
            os.path.join(ROOT, "tests", "hip", "expandcheck.hip"), os.path.join(ROOT, "halo2-plonky2-verifier_amd", "csrc", "expand.hip"), "-o", out]


# ---------------------------------------------------------------------------------------------- the gadgets
def range_check(x, bits, L):
    """RangeChip::range_check(x, bits) with lookup_bits L: the limbs of the low `bits` bits as an inner product with 2^(jL) ([l0, l1, 2^L, l0 + l1 2^L,
    l2, 2^2L, ...]), then the last limb's fix-up when bits is no multiple of L (assert_bit, or a product with 2^(L - rem) that is looked up)."""
    n, rem = (bits + L - 1) // L, bits % L
    limb = [(x >> (j * L)) & ((1 << L) - 1) for j in range(n)]
    cells, last = [], x
    if n > 1:
        acc = limb[0]; cells = [limb[0]]
        for j in range(1, n):
            acc = (acc + (limb[j] << (j * L))) % R
            cells += [limb[j], 1 << (j * L), acc]
        last = limb[n - 1]
    if rem == 1: cells += [0, last, last, last]
    elif rem > 1: cells += [0, last, 1 << (L - rem), (last << (L - rem)) % R]
    return cells


def check_less_than_safe(x, L, bound=P):
    """RangeChip::check_less_than_safe(x, bound): range_check(x, rb); [x + 2^rb - bound, bound, 1, x + 2^rb, -2^rb, 1, x]; range_check of the first, rb bits."""
    rb = (bound.bit_length() + L - 1) // L * L
    d = (x + (1 << rb) - bound) % R
    return range_check(x, rb, L) + [d, bound, 1, (x + (1 << rb)) % R, (-(1 << rb)) % R, 1, x] + range_check(d, rb, L)


def load_witness(x, L):
    """GoldilocksChip::load_witness (base.rs:107-119): the witness cell, then its range check against p."""
    return [x] + check_less_than_safe(x, L)


def gate(a, b, c):
    """the vertical gate of gate.add / mul / mul_add: [c, a, b, a b + c]"""
    return [c, a, b, (a * b + c) % R]


def reduce_tail(V, L, fault=None):
    """GoldilocksChip::reduce (base.rs:346-368) behind the cell that holds V: quotient (V div p, reduced mod p) and remainder as witnesses, the constant p,
    and the gate [r, q, p, q p + r] (which equals V only while V div p < p)."""
    q, r = divmod(V, P)
    if fault == "no_qhi": q &= M64                 # (the faulty copy of tests/test_expand_refs.py: the quotient's 65th bit lost)
    q %= P
    return load_witness(q, L) + load_witness(r, L) + [P] + [r, q, P, (q * P + r) % R]


def expand(t, rec, L, fault=None):
    """The cells of one record {a, b, c, d} of fixed template t."""
    a, b, c, d = rec
    if t == T_CONST1: return [a]
    if t == T_CONST4: return [a, b, c, d]
    if t == T_REP12: return [a] * 12
    if t == T_GATE: return gate(a, b, c)
    if t == T_KB_GATE: return [b] + gate(a, b, c)                                    # sub_no_reduce: load_neg_one, then the gate
    if t == T_REDUCE: return reduce_tail(a + (b << 64), L, fault)
    if t == T_GLOP: return gate(a, b, c) + reduce_tail(a * b + c, L, fault)
    if t == T_KA_GLOP: return [a] + gate(a, b, c) + reduce_tail(a * b + c, L, fault)
    if t == T_KB_GLOP: return [b] + gate(a, b, c) + reduce_tail(a * b + c, L, fault)
    if t == T_LOADW: return load_witness(a, L)
    if t == T_LOADW2: return load_witness(a, L) + load_witness(b, L)
    if t == T_CLT_SAFE: return check_less_than_safe(a, L)
    raise ValueError("template %d" % t)


def ncells(t, L):
    return len(expand(t, (0, 0, 0, 0), L))


def to_mont(v):
    return (v << 256) % R


def col_map(i, starts, k):
    """the contract of records.h: flat cell i lives at (c << k) + (i - starts[c]) for the LAST column c with starts[c] <= i"""
    c = bisect.bisect_right(starts, i) - 1
    return (c << k) + (i - starts[c])


# ---------------------------------------------------------------------------------------------- operands: the classes, then random ones
def glop_classes(a, b, c):
    """the operand classes of V = a b + c, from the integers alone"""
    V = a * b + c; q, r = divmod(V, P); s = set()
    if V == 0: s.add("V=0")
    if V < P: s.add("q=0")
    if r == 0: s.add("r=0")
    if r == P - 1: s.add("r=p-1")
    if V == P * (P - 1) + (P - 1): s.add("q=r=p-1")
    if a == b == c == M64: s.add("all-ones")
    if V >= P * P: s.add("V>=p^2")
    if q >= 1 << 64: s.add("qhi")
    if max(a, b, c) >= P: s.add("off-domain")
    return s


GLOP_CLASSES = ["V=0", "q=0", "r=0", "r=p-1", "q=r=p-1", "all-ones", "V>=p^2", "qhi", "off-domain"]
_A, _B = 0x123456789ABCDEF1 % P, 0xFEDCBA9876543211 % P
GLOP_EDGES = [(0, 0, 0), (1, 5, 7), (1, P - 2, 1), (_A, _B, (-_A * _B) % P), (_A, _B, (P - 1 - _A * _B) % P), (P - 1, P + 1, 0), (P - 1, P - 1, P - 1), (M64, M64, M64),
              (P, P, 0), (P, P, 1), (P + 1, P, 0), (P, P, P - 1), (M64, P, 0), (M64, M64, 0), (M64, M64 - 1, 5), (2**64 - 2**31, M64, 1), (P - 1, P - 1, 0), (0, M64, M64), (1, P, 0)]
# the value list of tests/test_gpu_eager.py::test_reduce_at_the_edges_of_its_range
REDUCE_EDGES = [v for v in [0, 1, P - 1, P, P + 1, 2**64 - 1, 2**64, P * (P - 1) + (P - 1), P * P - 1, P * P, P * P + 1, (P - 2) * 2**64, 2**127, 2**128 - 2**64, 2**128 - 1,
                            (2**64 + 2**32) * P - 1, (2**64 + 2**32) * P] if v < 2**128]


def witness_edges(L):
    """x of a load_witness / check_less_than_safe: the issue's words, the limb patterns at this L, and both sides of x + 2^RB - p = 2^64 (RB = 64 at L = 8)"""
    nl = (64 + L - 1) // L; lm = (1 << L) - 1
    even = sum(lm << (j * L) for j in range(0, nl, 2)) & M64
    odd = sum(lm << (j * L) for j in range(1, nl, 2)) & M64
    top = (M64 >> ((nl - 1) * L)) << ((nl - 1) * L)
    return [0, 1, P - 1, P, P + 1, M64, even, odd, top, 1 << ((nl - 1) * L), 2**64 - 2**32, 2**64 - 2**32 - 1, 2**32, 2**32 - 1, lm, lm + 1]


def operands(t, L, seed, nrandom):
    """records {a, b, c, d} of template t: every class first, then random ones (half of them on the Goldilocks domain, half any 64-bit words)"""
    rng = random.Random(seed * 100 + t)
    w = lambda i: rng.randrange(P) if i % 2 == 0 else rng.randrange(1 << 64)
    if t in GLOPS:
        return [(a, b, c, 0) for a, b, c in GLOP_EDGES] + [(w(i), w(i), w(i), 0) for i in range(nrandom)]
    if t == T_REDUCE:
        return [(v & M64, v >> 64, 0, 0) for v in REDUCE_EDGES] + [(rng.randrange(1 << 64), rng.randrange(1 << 64), 0, 0) for i in range(nrandom)]
    if t in (T_LOADW, T_CLT_SAFE):
        return [(x, 0, 0, 0) for x in witness_edges(L)] + [(w(i), 0, 0, 0) for i in range(nrandom)]
    if t == T_LOADW2:
        e = witness_edges(L)
        return [(x, e[(i + 5) % len(e)], 0, 0) for i, x in enumerate(e)] + [(w(i), w(i + 1), 0, 0) for i in range(nrandom)]
    if t in (T_GATE, T_KB_GATE):
        return [(M64, M64, M64, 0), (0, 0, 0, 0), (M64, 1, 0, 0), (P, P, P, 0), (1, M64, M64, 0), (1 << 63, 2, 0, 0)] + [(w(i), w(i), w(i), 0) for i in range(nrandom)]
    if t == T_CONST4:
        return [(0, 0, 0, 0), (M64, M64, M64, M64), (0, M64, 0, M64), (M64, 0, M64, 0)] + [(w(i), w(i), w(i), w(i)) for i in range(nrandom)]
    return [(0, 0, 0, 0), (M64, 0, 0, 0)] + [(w(i), 0, 0, 0) for i in range(nrandom)]      # T_CONST1, T_REP12


# ---------------------------------------------------------------------------------------------- geometry: template sequences and cell offsets
# three passes of expand_fast (FAST_T = 16 records each; it flushes groups of four): groups that are all Goldilocks-op blocks next to groups that mix a short
# template with long ones, a pass that takes the all-GLOP shortcut in every group, and the two own-lane templates next to each other and alone
PATTERN = [T_GLOP, T_KA_GLOP, T_KB_GLOP, T_GLOP, T_GLOP, T_GLOP, T_KB_GLOP, T_KA_GLOP, T_REDUCE, T_LOADW, T_LOADW2, T_CLT_SAFE, T_CONST1, T_GATE, T_KB_GATE, T_GLOP,
           T_CONST4, T_GLOP, T_REP12, T_KA_GLOP, T_LOADW, T_CONST1, T_REDUCE, T_GATE, T_KB_GLOP, T_KB_GLOP, T_KA_GLOP, T_GLOP, T_CLT_SAFE, T_LOADW2, T_CONST4, T_REP12,
           T_GLOP, T_KB_GLOP, T_KA_GLOP, T_GLOP, T_KA_GLOP, T_KA_GLOP, T_GLOP, T_KB_GLOP, T_REDUCE, T_REDUCE, T_GLOP, T_REDUCE, T_KB_GLOP, T_GLOP, T_GLOP, T_KA_GLOP]
SHORT = [T_CONST1, T_GATE, T_CONST1, T_KB_GATE, T_CONST1, T_CONST4, T_CONST1, T_GATE]


def template_sequence(nrec, first=None, long_every=1):
    """long_every 1: PATTERN repeated.  n > 1: one record of PATTERN, then n - 1 short ones (the many-proof cases: most cells would be the same anyway)"""
    seq = []
    for i in range(nrec):
        seq.append(PATTERN[(i // long_every) % len(PATTERN)] if i % long_every == 0 else SHORT[i % len(SHORT)])
    if first is not None: seq[0] = first
    return seq


def offsets(tmpls, L, gaps=True):
    """consecutive blocks from flat cell 0; with gaps: one to three cells left out behind every seventh record (the direct cells of a plan: nobody's)"""
    offs, at = [], 0
    for i, t in enumerate(tmpls):
        offs.append(at); at += ncells(t, L)
        if gaps and i % 7 == 6: at += (i // 7) % 3 + 1
    return offs, at


class Case:
    """One launch of launch_expand: the words of the case file, and what the test expects of it."""

    def __init__(self, name, L, tmpls, offs, end, nproofs, counter, mont=False, grid_x=2, roam_per_cu=0, starts=None, k=0, seed=1, nrandom=200, rec_pad=5, cell_pad=37, pool_bits=None):
        self.name, self.L, self.tmpls, self.offs, self.nproofs, self.counter, self.mont = name, L, list(tmpls), list(offs), nproofs, int(counter), int(mont)
        self.grid_x, self.roam_per_cu, self.starts, self.k = grid_x, roam_per_cu, list(starts or []), k
        self.nrec = len(tmpls); self.rec_stride = self.nrec + (rec_pad if nproofs > 1 else 0); self.flat_end = end
        self.cell_stride = ((len(self.starts) << k) if self.starts else end) + cell_pad
        self.sizes = [ncells(t, L) for t in range(12)]
        pools = {t: operands(t, pool_bits or L, seed, nrandom) for t in set(tmpls)}      # (pool_bits: the limb patterns of another lookup_bits)
        per = {t: 0 for t in pools}; idx = []
        for t in tmpls: idx.append(per[t]); per[t] += 1
        # proof p goes on in every template's pool where proof p - 1 stopped
        self.recs = [[pools[t][(idx[i] + p * per[t]) % len(pools[t])] for i, t in enumerate(tmpls)] for p in range(nproofs)]

    # which kernel launch_expand picks for these arguments (expand.hip launch_expand), and why
    def fast(self):
        return bool(self.counter) and self.L in FAST_BITS and len(self.starts) <= FAST_MAX_COLS

    def units(self):
        return (self.nrec + UNIT_RECS - 1) // UNIT_RECS

    def roams(self):
        return self.fast() and self.roam_per_cu > 0 and self.units() >= 16 and self.nproofs <= 4096

    def kernel(self):
        cols = "true" if self.starts else "false"
        if self.fast():      # a work counter, no literal pool, fixed templates only, an instantiated lookup_bits, a column table that fits LDS
            return "expand_fast%s<%d, %s, %s>" % ("_mont" if self.mont else "", self.L, "true" if self.roams() else "false", cols)
        return "%s<32, 5, %s>" % ("expand_kernel_mont" if self.mont else "expand_kernel_t", cols)

    def conditions(self):
        """the line the harness prints before it launches"""
        return "conditions: counter=%d lookup_bits=%d fast_bits=%d ncols=%d cols_fit=%d units256=%d roam_per_cu=%d mont=%d nproofs=%d" % (
            self.counter, self.L, int(self.L in FAST_BITS), len(self.starts), int(len(self.starts) <= FAST_MAX_COLS), self.units(), self.roam_per_cu, self.mont, self.nproofs)

    def total_cells(self):
        return 2 * GUARD + self.nproofs * self.cell_stride


def pack_case(cs):
    head = [MAGIC, cs.L, cs.nproofs, cs.nrec, cs.rec_stride, cs.cell_stride, cs.grid_x, cs.roam_per_cu, cs.counter, cs.mont, len(cs.starts), cs.k, GUARD, 0, 0, 0]
    meta = [(t << 56) | o for t, o in zip(cs.tmpls, cs.offs)]
    recs = np.full((cs.nproofs, cs.rec_stride, 4), 0xDEADBEEFDEADBEEF, dtype="<u8")      # (the records behind nrec belong to nobody)
    for p in range(cs.nproofs):
        recs[p, :cs.nrec] = np.array(cs.recs[p], dtype="<u8")
    return np.array(head + cs.starts + meta, dtype="<u8").tobytes() + recs.tobytes()


def unpack_case(blob):
    """the header and arrays back from the words (the round trip of the layout)"""
    w = np.frombuffer(blob, dtype="<u8")
    h = [int(x) for x in w[:HEADER]]
    assert h[0] == MAGIC and h[12] == GUARD and h[13:] == [0, 0, 0]
    L, nproofs, nrec, rec_stride, cell_stride, grid_x, roam, counter, mont, ncols, k = h[1:12]
    at = HEADER; starts = [int(x) for x in w[at:at + ncols]]; at += ncols
    meta = [int(x) for x in w[at:at + nrec]]; at += nrec
    recs = w[at:].reshape(nproofs, rec_stride, 4)
    return dict(L=L, nproofs=nproofs, nrec=nrec, rec_stride=rec_stride, cell_stride=cell_stride, grid_x=grid_x, roam_per_cu=roam, counter=counter, mont=mont, starts=starts, k=k,
                tmpls=[m >> 56 for m in meta], offs=[m & ((1 << 56) - 1) for m in meta], recs=recs)


# ---------------------------------------------------------------------------------------------- expected buffers and the checker
_cache = {}


def record_bytes(t, rec, L, mont, fault=None):
    key = (t, rec, L, mont, fault)
    b = _cache.get(key)
    if b is None:
        cells = expand(t, rec, L, "no_qhi" if fault == "no_qhi" else None)
        assert all(0 <= v < R for v in cells)
        if mont:
            if fault == "words2":      # the faulty copy: a three-word flush step of expand_fast_mont converted as two words
                vs = VLIST_START.get(t)
                cells = [to_mont(v & M64 if vs is not None and step_has_three_words(L, (vs + s) // 16) else v) for s, v in enumerate(cells)]
            else:
                cells = [to_mont(v) for v in cells]
        b = _cache[key] = b"".join(v.to_bytes(32, "little") for v in cells)
    return b


def expected_buffer(cs, fault=None):
    """The whole result file of a case: guards, every proof's slice with its records' cells (mapped to columns), the sentinel everywhere else."""
    buf = np.full((cs.total_cells(), 32), SENTINEL, dtype=np.uint8)
    order = sorted(range(cs.nrec), key=lambda i: cs.offs[i])
    for p in range(cs.nproofs):
        parts, at = [], 0
        for i in order:
            o = cs.offs[i]
            assert o >= at, "records overlap"
            if o > at: parts.append(SENT_CELL * (o - at))
            b = record_bytes(cs.tmpls[i], cs.recs[p][i], cs.L, cs.mont, fault)
            if fault == "c_lo" and cs.tmpls[i] in VLIST_START: b = SENT_CELL * min(8, len(b) // 32) + b[32 * min(8, len(b) // 32):]      # the faulty copy: the first flush step's cells never stored
            parts.append(b); at = o + len(b) // 32
        assert at <= cs.flat_end
        parts.append(SENT_CELL * (cs.flat_end - at))      # (a gap behind the last record)
        flat = np.frombuffer(b"".join(parts), dtype=np.uint8).reshape(-1, 32)
        base = GUARD + p * cs.cell_stride
        if not cs.starts: buf[base:base + len(flat)] = flat
        else:
            for c, s in enumerate(cs.starts):
                e = cs.starts[c + 1] if c + 1 < len(cs.starts) else max(len(flat), s)
                e = min(e, len(flat))
                if e > s: buf[base + (c << cs.k):base + (c << cs.k) + (e - s)] = flat[s:e]
            if fault == "over_b":      # the faulty copy: behind a column boundary the cells 8 .. 15 of a 16-cell flush step keep the previous column's shift
                for i in order:
                    vs = VLIST_START.get(cs.tmpls[i])
                    c = bisect.bisect_right(cs.starts, cs.offs[i]) - 1
                    if vs is None or c + 1 >= len(cs.starts): continue
                    for s in range(cs.sizes[cs.tmpls[i]]):
                        f = cs.offs[i] + s
                        if f >= cs.starts[c + 1] and (vs + s) % 16 >= 8:
                            buf[base + (c << cs.k) + f - cs.starts[c]] = buf[base + col_map(f, cs.starts, cs.k)]
                            buf[base + col_map(f, cs.starts, cs.k)] = SENTINEL
    return buf


# What the faulty copies need to know of expand_fast, and only they: where a template starts in its virtual cell list (own-lane templates: not in it), and which
# 16-cell flush steps hold a cell of x + 2^RB - p and its kin but neither V nor q p + r.
VLIST_START = {T_KA_GLOP: 0, T_KB_GLOP: 0, T_GLOP: 1, T_REDUCE: 5, T_LOADW: 5, T_LOADW2: 5, T_CLT_SAFE: 6, T_GATE: 1, T_KB_GATE: 0, T_CONST1: 2}


def step_has_three_words(L, c):
    nl = (64 + L - 1) // L; rc = 3 * nl - 2; lw = 1 + rc + 7 + rc; vt = 5 + 2 * lw + 5
    vs = [v for v in range(16 * c, min(16 * c + 16, vt))]
    return not any(v == 4 or v == vt - 1 for v in vs) and any(5 <= v < 5 + 2 * lw and (v - 5) % lw > rc for v in vs)


def locate(cs, cell):
    """buffer cell -> a description of whose it is"""
    if cell < GUARD: return "front guard cell %d" % (cell - GUARD)
    if cell >= GUARD + cs.nproofs * cs.cell_stride: return "rear guard cell +%d" % (cell - GUARD - cs.nproofs * cs.cell_stride)
    p, d = divmod(cell - GUARD, cs.cell_stride)
    flats = [d]
    if cs.starts:
        c, o = d >> cs.k, d & ((1 << cs.k) - 1)
        if c >= len(cs.starts): return "proof %d, cell %d: behind the last column" % (p, d)
        flats = [cs.starts[c] + o]
        if c + 1 < len(cs.starts) and flats[0] >= cs.starts[c + 1]: return "proof %d, column %d row %d: behind the column's last flat cell" % (p, c, o)
    f = flats[0]
    order = getattr(cs, "_order", None)
    if order is None:
        order = cs._order = sorted(range(cs.nrec), key=lambda i: cs.offs[i]); cs._sorted_offs = [cs.offs[i] for i in order]
    j = bisect.bisect_right(cs._sorted_offs, f) - 1
    if j >= 0:
        i = order[j]; s = f - cs.offs[i]
        if s < cs.sizes[cs.tmpls[i]]:
            return "proof %d, record %d (%s %s), slot %d, flat cell %d" % (p, i, TNAMES[cs.tmpls[i]], " ".join("%#x" % x for x in cs.recs[p][i]), s, f)
    return "proof %d, flat cell %d: no record's cell" % (p, f)


def check(cs, got):
    """got: the result file as a (cells, 32) uint8 array.  A message for EVERY differing cell: case, proof, record, template and slot; sentinel cells that were
    overwritten and record cells left as sentinel are named as such."""
    if got.size != cs.total_cells() * 32: return ["%s: result file of %d bytes, expected %d" % (cs.name, got.size, cs.total_cells() * 32)]
    got = got.reshape(-1, 32); want = expected_buffer(cs)
    bad = np.nonzero((got != want).any(axis=1))[0]
    sent = np.frombuffer(SENT_CELL, dtype=np.uint8)
    msgs = []
    for cell in bad:
        g, w = int.from_bytes(got[cell].tobytes(), "little"), int.from_bytes(want[cell].tobytes(), "little")
        where = locate(cs, int(cell))
        if (want[cell] == sent).all(): msgs.append("%s [%s]: sentinel overwritten at %s: got %#x" % (cs.name, cs.kernel(), where, g))
        elif (got[cell] == sent).all(): msgs.append("%s [%s]: cell left as sentinel at %s: want %#x" % (cs.name, cs.kernel(), where, w))
        else: msgs.append("%s [%s]: wrong cell at %s: got %#x want %#x" % (cs.name, cs.kernel(), where, g, w))
    return msgs


# ---------------------------------------------------------------------------------------------- the cases
STATIC_NREC = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1025]
FIRSTS = [T_LOADW, T_CLT_SAFE, T_CONST1, None]      # the record at flat cell 0 (its virtual list starts at 5, 6, 2: the negative `first`); None: PATTERN's own


def static_case(L, nrec, mont=False):
    """expand_fast<L, false, false>: a work counter, flat, no roaming; two or three proofs with padded strides, gaps between the records"""
    i = STATIC_NREC.index(nrec) if nrec in STATIC_NREC else 0
    tm = template_sequence(nrec, FIRSTS[i % 4]); offs, end = offsets(tm, L)
    return Case("static L=%d nrec=%d%s" % (L, nrec, " mont" if mont else ""), L, tm, offs, end, nproofs=3 if nrec > 1000 else 2 + i % 2, counter=1, mont=mont, seed=L + i)


ROAM_SHAPES = [(1, 3), (2, 3), (1, 70), (2, 70)]      # (roam_per_cu, proofs): 70 proofs are more than one look at 64 counters


def roam_case(L, roam_per_cu, nproofs, mont=False):
    """expand_fast<L, true, false>: nrec >= 3841 makes 16 work units.  Three proofs: every template's edge list and 200 random records of it, each expanded once
    and cached; 70 proofs: a few hundred distinct records, one long record in 32."""
    nrec = 3841 + (5 if roam_per_cu == 2 else 0)
    tm = template_sequence(nrec, None, 2 if nproofs <= 3 else 32); offs, end = offsets(tm, L)
    return Case("roam L=%d per_cu=%d proofs=%d%s" % (L, roam_per_cu, nproofs, " mont" if mont else ""), L, tm, offs, end, nproofs=nproofs, counter=1, mont=mont, grid_x=8,
                roam_per_cu=roam_per_cu, seed=L + roam_per_cu, nrandom=200 if nproofs <= 3 else 8)


def _find(tm, t, after, taken):
    for i in range(after, len(tm)):
        if tm[i] == t and all(abs(i - j) >= 3 for j in taken): return i
    raise AssertionError("no free %s record" % TNAMES[t])


def column_boundaries(tm, offs, L):
    """Flat cells where a column starts, each in a record of its own, at least three records apart (a record crosses at most one boundary): the first cell of a record,
    its last cell, strictly inside, at the 8-cell and 16-cell flush-step edges of a Goldilocks-op block (virtual cells 8, 16, 24 and 32: T_GLOP starts at virtual cell 1),
    inside a T_CONST4 and a T_REP12, in a T_LOADW at cell 0's neighbour, and in a gap between two records.  Returns {label: flat cell}."""
    taken, out = [], {}
    def pick(t, label, slot):
        i = _find(tm, t, (taken[-1] + 3) if taken else 1, taken); taken.append(i)
        out[label] = offs[i] + (slot if slot >= 0 else ncells(t, L) + slot)
    pick(T_GLOP, "first cell of a record", 0)
    pick(T_KA_GLOP, "last cell of a record", -1)
    pick(T_KB_GLOP, "strictly inside", 21)
    pick(T_GLOP, "8-cell step edge", 7)
    pick(T_GLOP, "16-cell step edge", 15)
    pick(T_KA_GLOP, "8-cell step edge (24)", 24)
    pick(T_KB_GLOP, "16-cell step edge (32)", 32)
    pick(T_CONST4, "inside T_CONST4", 2)
    pick(T_REP12, "inside T_REP12", 5)
    pick(T_LOADW2, "inside T_LOADW2", 9)
    pick(T_REDUCE, "inside T_REDUCE", 11)
    pick(T_CLT_SAFE, "second cell of T_CLT_SAFE", 1)
    g = next(i for i in range(taken[-1] + 3, len(tm)) if i % 7 == 6)      # offsets() leaves a gap behind this record
    out["between two records"] = offs[g] + ncells(tm[g], L)
    return out


def column_case(L, mont=False, generic_cols=0, nrec=300, counter=1, nproofs=2):
    """Column form.  generic_cols: that many more, short, columns in the empty cells behind the last record (more than 64 columns: the generic kernel)"""
    tm = template_sequence(nrec); offs, end = offsets(tm, L)
    if nrec >= 200: bounds = column_boundaries(tm, offs, L)
    else:      # the small cases of the generic kernel: a boundary inside every third record (short columns keep 2^k, and the buffer, small)
        bounds = {"inside record %d" % i: offs[i] + ncells(tm[i], L) // 2 for i in range(0, nrec, 3) if ncells(tm[i], L) >= 2}
    starts = sorted({0, *bounds.values()})
    starts += [end + 3 + 3 * j for j in range(generic_cols)]
    k = max(1, max(b - a for a, b in zip(starts, starts[1:] + [max(end, starts[-1] + 1)])) - 1).bit_length()
    cs = Case("columns L=%d nrec=%d ncols=%d%s%s" % (L, nrec, len(starts), " mont" if mont else "", "" if counter else " no counter"), L, tm, offs, end, nproofs=nproofs,
              counter=counter, mont=mont, starts=starts, k=k, seed=L + 3)
    cs.bounds = bounds
    return cs


GENERIC_NREC = [1, 31, 32, 33, 100]


def generic_case(L, nrec, counter, cols, mont):
    """expand_kernel_t / expand_kernel_mont <32, 5, cols>: a lookup_bits the fast kernel is not instantiated for (17, 20), or no work counter"""
    if cols: return column_case(L, mont, generic_cols=200, nrec=nrec, counter=counter)
    i = GENERIC_NREC.index(nrec)
    tm = template_sequence(nrec, FIRSTS[i % 4]); offs, end = offsets(tm, L)
    return Case("generic L=%d nrec=%d%s%s" % (L, nrec, " mont" if mont else "", "" if counter else " no counter"), L, tm, offs, end, nproofs=2 + i % 2, counter=counter, mont=mont,
                grid_x=3, seed=L + i)


def shared_layout_cases(mont=False):
    """L = 20 and L = 21 share a cell layout (four limbs, RB 80 / 84): the same records and offsets through the generic and the fast kernel"""
    out = []
    for L in (20, 21):
        tm = template_sequence(257); offs, end = offsets(tm, 21)
        assert offsets(tm, 20) == (offs, end)
        out.append(Case("shared layout L=%d%s" % (L, " mont" if mont else ""), L, tm, offs, end, nproofs=2, counter=1, mont=mont, seed=77, pool_bits=21))
    return out


def class_counts(cs):
    """per operand class of the Goldilocks-op records, and per geometry class, what a case holds"""
    ops = {c: 0 for c in GLOP_CLASSES}
    for p in range(cs.nproofs):
        for t, r in zip(cs.tmpls, cs.recs[p]):
            if t in GLOPS:
                for c in glop_classes(*r[:3]): ops[c] += 1
    geo = dict(records=cs.nrec, proofs=cs.nproofs, cells=sum(cs.sizes[t] for t in cs.tmpls) * cs.nproofs, passes=(cs.nrec + FAST_T - 1) // FAST_T,
               short_last_pass=int(cs.nrec % FAST_T != 0), short_last_row=int(cs.nrec % ROW_RECS != 0), units=cs.units(),
               all_glop_groups=sum(1 for g in range(0, cs.nrec - 3, 4) if all(t in GLOPS or t == T_REDUCE for t in cs.tmpls[g:g + 4])),
               mixed_groups=sum(1 for g in range(0, cs.nrec - 3, 4) if any(t in GLOPS for t in cs.tmpls[g:g + 4]) and any(cs.sizes[t] <= 5 for t in cs.tmpls[g:g + 4])),
               own_lane=sum(1 for t in cs.tmpls if t in (T_CONST4, T_REP12)), gaps=sum(1 for i in range(cs.nrec) if i % 7 == 6),
               templates=len(set(cs.tmpls)), distinct_records=len({(t, r) for p in range(cs.nproofs) for t, r in zip(cs.tmpls, cs.recs[p])}))
    return ops, geo
