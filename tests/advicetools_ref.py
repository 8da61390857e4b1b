"""Plain references of what csrc/advicetools.hip computes on a finished advice stream: Python integers mod r, numpy only to move host
copies around.  Nothing here comes from the package: the digest is written out again from the formula in include/h2w.h.
tests/test_advicetools_refs.py holds these to the oracle before tests/test_gpu_advicetools.py lets them judge a kernel.

`cells` of the checks is a numpy uint64 array [n][4] (little-endian limbs), a list of Python integers (ints() of such an array), or a
dict {cell index: value}: a partial stream, for streams of which a test looks only at the windows it corrupts."""
import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
M64 = (1 << 64) - 1


# What ONE pass of each kernel's grid-stride loop covers, read from the launch lines of csrc/advicetools.hip (blocks x 256 threads; k_check_gates
# takes a selector byte = 8 cells per thread, the layout kernels a 16-byte half cell).  The device tests place their cases by these;
# test_advicetools_refs.py reads the launch lines again with launch_blocks(), so a changed launch line fails there until these follow.
BLOCKS = dict(k_check_gates=2048, k_check_lookups=1024, k_check_equalities=1024, k_layout_columns=4096, k_layout_lookup=4096, k_digest=2048, k_to_montgomery=4096)
THREADS = 256
GATE_PASS_CELLS = BLOCKS["k_check_gates"] * THREADS * 8            # 4,194,304
LOOKUP_PASS = BLOCKS["k_check_lookups"] * THREADS                  # 262,144 registrations
EQUALITY_PASS = BLOCKS["k_check_equalities"] * THREADS             # 262,144 items
COLUMN_PASS_ROWS = BLOCKS["k_layout_columns"] * THREADS // 2       # 2^19 rows of a column
LOOKUP_LAYOUT_PASS_CELLS = BLOCKS["k_layout_lookup"] * THREADS // 2
DIGEST_PASS = BLOCKS["k_digest"] * THREADS                         # 524,288 cells
MONTGOMERY_PASS = BLOCKS["k_to_montgomery"] * THREADS              # 1,048,576 cells


def launch_blocks(source):
    """{kernel: blocks in x} of the hipLaunchKernelGGL lines of advicetools.hip (k_layout_columns: the cap of its computed grid), and the block sizes seen."""
    import re
    out, threads = {}, set()
    for m in re.finditer(r"hipLaunchKernelGGL\((k_\w+), dim3\((\w+)[,)][^;]*?dim3\((\d+)\)", source):
        x = m.group(2)
        if not x.isdigit():
            x = re.search(r"const unsigned %s = [^;]*, (\d+)\);" % x, source).group(1)
        assert out.setdefault(m.group(1), int(x)) == int(x)
        threads.add(int(m.group(3)))
    return out, threads


def to_int(limbs):
    return sum(int(limbs[j]) << (64 * j) for j in range(4))


def to_limbs(v):
    assert 0 <= v < 1 << 256
    return [(v >> (64 * j)) & M64 for j in range(4)]


def pack(values):
    """Python integers -> uint64 [n][4]."""
    return np.array([to_limbs(v) for v in values], dtype=np.uint64).reshape(-1, 4)


def ints(cells):
    """uint64 [n][4] -> a list of Python integers (a whole stream at once: a million cells a second)."""
    return [w[0] | w[1] << 64 | w[2] << 128 | w[3] << 192 for w in np.asarray(cells, dtype=np.uint64).reshape(-1, 4).tolist()]


def _values(cells):
    return ints(cells) if isinstance(cells, np.ndarray) else cells


def gate_cells(selector_bits, n_cells):
    sel = np.unpackbits(np.frombuffer(bytes(selector_bits), dtype=np.uint8), bitorder="little")[:n_cells]
    return np.nonzero(sel)[0].tolist()


def bad_gates(cells, selector_bits, n_cells, gates=None):
    """Selector-enabled cells i whose vertical gate a[i] + a[i+1] a[i+2] = a[i+3] fails.  gates: count only these (each must be enabled)."""
    v = _values(cells)
    if gates is None:
        enabled = gate_cells(selector_bits, n_cells)
    else:
        bits = bytes(selector_bits)
        assert all(0 <= g < n_cells and bits[g >> 3] >> (g & 7) & 1 for g in gates)
        enabled = sorted(set(gates))
    bad = 0
    for i in enabled:
        if i + 3 >= n_cells:
            bad += 1
            continue
        a, x, y, d = v[i], v[i + 1], v[i + 2], v[i + 3]
        if a >= R or x >= R or y >= R or d >= R:      # not a field element: no gate holds on it, whatever it is congruent to
            bad += 1
        elif (a + x * y - d) % R != 0:
            bad += 1
    return bad


def bad_lookups(cells, lookup_cells, lookup_bits, registrations=None):
    """Registrations (not cells: a cell registered twice counts twice) whose cell is not below 2^lookup_bits."""
    v = _values(cells)
    js = range(len(lookup_cells)) if registrations is None else sorted(set(registrations))
    bound = 1 << lookup_bits
    return sum(1 for j in js if v[lookup_cells[j]] >= bound)


def bad_equalities(cells, pairs, const_cells, const_values):
    """(pairs whose two cells differ, constant equalities whose cell is not the constant): all 256 bits compared, nothing reduced."""
    v = _values(cells)
    b0 = sum(1 for a, b in pairs if v[a] != v[b])
    b1 = sum(1 for c, k in zip(const_cells, const_values) if v[c] != k)
    return b0, b1


def columns(cells, break_points, k):
    """uint64 [len(break_points) + 1][2^k][4]: column c starts at the previous column's last cell (repeated), is break_points[c] + 1 cells
    long (the last one takes the rest), rows beyond are zero."""
    n, rows = cells.shape[0], 1 << k
    out = np.zeros((len(break_points) + 1, rows, 4), dtype=np.uint64)
    start = 0
    for c in range(len(break_points) + 1):
        ln = int(break_points[c]) + 1 if c < len(break_points) else n - start
        assert 0 < ln <= rows and start + ln <= n
        out[c, :ln] = cells[start:start + ln]
        start += ln - 1
    return out


def lookup_columns(cells, lookup_cells, k, unusable_rows):
    """uint64 [ncols][2^k][4]: the looked-up cells in registration order down columns of 2^k - unusable_rows rows, the rest zero."""
    rows = 1 << k
    max_rows = rows - unusable_rows
    assert max_rows > 0
    nl = len(lookup_cells)
    ncols = (nl + max_rows - 1) // max_rows
    out = np.zeros((ncols, rows, 4), dtype=np.uint64)
    lc = np.asarray(lookup_cells, dtype=np.int64)
    for c in range(ncols):
        part = lc[c * max_rows:(c + 1) * max_rows]
        out[c, :len(part)] = cells[part]
    return out


def digests(cells, ns):
    """include/h2w.h: digest[j] = sum over cells i of limb_j(cell i) * ((((i + 1) * 0x9E3779B97F4A7C15) | 1) + 2 j) mod 2^64 - of the first n cells,
    for every n in ns (one walk: {n: [4 words]})."""
    a0 = a1 = a2 = a3 = 0
    want, out = set(ns), {}
    if 0 in want:
        out[0] = [0, 0, 0, 0]
    for i, (l0, l1, l2, l3) in enumerate(np.asarray(cells, dtype=np.uint64).reshape(-1, 4)[:max(want, default=0)].tolist()):
        m = (((i + 1) * 0x9E3779B97F4A7C15) & M64) | 1
        a0 += l0 * m; a1 += l1 * (m + 2); a2 += l2 * (m + 4); a3 += l3 * (m + 6)
        if i + 1 in want:
            out[i + 1] = [a0 & M64, a1 & M64, a2 & M64, a3 & M64]
    assert set(out) == want
    return out


def digest(cells):
    n = np.asarray(cells).reshape(-1, 4).shape[0]
    return digests(cells, [n])[n]


def to_montgomery(v):
    return (v << 256) % R
