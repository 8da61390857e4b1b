"""csrc/advicetools.hip - the checkers, layout tools, digest and form conversion that the rest of the suite accepts streams by - held to exact values:
every expectation is an equality with tests/advicetools_ref.py (Python integers; held to the oracle by tests/test_advicetools_refs.py), per call.

Gates and lookups need a plan (its selector bitmap and registrations): the base streams are GPU-generated streams of valid proofs, equal byte for byte
to the oracle's, on which the oracle's MockProver passes - so every gate and lookup that touches no corrupted cell holds, and the reference is
evaluated on the gate windows and registrations that touch one.  Equalities, columns, digest and conversion run on synthetic cells without a plan.
Cases are placed by the grid-stride pass sizes of the launch lines (advicetools_ref.BLOCKS, re-read from the source by test_advicetools_refs.py)."""
import ctypes as C

import numpy as np
import pytest

import advicetools_ref as ref

pytestmark = pytest.mark.gpu

BITS = 21
POISON = -1      # int64 limbs of all ones: no field element, fails every check that reads it


def _st():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _rows(values):
    """Python integers -> int64 tensor [n][4] (host)."""
    import torch
    return torch.from_numpy(ref.pack(values).view(np.int64))


def _dev(a):
    """uint64 numpy [..][4] -> int64 device tensor."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


class _Stream:
    pass


def _oracle_stream(h2w, h2w_api, oracle, consts, mode, d, q, cap):
    """The host half of a base stream: the plan, a valid proof, the oracle's stream of it (its MockProver passes) and the oracle's keygen lists."""
    ko, kh = consts
    s = _Stream()
    sh = h2w.fibonacci_shape(d, q, cap_height=cap, hash_mode=mode); osh = oracle.fibonacci_shape(d, q, cap_height=cap, hash_mode=mode)
    s.plan = h2w_api.Plan(sh, kh)
    s.proof = oracle.prove_fri(osh, ko, 2024)
    ctx = oracle.Ctx(BITS, witness_gen_only=False)
    assert oracle.verify_stark(ctx, osh, ko, s.proof) == 0
    mp = ctx.mock_prover()
    assert mp["bad"] == 0 and mp["semantic_failed"] == 0 and mp["gates"] > 0 and mp["lookups"] > 0, mp
    s.n = ctx.num_cells()
    s.host = ctx.advice_array().copy()
    s.sel, s.lk = ctx.selectors(), ctx.lookup_cells()
    ctx.close()
    assert s.plan.num_cells == s.n and s.plan.selectors() == s.sel and s.plan.lookup_cells() == s.lk
    s.gates = np.array(ref.gate_cells(s.sel, s.n), dtype=np.int64)
    s.lk_np = np.array(s.lk, dtype=np.int64)
    assert (np.diff(s.lk_np) > 0).all()                            # registration order is stream order, no cell twice: searchsorted finds registrations
    s.is_gate = np.zeros(s.n + 8, dtype=bool); s.is_gate[s.gates] = True
    return s


@pytest.fixture(scope="module")
def valid_stream(h2w, h2w_api, oracle, consts):
    """get(mode, d, q, cap): plan, oracle keygen lists and the GPU-generated stream of a valid proof of the shape - made once a module, never written to."""
    import torch
    made = {}

    def get(mode, d, q, cap):
        key = (mode, d, q, cap)
        if key in made:
            return made[key]
        s = _oracle_stream(h2w, h2w_api, oracle, consts, mode, d, q, cap)
        d_proofs = torch.frombuffer(bytearray(bytes(s.proof)), dtype=torch.int64).cuda()
        adv = torch.zeros(s.n * 4, dtype=torch.int64, device="cuda")
        ws = torch.zeros(s.plan.workspace_bytes(1), dtype=torch.uint8, device="cuda")
        s.plan.run(d_proofs.data_ptr(), 1, adv.data_ptr(), ws.data_ptr(), _st())
        torch.cuda.synchronize()
        assert s.plan.status(ws.data_ptr(), 1, _st()) == [0]
        assert np.array_equal(_host(adv).reshape(-1, 4), s.host)      # byte for byte the stream the oracle's MockProver passed
        s.dev = adv.view(-1, 4)
        made[key] = s
        return s

    yield get
    for s in made.values():
        s.plan.close()


def _old(s, c):
    return ref.to_int(s.host[c])


def _expected(s, corr):
    """(failed gates, failed lookups) of the base stream with corr = {proof: {cell: value}} written in, and the same per proof.  The base stream is valid:
    only gates whose window holds a written cell, and registrations of written cells, can fail."""
    per = []
    for p in sorted(corr):
        ch = corr[p]
        cells = {i: _old(s, i) for c in ch for i in range(max(0, c - 3), min(s.n, c + 4))}
        cells.update(ch)
        gates = sorted({g for c in ch for g in range(max(0, c - 3), c + 1) if s.is_gate[g]})
        regs = [int(j) for c in ch for j in range(np.searchsorted(s.lk_np, c, "left"), np.searchsorted(s.lk_np, c, "right"))]
        per.append((ref.bad_gates(cells, s.sel, s.n, gates=gates), ref.bad_lookups(cells, s.lk, BITS, registrations=regs)))
    return (sum(g for g, _ in per), sum(l for _, l in per)), per


def _batch(s, n_proofs, gap):
    import torch
    stride = s.n + gap
    buf = torch.full((n_proofs * stride, 4), POISON, dtype=torch.int64, device="cuda")      # the gaps stay poisoned
    for p in range(n_proofs):
        buf[p * stride:p * stride + s.n] = s.dev
    return buf, stride


def _check(s, buf, stride, n_proofs, corr):
    """Write corr into the batch, ask the device, put the cells back; (got, want, want per proof)."""
    import torch
    where = torch.tensor([p * stride + c for p in sorted(corr) for c in corr[p]], device="cuda")
    src = torch.tensor([c for p in sorted(corr) for c in corr[p]], device="cuda")
    buf[where] = _rows([corr[p][c] for p in sorted(corr) for c in corr[p]]).cuda()
    got = s.plan.check_constraints(buf.data_ptr(), n_proofs, _st(), proof_stride=stride)
    buf[where] = s.dev[src]
    want, per = _expected(s, corr)
    return got, want, per


def _breaking(s, gates, role, value=lambda v: (v + 1) % ref.R):
    """The first gate of `gates` whose cell `role` (0 a, 1 x, 2 y, 3 d), set to value(old), fails that very gate by the reference: (cell, new value)."""
    for g in gates:
        g = int(g)
        c = g + role
        v = value(_old(s, c))
        cells = {g + t: _old(s, g + t) for t in range(4)}
        cells[c] = v
        if ref.bad_gates(cells, s.sel, s.n, gates=[g]) == 1:
            return c, v
    raise AssertionError("no such gate")


@pytest.mark.parametrize("mode", [1, 0])
def test_constraint_counts_are_exact_over_a_batch(valid_stream, mode):
    """Three proofs at proof_stride = num_cells + 5 with poisoned gaps, different corruptions in each (so a kernel that reads proof 0 three times, or drops
    the stride, miscounts), every count equal to the reference's: a gate's a, x, y and d cell; the first and the last gate, selector bits 0 and 7, a gate
    in the last selector byte; a d cell that is the next gate's a (two gates, one cell); cells moved by + r (congruent, no field elements: they count);
    looked-up cells at 2^bits exactly, at 2^bits - 1 (holds), with only a high limb set, at the first and the last registration."""
    s = valid_stream(mode, 6, 2, 2)
    buf, stride = _batch(s, 3, 5)
    assert s.plan.check_constraints(buf.data_ptr(), 3, _st(), proof_stride=stride) == (0, 0)
    cases = _batch_cases(s)
    for name, by_proof in cases.items():
        corr = {p: dict(cs) for p, cs in by_proof.items()}
        got, want, per = _check(s, buf, stride, 3, corr)
        print(f"mode {mode} {name}: device {got} reference {want} per proof {per}")
        assert got == want, (name, got, want, per)
        _batch_case_is_what_it_is_for(name, want, per)
    # every corruption above at once (where two cases write one cell the later wins, on the device as in the reference)
    corr = _all_at_once(cases)
    got, want, per = _check(s, buf, stride, 3, corr)
    print(f"mode {mode} everything at once: device {got} reference {want} per proof {per}")
    assert got == want and want[0] >= 12 and want[1] >= 6, (got, want, per)
    assert s.plan.check_constraints(buf.data_ptr(), 3, _st(), proof_stride=stride) == (0, 0)      # and the batch is as it was


def _all_at_once(cases):
    corr = {}
    for by_proof in cases.values():
        for p, cs in by_proof.items():
            corr.setdefault(p, {}).update(dict(cs))
    return corr


def _batch_case_is_what_it_is_for(name, want, per):
    """What a case's reference counts must look like for the case to test what its name says (the inputs' own properties, nothing of the device)."""
    if name in ("a/x/y/d", "+ r"):
        assert len({pg for pg, _ in per}) == 3 and min(pg for pg, _ in per) >= 1, (name, per)      # a different count in every proof
    if name == "lookups":
        assert [pl for _, pl in per] == [1, 2, 3], per
    if name == "d is the next gate's a":
        assert want[0] == 2, want
    if name in ("a + r alone", "last selector byte", "selector bit 0", "selector bit 7"):
        assert want[0] >= 1
    if name == "2^bits - 1 alone":
        assert want[1] == 0
    if name == "2^bits alone":
        assert want[1] == 1


def _batch_cases(s):
    """{case: {proof: [(cell, value), ...]}} for a stream of (6, 2, cap 2), chosen from the oracle's stream and lists alone."""
    g, n = s.gates, s.n
    last_byte = g[g // 8 == (n + 7) // 8 - 1]
    assert len(last_byte) >= 1, "the shape was chosen for a gate in its last selector byte"
    mid = len(g) // 2
    plus_r = lambda v: v + ref.R
    small = [int(x) for x in g[mid:mid + 4000] if _old(s, int(x)) + _old(s, int(x) + 1) * _old(s, int(x) + 2) < ref.R]      # a + r passes one conditional subtraction
    dbl = [int(x) for x in g[mid:mid + 4000] if s.is_gate[x + 3] and not s.is_gate[x + 1] and not s.is_gate[x + 2]]
    lk = s.lk
    cases = {
        "a/x/y/d": {0: [_breaking(s, g[:1], 0)], 1: [_breaking(s, g[g % 8 == 0][7:], 1), _breaking(s, g[g % 8 == 7][7:], 2)],
                    2: [_breaking(s, g[-1:], 3), _breaking(s, g[mid:], 3), _breaking(s, g[mid // 2:], 0), _breaking(s, g[mid // 3:], 2)]},
        "last selector byte": {2: [_breaking(s, last_byte[-1:], 0)]},
        "selector bit 0": {1: [_breaking(s, g[g % 8 == 0][-9:], 3)]},
        "selector bit 7": {2: [_breaking(s, g[g % 8 == 7][-9:], 3)]},
        "d is the next gate's a": {2: [(dbl[0] + 3, (_old(s, dbl[0] + 3) + 1) % ref.R)]},
        "+ r": {0: [_breaking(s, small, 0, plus_r)], 1: [_breaking(s, g[mid + 5000:], 1, plus_r), _breaking(s, g[mid + 6000:], 2, plus_r)],
                2: [_breaking(s, g[mid + 7000:], 3, plus_r), _breaking(s, g[:1], 0, plus_r), _breaking(s, g[-1:], 3, plus_r)]},
        "a + r alone": {1: [_breaking(s, small[1:], 0, plus_r)]},
        "lookups": {0: [(lk[0], 1 << BITS)], 1: [(lk[len(lk) // 2], (1 << BITS) - 1), (lk[len(lk) // 3], 1 << 192), (lk[len(lk) // 5], 1 << 64)],
                    2: [(lk[-1], 1 << BITS), (lk[1], 1 << 128), (lk[-2], (1 << 255) + 5)]},
        "2^bits - 1 alone": {2: [(lk[-1], (1 << BITS) - 1)]},
        "2^bits alone": {1: [(lk[-1], 1 << BITS)]},
    }
    return cases


def _pass_cases(s):
    """[(cell, value)] for the stream of (6, 1, cap 0) with Goldilocks caps: the last lane of the first pass, the start and the end of the later ones."""
    lk, g = s.lk, s.gates
    first_pass = g[g < ref.GATE_PASS_CELLS]
    assert first_pass[-1] // 8 == ref.GATE_PASS_CELLS // 8 - 1, "the last gate of the first pass belongs to its last lane"
    second = g[g >= ref.GATE_PASS_CELLS]
    singles = [_breaking(s, first_pass[-1:], 3), _breaking(s, second[:1], 3), _breaking(s, second[len(second) // 2:], 1), _breaking(s, g[-1:], 3)]
    singles += [(lk[j], 1 << BITS) for j in (ref.LOOKUP_PASS - 1, ref.LOOKUP_PASS, 2 * ref.LOOKUP_PASS - 1, 2 * ref.LOOKUP_PASS, 4 * ref.LOOKUP_PASS + 5, len(lk) - 1)]
    return singles


def test_constraint_counts_in_the_second_pass_of_the_grids(valid_stream):
    """One pass of k_check_gates covers 2048 x 256 selector bytes = 4,194,304 cells, one of k_check_lookups 1024 x 256 = 262,144 registrations.  The smallest
    Fibonacci shape the witness path is run at elsewhere whose stream exceeds both is (6, 1, cap 0) with Goldilocks caps.  Corruptions in the last lane of
    the first pass, at the start and the end of the later ones, alone and together; nothing of the stream is downloaded (the base is the oracle's)."""
    s = valid_stream(0, 6, 1, 0)
    n, lk, g = s.n, s.lk, s.gates
    print(f"stride-pass shape (6, 1, rate_bits 1, cap_height 0, Goldilocks caps): num_cells {n} num_lookups {len(lk)} gates {len(g)}")
    assert n > ref.GATE_PASS_CELLS and len(lk) > 4 * ref.LOOKUP_PASS
    buf, stride = s.dev.clone(), n
    assert s.plan.check_constraints(buf.data_ptr(), 1, _st()) == (0, 0)
    singles = _pass_cases(s)
    for c, v in singles:
        got, want, _ = _check(s, buf, stride, 1, {0: {c: v}})
        print(f"cell {c}: device {got} reference {want}")
        assert got == want and sum(want) >= 1, (c, got, want)
    got, want, _ = _check(s, buf, stride, 1, {0: dict(singles)})
    print(f"all {len(singles)}: device {got} reference {want}")
    assert got == want and want[0] >= 4 and want[1] == 6, (got, want)


def test_constraint_counts_on_a_status_4_stream(h2w, h2w_api, oracle, consts):
    """PoseidonBN254 caps, a hash of the proof set to r + 1: status 4, and the stream keeps an unreduced cell.  The device's counts over that stream are the
    reference's over all of it - where a gate reads the unreduced cell it fails, whatever the cell is congruent to."""
    import torch
    ko, kh = consts
    sh = h2w.fibonacci_shape(6, 1, cap_height=0, hash_mode=1); osh = oracle.fibonacci_shape(6, 1, cap_height=0, hash_mode=1)
    plan = h2w_api.Plan(sh, kh)
    pr = oracle.synth_proof(osh, 31)
    for j, w in enumerate(ref.to_limbs(ref.R + 1)):
        pr[j] = w                                  # trace_cap[0]
    d_proofs = torch.frombuffer(bytearray(bytes(pr)), dtype=torch.int64).cuda()
    adv = torch.zeros(plan.num_cells * 4, dtype=torch.int64, device="cuda")
    ws = torch.zeros(plan.workspace_bytes(1), dtype=torch.uint8, device="cuda")
    plan.run(d_proofs.data_ptr(), 1, adv.data_ptr(), ws.data_ptr(), _st())
    torch.cuda.synchronize()
    assert plan.status(ws.data_ptr(), 1, _st()) == [4]
    got = plan.check_constraints(adv.data_ptr(), 1, _st())
    cells = ref.ints(_host(adv))
    unreduced = [i for i, v in enumerate(cells) if v >= ref.R]
    sel = plan.selectors()
    touched = [gt for i in unreduced for gt in range(max(0, i - 3), i + 1) if sel[gt >> 3] >> (gt & 7) & 1]
    want = (ref.bad_gates(cells, sel, plan.num_cells), ref.bad_lookups(cells, plan.lookup_cells(), BITS))
    print(f"status-4 stream: {len(unreduced)} unreduced cells {unreduced[:6]}, gates reading one {len(touched)}; device {got} reference {want}")
    assert len(unreduced) >= 1
    assert got == want
    plan.close()


# ---------------------------------------------------------------- equalities: synthetic, no plan

def _equalities(h2w, buf, n, stride, n_proofs, pairs, cc, cv):
    """h2w_check_equalities on numpy lists (pairs int64/uint64 [m][2], cc [t], cv uint64 [t][4]); (rc, bad pairs, bad constants)."""
    bad = (C.c_uint64 * 2)(7, 7)
    pairs = np.ascontiguousarray(pairs, dtype=np.uint64); cc = np.ascontiguousarray(cc, dtype=np.uint64); cv = np.ascontiguousarray(cv, dtype=np.uint64)
    rc = h2w.lib().h2w_check_equalities(buf.data_ptr(), n, stride, n_proofs, pairs.ctypes.data if len(pairs) else None, len(pairs),
                                        cc.ctypes.data if len(cc) else None, cv.ctypes.data if len(cc) else None, len(cc), bad, _st())
    return rc, int(bad[0]), int(bad[1])


def test_equality_counts_are_exact(h2w):
    """2 x 262,144 + 37 items over 2 proofs of 4,096 cells at stride 4,100: two full passes of the 1024 x 256 grid and a tail.  About 1 % fail, with failures
    forced into the last lane of the first pass, both halves of the second and the last 37; some differ in limb 3 only; proof 1 differs from proof 0 in
    three cells, so its counts are others."""
    import torch
    rng = np.random.default_rng(20260519)
    n, stride, P = 4096, 4100, ref.EQUALITY_PASS
    total = 2 * P + 37
    n_pairs = 300000
    n_const = total - n_pairs
    pool = rng.integers(0, 1 << 64, size=(8, 4), dtype=np.uint64)
    pool[1] = pool[0]; pool[1, 3] ^= np.uint64(1 << 40)                     # classes 0 and 1 differ in limb 3 only
    cls = rng.integers(0, 8, n)
    members = [np.nonzero(cls == c)[0] for c in range(8)]
    cells = [pool[cls], pool[cls].copy()]
    for i in (5, 2048, 4095):
        cells[1][i, 3] ^= np.uint64(1)
    host = np.full((2 * stride, 4), np.uint64(ref.M64), dtype=np.uint64)
    host[:n] = cells[0]; host[stride:stride + n] = cells[1]
    buf = _dev(host)
    forced = np.array([P - 1, P, P + 1, P + P // 2 - 1, P + P // 2, 2 * P - 1, 2 * P, 2 * P + 17, total - 1, n_pairs - 1, n_pairs])
    fail = rng.random(total) < 0.01
    fail[forced] = True
    assert fail[P:P + P // 2].sum() > 100 and fail[P + P // 2:2 * P].sum() > 100 and fail[2 * P:].sum() >= 3
    first = rng.integers(0, n, total)                                      # the pair's first cell / the constant's cell
    limb3 = fail & (rng.random(total) < 0.3)
    limb3[forced[::2]] = True
    first[limb3] = members[0][rng.integers(0, len(members[0]), limb3.sum())]
    other = (cls[first] + np.where(fail, rng.integers(1, 8, total), 0)) % 8      # the class of the second cell / of the constant
    other[limb3] = 1
    second = np.empty(total, dtype=np.int64)
    for c in range(8):
        m = other == c
        second[m] = members[c][rng.integers(0, len(members[c]), m.sum())]
    pairs = np.stack([first[:n_pairs], second[:n_pairs]], axis=1)
    cc, cv = first[n_pairs:], pool[other[n_pairs:]]
    pl, ccl, cvl = [tuple(x) for x in pairs.tolist()], cc.tolist(), ref.ints(cv)
    per = [ref.bad_equalities(ref.ints(c), pl, ccl, cvl) for c in cells]
    print(f"equalities: {n_pairs} pairs + {n_const} constants, failing per proof {per}, designed to fail {int(fail.sum())}")
    assert per[0] == (int(fail[:n_pairs].sum()), int(fail[n_pairs:].sum()))      # proof 0 fails exactly where it was made to
    assert per[1][0] > per[0][0] and per[1][1] > per[0][1]
    want = (per[0][0] + per[1][0], per[0][1] + per[1][1])
    assert _equalities(h2w, buf, n, stride, 2, pairs, cc, cv) == (0,) + want
    assert _equalities(h2w, buf, n, stride, 1, pairs, cc, cv) == (0,) + per[0]
    assert _equalities(h2w, buf[stride:], n, stride, 1, pairs, cc, cv) == (0,) + per[1]
    assert _equalities(h2w, buf, n, stride, 2, pairs, cc[:0], cv[:0]) == (0, want[0], 0)          # pairs alone
    assert _equalities(h2w, buf, n, stride, 2, pairs[:0], cc, cv) == (0, 0, want[1])              # constants alone
    # one item: a pair that differs in limb 3 only; in proof 1 alone; a constant; a pair that holds
    a0, a1 = int(members[0][0]), int(members[1][0])
    assert _equalities(h2w, buf, n, stride, 2, [[a0, a1]], cc[:0], cv[:0]) == (0, 2, 0)
    same = int(members[cls[5]][members[cls[5]] != 5][0])
    assert _equalities(h2w, buf, n, stride, 2, [[5, same]], cc[:0], cv[:0]) == (0, 1, 0)
    assert _equalities(h2w, buf, n, stride, 2, pairs[:0], [4095], pool[cls[4095]][None]) == (0, 0, 1)
    assert _equalities(h2w, buf, n, stride, 2, [[a0, a0]], cc[:0], cv[:0]) == (0, 0, 0)
    # a cell index equal to n_cells is refused, in either list, wherever it stands
    bad_pairs = pairs.copy(); bad_pairs[-1, 1] = n
    assert _equalities(h2w, buf, n, stride, 2, bad_pairs, cc, cv)[0] == -1 and "equality refers to a cell outside the stream" in h2w.last_error()
    bad_cc = cc.copy(); bad_cc[-1] = n
    assert _equalities(h2w, buf, n, stride, 2, pairs, bad_cc, cv)[0] == -1 and "constant equality refers to a cell outside the stream" in h2w.last_error()
    bad_pairs[-1, 1] = n - 1
    assert _equalities(h2w, buf, n, stride, 2, bad_pairs, cc, cv)[0] == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------- columns: synthetic, no plan

def _columns(h2w, cells, stride, n_proofs, n, bp, k):
    """h2w_layout_columns of n_proofs streams of n cells laid at `stride` in poisoned memory into a poisoned output; uint64 [n_proofs][cols][2^k][4]."""
    import torch
    host = np.full((n_proofs * stride, 4), np.uint64(0x1111111111111111), dtype=np.uint64)
    for p in range(n_proofs):
        host[p * stride:p * stride + n] = cells[p]
    adv = _dev(host)
    out = torch.full((n_proofs * (len(bp) + 1) << k, 4), 0x2B2B2B2B2B2B2B2B, dtype=torch.int64, device="cuda")
    arr = (C.c_uint64 * max(len(bp), 1))(*bp)
    rc = h2w.lib().h2w_layout_columns(adv.data_ptr(), n, stride, n_proofs, arr if bp else None, len(bp), k, out.data_ptr(), _st())
    assert rc == 0, h2w.last_error()
    torch.cuda.synchronize()
    return _host(out).reshape(n_proofs, len(bp) + 1, 1 << k, 4)


@pytest.mark.parametrize("case", [dict(k=3, n=5, bp=[]), dict(k=3, n=8, bp=[]), dict(k=3, n=8, bp=[7]), dict(k=3, n=10, bp=[7]), dict(k=3, n=11, bp=[1, 1, 7]),
                                  dict(k=5, n=40, bp=[31, 5], proofs=3, stride=47), dict(k=5, n=63, bp=[31], proofs=3, stride=64),
                                  dict(k=5, n=40, bp=[1, 2, 3, 31], proofs=2, stride=43)],
                         ids=lambda c: "k%d-n%d-bp%s-p%d" % (c["k"], c["n"], "_".join(map(str, c["bp"])) or "none", c.get("proofs", 1)))
def test_columns_at_their_edges(h2w, case):
    """No break point; a column exactly 2^k long; a last column that is the repeated boundary cell alone; columns of two cells; three proofs at a stride
    beyond the stream - every byte of the poisoned output against the reference."""
    rng = np.random.default_rng(case["n"] * 131 + case["k"])
    k, n, bp, n_proofs = case["k"], case["n"], case["bp"], case.get("proofs", 1)
    cells = [rng.integers(1, 1 << 64, size=(n, 4), dtype=np.uint64) for _ in range(n_proofs)]
    got = _columns(h2w, cells, case.get("stride", n), n_proofs, n, bp, k)
    for p in range(n_proofs):
        want = ref.columns(cells[p], bp, k)
        assert np.array_equal(got[p], want), (case, p, np.nonzero((got[p] != want).any(axis=2)))
    if case["n"] == 8 and bp == [7]:
        assert (got[0, 1, 0] == cells[0][7]).all() and not got[0, 1, 1:].any()      # the boundary cell alone


def test_columns_beyond_one_pass_of_the_grid(h2w):
    """k = 20: a column is 2^21 half cells, the grid 4096 x 256 - two passes a column.  Two columns whose assigned prefixes end inside the second pass."""
    k = 20
    rng = np.random.default_rng(20)
    bp = [ref.COLUMN_PASS_ROWS + 175713]
    n = bp[0] + ref.COLUMN_PASS_ROWS + 75001
    cells = rng.integers(1, 1 << 64, size=(n, 4), dtype=np.uint64)
    got = _columns(h2w, [cells], n, 1, n, bp, k)[0]
    l0, l1 = bp[0] + 1, n - bp[0]
    assert l0 > ref.COLUMN_PASS_ROWS and l1 > ref.COLUMN_PASS_ROWS and max(l0, l1) < 1 << k
    assert np.array_equal(got[0, :l0], cells[:l0]) and not got[0, l0:].any()
    assert np.array_equal(got[1, 0], cells[bp[0]]) and np.array_equal(got[1, :l1], cells[bp[0]:]) and not got[1, l1:].any()
    assert np.array_equal(got, ref.columns(cells, bp, k))


def test_lookup_columns_against_the_reference(h2w, h2w_api, consts):
    """The smallest plan's registrations over random cells (every other cell poisoned): unusable_rows 0 and 9 on two proofs at a stride beyond the stream,
    and 1,000 - columns of 24 rows at k = 10, thousands of them, far more than one pass of the 4096 x 256 grid.  The size query agrees with the call."""
    import torch
    _, kh = consts
    k = 10
    plan = h2w_api.Plan(h2w.fibonacci_shape(6, 1, cap_height=0, hash_mode=1), kh)
    n, lk = plan.num_cells, np.array(plan.lookup_cells(), dtype=np.int64)
    stride = n + 3
    rng = np.random.default_rng(10)
    host = np.full((2 * stride, 4), np.uint64(0x3333333333333333), dtype=np.uint64)
    for p in range(2):
        host[p * stride + lk] = rng.integers(1, 1 << 64, size=(len(lk), 4), dtype=np.uint64)
    adv = _dev(host)
    for unusable, n_proofs in ((0, 2), (9, 2), (1000, 1)):
        want = [ref.lookup_columns(host[p * stride:p * stride + n], lk, k, unusable) for p in range(n_proofs)]
        ncols = want[0].shape[0]
        assert ncols == (len(lk) + (1 << k) - unusable - 1) // ((1 << k) - unusable)
        assert plan.num_lookup_columns(k, unusable) == ncols
        out = torch.full((n_proofs * ncols << k, 4), 0x4D4D4D4D4D4D4D4D, dtype=torch.int64, device="cuda")
        assert plan.layout_lookup_columns(adv.data_ptr(), n_proofs, k, out.data_ptr(), unusable_rows=unusable, stream=_st(), proof_stride=stride) == ncols
        torch.cuda.synchronize()
        got = _host(out).reshape(n_proofs, ncols, 1 << k, 4)
        print(f"lookup columns: unusable_rows {unusable}: {ncols} columns, {ncols << (k + 1)} half cells a proof (one pass: {2 * ref.LOOKUP_LAYOUT_PASS_CELLS})")
        for p in range(n_proofs):
            assert np.array_equal(got[p], want[p]), (unusable, p)
        if unusable == 1000:
            assert ncols > 2000 and ncols << (k + 1) > 2 * ref.LOOKUP_LAYOUT_PASS_CELLS
        del out, got, want
    plan.close()


# ---------------------------------------------------------------- digest and conversion: synthetic, no plan

def _digest(h2w, t, n):
    import torch
    out = torch.full((4,), 0x77, dtype=torch.int64, device="cuda")      # the call clears it
    assert h2w.lib().h2w_advice_digest(t.data_ptr(), n, out.data_ptr(), _st()) == 0, h2w.last_error()
    return [int(x) & ref.M64 for x in out.cpu().tolist()]


NS = [0, 1, 63, 64, 65, ref.DIGEST_PASS, ref.DIGEST_PASS + 1, 2 * ref.DIGEST_PASS + 1]


@pytest.mark.parametrize("kind", ["random", "ones"])
def test_digest_of_prefixes(h2w, kind):
    """n = 0, 1, around a wavefront, one pass of the 2048 x 256 grid exactly, one more, two passes and one - on random cells and on all-ones limbs, where
    every product and every sum wraps."""
    rng = np.random.default_rng(4)
    cells = rng.integers(0, 1 << 64, size=(NS[-1], 4), dtype=np.uint64) if kind == "random" else np.full((NS[-1], 4), np.uint64(ref.M64), dtype=np.uint64)
    t = _dev(cells)
    want = ref.digests(cells, NS)
    for n in NS:
        assert _digest(h2w, t, n) == want[n], n
    assert len({tuple(want[n]) for n in NS}) == len(NS)


def test_digest_depends_on_position_and_limb(h2w):
    rng = np.random.default_rng(5)
    cells = rng.integers(0, 1 << 64, size=(65, 4), dtype=np.uint64)
    seen = {}
    swapped = cells.copy(); swapped[[3, 64]] = swapped[[64, 3]]
    moved = cells.copy(); moved[7, 1], moved[7, 2] = cells[7, 2], cells[7, 1]
    shifted = cells.copy(); shifted[0, 0], shifted[0, 3] = cells[0, 3], cells[0, 0]
    for name, c in (("base", cells), ("cells 3 and 64 swapped", swapped), ("limbs 1 and 2 of cell 7 swapped", moved), ("limbs 0 and 3 of cell 0 swapped", shifted)):
        got = _digest(h2w, _dev(c), 65)
        assert got == ref.digest(c), name
        seen[name] = tuple(got)
    assert len(set(seen.values())) == 4, seen


def test_montgomery_conversion_is_exact(h2w):
    """Every cell becomes v 2^256 mod r: 0, 1, r - 1, 2^64, 2^128, 2^253 and random canonical values, over one pass of the 4096 x 256 grid and one cell more;
    n = 1, one pass exactly and one more leave the poisoned cell past n alone."""
    import torch
    rng = np.random.default_rng(6)
    N = ref.MONTGOMERY_PASS + 1
    special = [0, 1, ref.R - 1, 1 << 64, 1 << 128, 1 << 253, ref.R - 2, (1 << 253) + 1, ref.M64, (1 << 192) - 1]
    cells = rng.integers(0, 1 << 64, size=(N, 4), dtype=np.uint64)
    cells[:, 3] = rng.integers(0, ref.R >> 192, size=N, dtype=np.uint64)      # limb 3 below r's: canonical
    cells[:len(special)] = ref.pack(special)
    cells[-len(special):] = ref.pack(special[::-1])                               # and in the lanes of the second pass
    vals = ref.ints(cells)
    assert max(vals) < ref.R
    poison = np.full((1, 4), np.uint64(ref.M64), dtype=np.uint64)
    results = {}
    for n in (N, ref.MONTGOMERY_PASS, 1):
        t = _dev(np.concatenate([cells[:n], poison, cells[n + 1:]]) if n < N else np.concatenate([cells, poison]))
        assert h2w.lib().h2w_advice_to_montgomery(t.data_ptr(), n, _st()) == 0, h2w.last_error()
        torch.cuda.synchronize()
        results[n] = _host(t)
        assert (results[n][n] == poison[0]).all(), n                              # the neighbour past n is untouched
    got = ref.ints(results[N][:N])
    bad = [i for i, (v, g) in enumerate(zip(vals, got)) if g != ref.to_montgomery(v)]
    assert not bad, (len(bad), bad[:5])
    assert [got[i] for i in range(3)] == [0, (1 << 256) % ref.R, ref.R - (1 << 256) % ref.R]
    # the shorter calls: the same cells converted (checked above, cell by cell), the rest as it was
    for n in (ref.MONTGOMERY_PASS, 1):
        assert np.array_equal(results[n][:n], results[N][:n]) and np.array_equal(results[n][n + 1:], cells[n + 1:]), n
