"""What h2w_fri_verdict_batch must say about a proof, from the CPU oracle alone (tests/test_verdict_host.py, tests/test_gpu_verdict.py).

oracle.verify_stark runs on a keygen context (witness_gen_only=False), which records every copy constraint.  The constraints of the gadget's own
wiring hold for any proof (mock_prover()["bad"] == 0 is asserted), so a pair of ctx.equalities() whose two cells differ is one of the chips'
assert_equal calls on the proof: their number is the verdict's n_failed.  The PoW bit is expected exactly when a registered lookup cell
exceeds lookup_bits (the only lookup a proof can break is the proof-of-work range check, verifier.h:180).  That range check holds one copy
constraint of its own - the response against the sum of its limbs - which fails with it when the response does not fit the limbs: it is counted
like any failing pair and belongs to no query.

flags and first_query need every failing pair's check.  The semantic pairs are static per shape, and a uniformly random proof fails all of
them (semantic_map asserts the count the protocol gives: per query a root per tree, two words per fold step and two for the final
polynomial).  Sorted by their later cell they lie in program order - query by query; within a query the initial trees' roots, per fold step
its consistency check then its tree's root, then the final polynomial (fri/mod.rs:337-444) - so a pair's place names its query and its flag.
"""
import ctypes as C

import numpy as np

import pyoracle as O

POW, MERKLE_TRACE, MERKLE_PERM_Z, MERKLE_QUOTIENT, MERKLE_STEP, FOLD, FINAL = 1, 2, 4, 8, 16, 32, 64
NO_QUERY = 0xFFFFFFFF
GL_P = 0xFFFFFFFF00000001


def fold_steps(sh):
    """Fold steps of the shape (plonky2 FriParams, ConstantArityBits)."""
    db, n = sh.degree_bits, 0
    while db > sh.final_poly_bits and db + sh.rate_bits - sh.arity_bits >= sh.cap_height:
        db -= sh.arity_bits
        n += 1
    return n


def site_flags(sh):
    """The flag of every semantic pair of ONE query, in program order."""
    root = 4 if sh.hash_mode == 0 else 1      # a Goldilocks-Poseidon root is four words (hash/poseidon/hash.rs:148-159), a PoseidonBN254 root one
    trees = [MERKLE_TRACE, MERKLE_PERM_Z, MERKLE_QUOTIENT] if sh.n_perm_z > 0 else [MERKLE_TRACE, MERKLE_QUOTIENT]
    out = []
    for t in trees:
        out += [t] * root
    for _ in range(fold_steps(sh)):
        out += [FOLD] * 2 + [MERKLE_STEP] * root
    return out + [FINAL] * 2


def _u64s(ctx, count, fill, per):
    out = np.zeros(max(per * int(count(ctx.p)), 1), dtype=np.uint64)
    fill(ctx.p, out.ctypes.data)
    return out[:per * int(count(ctx.p))].astype(np.int64)


def oracle_run(osh, ko, proof, allow_internal=0, peek=None):
    """One oracle run: (failing pairs as an (n, 2) array, PoW bit, how many of the pairs are the gadget's own wiring).
    allow_internal: a proof with a word outside its field breaks the range check of that word's load (status 4 reports it; the reference's types
    cannot hold such a proof): only for such a proof may constraints of the wiring fail, and they must be copy constraints.
    peek: called with the advice array while it lives; what it returns is appended to the result."""
    buf = proof if not isinstance(proof, np.ndarray) else (C.c_uint64 * len(proof))(*[int(x) for x in proof])
    ctx = O.Ctx(osh.lookup_bits, witness_gen_only=False)
    try:
        assert O.verify_stark(ctx, osh, ko, buf) == 0, ctx.error()
        adv = ctx.advice_array()
        eq = _u64s(ctx, ctx.L.orc_num_equalities, ctx.L.orc_equalities, 2).reshape(-1, 2)      # (ctx.equalities(), without a Python tuple per pair)
        failing = eq[(adv[eq[:, 0]] != adv[eq[:, 1]]).any(axis=1)].copy()
        mp = ctx.mock_prover()
        assert mp["bad"] <= allow_internal, mp      # every failing pair is a semantic one
        lk = adv[_u64s(ctx, ctx.L.orc_num_lookups, ctx.L.orc_lookup_cells, 1)]      # (ctx.lookup_cells())
        bad_lk = int(((lk[:, 1:] != 0).any(axis=1) | ((lk[:, 0] >> np.uint64(osh.lookup_bits)) != 0)).sum())
        assert mp["semantic_failed"] == len(failing) - mp["bad"] + bad_lk, (mp, len(failing), bad_lk)      # the wiring's failures are pairs, the failing lookups the PoW's
        return (failing, bad_lk > 0, mp["bad"]) + ((peek(adv),) if peek else ())
    finally:
        ctx.close()


def semantic_map(osh, failing_of_random, pow_bit_of_random, internal=0):
    """{later cell of a chip-level semantic pair: (query, flag)} from oracle_run's result for a uniformly random proof of the shape.
    One more pair can fail in front of them, in the prologue: RangeChip::range_check constrains the PoW response to equal
    the sum of its ceil((64 - pow_bits) / lookup_bits) limbs, which a response too large for those limbs breaks (with the lookup, so only under the PoW bit)."""
    assert internal == 0
    per_q = site_flags(osh)
    later = np.sort(failing_of_random.max(axis=1))
    assert len(set(later.tolist())) == len(later)
    extra = len(later) - osh.num_queries * len(per_q)
    assert extra == 0 or (extra == 1 and pow_bit_of_random), (len(later), osh.num_queries, len(per_q), pow_bit_of_random)
    later = later[extra:]
    return {int(c): (i // len(per_q), per_q[i % len(per_q)]) for i, c in enumerate(later)}


def expected(osh, ko, proof, smap, allow_internal=0):
    """(flags, n_failed, first_query) of one proof; status is the witness call's business (h2w_plan_status).  n_failed counts the semantic pairs."""
    return verdict_of(smap, *oracle_run(osh, ko, proof, allow_internal))


def verdict_of(smap, failing, pow_bit, internal):
    flags, first, unowned = (POW if pow_bit else 0), NO_QUERY, 0
    for a, b in failing.tolist():
        if max(a, b) in smap:
            q, f = smap[max(a, b)]
            flags |= f
            first = min(first, q)
        else:      # in front of the query rounds: the PoW response against its limb sum, or (allow_internal) the load of the word outside its field
            assert max(a, b) < min(smap), (a, b)
            unowned += 1
    assert unowned - internal in ((0, 1) if pow_bit else (0,)), (unowned, internal, pow_bit)
    return flags, len(failing) - internal, first


def expected_many(osh, ko, proofs, smap, workers=8, allow_internal=()):
    """expected() of several proofs.  The oracle runs side by side (a keygen run of one small proof takes seconds with Goldilocks caps; the
    library holds no state between contexts once it has run once, which building smap has seen to); equal proofs are run once."""
    from concurrent.futures import ThreadPoolExecutor
    keys = [bytes(p) if not isinstance(p, np.ndarray) else p.tobytes() for p in proofs]
    uniq = {}
    for i, (k, p) in enumerate(zip(keys, proofs)):
        uniq.setdefault(k, (p, 1 if i in allow_internal else 0))      # allow_internal: indices of the proofs with a word outside its field
    with ThreadPoolExecutor(max_workers=workers) as ex:
        res = dict(zip(uniq, ex.map(lambda pa: expected(osh, ko, pa[0], smap, pa[1]), uniq.values())))
    return [res[k] for k in keys]


def shape_pair(h2w, oracle, mode, degree_bits=6, queries=2, rate_bits=1, cap_height=2, **over):
    """(product shape, oracle shape): fibonacci_shape with fields overridden."""
    sh = h2w.fibonacci_shape(degree_bits, queries, rate_bits=rate_bits, cap_height=cap_height, hash_mode=mode)
    osh = oracle.fibonacci_shape(degree_bits, queries, rate_bits=rate_bits, cap_height=cap_height, hash_mode=mode)
    for k, v in over.items():
        setattr(sh, k, v); setattr(osh, k, v)
    return sh, osh


def bump(words, at):
    """A copy of the proof with word `at` + 1 mod p."""
    c = words.copy()
    c[at] = (int(c[at]) + 1) % GL_P
    return c


def sibling_word(layout, q, tree, j):
    """First word of sibling j of `tree` (an entry of layout["oracles"] or layout["steps"]) of query q."""
    return layout["queries"] + q * layout["query_words"] + tree["off"] + tree["leaf"] + 4 * j


def selected_eval(adv0, valid, smap, layout, q, step):
    """The index, among fold step `step`'s evaluations of query q, of the one the query's index selects - read off the oracle's run of the
    valid proof (adv0: the low words of its advice): the fold step's consistency check compares the selected evaluation, and its cells show it."""
    cells = sorted(c for c, (qq, f) in smap.items() if qq == q and f == FOLD)[2 * step:2 * step + 2]
    want = [int(adv0[c]) for c in cells]
    t = layout["steps"][step]
    ew = layout["queries"] + q * layout["query_words"] + t["off"]
    hits = [k for k in range(t["leaf"] // 2) if [int(valid[ew + 2 * k]), int(valid[ew + 2 * k + 1])] == want]
    assert len(hits) == 1, hits
    return hits[0]


def build_batch(osh, ko, layout, prove_seed=77, random_seed=5, workers=16):
    """The batch of one shape (tests/test_gpu_verdict.py): the names and words of its proofs, their expected (flags, n_failed, first_query), the
    indices of the proofs with a word outside its field, and for every sibling corruption {batch index: (its tree's flag, its query)}.
    Every corruption is +1 mod p on one word of the valid proof.  The oracle runs go side by side: first the two everything rests on - the random
    proof's (the semantic map) and the valid proof's (its advice says which evaluation a query selects) -, then the others'."""
    from concurrent.futures import ThreadPoolExecutor
    valid = np.frombuffer(bytes(O.prove_fri(osh, ko, prove_seed)), dtype=np.uint64)
    rand = np.frombuffer(bytes(O.synth_proof(osh, random_seed)), dtype=np.uint64)
    with ThreadPoolExecutor(max_workers=workers) as ex:
        f_rand = ex.submit(oracle_run, osh, ko, rand)
        f_valid = ex.submit(oracle_run, osh, ko, valid, 0, lambda adv: adv[:, 0].copy())
        run_rand, run_valid = f_rand.result(), f_valid.result()
        smap = semantic_map(osh, *run_rand)
        L, nq = layout, osh.num_queries
        qbase = lambda q: L["queries"] + q * L["query_words"]
        trees = L["oracles"] + L["steps"]
        tree_flags = ([MERKLE_TRACE, MERKLE_PERM_Z, MERKLE_QUOTIENT] if osh.n_perm_z > 0 else [MERKLE_TRACE, MERKLE_QUOTIENT]) + [MERKLE_STEP] * len(L["steps"])
        names, words, siblings = ["valid"], [valid], {}
        add = lambda name, w: (names.append(name), words.append(w))
        for i, (t, f) in enumerate(zip(trees, tree_flags)):      # a sibling of each tree: queries, levels and words of the hash in turn
            if t["sibs"] == 0:
                continue
            q, j = i % nq, (i * 3) % t["sibs"]
            siblings[len(words)] = (f, q)
            add(f"sibling {j} of tree {i} of query {q}", bump(valid, sibling_word(L, q, t, j) + i % 4))
        add("initial leaf word", bump(valid, qbase(nq - 1) + L["oracles"][-1]["off"]))
        if L["steps"]:      # the last step: the consistency check of the selected evaluation fails in that step itself
            s = len(L["steps"]) - 1
            k = selected_eval(run_valid[3], valid, smap, L, 0, s)
            ew = qbase(0) + L["steps"][s]["off"]
            add("step evaluation at the selected index", bump(valid, ew + 2 * k))
            add("step evaluation off the selected index", bump(valid, ew + 2 * ((k + 1) % (L["steps"][s]["leaf"] // 2)) + 1))
        add("final-polynomial coefficient", bump(valid, L["final_poly"] + 1))
        add("PoW witness", bump(valid, L["pow_witness"]))
        caps = [("trace cap", L["trace_cap"]), ("quotient cap", L["quotient_cap"])] + ([("permutation cap", L["perm_cap"])] if osh.n_perm_z > 0 else [])
        caps += [(f"commit cap {i}", L["commit_caps"] + 4 * L["cap_size"] * i) for i in range(len(L["steps"]))]
        for i, (name, w) in enumerate(caps):
            add(name + " word", bump(valid, w + (5 * i + 1) % (4 * L["cap_size"])))
        i_rand = len(words); add("random", rand)
        outside = valid.copy(); outside[L["openings"] + 3] = GL_P + 2
        noncanonical = {len(words)}; add("a Goldilocks word >= p", outside)
        add("valid again", valid)
        known = {0: verdict_of(smap, *run_valid[:3]), i_rand: verdict_of(smap, *run_rand), len(words) - 1: verdict_of(smap, *run_valid[:3])}
        todo = [i for i in range(len(words)) if i not in known]
        for i, v in zip(todo, ex.map(lambda i: expected(osh, ko, words[i], smap, 1 if i in noncanonical else 0), todo)):
            known[i] = v
    return names, words, [known[i] for i in range(len(words))], noncanonical, siblings
