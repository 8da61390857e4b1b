#!/usr/bin/env python3
"""Trace h2w_chip_verify_stark once, lower it, replay it on --batch proofs: wall time per launch (and, under rocprofv3 --kernel-trace, the duration of
every k_replay dispatch: one per template, depth by depth).  usage: replay_timing.py [--config cfg3] [--hash bn254|gl] [--batch 64] [--reps 2]
--world W --rank R: after the unsharded launches of --batch proofs, what rank R of W runs: a launch of W x batch proofs into its packed buffer
(h2w_fri_witness_batch_shard_compact) - its own-cell rate beside the unsharded rate, and whether the buffer equals the compiled plan's packed buffer.
--fuse: BOTH plans from the one trace - h2w_plan_from_trace and h2w_plan_from_trace_ex with H2W_TRACE_FUSE_GL_PERMUTE - in one process: for each, ms per
launch, cells/s, the time of every kernel of a launch (h2w_plan_trace_timing: k_replay depth by depth, the permutation records' kernel, the expansion),
one proof enqueue to completion, and whether the two streams are equal.  --out FILE: the JSON lines appended to FILE as well.
--fuse-bn: THREE plans from the one trace - unfused, H2W_TRACE_FUSE_GL_PERMUTE, and both flags (H2W_TRACE_FUSE_BN_PERMUTE as well) - in one process: the
same figures for each (the third reports the PoseidonBN254 emission kernel too), and whether proof 0's h2w_advice_digest is equal across the three.
--form montgomery: the hand-off in halo2curves' form, three routes in one process on plans with both fuse flags: (a) the canonical stream, (b) the
canonical stream followed by h2w_advice_to_montgomery over it - both on a plan lowered WITHOUT H2W_TRACE_OUTPUT_FORMS, the kernels as they were before
that flag -, (c) H2W_OPT_OUTPUT_FORM = Montgomery on a plan lowered with it, (c') the same with the fused PoseidonBN254 permutations' cells emitted
canonical and converted by the ranged kernel (the emitter's Montgomery instantiation switched off: H2W_TRACE_BN_RANGED in the environment at lowering).  Per route and repetition: ms of the whole call (enqueue to completion) and
of every kernel (h2w_plan_trace_timing), the spread of the repetitions, and whether (c) wrote the bytes of (b)."""
import argparse, importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = {"cfg1": (10, 4, 1), "cfg2": (16, 28, 2), "cfg3": (20, 28, 1), "cfg5": (20, 84, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3"); ap.add_argument("--hash", default="bn254"); ap.add_argument("--batch", type=int, default=64); ap.add_argument("--reps", type=int, default=2); ap.add_argument("--streams", type=int, default=1)
    ap.add_argument("--world", type=int, default=1); ap.add_argument("--rank", type=int, default=0)
    ap.add_argument("--fuse", action="store_true"); ap.add_argument("--fuse-bn", action="store_true"); ap.add_argument("--out", default=None)
    ap.add_argument("--form", default="canonical", choices=["canonical", "montgomery"])
    a = ap.parse_args()
    import numpy as np
    import torch
    h2w = importlib.import_module("halo2-plonky2-verifier_amd"); api = importlib.import_module("halo2-plonky2-verifier_amd.api")
    d, q, rb = CONFIGS[a.config]
    sh = h2w.fibonacci_shape(d, q, rate_bits=rb, hash_mode=1 if a.hash == "bn254" else 0)
    k = h2w.published_consts()
    ref = api.Plan(sh, k, 0)
    words = ref.proof_words
    prng = np.random.default_rng(7)
    host = prng.integers(0, 1 << 60, a.batch * max(a.world, 1) * words, dtype=np.int64)
    ctx = api.Context(21, True, 0); ctx.trace_begin()
    t0 = time.perf_counter(); api.verify_stark(ctx, sh, k, host[:words].astype(np.uint64)); t1 = time.perf_counter()
    plan = api.Plan.from_trace(ctx, words); t2 = time.perf_counter()
    fused = api.Plan.from_trace(ctx, words, fuse_consts=k) if a.fuse or a.fuse_bn else None; t3 = time.perf_counter()
    fused_bn = api.Plan.from_trace(ctx, words, fuse_consts=k, fuse_bn=True) if a.fuse_bn or a.form == "montgomery" else None; t4 = time.perf_counter()
    forms = api.Plan.from_trace(ctx, words, fuse_consts=k, fuse_bn=True, output_forms=True) if a.form == "montgomery" else None; t5 = time.perf_counter()
    forms_ranged = None
    if a.form == "montgomery":      # (c'): the same lowering with the fused permutations' cells left to the ranged kernel (csrc/plan.h trace_bn_ranged)
        os.environ["H2W_TRACE_BN_RANGED"] = "1"
        forms_ranged = api.Plan.from_trace(ctx, words, fuse_consts=k, fuse_bn=True, output_forms=True)
        del os.environ["H2W_TRACE_BN_RANGED"]
    ctx.close()
    proofs = torch.from_numpy(host).cuda()      # (the unsharded launches take the first --batch)
    if a.form == "montgomery":
        montgomery_report(a, api, torch, fused_bn, forms, forms_ranged, proofs, {"trace_s": round(t1 - t0, 3), "lower_fused_gl_bn_s": round(t4 - t3, 3), "lower_output_forms_s": round(t5 - t4, 3)})
        return
    if a.fuse_bn:
        fuse_bn_report(a, torch, [("unfused", plan), ("fused_gl", fused), ("fused_gl_bn", fused_bn)], proofs,
                       {"trace_s": round(t1 - t0, 3), "lower_s": round(t2 - t1, 3), "lower_fused_gl_s": round(t3 - t2, 3), "lower_fused_gl_bn_s": round(t4 - t3, 3)})
        return
    if a.fuse:
        fuse_report(a, torch, plan, fused, proofs, {"trace_s": round(t1 - t0, 3), "lower_s": round(t2 - t1, 3), "lower_fused_s": round(t3 - t2, 3)})
        return
    adv = torch.empty(a.batch * plan.num_cells * 32, dtype=torch.uint8, device="cuda"); ws = torch.zeros(plan.workspace_bytes(a.batch), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    if a.streams > 1:      # launches in flight: the root kernel of one (two wavefronts) runs beside the other's Merkle lanes
        strs = [torch.cuda.Stream() for _ in range(a.streams)]
        advs = [adv] + [torch.empty_like(adv) for _ in range(a.streams - 1)]; wss = [ws] + [torch.zeros_like(ws) for _ in range(a.streams - 1)]
        for j in range(a.streams):
            plan.run(proofs.data_ptr(), a.batch, advs[j].data_ptr(), wss[j].data_ptr(), strs[j].cuda_stream)
        torch.cuda.synchronize(); t = time.perf_counter(); nl = 3 * a.streams
        for j in range(nl):
            plan.run(proofs.data_ptr(), a.batch, advs[j % a.streams].data_ptr(), wss[j % a.streams].data_ptr(), strs[j % a.streams].cuda_stream)
        torch.cuda.synchronize(); dt = time.perf_counter() - t
        print(json.dumps({"config": a.config, "hash": a.hash, "batch": a.batch, "streams": a.streams, "launches": nl, "ms_per_launch": round(dt / nl * 1e3, 2), "G_cells_per_s": round(plan.num_cells * a.batch * nl / dt / 1e9, 2)}))
        del advs, wss
    ms = []
    for i in range(a.reps + 1):
        torch.cuda.synchronize(); t = time.perf_counter()
        plan.run(proofs.data_ptr(), a.batch, adv.data_ptr(), ws.data_ptr(), st)
        torch.cuda.synchronize(); ms.append((time.perf_counter() - t) * 1e3)
    assert plan.status(ws.data_ptr(), a.batch, st) == [0] * a.batch
    # tie to the compiled plan's stream of proof 0
    chk = torch.empty(ref.num_cells * 32, dtype=torch.uint8, device="cuda"); cws = torch.zeros(ref.workspace_bytes(1), dtype=torch.uint8, device="cuda")
    ref.run(proofs.data_ptr(), 1, chk.data_ptr(), cws.data_ptr(), st); torch.cuda.synchronize()
    unsharded_rate = plan.num_cells * a.batch / (min(ms[1:]) * 1e-3) / 1e9
    print(json.dumps({"config": a.config, "hash": a.hash, "batch": a.batch, "trace_s": round(t1 - t0, 3), "lower_s": round(t2 - t1, 3), "records": plan.num_records, "ws_GB": round(plan.workspace_bytes(a.batch) / 1e9, 2),
                      "ms_per_launch": [round(x, 2) for x in ms[1:]], "G_cells_per_s": round(unsharded_rate, 2), "proof0_equals_compiled_plan": bool(torch.equal(chk, adv[:ref.num_cells * 32]))}))
    if a.world > 1:
        del adv, ws, chk, cws
        n, W, R = a.batch * a.world, a.world, a.rank
        cells = plan.shard_cells(n, R, W)
        buf = torch.zeros((cells, 4), dtype=torch.int64, device="cuda"); ws = torch.zeros(plan.shard_workspace_bytes(n, R, W), dtype=torch.uint8, device="cuda")
        ms = []
        for i in range(a.reps + 1):
            torch.cuda.synchronize(); t = time.perf_counter()
            plan.run_shard_compact(proofs.data_ptr(), n, buf.data_ptr(), ws.data_ptr(), R, W, st)
            torch.cuda.synchronize(); ms.append((time.perf_counter() - t) * 1e3)
        ok = plan.status(ws.data_ptr(), n, st) == [0] * n
        del ws
        want = torch.zeros_like(buf); cws = torch.zeros(ref.shard_workspace_bytes(n, R, W), dtype=torch.uint8, device="cuda")
        ref.run_shard_compact(proofs.data_ptr(), n, want.data_ptr(), cws.data_ptr(), R, W, st); torch.cuda.synchronize()      # (both zeroed: the slack of a query slot is written by neither)
        own_rate = cells / (min(ms[1:]) * 1e-3) / 1e9
        print(json.dumps({"config": a.config, "hash": a.hash, "world": W, "rank": R, "proofs_per_launch": n, "own_cells": cells, "ms_per_launch": [round(x, 2) for x in ms[1:]],
                          "own_G_cells_per_s": round(own_rate, 2), "unsharded_G_cells_per_s": round(unsharded_rate, 2), "ratio": round(own_rate / unsharded_rate, 3), "status_ok": ok,
                          "packed_equals_compiled_plan": bool(torch.equal(buf, want))}))


def fuse_report(a, torch, plan, fused, proofs, times):
    st = torch.cuda.current_stream().cuda_stream
    lines = [dict(config=a.config, hash=a.hash, batch=a.batch, reps=a.reps, cells_per_proof=plan.num_cells, trace_info=fused.trace_info(), **times)]
    streams = []
    for name, pl in (("unfused", plan), ("fused", fused)):
        adv = torch.empty(a.batch * pl.num_cells * 32, dtype=torch.uint8, device="cuda"); ws = torch.zeros(pl.workspace_bytes(a.batch), dtype=torch.uint8, device="cuda")
        pl.trace_timing()                                  # events on
        ms, kern = [], []
        for i in range(a.reps + 1):                        # (the first launch is the warm-up)
            torch.cuda.synchronize(); t = time.perf_counter()
            pl.run(proofs.data_ptr(), a.batch, adv.data_ptr(), ws.data_ptr(), st)
            torch.cuda.synchronize(); ms.append((time.perf_counter() - t) * 1e3); kern.append(pl.trace_timing())
        assert pl.status(ws.data_ptr(), a.batch, st) == [0] * a.batch
        one = []
        for i in range(a.reps + 1):                        # one proof, enqueue to completion
            torch.cuda.synchronize(); t = time.perf_counter()
            pl.run(proofs.data_ptr(), 1, adv.data_ptr(), ws.data_ptr(), st)
            torch.cuda.synchronize(); one.append((time.perf_counter() - t) * 1e3)
        pl.run(proofs.data_ptr(), a.batch, adv.data_ptr(), ws.data_ptr(), st); torch.cuda.synchronize()
        streams.append(adv)
        nd = len(kern[0]) - 2                              # k_replay launches (one per depth), then the records' kernel, then the expansion
        lines.append({"plan": name, "records": pl.num_records, "ws_GB": round(pl.workspace_bytes(a.batch) / 1e9, 3), "ms_per_launch": [round(x, 3) for x in ms[1:]],
                      "G_cells_per_s": [round(pl.num_cells * a.batch / (x * 1e-3) / 1e9, 3) for x in ms[1:]],
                      "k_replay_ms_by_depth": [[round(x, 3) for x in kk[:nd]] for kk in kern[1:]], "glp_emit_ms": [round(kk[nd], 3) for kk in kern[1:]],
                      "expand_ms": [round(kk[nd + 1], 3) for kk in kern[1:]], "one_proof_ms": [round(x, 3) for x in one[1:]]})
    lines.append({"streams_equal": bool(torch.equal(streams[0], streams[1]))})
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


def fuse_bn_report(a, torch, plans, proofs, times):
    st = torch.cuda.current_stream().cuda_stream
    last = plans[-1][1]
    lines = [dict(config=a.config, hash=a.hash, batch=a.batch, reps=a.reps, cells_per_proof=last.num_cells, trace_info=last.trace_info(), trace_info_bn=last.trace_info_bn(), **times)]
    digests = []
    for name, pl in plans:
        adv = torch.empty(a.batch * pl.num_cells * 32, dtype=torch.uint8, device="cuda"); ws = torch.zeros(pl.workspace_bytes(a.batch), dtype=torch.uint8, device="cuda")
        pl.trace_timing()                                  # events on
        ms, kern = [], []
        for i in range(a.reps + 1):                        # (the first launch is the warm-up)
            torch.cuda.synchronize(); t = time.perf_counter()
            pl.run(proofs.data_ptr(), a.batch, adv.data_ptr(), ws.data_ptr(), st)
            torch.cuda.synchronize(); ms.append((time.perf_counter() - t) * 1e3); kern.append(pl.trace_timing())
        assert pl.status(ws.data_ptr(), a.batch, st) == [0] * a.batch
        one = []
        for i in range(a.reps + 1):                        # one proof, enqueue to completion
            torch.cuda.synchronize(); t = time.perf_counter()
            pl.run(proofs.data_ptr(), 1, adv.data_ptr(), ws.data_ptr(), st)
            torch.cuda.synchronize(); one.append((time.perf_counter() - t) * 1e3)
        dg = torch.zeros(4, dtype=torch.int64, device="cuda")
        pl.advice_digest(adv.data_ptr(), pl.num_cells, dg.data_ptr(), st); torch.cuda.synchronize()
        digests.append([int(x) & 0xFFFFFFFFFFFFFFFF for x in dg.cpu().tolist()])
        bn = name == "fused_gl_bn"                         # k_replay launches (one per depth), the records' kernel, (the PoseidonBN254 emission,) the expansion
        nd = len(kern[0]) - (3 if bn else 2)
        ln = {"plan": name, "records": pl.num_records, "ws_GB": round(pl.workspace_bytes(a.batch) / 1e9, 3), "ms_per_launch": [round(x, 3) for x in ms[1:]],
              "G_cells_per_s": [round(pl.num_cells * a.batch / (x * 1e-3) / 1e9, 3) for x in ms[1:]],
              "k_replay_ms_by_depth": [[round(x, 3) for x in kk[:nd]] for kk in kern[1:]], "glp_emit_ms": [round(kk[nd], 3) for kk in kern[1:]]}
        if bn:
            ln["bn_emit_ms"] = [round(kk[nd + 1], 3) for kk in kern[1:]]
        ln["expand_ms"] = [round(kk[-1], 3) for kk in kern[1:]]; ln["one_proof_ms"] = [round(x, 3) for x in one[1:]]; ln["proof0_digest"] = ["%016x" % x for x in digests[-1]]
        lines.append(ln)
        del adv, ws
    lines.append({"proof0_digests_equal": digests[0] == digests[1] == digests[2]})
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    assert lines[-1]["proof0_digests_equal"], "the three plans' streams of proof 0 differ"


def montgomery_report(a, api, torch, base, forms, forms_ranged, proofs, times):
    st = torch.cuda.current_stream().cuda_stream
    n, cells = a.batch, a.batch * base.num_cells
    assert forms.num_cells == base.num_cells and forms.workspace_bytes(n) == base.workspace_bytes(n)
    adv = torch.empty(cells * 32, dtype=torch.uint8, device="cuda"); ws = torch.zeros(base.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    lines = [dict(config=a.config, hash=a.hash, batch=n, reps=a.reps, cells_per_launch=cells, trace_info_bn=base.trace_info_bn(),
                  record_cells_per_proof=forms.num_record_cells, direct_cells_per_proof=forms.num_cells - forms.num_record_cells, **times)]
    forms.set_output_form(api.FORM_MONTGOMERY); forms_ranged.set_output_form(api.FORM_MONTGOMERY)
    keep = {}
    for route, pl, second_pass in (("a_canonical", base, False), ("b_canonical_then_second_pass", base, True), ("c_montgomery_form", forms, False),
                                   ("c_ranged_pass_for_fused_cells", forms_ranged, False)):
        pl.trace_timing()                                  # events on
        ms, kern = [], []
        for i in range(a.reps + 1):                        # (the first launch is the warm-up)
            torch.cuda.synchronize(); t = time.perf_counter()
            pl.run(proofs.data_ptr(), n, adv.data_ptr(), ws.data_ptr(), st)
            if second_pass:
                assert pl.L.h2w_advice_to_montgomery(adv.data_ptr(), cells, st) == 0
            torch.cuda.synchronize(); ms.append((time.perf_counter() - t) * 1e3); kern.append(pl.trace_timing())
        assert pl.status(ws.data_ptr(), n, st) == [0] * n
        keep[route] = adv[:base.num_cells * 32].clone()    # proof 0
        with_direct = pl is not base                          # k_replay depth by depth, the records' kernel, the PoseidonBN254 emission, (the direct cells' conversion,) the expansion
        nd = len(kern[0]) - (4 if with_direct else 3)
        ln = {"route": route, "ms_per_call": [round(x, 3) for x in ms[1:]], "ms_per_call_min": round(min(ms[1:]), 3), "ms_per_call_spread": round(max(ms[1:]) - min(ms[1:]), 3),
              "k_replay_ms_by_depth": [[round(x, 3) for x in kk[:nd]] for kk in kern[1:]], "glp_emit_ms": [round(kk[nd], 3) for kk in kern[1:]],
              "bn_emit_ms": [round(kk[nd + 1], 3) for kk in kern[1:]]}
        if with_direct:
            ln["direct_to_montgomery_ms"] = [round(kk[nd + 2], 3) for kk in kern[1:]]
        ln["expand_ms"] = [round(kk[-1], 3) for kk in kern[1:]]
        lines.append(ln)
    a_ms, b_ms, c_ms, cr_ms = (lines[i] for i in (1, 2, 3, 4))
    spread = max(b_ms["ms_per_call_spread"], c_ms["ms_per_call_spread"], cr_ms["ms_per_call_spread"])
    lines.append({"proof0_c_equals_b": bool(torch.equal(keep["c_montgomery_form"], keep["b_canonical_then_second_pass"])),
                  "proof0_c_ranged_equals_b": bool(torch.equal(keep["c_ranged_pass_for_fused_cells"], keep["b_canonical_then_second_pass"])),
                  "c_ranged_minus_c_ms": round(cr_ms["ms_per_call_min"] - c_ms["ms_per_call_min"], 3),
                  "c_below_c_ranged_by_more_than_the_spread": cr_ms["ms_per_call_min"] - c_ms["ms_per_call_min"] > spread,
                  "proof0_b_differs_from_a": not bool(torch.equal(keep["a_canonical"], keep["b_canonical_then_second_pass"])),
                  "c_over_b": round(c_ms["ms_per_call_min"] / b_ms["ms_per_call_min"], 3), "b_minus_c_ms": round(b_ms["ms_per_call_min"] - c_ms["ms_per_call_min"], 3),
                  "spread_ms": spread, "c_below_b_by_more_than_the_spread": b_ms["ms_per_call_min"] - c_ms["ms_per_call_min"] > spread})
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    assert lines[-1]["proof0_c_equals_b"], "the Montgomery form's stream of proof 0 is not the converted canonical stream"


if __name__ == "__main__":
    main()
