#!/usr/bin/env python3
"""What a verdict of a TRACED plan costs (h2w_trace_verdict_batch, include/h2w.h 2d) on cfg 3 (2^20 rows, 28 queries) with PoseidonBN254 caps, on
batches of valid proofs made on the device (h2w_prove_fri_batch from random polynomials), each call alone on the chip, one process per plan:
  verdict_ms    h2w_trace_verdict_batch                                              device events around the call
  witness_ms    h2w_fri_witness_batch of the same plan on the same batch             device events around the call; witness_kernels_ms: h2w_plan_trace_timing
                                                                                     (k_replay depth by depth, the emission kernels, the expansion)
  route_ms      the verdict a traced plan had before: the stream, then h2w_check_equalities over the traced plan's keygen lists (uploaded by the call) and
                h2w_check_constraints                                                wall clock between device synchronisations (both checks synchronise)
  compiled_verdict_ms   as context: h2w_fri_verdict_batch of the compiled plan of the shape on the same proofs
--plan unfused | fused: h2w_plan_from_trace, or h2w_plan_from_trace_ex with H2W_TRACE_FUSE_GL_PERMUTE | H2W_TRACE_FUSE_BN_PERMUTE.  A warm-up, then --reps
calls: the median and the spread (max - min).  The one condition the figures are held to: verdict_ms <= witness_ms + the larger of the two spreads
("verdict_within_witness").  The result is merged into --out under the plan's name."""
import argparse, ctypes as C, importlib, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
h2w = importlib.import_module("halo2-plonky2-verifier_amd"); api = importlib.import_module("halo2-plonky2-verifier_amd.api")

ap = argparse.ArgumentParser()
ap.add_argument("--plan", default="unfused", choices=["unfused", "fused"])
ap.add_argument("--batches", default="1,64")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--route", default="yes", choices=["yes", "no"])
ap.add_argument("--degree-bits", type=int, default=20); ap.add_argument("--queries", type=int, default=28)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_verdict_cfg3.json"))
args = ap.parse_args()
kh = h2w.published_consts(); med = statistics.median
stat = lambda ms: {"median": round(med(ms), 4), "spread": round(max(ms) - min(ms), 4), "all": [round(x, 4) for x in ms]}

sh = h2w.fibonacci_shape(args.degree_bits, args.queries, hash_mode=1)
cplan = api.Plan(sh, kh); pr = api.Prover(sh, kh)
words = cplan.proof_words
t0 = time.perf_counter()
ctx = api.Context(sh.lookup_bits, args.route == "no", 0); ctx.trace_begin()      # (keygen lists for the route leg: witness_gen_only = 0)
api.verify_stark(ctx, sh, kh, np.random.default_rng(7).integers(0, 1 << 60, words, dtype=np.int64).astype(np.uint64)); t1 = time.perf_counter()
plan = api.Plan.from_trace(ctx, words) if args.plan == "unfused" else api.Plan.from_trace(ctx, words, fuse_consts=kh, fuse_bn=True); t2 = time.perf_counter()
ctx.close()
info = plan.trace_verdict_info(); assert info["available"] == 1, info
res = {"workload": "2^%d rows, %d queries, lookup_bits 21, PoseidonBN254 caps; valid proofs from h2w_prove_fri_batch; warm-up + %d calls" % (args.degree_bits, args.queries, args.reps),
       "trace_s": round(t1 - t0, 2), "lower_s": round(t2 - t1, 2), "trace_info": plan.trace_info(), "trace_info_bn": plan.trace_info_bn(), "verdict_info": info,
       "cells_per_proof": plan.num_cells, "batches": {}}
s = torch.cuda.current_stream().cuda_stream
ACCEPT = np.array([0, 0, 0xFFFFFFFF, 0], dtype=np.uint32)


def timed(call, check):
    ms = []
    for r in range(args.reps + 1):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        torch.cuda.synchronize(); e0.record(); call(); e1.record(); torch.cuda.synchronize()
        if r:
            ms.append(e0.elapsed_time(e1))
    check()
    return ms


lists = None
for B in [int(x) for x in args.batches.split(",")]:
    g = torch.Generator(device="cuda"); g.manual_seed(0xF1B0 + B)
    coefs = torch.randint(0, 1 << 62, (B * pr.num_polys << args.degree_bits,), dtype=torch.int64, device="cuda", generator=g)
    proofs = torch.zeros(B * words, dtype=torch.int64, device="cuda")
    pr.prove_batch(coefs.data_ptr(), [1, 2, 3] * B, proofs.data_ptr(), B, s); torch.cuda.synchronize()
    del coefs
    out = torch.zeros(4 * B, dtype=torch.int32, device="cuda")
    ws = torch.zeros(plan.workspace_bytes(B), dtype=torch.uint8, device="cuda")
    advice = torch.empty(B * plan.num_cells * 32, dtype=torch.uint8, device="cuda")
    accepted = lambda: (out.cpu().numpy().view(np.uint32).reshape(B, 4) == ACCEPT).all()

    def check_verdicts():
        assert accepted(), out.cpu().numpy().view(np.uint32).reshape(B, 4)
        out.zero_()
    vms = timed(lambda: plan.trace_verdict(proofs.data_ptr(), B, ws.data_ptr(), s, verdict_ptr=out.data_ptr()), check_verdicts)
    cms = timed(lambda: cplan.verdict(proofs.data_ptr(), B, s, verdict_ptr=out.data_ptr()), check_verdicts)
    plan.trace_timing()      # events on
    kern = []

    def witness():
        plan.run(proofs.data_ptr(), B, advice.data_ptr(), ws.data_ptr(), s)
    wms = timed(witness, lambda: None)
    kern = plan.trace_timing()
    assert plan.status(ws.data_ptr(), B, s) == [0] * B
    vms2 = timed(lambda: plan.trace_verdict(proofs.data_ptr(), B, ws.data_ptr(), s, verdict_ptr=out.data_ptr()), check_verdicts)      # again, behind the witness calls
    row = {"verdict_ms": stat(vms), "verdict_ms_after_witness": stat(vms2), "witness_ms": stat(wms), "witness_kernels_ms": [round(x, 3) for x in kern], "witness_kernels_sum_ms": round(sum(kern), 3),
           "compiled_verdict_ms": stat(cms), "ws_GB": round(plan.workspace_bytes(B) / 1e9, 3)}
    slack = max(row["verdict_ms"]["spread"], row["witness_ms"]["spread"])
    row["verdict_over_witness"] = round(med(vms) / med(wms), 4); row["verdict_within_witness"] = bool(med(vms) <= med(wms) + slack)
    if args.route == "yes":
        L = plan.L
        if lists is None:
            t = time.perf_counter()
            n = int(L.h2w_plan_num_equalities(plan.p)); pairs = np.zeros(max(2 * n, 1), dtype=np.uint64)
            assert L.h2w_plan_equalities(plan.p, pairs.ctypes.data_as(C.POINTER(C.c_uint64))) == 0, h2w.last_error()
            m = int(L.h2w_plan_num_const_equalities(plan.p)); cells = np.zeros(max(m, 1), dtype=np.uint64); vals = np.zeros((max(m, 1), 4), dtype=np.uint64)
            assert L.h2w_plan_const_equalities(plan.p, None, cells.ctypes.data_as(C.POINTER(C.c_uint64)), vals.ctypes.data) == 0, h2w.last_error()
            lists = (pairs, n, cells, vals, m); res["equalities"] = n; res["const_equalities"] = m; res["equality_lists_host_s"] = round(time.perf_counter() - t, 2)
        pairs, npairs, cc, cv, nconst = lists
        rms = []
        for r in range(min(args.reps, 3) + 1):
            torch.cuda.synchronize(); t = time.perf_counter()
            witness()
            bad = (C.c_uint64 * 2)(); bad2 = (C.c_uint64 * 2)()
            assert L.h2w_check_equalities(advice.data_ptr(), plan.num_cells, plan.num_cells, B, pairs.ctypes.data, npairs, cc.ctypes.data, cv.ctypes.data, nconst, bad, s) == 0, h2w.last_error()
            assert L.h2w_check_constraints(plan.p, advice.data_ptr(), plan.num_cells, B, bad2, s) == 0, h2w.last_error()
            torch.cuda.synchronize()
            assert list(bad) == [0, 0] and list(bad2) == [0, 0], (list(bad), list(bad2))
            if r:
                rms.append((time.perf_counter() - t) * 1e3)
        row["route_ms"] = stat(rms); row["verdict_over_route"] = round(med(vms) / med(rms), 5)
    res["batches"][str(B)] = row
    print(json.dumps({args.plan: {str(B): row}}), flush=True)
    del advice, ws, proofs, out; torch.cuda.empty_cache()
plan.close(); cplan.close(); pr.close()
doc = {}
if os.path.exists(args.out):
    with open(args.out) as f:
        doc = json.load(f)
doc[args.plan] = res
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(doc, f, indent=1); f.write("\n")
print(json.dumps({args.plan: res}))
