#!/usr/bin/env python3
"""What a verdict costs on cfg 3 (2^20 rows, 28 queries), both hash modes, on batches of 1 and 64 valid proofs made on the device (h2w_prove_fri_batch
from random polynomials; no oracle involved), each alone on the chip, in one process:
  verdict_ms   h2w_fri_verdict_batch                                         device events around the call
  witness_ms   h2w_fri_witness_batch of the same batch                       h2w_plan_timing, whole call
  route_ms     the only verdict there was before: the stream, then h2w_check_equalities (the static lists uploaded by the call) and h2w_check_constraints
               over it                                                        wall clock between device synchronisations (both checks synchronise)
--forms: h2w_fri_verdict_batch_ex under each of the listed flags as well - quad, row, auto, each with an optional +fork (the glue kernel on the plan's
side stream) -, timed like verdict_ms on the same proofs, into the batch's "forms" (row is a PoseidonBN254 form: left out with Goldilocks caps).
--witness-batches: the batches the witness leg is run for (default: all of them).
A warm-up, then the median of --reps calls.  A batch whose advice does not fit --advice-gb is run in chunks of whole proofs, the chunks' times summed
(the verdict call itself always takes the whole batch).  --route: the hash modes the route leg is run for (its equality lists come from a keygen replay of
the shape on the host: 24 s with Goldilocks caps, and one proof per check call there - half a minute for 64 proofs).  Writes one JSON document (--out)."""
import argparse, ctypes as C, importlib, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
h2w = importlib.import_module("halo2-plonky2-verifier_amd"); api = importlib.import_module("halo2-plonky2-verifier_amd.api")

ap = argparse.ArgumentParser()
ap.add_argument("--hash", default="both", choices=["both", "bn254", "gl"])
ap.add_argument("--batches", default="1,64")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--advice-gb", type=float, default=58.0, help="advice per witness call at most (bench.py's automatic batch size)")
ap.add_argument("--route", default="both", choices=["none", "bn254", "gl", "both"])
ap.add_argument("--forms", default="", help="comma list of quad|row|auto[+fork]: h2w_fri_verdict_batch_ex under these flags too")
ap.add_argument("--witness-batches", default="", help="comma list of the batches the witness leg is run for (default: all)")
ap.add_argument("--degree-bits", type=int, default=20); ap.add_argument("--queries", type=int, default=28)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verdict_cfg3.json"))
args = ap.parse_args()
kh = h2w.published_consts()
med = statistics.median
FORM_FLAGS = {"quad": api.VERDICT_FORM_QUAD, "row": api.VERDICT_FORM_ROW, "auto": api.VERDICT_FORM_AUTO}
forms = [f for f in args.forms.split(",") if f]
for f in forms:
    assert f.split("+")[0] in FORM_FLAGS and f.split("+")[1:] in ([], ["fork"]), "--forms: quad|row|auto[+fork], not " + f
witness_batches = [int(x) for x in args.witness_batches.split(",") if x]
result = {"workload": "2^%d rows, %d queries, lookup_bits 21; valid proofs from h2w_prove_fri_batch; warm-up + median of %d" % (args.degree_bits, args.queries, args.reps), "modes": {}}


def equality_lists(plan, proof_words_host):
    """The plan's static lists as ctypes-ready numpy arrays (h2w_plan_equalities / h2w_plan_const_equalities)."""
    L = plan.L
    n = int(L.h2w_plan_num_equalities(plan.p)); pairs = np.zeros(max(2 * n, 1), dtype=np.uint64)
    assert L.h2w_plan_equalities(plan.p, pairs.ctypes.data_as(C.POINTER(C.c_uint64))) == 0, h2w.last_error()
    m = int(L.h2w_plan_num_const_equalities(plan.p)); cells = np.zeros(max(m, 1), dtype=np.uint64); vals = np.zeros((max(m, 1), 4), dtype=np.uint64)
    assert L.h2w_plan_const_equalities(plan.p, proof_words_host.ctypes.data, cells.ctypes.data_as(C.POINTER(C.c_uint64)), vals.ctypes.data) == 0, h2w.last_error()
    return pairs, n, cells, vals, m


for name, mode in (("bn254", 1), ("gl", 0)):
    if args.hash not in ("both", name):
        continue
    sh = h2w.fibonacci_shape(args.degree_bits, args.queries, hash_mode=mode)
    plan = api.Plan(sh, kh); pr = api.Prover(sh, kh)
    per_mode = {"cells_per_proof": plan.num_cells, "advice_GB_per_proof": round(plan.num_cells * 32 / 1e9, 3), "batches": {}}
    lists = None
    for B in [int(x) for x in args.batches.split(",")]:
        g = torch.Generator(device="cuda"); g.manual_seed(0xF1B0 + B)
        coefs = torch.randint(0, 1 << 62, (B * pr.num_polys << args.degree_bits,), dtype=torch.int64, device="cuda", generator=g)
        proofs = torch.zeros(B * plan.proof_words, dtype=torch.int64, device="cuda")
        pr.prove_batch(coefs.data_ptr(), [1, 2, 3] * B, proofs.data_ptr(), B, torch.cuda.current_stream().cuda_stream); torch.cuda.synchronize()
        del coefs
        s = torch.cuda.current_stream().cuda_stream
        out = torch.zeros(4 * B, dtype=torch.int32, device="cuda")
        # ---- the verdict call
        def verdict_ms(flags):
            ms = []
            out.zero_(); torch.cuda.synchronize()
            for r in range(args.reps + 1):
                e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
                e0.record(); plan.verdict(proofs.data_ptr(), B, s, verdict_ptr=out.data_ptr(), flags=flags); e1.record(); torch.cuda.synchronize()
                if r:
                    ms.append(e0.elapsed_time(e1))
            v = out.cpu().numpy().view(np.uint32).reshape(B, 4)
            assert (v == np.array([0, 0, 0xFFFFFFFF, 0], dtype=np.uint32)).all(), v      # every proof is accepted
            return ms
        ms = verdict_ms(None)
        row = {"verdict_ms": round(med(ms), 4), "verdict_ms_all": [round(x, 4) for x in ms]}
        if forms:
            row["paths"] = B * args.queries * (len(plan.proof_layout()["oracles"]) + len(plan.proof_layout()["steps"]))
            row["auto_is"] = {api.VERDICT_FORM_QUAD: "quad", api.VERDICT_FORM_ROW: "row"}[plan.verdict_form(B)]
            row["forms"] = {}
            for f in forms:
                if mode == 0 and f.startswith("row"):
                    continue
                fms = verdict_ms(FORM_FLAGS[f.split("+")[0]] | (api.VERDICT_FORK if f.endswith("+fork") else 0))
                row["forms"][f] = {"ms": round(med(fms), 4), "ms_all": [round(x, 4) for x in fms]}
        if witness_batches and B not in witness_batches:
            per_mode["batches"][str(B)] = row
            print(json.dumps({name: {str(B): row}}), flush=True)
            del proofs, out; torch.cuda.empty_cache()
            continue
        # ---- the witness call, in chunks that fit
        chunk = max(1, min(B, int(args.advice_gb * 1e9 / (plan.num_cells * 32))))
        advice = torch.empty(chunk * plan.num_cells * 32, dtype=torch.uint8, device="cuda"); ws = torch.zeros(plan.workspace_bytes(chunk), dtype=torch.uint8, device="cuda")
        def witness(first, n):
            plan.run(proofs.data_ptr() + first * plan.proof_words * 8, n, advice.data_ptr(), ws.data_ptr(), s); torch.cuda.synchronize()
            return plan.timing()[4]
        wms = []
        for r in range(args.reps + 1):
            t = sum(witness(f, min(chunk, B - f)) for f in range(0, B, chunk))
            if r:
                wms.append(t)
        row.update(witness_ms=round(med(wms), 4), witness_chunk=chunk, witness_Gcells_per_s=round(B * plan.num_cells / med(wms) / 1e6, 2), verdict_over_witness=round(med(ms) / med(wms), 4))
        # ---- the route of the parent commit
        if args.route in ("both", name):
            if lists is None:
                t0 = time.perf_counter(); lists = equality_lists(plan, proofs[:plan.proof_words].cpu().numpy().view(np.uint64)); per_mode["equality_lists_host_s"] = round(time.perf_counter() - t0, 2)
                per_mode["equalities"] = lists[1]; per_mode["const_equalities"] = lists[4]
            pairs, npairs, cc, cv, nconst = lists
            def route(first, n):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                plan.run(proofs.data_ptr() + first * plan.proof_words * 8, n, advice.data_ptr(), ws.data_ptr(), s)
                bad = (C.c_uint64 * 2)(); bad2 = (C.c_uint64 * 2)()
                if mode == 0:      # (with Goldilocks caps the constant equalities hold proof words: their values are per proof, one proof per call)
                    w = proofs[first * plan.proof_words:(first + 1) * plan.proof_words].cpu().numpy().view(np.uint64)
                    assert plan.L.h2w_plan_const_equalities(plan.p, w.ctypes.data, cc.ctypes.data_as(C.POINTER(C.c_uint64)), cv.ctypes.data) == 0, h2w.last_error()
                assert plan.L.h2w_check_equalities(advice.data_ptr(), plan.num_cells, plan.num_cells, n, pairs.ctypes.data, npairs, cc.ctypes.data, cv.ctypes.data, nconst, bad, s) == 0, h2w.last_error()
                assert plan.L.h2w_check_constraints(plan.p, advice.data_ptr(), plan.num_cells, n, bad2, s) == 0, h2w.last_error()
                torch.cuda.synchronize()
                assert list(bad) == [0, 0] and list(bad2) == [0, 0], (list(bad), list(bad2))
                return (time.perf_counter() - t0) * 1e3
            rchunk = 1 if mode == 0 else chunk
            rms = []
            for r in range(min(args.reps, 3) + 1):
                t = sum(route(f, min(rchunk, B - f)) for f in range(0, B, rchunk))
                if r:
                    rms.append(t)
            row.update(route_ms=round(med(rms), 3), route_chunk=rchunk, verdict_over_route=round(med(ms) / med(rms), 5))
        per_mode["batches"][str(B)] = row
        print(json.dumps({name: {str(B): row}}), flush=True)
        del advice, ws, proofs, out; torch.cuda.empty_cache()
    result["modes"][name] = per_mode
    plan.close(); pr.close()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1); f.write("\n")
print(json.dumps(result))
