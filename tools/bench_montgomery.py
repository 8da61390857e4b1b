#!/usr/bin/env python3
"""What the Montgomery output form (H2W_OPT_OUTPUT_FORM) costs and saves on cfg 3 (2^20 rows, 28 queries), both hash modes, with the batch size
and the four-launches-in-flight schedule of bench.py's default run, in one process:
  (a) canonical generation;
  (b) canonical generation followed by h2w_advice_to_montgomery over the same cells (the only way to the form before the option existed);
  (c) generation with the Montgomery form selected;
plus the expansion kernel alone in both forms (h2w_plan_timing_ex slot 5 of isolated launches).  Random in-range proof words: the kernels'
work does not depend on the values.  --only c: just leg (c), for a kernel trace of its own.  Writes one JSON document (--out)."""
import argparse, ctypes as C, importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
h2w = importlib.import_module("halo2-plonky2-verifier_amd"); api = importlib.import_module("halo2-plonky2-verifier_amd.api")

ap = argparse.ArgumentParser()
ap.add_argument("--hash", default="both", choices=["both", "bn254", "gl"])
ap.add_argument("--streams", type=int, default=4)
ap.add_argument("--launches", type=int, default=16, help="timed launches per leg (after one warm-up launch per stream)")
ap.add_argument("--advice-gb", type=float, default=58.0, help="advice per launch (bench.py's automatic batch size)")
ap.add_argument("--only", default="abc")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "montgomery_form_cfg3.json"))
args = ap.parse_args()
kh = h2w.published_consts()
result = {"workload": "cfg3 (2^20 rows, 28 queries, lookup_bits 21), %d launches in flight, %d timed launches per leg" % (args.streams, args.launches), "modes": {}}
for name, mode in (("bn254", 1), ("gl", 0)):
    if args.hash not in ("both", name):
        continue
    plan = api.Plan(h2w.fibonacci_shape(20, 28, hash_mode=mode), kh)
    B = max(1, int(args.advice_gb * 1e9 / (plan.num_cells * 32)))
    cells = B * plan.num_cells
    proofs = torch.randint(0, 1 << 62, (B * plan.proof_words,), dtype=torch.int64, device="cuda")
    streams = [torch.cuda.Stream() for _ in range(args.streams)]
    adv = [torch.empty(cells * 32, dtype=torch.uint8, device="cuda") for _ in streams]
    ws = [torch.zeros(plan.workspace_bytes(B), dtype=torch.uint8, device="cuda") for _ in streams]

    def leg(form, second_pass):
        plan.set_output_form(form)
        def launch(i):
            s = streams[i % len(streams)].cuda_stream
            plan.run(proofs.data_ptr(), B, adv[i % len(streams)].data_ptr(), ws[i % len(streams)].data_ptr(), s)
            if second_pass:
                assert plan.L.h2w_advice_to_montgomery(adv[i % len(streams)].data_ptr(), cells, s) == 0
        for i in range(len(streams)):
            launch(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True); e0.record()
        for s in streams:
            s.wait_event(e0)
        for i in range(args.launches):
            launch(i)
        for s in streams:
            torch.cuda.current_stream().wait_stream(s)
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.launches

    def expand_alone(form):
        plan.set_output_form(form); ms = (C.c_float * 8)(); best = None
        for _ in range(3):
            plan.run(proofs.data_ptr(), B, adv[0].data_ptr(), ws[0].data_ptr(), streams[0].cuda_stream); torch.cuda.synchronize()
            assert plan.L.h2w_plan_timing_ex(plan.p, 0, ms) == 0
            best = ms[5] if best is None else min(best, ms[5])
        return best
    r = {"batch": B, "cells_per_launch": cells, "record_cells_per_proof": plan.num_record_cells, "direct_cells_per_proof": plan.num_cells - plan.num_record_cells}
    if "a" in args.only: r["a_canonical_ms"] = leg(api.FORM_CANONICAL, False)
    if "b" in args.only: r["b_canonical_then_second_pass_ms"] = leg(api.FORM_CANONICAL, True)
    if "c" in args.only: r["c_montgomery_form_ms"] = leg(api.FORM_MONTGOMERY, False)
    if args.only == "abc":
        r["c_over_b"] = r["c_montgomery_form_ms"] / r["b_canonical_then_second_pass_ms"]; r["c_over_a"] = r["c_montgomery_form_ms"] / r["a_canonical_ms"]
        r["expand_alone_canonical_ms"] = expand_alone(api.FORM_CANONICAL); r["expand_alone_montgomery_ms"] = expand_alone(api.FORM_MONTGOMERY)
        for k_, ms_ in (("a", r["a_canonical_ms"]), ("b", r["b_canonical_then_second_pass_ms"]), ("c", r["c_montgomery_form_ms"])):
            r[k_ + "_Gcells_per_s"] = cells / ms_ / 1e6
        r["expand_alone_canonical_TBps"] = B * plan.num_record_cells * 32 / r["expand_alone_canonical_ms"] / 1e9
        r["expand_alone_montgomery_TBps"] = B * plan.num_record_cells * 32 / r["expand_alone_montgomery_ms"] / 1e9
    plan.set_output_form(api.FORM_CANONICAL)
    result["modes"][name] = {k_: (round(v, 4) if isinstance(v, float) else v) for k_, v in r.items()}
    print(json.dumps({name: result["modes"][name]}), flush=True)
    del adv, ws, proofs; plan.close(); torch.cuda.empty_cache()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1); f.write("\n")
print(json.dumps(result))
