#!/usr/bin/env python3
"""What the batched Merkle chip op (h2w_chipbatch_new_hash, H2W_OP_MERKLE_VERIFY) delivers, leaf length 20, in two configurations:
  bn254  hash_mode 1, depth 20, cap_height 4, n = 4096 instances per call
  gl     hash_mode 0, depth 10, cap_height 0, n = 64
h2w_chipbatch_run is timed with device events: warm-up calls, then the median of --runs single calls.  Reported per configuration: instances/s,
cells/s, advice bytes (32 B x cells) over time against the 8 TB/s HBM peak, and - on the same host - the same op through the eager level
(h2w_chip_merkle_verify on ONE reused context: loads, the op, h2w_ctx_advice_device, per instance; fewer instances, the rate scaled).
Random in-range operands: neither path's work depends on the values.  Writes one JSON document (--out).
--values: h2w_chipbatch_values (results and verdicts, no advice) beside h2w_chipbatch_run on the same handle and the same operands, the same way
(device events, warm-up, median): instances/s of both, every form the hash mode admits; with --sweep also the form sweep of hash_mode 1 - depth 20,
cap_height 4, n = 1 .. 16,384 by powers of two, each call alone on the chip, H2W_CHIPBATCH_FORM_QUAD against _ROW - and the largest n at which the
row form is not the slower one.  No ratio is asserted.  Writes profiles/chipbatch_values.json (--out)."""
import argparse, ctypes as C, importlib, json, os, random, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
h2w = importlib.import_module("halo2-plonky2-verifier_amd"); api = importlib.import_module("halo2-plonky2-verifier_amd.api")

P = 2**64 - 2**32 + 1
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
HBM_PEAK = 8e12
N_IN = 20

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--eager-instances", type=int, default=8)
ap.add_argument("--only", default="both", choices=["both", "bn254", "gl"])
ap.add_argument("--values", action="store_true", help="time h2w_chipbatch_values beside h2w_chipbatch_run")
ap.add_argument("--sweep", action="store_true", help="with --values: the QUAD / ROW form sweep over n")
ap.add_argument("--out", default=None)
args = ap.parse_args()
args.out = args.out or os.path.join(ROOT, "profiles", "chipbatch_values.json" if args.values else "chipbatch_hash.json")
kh = h2w.published_consts(); L = h2w.lib()
result = {"op": "H2W_OP_MERKLE_VERIFY, leaf length %d, lookup_bits 21, published tables" % N_IN,
          "timing": "device events around one h2w_chipbatch_run, %d warm-up calls, median of %d" % (args.warmup, args.runs), "configs": {}}


def operands(rnd, mode, depth, cap):
    """One instance: leaf, index, cap, siblings (include/h2w.h 2c)."""
    w = [rnd.randrange(P) for _ in range(N_IN)] + [rnd.randrange(1 << depth)]
    for _ in range((1 << cap) + depth - cap):
        if mode == 0:
            w += [rnd.randrange(P) for _ in range(4)]
        else:
            x = rnd.randrange(R); w += [(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    return w


def eager_rate(mode, depth, cap, rows):
    """Instances per second of h2w_chip_merkle_verify on one reused eager context (the host computes every value; the GPU expands)."""
    ctx = api.Context(21); A = h2w.Assigned; n_cap, n_sib = 1 << cap, depth - cap

    def gl_wit(v):
        g = A(); assert L.h2w_gl_load_witness(ctx.p, v, C.byref(g)) == 0; return g

    def gl_const(v):
        g = A(); assert L.h2w_gl_load_constant(ctx.p, v, C.byref(g)) == 0; return g

    def hash_wires(ws):
        if mode == 0:
            return [gl_const(x) for x in ws]
        g = A(); assert L.h2w_load_witness(ctx.p, C.byref(h2w.Fr.from_int(sum(x << (64 * i) for i, x in enumerate(ws)))), C.byref(g)) == 0
        return [g]

    def one(w):
        ctx.reset()
        leaf = [gl_wit(x) for x in w[:N_IN]]; idx = w[N_IN]
        bits = [gl_const((idx >> i) & 1) for i in range(depth)]; cap_index = gl_const(idx >> n_sib)      # (the index bits as constants: fewer cells than the batched op's num_to_bits)
        hs = w[N_IN + 1:]
        capw = [x for i in range(n_cap) for x in hash_wires(hs[4 * i:4 * i + 4])]
        sibw = [x for i in range(n_cap, n_cap + n_sib) for x in hash_wires(hs[4 * i:4 * i + 4])]
        assert L.h2w_chip_merkle_verify(ctx.p, C.byref(kh), mode, (A * N_IN)(*leaf), N_IN, (A * depth)(*bits), depth, C.byref(cap_index),
                                        (A * len(capw))(*capw), n_cap, (A * len(sibw))(*sibw) if sibw else None, n_sib) == 0, h2w.last_error()
        ctx.advice_device()
    one(rows[0]); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for w in rows:
        one(w)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    cells = ctx.num_cells(); ctx.close()
    return len(rows) / dt, cells


def timed(call):
    """Median, min and max ms of one call between two device events, after the warm-up calls."""
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.runs):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record(); call(); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def values_bench():
    FORMS = {"quad": h2w.H2W_CHIPBATCH_FORM_QUAD, "row": h2w.H2W_CHIPBATCH_FORM_ROW}
    s = torch.cuda.current_stream().cuda_stream
    doc = {"op": result["op"], "timing": "device events around one call, %d warm-up calls, median of %d; every call alone on the chip" % (args.warmup, args.runs), "values_against_witness": {}}
    for name, mode, depth, cap, n in (("bn254", 1, 20, 4, 4096), ("gl", 0, 10, 0, 64)):
        if args.only not in ("both", name):
            continue
        rnd = random.Random(20 + mode)
        b = api.ChipBatch.new_hash(h2w.H2W_OP_MERKLE_VERIFY, kh, hash_mode=mode, n_in=N_IN, depth=depth, cap_height=cap)
        nc = b.num_cells()
        base = [operands(rnd, mode, depth, cap) for _ in range(min(n, 64))]
        d_ops = torch.tensor(np.array([base[i % len(base)] for i in range(n)], dtype=np.uint64).view(np.int64).reshape(-1), dtype=torch.int64, device="cuda")
        advice = torch.empty(n * nc * 32, dtype=torch.uint8, device="cuda"); status = torch.zeros(n, dtype=torch.int32, device="cuda")
        verdict = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
        med, lo, hi = timed(lambda: b.run(d_ops.data_ptr(), n, advice.data_ptr(), status.data_ptr(), s))
        r = {"hash_mode": mode, "depth": depth, "cap_height": cap, "instances": n, "cells_per_instance": nc,
             "witness_ms_median": med, "witness_ms_min": lo, "witness_ms_max": hi, "witness_instances_per_s": n / med * 1e3}
        for fname, form in FORMS.items():
            if mode == 0 and fname == "row":
                continue
            med, lo, hi = timed(lambda: b.values(d_ops.data_ptr(), n, 0, verdict.data_ptr(), form, s))
            key = "values_" + (fname if mode == 1 else "one_kernel")
            r.update({key + "_ms_median": med, key + "_ms_min": lo, key + "_ms_max": hi, key + "_instances_per_s": n / med * 1e3})
        v = verdict.cpu().view(n, 2)
        assert v[:, 0].tolist() == status.cpu().tolist() == [0] * n and int(v[:, 1].min()) > 0      # (random openings: every root check fails)
        doc["values_against_witness"][name] = {k: (round(x, 4) if isinstance(x, float) else x) for k, x in r.items()}
        print(json.dumps({name: doc["values_against_witness"][name]}), flush=True)
        del advice, d_ops; b.close(); torch.cuda.empty_cache()
    if args.sweep:
        mode, depth, cap = 1, 20, 4
        rnd = random.Random(21)
        b = api.ChipBatch.new_hash(h2w.H2W_OP_MERKLE_VERIFY, kh, hash_mode=mode, n_in=N_IN, depth=depth, cap_height=cap)
        base = [operands(rnd, mode, depth, cap) for _ in range(64)]
        nmax = 16384
        d_ops = torch.tensor(np.array([base[i % 64] for i in range(nmax)], dtype=np.uint64).view(np.int64).reshape(-1), dtype=torch.int64, device="cuda")
        verdict = torch.zeros(2 * nmax, dtype=torch.int32, device="cuda")
        rows = []
        for k in range(15):
            n = 1 << k
            row = {"n": n}
            for fname, form in FORMS.items():
                med, lo, hi = timed(lambda: b.values(d_ops.data_ptr(), n, 0, verdict.data_ptr(), form, s))
                row.update({fname + "_ms_median": round(med, 4), fname + "_ms_min": round(lo, 4), fname + "_ms_max": round(hi, 4)})
            rows.append(row); print(json.dumps(row), flush=True)
        not_slower = [r["n"] for r in rows if r["row_ms_median"] <= r["quad_ms_median"]]
        doc["form_sweep"] = {"op": "MERKLE_VERIFY, hash_mode 1, depth 20, cap_height 4, leaf length 20", "rows": rows,
                             "largest_n_at_which_row_is_not_the_slower_form": max(not_slower) if not_slower else 0}
        b.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1); f.write("\n")
    print(json.dumps(doc))


if args.values:
    values_bench()
    sys.exit(0)

for name, mode, depth, cap, n in (("bn254", 1, 20, 4, 4096), ("gl", 0, 10, 0, 64)):
    if args.only not in ("both", name):
        continue
    rnd = random.Random(20 + mode)
    b = api.ChipBatch.new_hash(h2w.H2W_OP_MERKLE_VERIFY, kh, hash_mode=mode, n_in=N_IN, depth=depth, cap_height=cap)
    nw, nc = b.num_operands(), b.num_cells()
    base = [operands(rnd, mode, depth, cap) for _ in range(min(n, 64))]
    rows = [base[i % len(base)] for i in range(n)]
    d_ops = torch.tensor(np.array(rows, dtype=np.uint64).view(np.int64).reshape(-1), dtype=torch.int64, device="cuda")
    advice = torch.empty(n * nc * 32, dtype=torch.uint8, device="cuda"); status = torch.zeros(n, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(args.warmup):
        b.run(d_ops.data_ptr(), n, advice.data_ptr(), status.data_ptr(), s)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n
    ms = []
    for _ in range(args.runs):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record(); b.run(d_ops.data_ptr(), n, advice.data_ptr(), status.data_ptr(), s); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    eager_ips, eager_cells = eager_rate(mode, depth, cap, base[:args.eager_instances])
    r = {"hash_mode": mode, "depth": depth, "cap_height": cap, "instances": n, "operand_words": nw, "cells_per_instance": nc,
         "ms_per_call_median": med, "ms_per_call_min": min(ms), "ms_per_call_max": max(ms),
         "instances_per_s": n / med * 1e3, "Gcells_per_s": n * nc / med / 1e6, "advice_TB_per_s": n * nc * 32 / med / 1e9,
         "share_of_8TBps_hbm_peak": n * nc * 32 / (med * 1e-3) / HBM_PEAK,
         "eager_instances_timed": args.eager_instances, "eager_cells_per_instance": eager_cells, "eager_instances_per_s": eager_ips}
    r["batched_over_eager"] = r["instances_per_s"] / eager_ips
    result["configs"][name] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
    print(json.dumps({name: result["configs"][name]}), flush=True)
    del advice, d_ops; b.close(); torch.cuda.empty_cache()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1); f.write("\n")
print(json.dumps(result))
