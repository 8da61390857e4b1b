#!/usr/bin/env python3
"""Times h2w_merkle_build (include/h2w.h 2e, csrc/merkletree.hip): device events around the calls, warmed up, one configuration at a time.
usage: python tools/bench_merkle.py --crossover [--hash gl|bn254|both] [--depths 12,16,20] [--n-in 5,20] [--trees 1,8,64] [--reps 5] [--out FILE.jsonl]
       python tools/bench_merkle.py --prover [--reps 3]
       python tools/bench_merkle.py --leaves [--reps 5]
--crossover  the two forms of the upper levels against each other: a build under H2W_MERKLE_CROWN_NONE and under CROWN_BITS = b, b = 0 .. min(depth, 14),
             ALTERNATING in one run (none, b, none, b, ..), the median of each.  The level of b bits is the crown's gain while T(b) < T(b - 1) (T(-1) = NONE):
             the crossover of a configuration is n_trees x 2^b at the b of the least T(b) (a lower bound where that is the last b tried).  One JSON line
             per configuration.
--prover     for orientation: h2w_prover_timing ms[1] (the Merkle commitments of the oracles, batches of 8) beside h2w_merkle_build calls of the same
             number of trees, depth and leaf widths (one call per oracle), cfg2 and cfg3 in both hash modes.
--leaves     leaves of 64 .. 4,096 words: the build's time and the read rate of the leaf words, bytes from the shapes / the time of the whole build
             call (leaf kernel, status check - a second read of the same words - and levels: a lower bound of the leaf kernel's own rate).
Leaves are random canonical words drawn on the device; no oracle involved."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = {"cfg2": (16, 28, 2), "cfg3": (20, 28, 1)}
NONE, OPT = 254, 1


def _timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


class Bench:
    def __init__(self, torch, api, kh, mode, n_in, depth, cap, n_trees, gen):
        self.torch, self.n_trees = torch, n_trees
        self.m = api.MerkleTree.new(kh, hash_mode=mode, n_in=n_in, depth=depth, cap_height=cap)
        self.leaves = torch.randint(0, 1 << 62, ((n_trees << depth) * n_in,), dtype=torch.int64, device="cuda", generator=gen)      # < 2^62 < p: canonical
        self.trees = torch.empty((n_trees * self.m.tree_words(),), dtype=torch.int64, device="cuda")
        self.status = torch.zeros((n_trees,), dtype=torch.int32, device="cuda")
        self.stream = torch.cuda.current_stream().cuda_stream

    def build_ms(self, crown):
        self.m.configure(OPT, crown)
        return _timed(self.torch, lambda: self.m.build(self.leaves.data_ptr(), self.n_trees, self.trees.data_ptr(), self.status.data_ptr(), self.stream))

    def close(self):
        assert self.status.cpu().tolist() == [0] * self.n_trees
        self.m.close()


def crossover(torch, api, kh, a, out):
    gen = torch.Generator(device="cuda"); gen.manual_seed(0x3E2C)
    modes = {"gl": (0,), "bn254": (1,), "both": (0, 1)}[a.hash]
    for mode in modes:
        for depth in a.depths:
            for n_in in a.n_in:
                for n_trees in a.trees:
                    bm = Bench(torch, api, kh, mode, n_in, depth, 0, n_trees, gen)
                    bm.build_ms(NONE); bm.build_ms(min(depth, 14))      # warm-up of both forms
                    row = {"tool": "bench_merkle", "what": "crossover", "hash_mode": mode, "depth": depth, "n_in": n_in, "n_trees": n_trees, "reps": a.reps, "ms_crown": {}, "ms_none_beside": {}}
                    for b in range(0, min(depth, 14) + 1):
                        tn, tb = [], []
                        for _ in range(a.reps):
                            tn.append(bm.build_ms(NONE)); tb.append(bm.build_ms(b))
                        row["ms_none_beside"][b] = round(statistics.median(tn), 4); row["ms_crown"][b] = round(statistics.median(tb), 4)
                    row["ms_none"] = round(statistics.median(row["ms_none_beside"].values()), 4)
                    best = min(row["ms_crown"], key=lambda b: (row["ms_crown"][b], b))      # (b >= depth - 1 are the same build: the lowest of a tie)
                    if row["ms_crown"][best] >= row["ms_none"]:
                        best = None
                    row["best_crown_bits"] = best
                    row["crossover_nodes"] = None if best is None else n_trees << best
                    row["at_the_sweep_s_edge"] = best is not None and best >= min(depth - 1, 14)      # the crown gained up to the last level tried: a lower bound
                    bm.close()
                    line = json.dumps(row)
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n"); out.flush()


def prover(torch, api, h2w, kh, a, out):
    gen = torch.Generator(device="cuda"); gen.manual_seed(0xF1B0)
    B = 8
    for cfg, (d, q, rb) in CONFIGS.items():
        for mode in (0, 1):
            sh = h2w.fibonacci_shape(d, q, rate_bits=rb, hash_mode=mode)
            pr = api.Prover(sh, kh)
            coefs = torch.randint(0, 1 << 62, (B * pr.num_polys << d,), dtype=torch.int64, device="cuda", generator=gen)
            proof = torch.zeros(B * pr.proof_words, dtype=torch.int64, device="cuda")
            s = torch.cuda.current_stream().cuda_stream
            ms1 = []
            for r in range(a.reps + 1):
                pr.prove_batch(coefs.data_ptr(), [1, 2, 3] * B, proof.data_ptr(), B, s)
                torch.cuda.synchronize()
                if r:
                    ms1.append(pr.timing()["commit"])
            pr.close(); del coefs, proof
            widths = [w for w in (sh.n_cols, sh.n_perm_z, sh.n_quotient) if w > 0]
            per = []
            for w in widths:
                bm = Bench(torch, api, kh, mode, w, d + rb, sh.cap_height, B, gen)
                bm.build_ms(api.H2W_MERKLE_CROWN_AUTO)
                per.append(statistics.median(bm.build_ms(api.H2W_MERKLE_CROWN_AUTO) for _ in range(a.reps)))
                bm.close()
            row = {"tool": "bench_merkle", "what": "prover", "config": cfg, "hash_mode": mode, "batch": B, "lde_bits": d + rb, "cap_height": sh.cap_height, "leaf_widths": widths,
                   "prover_ms1_merkle_commitments": round(statistics.median(ms1), 3), "merkle_build_ms_per_oracle": [round(x, 3) for x in per], "merkle_build_ms": round(sum(per), 3)}
            line = json.dumps(row)
            print(line, flush=True)
            if out:
                out.write(line + "\n"); out.flush()


def leaves(torch, api, kh, a, out):
    gen = torch.Generator(device="cuda"); gen.manual_seed(0x1EAF)
    for mode in (0, 1):
        for n_in, depth in ((64, 16), (256, 14), (1024, 12), (4096, 10)):
            bm = Bench(torch, api, kh, mode, n_in, depth, 0, 4, gen)
            bm.build_ms(NONE)
            ms = statistics.median(bm.build_ms(NONE) for _ in range(a.reps))
            nbytes = (4 << depth) * n_in * 8
            bm.close()
            row = {"tool": "bench_merkle", "what": "leaves", "hash_mode": mode, "n_in": n_in, "depth": depth, "n_trees": 4, "build_ms": round(ms, 4), "leaf_bytes": nbytes,
                   "leaf_words_read_rate_GBps_over_the_build_call": round(nbytes / ms / 1e6, 2)}
            line = json.dumps(row)
            print(line, flush=True)
            if out:
                out.write(line + "\n"); out.flush()


def main():
    ints = lambda s: [int(x) for x in s.split(",")]
    ap = argparse.ArgumentParser()
    ap.add_argument("--crossover", action="store_true"); ap.add_argument("--prover", action="store_true"); ap.add_argument("--leaves", action="store_true")
    ap.add_argument("--hash", default="both", choices=["gl", "bn254", "both"])
    ap.add_argument("--depths", type=ints, default=[12, 16, 20]); ap.add_argument("--n-in", type=ints, default=[5, 20]); ap.add_argument("--trees", type=ints, default=[1, 8, 64])
    ap.add_argument("--reps", type=int, default=5); ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    h2w = importlib.import_module("halo2-plonky2-verifier_amd"); api = importlib.import_module("halo2-plonky2-verifier_amd.api")
    api.H2W_MERKLE_CROWN_AUTO = h2w.H2W_MERKLE_CROWN_AUTO
    kh = h2w.published_consts()
    out = open(a.out, "a") if a.out else None
    if a.crossover:
        crossover(torch, api, kh, a, out)
    if a.prover:
        prover(torch, api, h2w, kh, a, out)
    if a.leaves:
        leaves(torch, api, kh, a, out)


if __name__ == "__main__":
    main()
