#!/usr/bin/env python3
"""bench.py — FRI-verifier witness-generation throughput on MI355X (BASELINE.json metric: witness cells/sec).

Workload (N = 1 default): BASELINE.json configs[2], the north-star target config — 2^20-row Fibonacci STARK, 28 FRI queries,
cap_height 4, PoseidonBN254 Merkle caps, lookup_bits 21 — on synthetic valid FRI instances that are resident in HBM before
the timed region starts.  `--config cfg1|cfg2|cfg5`, `--hash gl` select the other BASELINE configs.

One *launch* = one h2w_fri_witness_batch call (the whole hot path: prologue strands, query glue strands, Merkle strands,
expansion) over `--batch` proofs.  Launches go round-robin over `--streams` HIP streams with their own advice / workspace
buffers, so the latency-bound strands of one launch overlap the HBM-bound kernels of another.  One *step* = `--launches-per-step`
launches (default 24): a step is sized to ~0.22 s so that the timed region lasts seconds whatever `--steps` is (the driver's --steps 20: 4.5 s), and `--warmup`
steps (at least one) touch every stream's buffers before the clock starts.

N > 1 (`--gpus N`; launched by torch.distributed.run, or spawned by this script itself when WORLD_SIZE is not set): one rank
per GPU; rank 0 builds the proofs and ONE broadcast moves the proof block over RCCL (the only collective).
  * default: every rank generates the witnesses of its own shard of proofs ("weak" scaling: per-GPU work fixed);
  * `--shard-queries` (default for cfg5, BASELINE configs[4]): all ranks hold the same proofs and rank r generates the
    (proof, query) units u with u % N == r plus the prologue blocks of the proofs it owns (h2w_fri_witness_batch_shard_compact);
    a launch covers `--batch` x N proofs, so that a rank's launch has as many units - and writes as many bytes - as an unsharded
    launch of `--batch` proofs (a rank's packed buffers are 1 / N of the stream: it fits); total work is fixed ("strong" scaling).
  * `--emulate-rank R --world W` (N = 1): ONE process on ONE GPU runs exactly what rank R of W would run in that mode (the broadcast
    skipped: the proofs are generated in place), pipelined as usual, and reports that rank's own cells/s.  The path has no data-path
    collective, so this IS the per-GPU rate of a W-GPU run.
value = cells of all ranks / max-rank time.

A plain run sets up, warms up, times `--steps` steps and prints the line: the headline figure and nothing that needs runs of its own.
`--full` adds the other legs: per-kernel roofline figures from isolated launches (`--calib`), the one-proof latency, the Goldilocks-caps
secondary, the eager boundary and its replay, the committed PMC traffic, and the CPU baselines.  `--dump-outputs DIR` writes what the
last timed step computed to DIR/*.npy (float64) so that two builds can be compared output for output on the same seeded inputs.

The CPU oracle (oracle/) is imported by the `cpu_baseline` leg only (`--full`, rank 0, N = 1), never by the measured path.
Prints ONE JSON line on rank 0.
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CONFIGS = {
    # name: (degree_bits, num_queries, rate_bits, description)
    "cfg1": (10, 4, 1, "2^10-row Fibonacci STARK, 4 FRI queries, rate_bits=1, cap_height=4"),
    "cfg2": (16, 28, 2, "2^16-row Fibonacci STARK, 28 FRI queries, rate_bits=2, cap_height=4"),
    "cfg3": (20, 28, 1, "2^20-row Fibonacci STARK, 28 FRI queries, rate_bits=1, cap_height=4"),
    "cfg5": (20, 84, 1, "2^20-row Fibonacci STARK, 84 FRI queries, rate_bits=1, cap_height=4"),
}
HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured float4 copy)
VALU_ISSUE_PER_S = 256 * 4 * 2.4e9 / 4   # wave64 VALU instructions the chip can issue per second: 256 CUs x 4 SIMDs x 2.4 GHz / 4 cycles per instruction = 6.1e11
OPT_FORK_CHAINS = 1     # include/h2w.h H2W_OPT_FORK_CHAINS
OPT_SERIAL_EXPAND = 2   # include/h2w.h H2W_OPT_SERIAL_EXPAND
OPT_CHAIN_PASSES = 3    # include/h2w.h H2W_OPT_CHAIN_PASSES


def cpu_baseline(shape_args, hash_mode, lookup_bits, budget_s=12.0):
    """The oracle (CPU restatement, kind "port") timed single-threaded on this host, on the same workload shape.  Only the
    verifier gadget (load_proof_with_pis + verify_proof: the path) is timed: synthesising the proof and allocating the context
    happen outside the clock."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pyoracle as O
    sh = O.fibonacci_shape(shape_args[0], shape_args[1], rate_bits=shape_args[2], hash_mode=hash_mode, lookup_bits=lookup_bits)
    k = O.published_consts()
    n, cells, busy, t0 = 0, 0, 0.0, time.perf_counter()
    while True:
        pr = O.synth_proof(sh, 0xF1B00000 + n)
        ctx = O.Ctx(lookup_bits)
        if n > 0:
            ctx.reserve(cells // n)          # known size after the first proof: no realloc copies in the timed run
        t1 = time.perf_counter()
        O.verify_stark(ctx, sh, k, pr)
        busy += time.perf_counter() - t1
        cells += ctx.num_cells(); n += 1
        ctx.close()
        if time.perf_counter() - t0 > budget_s or n >= 64:
            break
    return {"value": cells / busy, "unit": "cells/s", "cores": 1, "kind": "port",
            "sample": f"{n} proof(s) of the same shape ({cells} cells) through oracle/liboracle.so, 1 thread, {busy:.1f} s inside the verifier gadget "
                      f"({time.perf_counter() - t0:.1f} s wall with proof synthesis and allocation, not counted)",
            "proofs_per_s": n / busy, "_cells": cells, "_proofs": n, "_seconds": busy}


def cpu_baseline_all_cores(shape_args, hash_mode, lookup_bits, cells_per_proof, budget_s=8.0):
    """The same oracle loop in one process per host core this process may run on (one proof per core; the reference itself
    is single-threaded, so this is the most a user of it could get from the box).  Workers are fresh interpreters that never touch
    the GPU; their number is bounded by memory (a context holds its whole advice stream) and can be capped with H2W_CPU_WORKERS."""
    try:
        ncores = len(os.sched_getaffinity(0))
    except AttributeError:
        ncores = os.cpu_count() or 1
    try:
        import psutil
        avail = psutil.virtual_memory().available
    except Exception:
        avail = 32 << 30
    cap = int(os.environ.get("H2W_CPU_WORKERS", "0")) or ncores        # every core this process may run on, unless capped
    most = max(1, min(ncores, cap, int(0.4 * avail // (cells_per_proof * 48))))      # a context holds its whole advice stream (32 B / cell + bookkeeping)
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-worker", json.dumps([list(shape_args), hash_mode, lookup_bits, budget_s])]

    def run(workers):
        t0 = time.perf_counter()
        procs = [subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True) for _ in range(workers)]
        res = [json.loads(p.communicate(timeout=budget_s * 12 + 240)[0].strip().splitlines()[-1]) for p in procs]
        wall = time.perf_counter() - t0
        cells = sum(r["cells"] for r in res); n = sum(r["proofs"] for r in res); span = max(r["seconds"] for r in res)
        return {"value": cells / span, "unit": "cells/s", "cores": workers, "host_cores_visible": ncores, "kind": "port",
                "sample": f"{n} proof(s) of the same shape over {workers} single-threaded oracle processes ({span:.1f} s inside the gadget each, {wall:.1f} s wall incl. start-up)",
                "proofs_per_s": n / span}
    # every core, and a quarter of them: one context per process streams ~1 GB per proof, so the host's memory system, not its core count, sets the rate
    runs = [run(w) for w in sorted({most, max(1, most // 4)})]
    best = max(runs, key=lambda r: r["value"])
    best["other_worker_counts"] = [{"cores": r["cores"], "value": r["value"], "proofs_per_s": r["proofs_per_s"]} for r in runs if r is not best]
    return best


def _cpu_worker(spec):
    shape_args, hash_mode, lookup_bits, budget_s = json.loads(spec)
    r = cpu_baseline(tuple(shape_args), hash_mode, lookup_bits, budget_s)
    print(json.dumps({"cells": r["_cells"], "proofs": r["_proofs"], "seconds": r["_seconds"]}))


def kernel_source_sha16():
    """sha256 over the kernel sources the library is built from (csrc/*.h, *.hip, *.cpp): committed PMC evidence names the sources it was taken on."""
    import hashlib
    h = hashlib.sha256()
    src = os.path.join(ROOT, "halo2-plonky2-verifier_amd", "csrc")
    for f in sorted(os.listdir(src)):
        if f.endswith((".h", ".hip", ".cpp")):
            h.update(f.encode()); h.update(open(os.path.join(src, f), "rb").read())
    return h.hexdigest()[:16]


DUMP_SAMPLE_CELLS = 1 << 19     # --dump-outputs: advice cells in the seeded sample (8 float64 limbs each: 32 MB)


def dump_outputs(dirname, plan, adv, ws, n_proofs, blocks, stream):
    """--dump-outputs: what one launch of the timed path hands its caller, as float64 arrays (every value exact) in dirname:
    status.npy: the device status word of each proof;
    advice_digest.npy: h2w_advice_digest of each of `blocks` equal blocks of the advice buffer (a proof each, unless sharded), its 4 u64 words as 8 u32 limbs;
    advice_sample.npy: a fixed, seeded sample of the buffer's 32-byte cells, each as 8 u32 limbs (little-endian), at the indices in advice_sample_cells.npy."""
    import numpy as np
    import torch
    os.makedirs(dirname, exist_ok=True)
    n = adv.numel() // 32
    per = n // blocks
    dig = torch.zeros(blocks * 4, dtype=torch.int64, device=adv.device)
    for j in range(blocks):
        plan.advice_digest(adv.data_ptr() + j * per * 32, per, dig.data_ptr() + j * 32, stream)
    torch.cuda.synchronize()
    idx = np.unique(np.random.default_rng(0xD0B5).integers(0, n, min(DUMP_SAMPLE_CELLS, n)))
    cells = adv.view(torch.int32).view(n, 8)
    chunk = 1 << 26      # cells per gather: the element indices inside one gather stay below 2^31
    parts = []
    for lo in range(0, n, chunk):
        sel = idx[np.searchsorted(idx, lo):np.searchsorted(idx, lo + chunk)] - lo
        if len(sel):
            parts.append(cells[lo:lo + chunk].index_select(0, torch.from_numpy(sel).to(adv.device)).cpu())

    def limbs(t):
        return t.numpy().view(np.uint32).astype(np.float64)
    np.save(os.path.join(dirname, "status.npy"), np.array(plan.status(ws.data_ptr(), n_proofs, stream), dtype=np.float64))
    np.save(os.path.join(dirname, "advice_digest.npy"), limbs(dig.cpu()).reshape(blocks, 8))
    np.save(os.path.join(dirname, "advice_sample.npy"), limbs(torch.cat(parts)).reshape(-1, 8))
    np.save(os.path.join(dirname, "advice_sample_cells.npy"), idx.astype(np.float64))


def _spawn_ranks(n):
    """`--gpus N` without a launcher: start N fresh rank processes (one per GPU) BEFORE anything touches the GPU here, relay rank 0's
    line, exit with the worst rank's code."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC (RCCL across processes on this driver)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=True))
    out0 = procs[0].communicate()[0]
    rcs = [p.wait() for p in procs]
    sys.stdout.write(out0)
    sys.exit(max(abs(rc) for rc in rcs))


def main():
    """A rank that dies leaves its traceback in a per-rank log file (an unattended multi-GPU run shows only rank 0's stdout)."""
    try:
        return _main()
    except BaseException as e:
        if isinstance(e, SystemExit) and not e.code:
            raise
        import traceback
        rank = os.environ.get("RANK", "0")
        logdir = os.environ.get("H2W_BENCH_LOG_DIR", os.path.join(ROOT, "gpurun_out"))
        try:
            os.makedirs(logdir, exist_ok=True)
            with open(os.path.join(logdir, f"bench_rank{rank}.log"), "a") as f:
                f.write(f"---- {time.strftime('%Y-%m-%d %H:%M:%S')} argv={sys.argv[1:]} WORLD_SIZE={os.environ.get('WORLD_SIZE')}\n")
                traceback.print_exc(file=f)
        except OSError:
            pass
        sys.stderr.write(f"[bench.py rank {rank}] failed: {e!r}\n")
        raise


def _main():
    if len(sys.argv) == 3 and sys.argv[1] == "--cpu-worker":
        return _cpu_worker(sys.argv[2])
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--config", default="cfg3", choices=sorted(CONFIGS))
    ap.add_argument("--hash", default="bn254", choices=["bn254", "gl"])
    ap.add_argument("--batch", type=int, default=0, help="proofs per launch (0 = auto: ~58 GB of advice per launch)")
    ap.add_argument("--streams", type=int, default=4, help="launches in flight, each on its own HIP stream with its own advice / workspace buffers")
    ap.add_argument("--launches-per-step", type=int, default=24)
    ap.add_argument("--lookup-bits", type=int, default=21)
    ap.add_argument("--advice-cap-gb", type=float, default=262.0, help="upper bound on the advice buffers of all launches in flight (the stream count is reduced to fit)")
    ap.add_argument("--calib", type=int, default=3, help="--full: isolated launches after the timed region (one at a time, chain kernel on the caller's stream) for the per-kernel roofline numbers")
    ap.add_argument("--proofs", default="valid", choices=["valid", "random"], help="synthetic inputs: valid FRI instances generated on the GPU by the ingest rank (h2w_prove_fri_batch, SURVEY 8d variant A) or uniform random words (variant B)")
    ap.add_argument("--shard-queries", action="store_true", help="N > 1: shard the (proof, query) units of the SAME proofs over the ranks (strong scaling; default for cfg5)")
    ap.add_argument("--layout", default="flat", choices=["flat", "columns"], help="columns: every kernel writes the FlexGate column layout directly (h2w_fri_witness_batch_columns, SURVEY 8f row 1)")
    ap.add_argument("--k", type=int, default=22, help="--layout columns: rows per column = 2^k")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines")
    ap.add_argument("--no-extras", action="store_true", help="--full: skip the legs beside the primary metric (one-proof latency, Goldilocks-caps secondary, eager boundary)")
    ap.add_argument("--full", action="store_true", help="also run the legs beside the headline figure (per-kernel roofline, latency, secondary, eager and replay, CPU baselines); "
                                                        "a plain run sets up, warms up, times --steps steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last step computed to DIR/*.npy (float64; see dump_outputs)")
    ap.add_argument("--compact", action="store_true", help="--shard-queries: every rank writes a packed buffer of its own blocks (h2w_fri_witness_batch_shard_compact; the default there)")
    ap.add_argument("--flat-shards", action="store_true", help="--shard-queries: every rank keeps a full-size advice buffer and writes its blocks at their global offsets")
    ap.add_argument("--no-fork", action="store_true", help="experiment: PoseidonBN254 chain kernels on the caller's stream (H2W_OPT_FORK_CHAINS = 0)")
    ap.add_argument("--serial-expand", type=int, default=-1, choices=[-1, 0, 1], help="H2W_OPT_SERIAL_EXPAND (-1: the library's default)")
    ap.add_argument("--chain-passes", type=int, default=0, choices=[0, 1, 2], help="H2W_OPT_CHAIN_PASSES (0: the library's default)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="torch.distributed backend for N>1 (nccl = RCCL; gloo only for rehearsing the N>1 logic on one GPU)")
    ap.add_argument("--share-gpu0", action="store_true", help="rehearsal only: every rank uses cuda:0")
    ap.add_argument("--emulate-rank", type=int, default=-1, help="N = 1: run what rank R of --world ranks runs in the (proof, query)-sharded mode, on this one GPU, and report that rank's own rate")
    ap.add_argument("--world", type=int, default=0, help="--emulate-rank: the world being emulated (default 8)")
    ap.add_argument("--gen-budget-s", type=float, default=300.0, help="rank 0 stops generating valid proofs after this many seconds and repeats the ones it has (the other ranks wait in the broadcast)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:       # a plain run: the headline figure only
        args.calib = 0; args.no_extras = args.no_cpu_baseline = True
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return _spawn_ranks(args.gpus)          # (nothing has touched the GPU yet)

    import torch
    import torch.distributed as dist
    import numpy as np
    h2w = importlib.import_module("halo2-plonky2-verifier_amd")
    api = importlib.import_module("halo2-plonky2-verifier_amd.api")
    D = importlib.import_module("halo2-plonky2-verifier_amd.distributed")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world} (launch one rank per GPU, or drop WORLD_SIZE to let bench.py spawn them)")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend=args.backend, rank=rank, world_size=world)
    if args.share_gpu0:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    d, q, rb, desc = CONFIGS[args.config]
    hash_mode = 1 if args.hash == "bn254" else 0
    emulate = args.emulate_rank >= 0
    if emulate:
        assert world == 1, "--emulate-rank is a single-process mode"
        args.world = args.world or 8
        assert 0 <= args.emulate_rank < args.world
    shard_queries = ((args.shard_queries or args.config == "cfg5") and world > 1) or emulate
    sh_rank, sh_world = (args.emulate_rank, args.world) if emulate else (rank, world)      # the sharding a launch runs with
    if shard_queries and not args.flat_shards:
        args.compact = True          # a rank's buffers hold its own blocks only: 1 / world of the stream, so world x the launches fit in flight
    shape = h2w.fibonacci_shape(d, q, rate_bits=rb, hash_mode=hash_mode, lookup_bits=args.lookup_bits)
    # Poseidon constants: the published plonky2 / circomlib parameter sets the reference links in (h2w_poseidon_published;
    # pinned to published known-answer vectors in tests/test_poseidon_published.py).
    consts = h2w.published_consts()
    plan = api.Plan(shape, consts, local_rank)
    if args.no_fork:
        plan.configure(OPT_FORK_CHAINS, 0)
    if args.serial_expand >= 0:
        plan.configure(OPT_SERIAL_EXPAND, args.serial_expand)
    if args.chain_passes:
        plan.configure(OPT_CHAIN_PASSES, args.chain_passes)

    cell_bytes = plan.num_cells * 32
    bps = None
    if args.layout == "columns":
        assert not shard_queries, "--layout columns is a single-rank / proof-sharded mode"
        bps = plan.break_points(args.k)
        cell_bytes = ((len(bps) + 1) << args.k) * 32      # a proof's columns: (break points + 1) x 2^k cells
    B = args.batch if args.batch > 0 else max(1, min(64, int(58.6e9 // cell_bytes)))
    S = max(1, args.streams)
    if shard_queries and args.compact:
        # A sharded rank must be bound by its work, not by the serial strands of a launch (VERDICT r03 task 1): a launch covers B x world proofs, so
        # the rank's (proof, query) units and bytes per launch are those of an unsharded launch of B proofs - its packed buffers are 1 / world of
        # the stream, so it fits.  (Round 3 kept B and raised the launches in flight instead: every kernel but the expansion ran at its serial floor.)
        B = min(B * sh_world, 65535)
    if args.share_gpu0:
        args.advice_cap_gb /= world
    free_b, _total_b = torch.cuda.mem_get_info(dev)         # leave 8 GB for the proofs and the allocator
    args.advice_cap_gb = min(args.advice_cap_gb, (free_b / (world if args.share_gpu0 else 1) - 8e9) / 1e9)

    def launch_bytes(b):
        adv = plan.shard_cells(b, sh_rank, sh_world) * 32 if (shard_queries and args.compact) else b * cell_bytes
        return adv + (plan.shard_workspace_bytes(b, sh_rank, sh_world) if shard_queries else plan.workspace_bytes(b))
    while S > 3 and S * launch_bytes(B) > args.advice_cap_gb * 1e9:      # stay inside the 288 GB of HBM: fewer launches in flight ...
        S -= 1
    while B > sh_world and S * launch_bytes(B) > args.advice_cap_gb * 1e9:      # ... then smaller ones
        B -= sh_world if shard_queries else 1
    while S > 1 and S * launch_bytes(B) > args.advice_cap_gb * 1e9:
        S -= 1
    R = max(args.launches_per_step, 1)
    total_proofs = B if shard_queries else B * world      # distinct proofs resident per step (every launch of a rank re-uses its B proofs)

    # ---- inputs: rank 0 synthesises all proofs, one RCCL broadcast moves the proof block
    words = plan.proof_words
    gen_seconds = n_generated = None
    if args.proofs == "valid" and args.backend != "gloo":
        # valid FRI instances (SURVEY 8d variant (A)): random committed polynomials, proved on the ingest rank's GPU in lockstep batches;
        # the proofs never visit the host.
        all_proofs = torch.zeros(total_proofs * words, dtype=torch.int64, device=dev)
        if rank == 0:
            t_gen = time.perf_counter()
            pr = api.Prover(shape, consts, local_rank)
            assert pr.proof_words == words
            gen = torch.Generator(device=dev); gen.manual_seed(0xF1B00000)
            chunk = max(1, min(total_proofs, (8 << 21) >> (d + rb)))              # ~5 GB of prover scratch at a time
            n_generated = total_proofs
            for first in range(0, total_proofs, chunk):
                if first and time.perf_counter() - t_gen > args.gen_budget_s:      # the other ranks are waiting in the broadcast: repeat what there is
                    n_generated = first
                    for at in range(first, total_proofs, first):
                        nb = min(first, total_proofs - at)
                        all_proofs[at * words:(at + nb) * words] = all_proofs[:nb * words]
                    break
                nb = min(chunk, total_proofs - first)
                coefs = torch.randint(0, 1 << 62, (nb * pr.num_polys << d,), dtype=torch.int64, device=dev, generator=gen)   # < 2^62 < p: canonical
                pr.prove_batch(coefs.data_ptr(), [1, 1, 2] * nb, all_proofs[first * words:].data_ptr(), nb, torch.cuda.current_stream(dev).cuda_stream)
                torch.cuda.synchronize(dev)
            gen_seconds = time.perf_counter() - t_gen
            pr.close(); del coefs
            torch.cuda.empty_cache()
        D.broadcast_proofs(all_proofs, src=0)       # the only collective (RCCL over xGMI): ingest rank -> all ranks
    else:
        host = torch.empty(total_proofs * words, dtype=torch.int64)
        if rank == 0:      # uniform random proof words (witness generation does not branch on validity, SURVEY 8d variant (B)); every word < 2^60:
            prng = np.random.default_rng(0xF1B00000)     # Goldilocks words canonical (< p), every 4-word hash a canonical Fr (< 2^252 < r)
            host[:] = torch.from_numpy(prng.integers(0, 1 << 60, total_proofs * words, dtype=np.int64))
        if args.backend == "gloo":                      # rehearsal: broadcast on the host, then upload
            D.broadcast_proofs(host, src=0)
            all_proofs = host.to(dev)
        else:
            all_proofs = host.to(dev)
            D.broadcast_proofs(all_proofs, src=0)       # the only collective (RCCL over xGMI): ingest rank -> all ranks
    if shard_queries:
        my_proofs = all_proofs
    else:
        lo, hi = D.shard_range(total_proofs, world, rank)
        assert hi - lo == B
        my_proofs = all_proofs[lo * words:hi * words]

    adv_bytes = plan.shard_cells(B, sh_rank, sh_world) * 32 if (shard_queries and args.compact) else B * cell_bytes
    # (zeroed for --dump-outputs: cells a mode leaves unwritten, such as other ranks' blocks, are then the same in every run)
    advices = [(torch.zeros if args.dump_outputs else torch.empty)(adv_bytes, dtype=torch.uint8, device=dev) for _ in range(S)]
    wss = [torch.empty(plan.shard_workspace_bytes(B, sh_rank, sh_world) if shard_queries else plan.workspace_bytes(B), dtype=torch.uint8, device=dev) for _ in range(S)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(S)]
    torch.cuda.synchronize()
    counter = [0]

    def launch(i=None):
        if i is None:
            i = counter[0] % S; counter[0] += 1
        if bps is not None:
            plan.run_columns(my_proofs.data_ptr(), B, bps, args.k, advices[i].data_ptr(), wss[i].data_ptr(), streams[i].cuda_stream)
        elif shard_queries:
            (plan.run_shard_compact if args.compact else plan.run_shard)(my_proofs.data_ptr(), B, advices[i].data_ptr(), wss[i].data_ptr(), sh_rank, sh_world, streams[i].cuda_stream)
        else:
            plan.run(my_proofs.data_ptr(), B, advices[i].data_ptr(), wss[i].data_ptr(), streams[i].cuda_stream)

    def step():
        for _ in range(R):
            launch()

    warm_steps = max(args.warmup, 1) if R >= 2 * S else max(args.warmup, -(-2 * S // R))      # every stream's buffers are touched twice before the clock starts
    for _ in range(warm_steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    elapsed = D.max_over_ranks(elapsed, torch.device("cpu") if args.backend == "gloo" else dev)
    for i in range(S):
        status = plan.status(wss[i].data_ptr(), B, streams[i].cuda_stream)
        assert status == [0] * B, f"device status {status}"
    if args.dump_outputs and rank == 0:       # every launch of a step runs on the same proofs: the buffers of the step's last launch
        last = (counter[0] - 1) % S
        dump_outputs(args.dump_outputs, plan, advices[last], wss[last], B, 1 if shard_queries else B, streams[last].cuda_stream)

    # per-kernel timing from the HIP events the library records on the streams it launches on
    # (a) over the timed region (launches overlap each other there, so these intervals include time-sharing);
    KEYS2 = ("prologue_values", "perm_records", "glue_strands" if hash_mode == 1 else "glue_and_merkle_strands", "chain_values", "chain_emit", "expand", "launch")
    KEYS1 = KEYS2[:3] + ("merkle_chains", None, "expand", "launch")        # one pass: ms[3] is k_merkle_bn_fused, ms[4] nothing

    def by_kernel(rows):
        passes = int(rows[0][7]) if hash_mode == 1 else 0
        keys = KEYS1 if passes == 1 else KEYS2
        avg = [sum(t[k] for t in rows) / len(rows) for k in range(7)]
        return {kk: avg[i] for i, kk in enumerate(keys) if kk and not (hash_mode == 0 and kk.startswith("chain_"))}, passes

    nback = min(args.steps * R, 64)
    overl, passes_timed = by_kernel([plan.timing_ex(i) for i in range(nback)])
    # how the expansion kernels of successive launches lie against each other (H2W_EV_EXPAND_START = 6, _END = 7): the gap from the
    # end of one to the start of the next (negative = they overlapped) and the spacing of their ends = the steady-state launch period
    ng = min(nback - 1, 24)
    gaps = [plan.event_gap(i + 1, 7, i, 6) for i in range(ng)]
    period = [plan.event_gap(i + 1, 7, i, 7) for i in range(ng)]
    schedule = {"launches": ng, "expand_end_to_next_expand_start_ms": {"avg": sum(gaps) / ng, "min": min(gaps), "max": max(gaps)},
                "expand_end_to_next_expand_end_ms": {"avg": sum(period) / ng, "min": min(period), "max": max(period)}} if ng > 0 else None

    # (b) isolated: one launch at a time on one stream, the chain kernels on the same stream (no intra-launch overlap), so that every
    #     kernel's event interval is its own duration; with PoseidonBN254 caps in both forms of the Merkle paths (H2W_OPT_CHAIN_PASSES)
    def isolated(passes=None):
        plan.configure(OPT_FORK_CHAINS, 0)
        if passes is not None:
            plan.configure(OPT_CHAIN_PASSES, passes)
        rows = []
        for _ in range(args.calib + 1):
            torch.cuda.synchronize()
            launch(0)
            torch.cuda.synchronize()
            rows.append(plan.timing_ex(0))
        plan.configure(OPT_FORK_CHAINS, 0 if args.no_fork else 1)
        plan.configure(OPT_CHAIN_PASSES, args.chain_passes)
        return by_kernel(rows[1:])[0]

    isol = isol_other = None
    if args.calib > 0:
        isol = isolated()
        if hash_mode == 1:
            isol_other = isolated(2 if passes_timed == 1 else 1)
    # (c) the expansion kernel with its launches back to back on the bench's streams (h2w_fri_expand_records: expansion only),
    #     three rounds over all streams; aggregate bytes / wall time
    b2b_gbs = None
    if args.calib > 0 and not shard_queries and bps is None:
        torch.cuda.synchronize()
        tb = time.perf_counter()
        rounds = 3
        for _ in range(rounds):
            for i in range(S):
                plan.expand_records(B, advices[i].data_ptr(), wss[i].data_ptr(), streams[i].cuda_stream)
        torch.cuda.synchronize()
        b2b_gbs = rounds * S * B * plan.num_record_cells * 32 / (time.perf_counter() - tb) / 1e9
    # (d) latency of ONE proof: a launch of a single proof, start to finish on an idle GPU (the library's default schedule), median of 10
    def one_proof_ms(pl, proof_ptr, adv, ws):
        st = streams[0].cuda_stream
        ts = []
        for _ in range(11):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            pl.run(proof_ptr, 1, adv.data_ptr(), ws.data_ptr(), st)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t1) * 1e3)
        return sorted(ts[1:])[len(ts[1:]) // 2]

    latency = None
    if args.calib > 0 and world == 1 and not args.no_extras and bps is None:
        latency = {("%s_%s_batch1_ms" % (args.config, args.hash)): one_proof_ms(plan, my_proofs.data_ptr(), advices[0], wss[0]),
                   "what": "wall time of one h2w_fri_witness_batch call on a single proof, enqueue to completion on an idle GPU (median of 10)"}
    n_ranks_seen = 1
    if world > 1:      # how many ranks the collective library itself saw: a sum of ones over RCCL (gloo in rehearsals)
        ones = torch.ones(1, dtype=torch.int64, device=torch.device("cpu") if args.backend == "gloo" else dev)
        dist.all_reduce(ones, op=dist.ReduceOp.SUM)
        n_ranks_seen = int(ones.item())
    per_rank = None
    if world > 1 and isol:
        gathered = [None] * world
        dist.all_gather_object(gathered, {"rank": rank, "kernel_ms_isolated": isol})
        per_rank = gathered

    # ---- secondary legs (N = 1): the same shape with Goldilocks-Poseidon caps; the level-1 (eager NativeChip) boundary
    secondary = eager = None
    if world == 1 and not emulate and not args.no_extras and args.config == "cfg3" and hash_mode == 1 and bps is None:
        for t in advices + wss:
            del t
        advices.clear(); wss.clear()
        torch.cuda.empty_cache()
        gshape = h2w.fibonacci_shape(d, q, rate_bits=rb, hash_mode=0, lookup_bits=args.lookup_bits)
        gplan = api.Plan(gshape, consts, local_rank)
        gB = max(1, int(58.6e9 // (gplan.num_cells * 32))); gS = max(1, args.streams)      # the primary's schedule: the same bytes per launch, the same launches in flight
        prng = np.random.default_rng(0xF1B00003)
        gproofs = torch.from_numpy(prng.integers(0, 1 << 60, gB * gplan.proof_words, dtype=np.int64)).to(dev)
        gadv = [torch.empty(gB * gplan.num_cells * 32, dtype=torch.uint8, device=dev) for _ in range(gS)]
        gws = [torch.empty(gplan.workspace_bytes(gB), dtype=torch.uint8, device=dev) for _ in range(gS)]

        while len(streams) < gS:
            streams.append(torch.cuda.Stream(device=dev))

        def glaunches(n):
            for j in range(n):
                gplan.run(gproofs.data_ptr(), gB, gadv[j % gS].data_ptr(), gws[j % gS].data_ptr(), streams[j % gS].cuda_stream)
        glaunches(3 * gS); torch.cuda.synchronize()      # three full rounds over the streams before the clock starts
        nl = 96
        t1 = time.perf_counter(); glaunches(nl); torch.cuda.synchronize(); gt = time.perf_counter() - t1
        # its dominant kernel alone (HIP events of the library on the launch stream, as for the primary): the expansion kernel
        gplan.configure(OPT_FORK_CHAINS, 0)
        grows = []
        for _ in range(args.calib + 1):
            torch.cuda.synchronize(); gplan.run(gproofs.data_ptr(), gB, gadv[0].data_ptr(), gws[0].data_ptr(), streams[0].cuda_stream); torch.cuda.synchronize()
            grows.append(gplan.timing_ex(0))
        gplan.configure(OPT_FORK_CHAINS, 1)
        g_ms = {kk: sum(r_[i] for r_ in grows[1:]) / len(grows[1:]) for i, kk in enumerate(("prologue_values", "perm_records", "glue_and_merkle_strands", None, None, "expand", "launch")) if kk}
        g_bytes = gB * gplan.num_record_cells * 32
        secondary = {"workload": f"{args.config} with Goldilocks-Poseidon Merkle caps ({gplan.num_cells} cells = {gplan.num_cells * 32 / 1e9:.1f} GB per proof), uniform random proof words",
                     "value": gplan.num_cells * gB * nl / gt, "unit": "cells/s", "proofs_per_launch": gB, "launches": nl, "launches_in_flight": gS, "seconds": gt,
                     "frac_of_hbm_peak": gplan.num_cells * gB * nl * 32 / gt / 1e9 / HBM_PEAK_GBS,
                     "kernel_ms_isolated": g_ms,
                     "roofline": {"bound": "hbm", "kernel": "expand_fast<%d, true>" % args.lookup_bits, "algorithmic_bytes": g_bytes, "achieved": g_bytes / (g_ms["expand"] * 1e-3) / 1e9,
                                  "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": g_bytes / (g_ms["expand"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                  "note": "32 B x the cells the expansion kernel writes per launch / its duration launched alone (the other kernels of this mode write records, not advice)"},
                     "same_as_primary_with": "--hash gl"}
        if latency is not None:
            latency[f"{args.config}_gl_batch1_ms"] = one_proof_ms(gplan, gproofs.data_ptr(), gadv[0], gws[0])
        del gadv, gws
        gplan.close(); torch.cuda.empty_cache()
        # the literal drop-in of north_star: the verifier's chips drive NativeChip-level calls (field/native.rs:28-193), one per operation, values
        # on the host; the cells are materialised on the GPU from the recorded block records when the advice is asked for
        hp = my_proofs[:plan.proof_words].cpu().numpy().astype(np.uint64)
        ctx = api.Context(args.lookup_bits, True, local_rank)
        t1 = time.perf_counter()
        api.verify_stark(ctx, shape, consts, hp)
        t2 = time.perf_counter()
        ptr = ctx.advice_device()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        eager = {"workload": f"{args.config}, PoseidonBN254 caps: h2w_chip_verify_stark = the gadget stack over nothing but the level-1 / level-2 C ABI (one call per NativeChip / GoldilocksChip operation)",
                 "cells": ctx.num_cells(), "value": ctx.num_cells() / (t3 - t1), "unit": "cells/s", "host_seconds": t2 - t1, "expand_seconds": t3 - t2, "advice_on": "device" if ptr else None}
        fp = ctx.footprint()
        ctx.reset()                      # the next proof through the same context: its host vectors are sized and mapped (h2w_ctx_reset)
        t1 = time.perf_counter()
        api.verify_stark(ctx, shape, consts, hp)
        eager["host_seconds_reused_context"] = time.perf_counter() - t1
        ctx.close()
        # a NEW context whose vectors were sized and mapped ahead (h2w_ctx_reserve with the footprint of an earlier run of the shape): what the first proof of a
        # service costs once the faults are taken out of the run (reserve_seconds: taking them, ahead of time)
        ctx = api.Context(args.lookup_bits, True, local_rank)
        t0 = time.perf_counter()
        ctx.reserve(*fp)
        t1 = time.perf_counter()
        api.verify_stark(ctx, shape, consts, hp)
        eager["host_seconds_reserved_context"] = time.perf_counter() - t1
        eager["reserve_seconds"] = t1 - t0
        eager["footprint"] = {"records": fp[0], "literal_cells": fp[1]}
        ctx.close()
        # record and replay (include/h2w.h 2d): the SAME operator-level run recorded once (trace mode), lowered by h2w_plan_from_trace, and replayed by
        # h2w_fri_witness_batch on the other proofs of the step - the reference's circuit as its own chips drive it, at GPU speed, with no hand-restated
        # gadget in between (the 190 G cells/s primary path above runs csrc/verifier.h, a restatement)
        try:
            tctx = api.Context(args.lookup_bits, True, local_rank)
            tctx.trace_begin()
            t1 = time.perf_counter()
            api.verify_stark(tctx, shape, consts, hp)
            t2 = time.perf_counter()
            rplan = api.Plan.from_trace(tctx, plan.proof_words, device_id=local_rank)
            t3 = time.perf_counter()
            tctx.close()
            # a replay launch is as long as its longest lane (the prologue's sponge: ~100 ms of ONE wavefront whatever the batch), so its rate is the batch and the
            # launches in flight: two streams (the root kernel of one launch is two wavefronts: it runs beside the Merkle lanes of the other), as many proofs as fit
            free_now, _ = torch.cuda.mem_get_info(dev)
            per_proof = rplan.num_cells * 32 + rplan.workspace_bytes(64) // 64
            rS = 2
            rB = int(max(8, min(96, (free_now - 12e9) // (rS * per_proof))))
            rproofs = my_proofs.repeat((rB + B - 1) // B)[:rB * plan.proof_words].contiguous()
            radvs = [torch.empty(rB * rplan.num_cells * 32, dtype=torch.uint8, device=dev) for _ in range(rS)]
            rwss = [torch.empty(rplan.workspace_bytes(rB), dtype=torch.uint8, device=dev) for _ in range(rS)]
            while len(streams) < rS:
                streams.append(torch.cuda.Stream(device=dev))
            for j in range(rS):
                rplan.run(rproofs.data_ptr(), rB, radvs[j].data_ptr(), rwss[j].data_ptr(), streams[j].cuda_stream)      # warm-up
            torch.cuda.synchronize()
            rn = 6
            t4 = time.perf_counter()
            for j in range(rn):
                rplan.run(rproofs.data_ptr(), rB, radvs[j % rS].data_ptr(), rwss[j % rS].data_ptr(), streams[j % rS].cuda_stream)
            torch.cuda.synchronize()
            rt = time.perf_counter() - t4
            radv, rws, rst = radvs[0], rwss[0], streams[0].cuda_stream
            assert rplan.status(rws.data_ptr(), rB, rst) == [0] * rB
            # the replayed stream of proof 0 against the primary path's stream of the same proof (both are oracle-checked in tests/; this ties the two here)
            chk = torch.empty(plan.num_cells * 32, dtype=torch.uint8, device=dev); cws = torch.empty(plan.workspace_bytes(1), dtype=torch.uint8, device=dev)
            plan.run(my_proofs.data_ptr(), 1, chk.data_ptr(), cws.data_ptr(), rst); torch.cuda.synchronize()
            same = bool(torch.equal(chk, radv[:plan.num_cells * 32]))
            eager["replay"] = {"what": "h2w_chip_verify_stark recorded ONCE in trace mode (one proof, level-1 / level-2 calls only), lowered by h2w_plan_from_trace, replayed by h2w_fri_witness_batch on the step's proofs",
                               "value": rplan.num_cells * rB * rn / rt, "unit": "cells/s", "proofs_per_launch": rB, "launches": rn, "launches_in_flight": rS, "ms_per_launch": rt / rn * 1e3,
                               "trace_seconds": t2 - t1, "lowering_seconds": t3 - t2, "records_per_proof": rplan.num_records, "workspace_GB": rplan.workspace_bytes(rB) / 1e9,
                               "proof_0_equals_primary_path_stream": same}
            del radv, rws, chk, cws, rproofs, radvs, rwss
            rplan.close(); torch.cuda.empty_cache()
        except Exception as e:      # the side leg must not take the bench line down
            eager["replay"] = {"error": repr(e)}

    if rank == 0:
        launches = args.steps * R
        total_cells = plan.num_cells * B * launches * (1 if shard_queries else world)
        if emulate:      # the cells rank sh_rank of sh_world writes: its prologue blocks and its (proof, query) blocks (h2w_plan_shard_block)
            lay = plan.strand_layout()
            own = D.shard_cells(B, q, sh_rank, sh_world, lay[0], lay[1], lay[2])
            total_cells = own * launches
        value = total_cells / elapsed
        # roofline of the kernel with the largest isolated duration among the kernels that write the advice (32 B per cell)
        share = (1.0 / sh_world) if shard_queries else 1.0      # a rank's share of the cells of a launch
        kbytes = {"expand": B * plan.num_record_cells * 32 * share}
        if hash_mode == 1:
            kbytes["chain_emit"] = kbytes["merkle_chains"] = B * plan.num_chain_cells * 32 * share
        names = {"expand": "expand_fast<%d, true>" % args.lookup_bits if args.lookup_bits in (21, 13, 8) else "expand_kernel_t", "chain_emit": "k_merkle_bn_emit", "chain_values": "k_merkle_bn_values",
                 "merkle_chains": "k_merkle_bn_fused", "prologue_values": "k_prologue_load + k_prologue_values", "perm_records": "k_glp_emit", "glue_strands": "k_strands",
                 "glue_and_merkle_strands": "k_strands + k_merkle_gl_values"}

        def table(iso, reg):
            out_ = {}
            for kk, ms in iso.items():
                if kk == "launch":
                    continue
                ent = {"kernel": names.get(kk, kk), "ms_isolated": ms}
                if reg is not None and kk in reg:
                    ent["ms_timed_region"] = reg[kk]
                if kk in kbytes:
                    ent["algorithmic_bytes"] = kbytes[kk]; ent["achieved_GBps"] = kbytes[kk] / (ms * 1e-3) / 1e9; ent["frac"] = ent["achieved_GBps"] / HBM_PEAK_GBS
                out_[kk] = ent
            return out_
        kernels = table(isol, overl) if isol else {}
        dom, achieved = "expand", None
        if isol:
            dom = max((kk for kk in kernels if kk in kbytes), key=lambda kk: kernels[kk]["ms_isolated"])
            achieved = kernels[dom]["achieved_GBps"]
        # HBM traffic of the dominant kernel per launch: PMC counters cannot be collected from inside this process; the rocprofv3 --pmc passes of the
        # same launch (tools/collect_evidence.sh pmc: WRITE_SIZE and FETCH_SIZE in separate passes, units of 1 KiB; FETCH_SIZE doubled: gfx950
        # counts a wide streaming read at half its bytes, MI355X_MICROARCH.md) are a committed file - used only for the workload they were taken on
        traffic, traffic_src, valu = None, None, None
        pmc_file = os.path.join(ROOT, "profiles", "r04_pmc_cfg3_bn254_b64.json")
        if isol and args.config == "cfg3" and hash_mode == 1 and B == 64 and world == 1 and not shard_queries and bps is None and args.lookup_bits == 21:
            src_sha = kernel_source_sha16()
            if not os.path.exists(pmc_file):
                traffic_src = {"file": None, "why_null": "no committed PMC pass for this workload"}
            else:
                try:
                    pmj = json.load(open(pmc_file))
                    if pmj.get("kernel_source_sha16") != src_sha:
                        traffic_src = {"file": "profiles/r04_pmc_cfg3_bn254_b64.json", "why_null": f"the PMC passes were taken on kernel sources {pmj.get('kernel_source_sha16')} (commit {pmj.get('commit')}), this run is {src_sha}: stale, not reported"}
                    else:
                        ent = next(v for k_, v in pmj["merkle_path_passes_%d" % (passes_timed or 1)].items() if names[dom].split("<")[0] in k_)
                        traffic = ent["WRITE_SIZE"] * 1024 + 2 * ent["FETCH_SIZE"] * 1024
                        traffic_src = {"file": "profiles/r04_pmc_cfg3_bn254_b64.json", "commit": pmj.get("commit"), "kernel_source_sha16": src_sha, "WRITE_SIZE_KiB": ent["WRITE_SIZE"], "FETCH_SIZE_KiB": ent["FETCH_SIZE"],
                                       "unit_check": pmj.get("unit_check"),
                                       "what": "bytes per launch = (WRITE_SIZE + 2 x FETCH_SIZE) x 1024, rocprofv3 --pmc passes of tools/launch_timing.py --batch 64 (a committed run of the same launch on the same kernel sources, not this process)"}
                        if "SQ_INSTS_VALU" in ent and isol:
                            ms_dom = kernels[dom]["ms_isolated"]
                            valu = {"SQ_INSTS_VALU_per_launch": ent["SQ_INSTS_VALU"], "wave_instructions_per_s": ent["SQ_INSTS_VALU"] / (ms_dom * 1e-3),
                                    "chip_issue_rate_per_s": VALU_ISSUE_PER_S, "frac": ent["SQ_INSTS_VALU"] / (ms_dom * 1e-3) / VALU_ISSUE_PER_S,
                                    "waves": ent.get("SQ_WAVES"), "simds": 1024, "waves_per_simd": (ent["SQ_WAVES"] / 1024 if ent.get("SQ_WAVES") else None)}
                except Exception as e:      # a malformed evidence file must not take the bench line down
                    traffic, traffic_src, valu = None, {"file": "profiles/r04_pmc_cfg3_bn254_b64.json", "why_null": repr(e)}, None
        out = {
            "metric": "FRI-verifier witness cells/sec", "value": value, "unit": "cells/s",
            "n_gpus": world, "n_ranks_seen": n_ranks_seen, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "strong" if shard_queries else "weak",
            "vs_baseline": None, "dtype": "u64", "data": "synthetic",
            "config": {"workload": f"{args.config}: {desc}, {'PoseidonBN254' if hash_mode else 'Goldilocks-Poseidon'} Merkle, lookup_bits={args.lookup_bits}",
                       "step": f"{R} launches of h2w_fri_witness_batch{'_shard' if shard_queries else ''} x {B} proofs, round-robin over {S} streams ({warm_steps} warm-up steps)",
                       "proofs_per_launch": B, "launches_per_step": R, "launches_in_flight": S, "proofs_per_gpu_per_step": B * R,
                       "cells_per_proof": plan.num_cells, "includes_witness_load_cells": True,
                       "layout": ("flat advice stream" if bps is None else f"FlexGate columns written directly: {len(bps) + 1} columns of 2^{args.k} rows per proof (break points of halo2-base assign_with_constraints, 9 unusable rows)"),
                       "merkle_path_passes": passes_timed if hash_mode == 1 else None,
                       "proofs": "valid FRI instances of random polynomials, generated on the GPU by the ingest rank (h2w_prove_fri_batch)" if args.proofs == "valid" and args.backend != "gloo" else "uniform random words of the proof's shape",
                       "parallelism": (f"(proof, query) units of the same {B} proofs dealt round-robin to {sh_world} ranks, prologue blocks to rank proof mod {sh_world}; every rank launches only its own units "
                                       f"({'packed per-rank advice buffers' if args.compact else 'blocks at their global offsets'}); one broadcast of the proofs, no data-path collective"
                                       if shard_queries else f"proof-sharded x{world}, one broadcast of the proofs, no data-path collective"),
                       "emulated_rank": ({"rank": sh_rank, "world": sh_world,
                                          "what": f"ONE process on ONE GPU running exactly the launches rank {sh_rank} of {sh_world} runs (h2w_fri_witness_batch_shard_compact(rank, world) over the same {B} proofs; the broadcast skipped); "
                                                  "value = that rank's own cells / s.  The path has no data-path collective, so this is the per-GPU rate of such a run; "
                                                  f"node_projection = value x {sh_world} is arithmetic, not a measurement"} if emulate else None),
                       "rank0_generation": ({"generated": n_generated, "resident": total_proofs, "budget_s": args.gen_budget_s,
                                             "note": "rank 0 generates every proof of the step on its GPU before the one broadcast (cfg 3: ~16 proofs/s with PoseidonBN254 caps, 512 proofs at --gpus 8 = ~32 s); past the budget it repeats the proofs it has"}
                                            if n_generated is not None else None)},
            "node_projection": (value * sh_world if emulate else None),
            "proofs_per_s": total_cells / plan.num_cells / elapsed,
            "input_generation": ({"proofs": total_proofs, "seconds": round(gen_seconds, 3), "proofs_per_s": round(total_proofs / gen_seconds, 1), "where": "GPU of rank 0, outside the timed region"} if gen_seconds else None),
            "advice_GBps": value * 32 / 1e9,
            "kernel_ms_isolated": isol,
            "kernel_ms_timed_region": overl,
            "kernel_ms_isolated_per_rank": per_rank,
            "expand_schedule_timed_region": schedule,
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": (achieved / HBM_PEAK_GBS if achieved else None),
                         "limiter": ("instruction issue and the depth of a Merkle path, not bytes: one quad walks 18 dependent PoseidonBN254 permutations (~300 dependent Montgomery products each); the kernel is priced against "
                                     "HBM because advice bytes are the metric's unit - valu_issue is its second roof" if names[dom].startswith("k_merkle_bn") else "HBM writes"),
                         "valu_issue": valu, "valu_issue_frac": (valu["frac"] if valu else None),
                         "traffic": traffic, "traffic_source": traffic_src, "algorithmic_bytes": kbytes.get(dom), "kernel": names[dom], "kernels": kernels,
                         "other_merkle_path_form": ({"merkle_path_passes": 2 if passes_timed == 1 else 1, "kernels": table(isol_other, None), "launch_ms_isolated": isol_other.get("launch")} if isol_other else None),
                         "whole_job_frac": value * 32 / 1e9 / HBM_PEAK_GBS / world,
                         "expand_back_to_back_GBps": b2b_gbs, "expand_back_to_back_frac": (b2b_gbs / HBM_PEAK_GBS if b2b_gbs else None),
                         "note": "kernel = the advice-writing kernel with the largest ISOLATED duration among the kernels of the timed region; achieved = its algorithmic bytes (32 B x the cells it "
                                 f"writes per launch) / its duration, launched alone ({args.calib} launches after the timed region, one at a time, every kernel on one stream; HIP events recorded by the "
                                 "library on that stream). other_merkle_path_form: the same launch with the other setting of H2W_OPT_CHAIN_PASSES (not what the timed region ran). whole_job_frac = value x 32 B / "
                                 "peak per GPU (all kernels, overlapped launches). traffic: HBM bytes of that kernel per launch from rocprofv3 --pmc passes of the same launch (traffic_source; null for workloads without such a file)"},
            "latency": latency, "secondary": secondary, "eager": eager,
        }
        if not args.no_cpu_baseline and world == 1:      # the CPU legs run at N = 1 only (rank 0's host)
            cb = cpu_baseline((d, q, rb), hash_mode, args.lookup_bits)
            out["cpu_baseline"] = {k: v for k, v in cb.items() if not k.startswith("_")}
            out["speedup_vs_cpu_baseline"] = value / cb["value"]
            if latency is not None:
                latency["cpu_ms_per_proof"] = 1e3 / cb["proofs_per_s"]
            out["cpu_baseline_all_cores"] = cpu_baseline_all_cores((d, q, rb), hash_mode, args.lookup_bits, plan.num_cells)
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
