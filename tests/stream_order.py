"""One protocol, "delayed producer, immediate consumer", that holds a stream-taking call to the stream order its header promises
(include/h2w.h: "stream-ordered", "no synchronisation", "`stream` waits for it").  No reference arithmetic lives here: the tests bring the words
a call must store for two input sets A and B (tests/test_gpu_stream_order.py) and this module arranges that only a call that runs in its place
on the caller's stream can store the words of A.

run_ordered(call, inputs, outputs, delay_ms, expect_no_sync):
   1. every input tensor holds B, every output tensor a sentinel; the device is idle (torch.cuda.synchronize())
   2. S = torch.cuda.Stream().  Torch's pool streams are created NON-BLOCKING (hipStreamNonBlocking): the legacy null stream does not wait for
      them and they do not wait for it.  The whole method rests on this: work that escapes to stream 0 runs at once, in front of the delay
   3. on S: a delay (torch.cuda._sleep, calibrated once per session with two events; a chain of large fills where that is not usable), event E_delay
   4. on S: A is copied into every input, device to device
   5. call(S.cuda_stream): the library call, or chain of calls, under test
   6. on S: every output is copied into a snapshot tensor of this run
   7. on S: B is copied back into every input - a kernel that runs later than its place in the stream reads B again
   8. blocked = E_delay.query(), read on the host before any wait: False proves that steps 4-7 were all enqueued while the delay was still running
   9. S.synchronize() alone; the snapshots go to the host
  10. torch.cuda.synchronize() before any buffer is released, on the failure path too: a faulty call never writes into memory handed on
  11. (snapshots, blocked)

What each fault does to the snapshot (tests/test_gpu_stream_order.py shows every one on stand-ins of torch ops, under the machine's queue setting):
   escape      a kernel launched on stream 0 runs during the delay, on B (or on the sentinels an earlier stage of a chain should have replaced)
   no wait-in  a side stream that does not wait for S: the same
   no join     a side stream S never waits for: the snapshot is taken in front of its work and holds sentinels
   stray sync  the host waits inside the call: blocked is True (expect_no_sync=True asserts it is not)
A call that may block (its header says so, or says nothing) proves the same only if the delay outlasts its enqueue: the helper times the host side
of steps 4-7 and measures the delay with events (`info`), and the test asserts the delay was at least 10x the time to the first blocking point -
where that cannot be separated, 10x the time of the same call on an idle stream (assert_delay_covers).  No pass criterion is a time: they are the
guard and exact-integer comparisons.

Streams: a test uses at most 4 at once - S, the null stream, a plan's side stream and an emit stream.  A process has 4 hardware queues on the
machines the suite runs on (GPU_MAX_HW_QUEUES=4) and streams that share a queue serialise, which would hide a fault, never invent one.

Measured on an MI355X (host side of steps 4-7, after the warm-up on the null stream, fibonacci_shape(8, 3, rate_bits=1, cap_height=2), 2 proofs): the
witness call enqueues in 0.05 - 0.12 ms unforked, in 0.3 - 0.8 ms with FORK_CHAINS 1 (with and without an emit stream, in either output form), and
in 7.6 ms at the most where the call is the first to fork from its caller stream - the plan creates the side stream of a caller stream at that
stream's first forked call, and S is new in every run.  Every other sequence here stays below 0.7 ms (h2w_prove_fri_batch aside, which waits inside).
ENQ_MEASURED_MS is that 7.6 ms, rounded up; DELAY_MS is 20x it (the floor of 100 ms does not bind).
"""
import time

ENQ_MEASURED_MS = 8.0      # the heaviest enqueue measured (module docstring)
DELAY_MS = max(100.0, 20 * ENQ_MEASURED_MS)
SENTINEL = 0xA5

_cal = {}


def _fill_chain(stream, ms_wanted, buf, per_fill_ms):
    import torch
    with torch.cuda.stream(stream):
        for _ in range(max(1, int(ms_wanted / per_fill_ms + 0.999))):
            buf.fill_(1)


def _calibrate():
    """Once per session: how many _sleep cycles, or how many fills, a millisecond is.  Sizes the delay and nothing else."""
    import torch
    if _cal:
        return _cal
    s = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cycles = 20_000_000
    try:
        with torch.cuda.stream(s):
            torch.cuda._sleep(1000)      # (the kernel's first launch loads its code)
            e0.record(s); torch.cuda._sleep(cycles); e1.record(s)
        s.synchronize()
        ms = e0.elapsed_time(e1)
        if ms > 0.5:
            _cal.update(kind="sleep", cycles_per_ms=cycles / ms)
    except (AttributeError, RuntimeError):
        pass
    if not _cal:
        buf = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
        with torch.cuda.stream(s):
            buf.fill_(1); e0.record(s)
            for _ in range(8):
                buf.fill_(1)
            e1.record(s)
        s.synchronize()
        _cal.update(kind="fill", buf=buf, per_fill_ms=max(e0.elapsed_time(e1) / 8, 1e-3))
    torch.cuda.synchronize()
    return _cal


def enqueue_delay(stream, ms):
    """A kernel, or a chain of them, that keeps `stream` busy for about `ms` milliseconds."""
    import torch
    cal = _calibrate()
    if cal["kind"] == "sleep":
        with torch.cuda.stream(stream):
            torch.cuda._sleep(int(ms * cal["cycles_per_ms"]))
    else:
        _fill_chain(stream, ms, cal["buf"], cal["per_fill_ms"])


def as_bytes(t):
    import torch
    return t.reshape(-1).view(torch.uint8)


def run_ordered(call, inputs, outputs, delay_ms=None, expect_no_sync=False, info=None):
    """inputs: [(device tensor, staged A, staged B)] - A and B device tensors of the input's shape and type, both valid inputs of the call;
    outputs: device tensors the call writes, or (tensor, fill byte) where the call needs another start value than the sentinel (a workspace: 0).
    Everything was allocated and staged on the default stream.  call(stream handle) enqueues the work under test.
    Returns ([numpy array of each output's snapshot, the output's shape and type], blocked).  info, a dict, receives enqueue_s (host time of steps 4-7),
    call_s (of step 5 alone) and delay_ms (the delay as the device's events measured it)."""
    import torch
    delay_ms = DELAY_MS if delay_ms is None else delay_ms
    _calibrate()
    outs = [(o, SENTINEL) if isinstance(o, torch.Tensor) else o for o in outputs]
    snaps = [torch.empty_like(o) for o, _ in outs]      # (made here, not inside the timed steps: an allocation may wait for the device)
    for t, a, b in inputs:
        assert a.shape == t.shape == b.shape and a.dtype == t.dtype == b.dtype
        t.copy_(b)
    for o, fill in outs:
        as_bytes(o).fill_(fill)
    for s in snaps:
        as_bytes(s).fill_(0x3C)
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    e_start, e_delay = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    try:
        e_start.record(S)
        enqueue_delay(S, delay_ms)
        e_delay.record(S)
        t0 = time.perf_counter()
        with torch.cuda.stream(S):
            for t, a, _ in inputs:
                t.copy_(a, non_blocking=True)
        t1 = time.perf_counter()
        call(S.cuda_stream)
        t2 = time.perf_counter()
        with torch.cuda.stream(S):
            for (o, _), s in zip(outs, snaps):
                s.copy_(o, non_blocking=True)
            for t, _, b in inputs:
                t.copy_(b, non_blocking=True)
        t3 = time.perf_counter()
        blocked = bool(e_delay.query())
        S.synchronize()
        host = [s.cpu().numpy() for s in snaps]
        if info is not None:
            info.update(enqueue_s=t3 - t0, call_s=t2 - t1, delay_ms=e_start.elapsed_time(e_delay), blocked=blocked)
    finally:
        torch.cuda.synchronize()
    if expect_no_sync:
        assert not blocked, "the host waited for the stream inside a call whose header says it does not synchronise (the delay had ended when the call returned)"
    return host, blocked


def assert_delay_covers(info, seconds, what):
    """The guard of a call that may block: the delay outlasted 10x `seconds` (the time to the call's first blocking point, or of the same call on an
    idle stream), so every launch in front of that point was enqueued while the delay was running."""
    assert info["delay_ms"] >= 10 * seconds * 1e3, f"{what}: a delay of {info['delay_ms']:.1f} ms does not cover 10 x {seconds * 1e3:.2f} ms"


def delay_for(seconds):
    """The delay for a call that takes `seconds` on an idle stream: 12x that (assert_delay_covers asks for 10x), DELAY_MS at least."""
    return max(DELAY_MS, 12 * seconds * 1e3)


def timed_warm_up(call):
    """The documented warm-up: the call once on the null stream, then torch.cuda.synchronize().  Then the same once more, timed: returns the host
    time of the call on an idle stream (for a call that waits inside, that holds its device work)."""
    import torch
    torch.cuda.synchronize()
    call(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call(0)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return t1 - t0
