"""Hand-driven operator programs replayed on the device, op by op against the oracle (include/h2w.h 2d: "bit-identical to running the calls on each of
them").  Every other replay test traces the verifier; these trace the programs of tests/replay_prog.py - the interpreter's ops at the edges of their
operands (0, p - 1, 2^32 +- 1, quotient edges, r - 1, non-canonical words, wide x narrow), lists of 1, 2, 63 and 64 entries, and the structure of the
lowering: operands exactly 255 / 256 / 257 slots back, constants at the end of the LDS part of the pools, runs of 255 Goldilocks ops, 1 / 63 / 64 / 65
instances of a parallel scope, several templates in one launch, imports into depth 2, an op with 255 fetched operand slots.  Per proof: the whole stream
equals the oracle's bytes, the status word is the expected one, the cells at the program's handles hold the values of a plain integer model (to which
the oracle's values are held too).  The off_* programs leave the value domain proof A's eager calls validated - selectors, indicators and bits above 1,
2^128 or more in front of a reduce: such a proof has status 5 and the oracle's cells in front of the offending op, its in-domain neighbours the whole
stream; values beyond a range that do fit (num_to_bits, range_check) keep status 0.  tests/test_replay_programs_lowering.py shows, without a GPU, that each program reaches what it was written for."""
import pytest

import replay_prog as rp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("prog", rp.PROGRAMS, ids=lambda p: p.name)
def test_a_program_replays_to_the_oracles_stream(h2w, h2w_api, oracle, prog):
    for n in prog.sizes:      # one proof and a batch whose last wavefront is partial
        proofs = prog.batch(n)
        rp.check_on_device(h2w, h2w_api, oracle, prog.fn, prog.proof_a(), proofs, prog.lookup_bits, prog.scopes)


@pytest.mark.parametrize("mode", [0])
def test_replay_of_a_verifier_with_64_cap_entries(h2w, h2w_api, oracle, consts, mode):
    """cap_height 6 on Goldilocks-Poseidon caps: 64 one-word entries per hash element selected inside verify_proof_to_cap_with_cap_index, imported from
    the root (128 fetched slots).  PoseidonBN254 caps are 64 wide entries, 320 slots: h2w_plan_from_trace refuses that trace
    (tests/test_replay_programs_lowering.py)."""
    from test_gpu_replay import trace_and_replay
    trace_and_replay(h2w, h2w_api, oracle, consts, (7, 2, 1, mode), 61, [62], cap_height=6)
