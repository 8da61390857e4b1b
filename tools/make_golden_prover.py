#!/usr/bin/env python3
"""Golden digests of the ORACLE prover's output (oracle/prover.inc) where running it inside a test would take minutes - BASELINE.json's
full sizes, and the small shape with 23 proof-of-work bits (the serial grind) -: sha256 of the flat proof words for the published Poseidon
tables and the inputs of orc_prove_fri_inputs(seed).  -> tests/golden/prover_digests.json.  The GPU generator must reproduce them
(tests/test_gpu_prover.py, tests/test_gpu_prover_shapes.py).  With case names as arguments only those are made again; the others are kept."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyoracle as O

# name: degree_bits, queries, rate_bits, hash_mode, seed, pow_bits.  The powhi seeds: the first of 0x5AFE1000.. whose smallest witness
# is at least 2^22, i.e. beyond the device prover's first search round
CASES = {"cfg2_gl": (16, 28, 2, 0, 0xF1B00000 + 16, 16), "cfg2_bn254": (16, 28, 2, 1, 0xF1B00000 + 16, 16), "cfg3_gl": (20, 28, 1, 0, 0xF1B00000 + 20, 16),
         "powhi_gl": (6, 2, 1, 0, 0x5AFE1001, 23), "powhi_bn254": (6, 2, 1, 1, 0x5AFE1000, 23)}
if __name__ == "__main__":
    k = O.published_consts()
    path = os.path.join(ROOT, "tests", "golden", "prover_digests.json")
    names = sys.argv[1:] or list(CASES)
    out = json.load(open(path)) if sys.argv[1:] else {}
    for name in names:
        d, q, rb, mode, seed, pow_bits = CASES[name]
        sh = O.fibonacci_shape(d, q, rate_bits=rb, hash_mode=mode); sh.pow_bits = pow_bits
        t = time.time()
        coefs, pis = O.prove_fri_inputs(sh, seed)
        words = O.prove_fri_coef(sh, k, coefs, pis)
        cs = 1 << sh.cap_height
        at = 8 * cs + 2 * (2 * sh.n_cols + 2 * sh.n_perm_z + sh.n_quotient) + 4 * cs      # ProofLayout::pow_witness (chips.h), with a permutation cap
        out[name] = {"degree_bits": d, "queries": q, "rate_bits": rb, "hash_mode": mode, "seed": seed, "pow_bits": pow_bits, "proof_words": len(words),
                     "sha256": hashlib.sha256(bytes(words)).hexdigest(), "pow_witness_word_index": at, "pow_witness": int(words[at]),
                     "oracle_seconds": round(time.time() - t, 1)}
        print(name, out[name], flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
