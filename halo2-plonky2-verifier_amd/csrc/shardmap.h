// shardmap.h — the packed layout of a sharded call (batchargs.h ShardMap, compact != 0), stated once for host and device.
//
// Rank r of W owns the prologue block of the proofs p with p % W == r and the (proof, query) units u = p * nq + q with u % W == r.  Its packed
// buffer holds only those blocks, back to back in (proof, block) order: the prologue block takes pro_ncell cells, every query block q_slot cells
// (the larger of the two query block sizes).
#pragma once
#include <stdint.h>
#include "field.h"

namespace h2w {

// Does rank r of W own block (proof, q)?  q < 0: the prologue block.  (Host code's one statement of the rule; a kernel writes it out.)
HD bool shard_owns(uint64_t W, uint64_t r, uint64_t nq, uint64_t proof, int64_t q) { return (q < 0 ? proof : proof * nq + (uint64_t)q) % W == r; }
// The local start cell of block (proof, q) in rank r's packed buffer; q < 0: the prologue block.  (The caller owns the block; the pointer a
// kernel adds the block's GLOBAL in-proof cell offsets to is out + this - the block's global start.)
HD uint64_t packed_block_start(uint64_t W, uint64_t r, uint64_t nq, uint64_t pro_ncell, uint64_t q_slot, uint64_t proof, int64_t q) {
    const uint64_t u0 = proof * nq;
    const uint64_t pro_before = (proof + W - 1 - r) / W, units_before = (u0 + W - 1 - r) / W;      // owned prologues / units of the proofs before this one
    uint64_t local = pro_before * pro_ncell + units_before * q_slot;
    if (q >= 0) {
        if (proof % W == r) local += pro_ncell;
        local += ((u0 + (uint64_t)q + W - 1 - r) / W - units_before) * q_slot;      // owned units of this proof before query q
    }
    return local;
}

}  // namespace h2w
