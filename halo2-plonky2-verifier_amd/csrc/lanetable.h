// lanetable.h — the lane table k_replay reads when a call does not run every (proof, instance) in place (ReplayArgs::lanes): what goes into it, as pure
// functions of the plan's templates and the call's key.  Plain C++: no HIP (tests/cpp/lanetable_check.cpp); the owner of the device copy is traceplan.h's.
//
// Template t's lanes are words [lane0[t], lane0[t + 1]): a word is g = proof * ninst + instance, the lane's place in the value store; bit 31 set: the lane
// computes its values and stores nothing else; NO_SLOT: padding (the interpreter's emit flag is uniform over a wavefront).
#pragma once
#include <cstdint>
#include <vector>
#include "tapefmt.h"
#include "shardmap.h"

namespace h2w {

constexpr uint32_t LANE_QUIET = 0x80000000u;
struct Lanes { std::vector<uint32_t> words, lane0; };
inline int64_t unit_query(uint32_t unit) { return unit == NO_SLOT ? -1 : (int64_t)unit; }      // a shard unit as shardmap.h's q (NO_SLOT: the root's block)

// The fill functions return null, or the refusal (before they fill the template it is about).
// A sharded call: the root lane of every proof - those of the proofs the rank owns first, then, from the next wavefront on, the others quiet (they
// compute the values the units import) -, and of every deeper template only the (proof, instance) pairs whose unit the rank owns (shardmap.h
// shard_owns; h2w_plan_shard_block, distributed.py unit_owner).  unit: the shard unit of every instance (InstD order).
inline const char *fill_sharded_lanes(const std::vector<TmplD> &tmpls, const std::vector<uint32_t> &unit, uint64_t n, uint64_t nq, uint64_t rank, uint64_t world, Lanes &out) {
    std::vector<uint32_t> &L = out.words; L.clear(); out.lane0.assign(tmpls.size() + 1, 0);
    for (size_t i = 0; i < tmpls.size(); i++) {
        const TmplD &T = tmpls[i]; out.lane0[i] = (uint32_t)L.size();
        if (n * T.ninst >= 0x80000000ull) return "h2w_fri_witness_batch_shard: too many (proof, instance) lanes in one call";
        if (T.depth == 0) {
            for (uint64_t pr = 0; pr < n; pr++) if (shard_owns(world, rank, nq, pr, -1)) L.push_back((uint32_t)pr);
            while ((L.size() - out.lane0[i]) % 64) L.push_back(NO_SLOT);
            for (uint64_t pr = 0; pr < n; pr++) if (!shard_owns(world, rank, nq, pr, -1)) L.push_back((uint32_t)pr | LANE_QUIET);
        } else
            for (uint64_t pr = 0; pr < n; pr++)
                for (uint32_t k = 0; k < T.ninst; k++) if (shard_owns(world, rank, nq, pr, unit_query(unit[T.inst0 + k]))) L.push_back((uint32_t)(pr * T.ninst + k));
    }
    out.lane0[tmpls.size()] = (uint32_t)L.size();
    return nullptr;
}
// ... and beside it the listed PoseidonBN254 permutations of the rank's blocks, dense: (proof, entry) as proof * nbnp + entry - the root's of the proofs
// it owns, a unit's where it owns the unit (the lanes above that run with emit set: the entries that get written)
inline const char *fill_sharded_bn_items(const std::vector<BnpD> &bnp, uint64_t n, uint64_t nq, uint64_t rank, uint64_t world, std::vector<uint32_t> &items) {
    items.clear();
    if (n * bnp.size() >= 0xffffffffull) return "h2w_fri_witness_batch_shard: too many fused permutations in one call";
    for (uint64_t pr = 0; pr < n; pr++)
        for (size_t e = 0; e < bnp.size(); e++) if (shard_owns(world, rank, nq, pr, unit_query(bnp[e].unit))) items.push_back((uint32_t)(pr * bnp.size() + e));
    return nullptr;
}
// The verdict call: every (proof, instance) place of every template, quiet - the sharded format for a world in which the rank owns nothing
inline const char *fill_quiet_lanes(const std::vector<TmplD> &tmpls, uint64_t n, Lanes &out) {
    std::vector<uint32_t> &L = out.words; L.clear(); out.lane0.assign(tmpls.size() + 1, 0);
    for (size_t i = 0; i < tmpls.size(); i++) {
        const uint64_t nl = n * tmpls[i].ninst; out.lane0[i] = (uint32_t)L.size();
        if (nl >= 0x80000000ull || L.size() + nl >= 0x80000000ull) return "h2w_trace_verdict_batch: too many (proof, instance) lanes in one call; split the batch";
        for (uint64_t g = 0; g < nl; g++) L.push_back((uint32_t)g | LANE_QUIET);
    }
    out.lane0[tmpls.size()] = (uint32_t)L.size();
    return nullptr;
}

}  // namespace h2w
