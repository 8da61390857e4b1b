// The lane tables of a traced plan's sharded and verdict calls (csrc/lanetable.h), on the host: the pure fill functions on one hand-made template
// set - a root, a depth-1 template of two instances (units 0, 1), a depth-2 template of four (units 0, 0, 1, 1) - for nq = 2, n in {1, 3, 65, 130},
// world in {2, 3}, every rank; the 2^31 refusals; the ownership rule (csrc/shardmap.h shard_owns), printed for the caller to hold
// h2w_plan_shard_block against.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>
#include "lanetable.h"

using namespace h2w;

static int failures = 0, n_tables = 0;
#define CHECK(c, ...) do { if (!(c)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// the rule, written out: the root's block goes with the proof, a unit with proof * nq + unit
static bool owns(uint64_t W, uint64_t r, uint64_t nq, uint64_t p, int64_t q) { return q < 0 ? p % W == r : (p * nq + (uint64_t)q) % W == r; }

int main() {
    const uint64_t nq = 2;
    const std::vector<TmplD> tmpls = {{0, 1, 1, 0, 0}, {10, 1, 2, 1, 1}, {20, 1, 4, 3, 2}};      // {tape0, nslots, ninst, inst0, depth}
    const std::vector<uint32_t> unit = {NO_SLOT, 0, 1, 0, 0, 1, 1};
    const std::vector<BnpD> bnp = {{0, 0, NO_SLOT, 0}, {100, 50, 0, 0}, {200, 150, 1, 0}, {300, 150, 1, 0}};
    for (uint64_t n : {1, 3, 65, 130})
        for (uint64_t W : {2, 3}) {
            std::map<std::pair<size_t, uint32_t>, int> emitted;      // (template, place) -> ranks that run it unmarked
            std::map<uint32_t, int> listed;
            for (uint64_t r = 0; r < W; r++) {
                Lanes L; const char *why = fill_sharded_lanes(tmpls, unit, n, nq, r, W, L); n_tables++;
                CHECK(!why, "n %llu world %llu rank %llu: refused: %s", (unsigned long long)n, (unsigned long long)W, (unsigned long long)r, why);
                CHECK(L.lane0.size() == tmpls.size() + 1 && L.lane0[0] == 0 && L.lane0[tmpls.size()] == L.words.size(), "lane0");
                // the root's section: the owned proofs in order, padding to a whole wavefront, the others in order and marked
                std::vector<uint32_t> want;
                for (uint64_t p = 0; p < n; p++) if (owns(W, r, nq, p, -1)) want.push_back((uint32_t)p);
                const size_t n_owned = want.size();
                while (want.size() % 64) want.push_back(NO_SLOT);
                for (uint64_t p = 0; p < n; p++) if (!owns(W, r, nq, p, -1)) want.push_back((uint32_t)p | 0x80000000u);
                CHECK(std::vector<uint32_t>(L.words.begin(), L.words.begin() + L.lane0[1]) == want, "n %llu world %llu rank %llu: root section", (unsigned long long)n, (unsigned long long)W, (unsigned long long)r);
                if (n == 130 && W == 2) CHECK(n_owned == 65 && want.size() == 128 + 65 && want[64] == 128 + r && want[65] == NO_SLOT && want[128] == ((uint32_t)(1 - r) | 0x80000000u), "65 owned proofs in front of the padding");
                if (n == 65 && W == 3 && r == 0) CHECK(n_owned == 22 && want[64] == (1u | 0x80000000u), "marked lanes from the next wavefront on");
                for (uint32_t p = 0; p < n_owned; p++) emitted[{0, want[p]}]++;
                // deeper sections: exactly the places whose unit the rank owns, ascending, unmarked
                for (size_t t = 1; t < tmpls.size(); t++) {
                    std::vector<uint32_t> w2;
                    for (uint64_t p = 0; p < n; p++)
                        for (uint32_t k = 0; k < tmpls[t].ninst; k++) if (owns(W, r, nq, p, unit[tmpls[t].inst0 + k])) w2.push_back((uint32_t)(p * tmpls[t].ninst + k));
                    CHECK(std::vector<uint32_t>(L.words.begin() + L.lane0[t], L.words.begin() + L.lane0[t + 1]) == w2, "n %llu world %llu rank %llu: template %zu", (unsigned long long)n, (unsigned long long)W, (unsigned long long)r, t);
                    for (size_t i = 0; i + 1 < w2.size(); i++) CHECK(w2[i] < w2[i + 1], "ascending");
                    for (uint32_t g : w2) { CHECK(!(g & 0x80000000u), "a marked unit lane"); emitted[{t, g}]++; }
                }
                // the fused PoseidonBN254 permutations of the rank's blocks
                std::vector<uint32_t> items; why = fill_sharded_bn_items(bnp, n, nq, r, W, items);
                CHECK(!why, "items refused: %s", why);
                std::vector<uint32_t> wi;
                for (uint64_t p = 0; p < n; p++) for (size_t e = 0; e < bnp.size(); e++) if (owns(W, r, nq, p, unit_query(bnp[e].unit))) wi.push_back((uint32_t)(p * bnp.size() + e));
                CHECK(items == wi, "n %llu world %llu rank %llu: items", (unsigned long long)n, (unsigned long long)W, (unsigned long long)r);
                for (uint32_t it : items) listed[it]++;
            }
            // over the ranks of a world: every (proof, instance) of every template unmarked exactly once, every (proof, entry) listed once
            size_t places = 0; for (const TmplD &T : tmpls) places += n * T.ninst;
            CHECK(emitted.size() == places, "n %llu world %llu: %zu places emitted of %zu", (unsigned long long)n, (unsigned long long)W, emitted.size(), places);
            for (const auto &e : emitted) CHECK(e.second == 1, "template %zu place %u emitted %d times", e.first.first, e.first.second, e.second);
            CHECK(listed.size() == n * bnp.size(), "items over the ranks");
            for (const auto &e : listed) CHECK(e.second == 1, "item %u listed %d times", e.first, e.second);
        }
    // the quiet table: every place of every template once, all marked, no padding
    for (uint64_t n : {1, 3, 65, 130}) {
        Lanes L; const char *why = fill_quiet_lanes(tmpls, n, L); n_tables++;
        CHECK(!why, "quiet refused: %s", why);
        std::vector<uint32_t> want, l0;
        for (const TmplD &T : tmpls) { l0.push_back((uint32_t)want.size()); for (uint64_t g = 0; g < n * T.ninst; g++) want.push_back((uint32_t)g | 0x80000000u); }
        l0.push_back((uint32_t)want.size());
        CHECK(L.words == want && L.lane0 == l0, "n %llu: the quiet table", (unsigned long long)n);
    }
    // 2^31 (proof, instance) places of one template: both refuse, with the root's section filled and nothing of the refused template
    {
        const std::vector<TmplD> big = {{0, 1, 1, 0, 0}, {10, 1, 1u << 26, 1, 1}};
        Lanes L; const char *why = fill_sharded_lanes(big, std::vector<uint32_t>(1, NO_SLOT), 32, nq, 0, 2, L);
        CHECK(why && !strcmp(why, "h2w_fri_witness_batch_shard: too many (proof, instance) lanes in one call"), "sharded: %s", why ? why : "(accepted)");
        CHECK(L.words.size() == 64 + 16, "sharded: %zu words behind the refusal", L.words.size());
        why = fill_quiet_lanes(big, 32, L);
        CHECK(why && !strcmp(why, "h2w_trace_verdict_batch: too many (proof, instance) lanes in one call; split the batch"), "quiet: %s", why ? why : "(accepted)");
        CHECK(L.words.size() == 32, "quiet: %zu words behind the refusal", L.words.size());
        std::vector<uint32_t> items;
        why = fill_sharded_bn_items(std::vector<BnpD>((1u << 16) + 2, BnpD{0, 0, NO_SLOT, 0}), 65535, nq, 0, 2, items);
        CHECK(why && !strcmp(why, "h2w_fri_witness_batch_shard: too many fused permutations in one call") && items.empty(), "items: %s", why ? why : "(accepted)");
    }
    // the ownership rule, for the caller to compare with h2w_plan_shard_block
    for (uint64_t W : {2, 3})
        for (uint64_t r = 0; r < W; r++)
            for (uint64_t p = 0; p < 130; p++)
                for (int64_t q = -1; q < (int64_t)nq; q++) {
                    CHECK(shard_owns(W, r, nq, p, q) == owns(W, r, nq, p, q), "shard_owns(%llu, %llu, %llu, %lld)", (unsigned long long)W, (unsigned long long)r, (unsigned long long)p, (long long)q);
                    printf("OWNS %llu %llu %llu %lld %d\n", (unsigned long long)W, (unsigned long long)r, (unsigned long long)p, (long long)q, shard_owns(W, r, nq, p, q) ? 1 : 0);
                }
    if (failures) { printf("FAIL %d\n", failures); return 1; }
    printf("OK tables: %d\n", n_tables);
    return 0;
}
