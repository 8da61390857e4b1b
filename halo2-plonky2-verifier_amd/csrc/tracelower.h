// tracelower.h — the lowering of a recorded tape (trace.h) to the device program of a traced plan: host code only, no kernel, no HIP call.
// h2w_plan_from_trace (traceplan.cpp) runs its stages in order - find_fusable, lower_trace, shard_units, pack_glop_runs, group_templates -, checks
// every template's tape (tapefmt.h tape_check) and uploads the result, a LoweredPlan of plain host vectors.
#pragma once
#include <map>
#include <string>
#include <unordered_map>
#include <vector>
#include "tapefmt.h"
#include "verdictfmt.h"
#include "trace.h"

namespace h2w {

constexpr int MAX_TMPL = 48;      // (the plan's tables as the device reads them - InstD, ImpD, TmplD, BnpD - are tapefmt.h's)

// ---- the lowering's own state
struct ValInfo { uint32_t seg, slot; uint8_t width, is_static; uint32_t lit; };
struct SegInfo {
    int parent = -1, depth = 0; uint32_t name = 0;
    std::vector<uint32_t> tape; uint32_t nslots = 0; std::vector<ImpD> imps /* tmpl field holds the producer SEGMENT until templates exist */; std::vector<uint32_t> inputs;
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> imp_of;
    uint64_t cell0 = 0, rec0 = 0, ncells = 0, nrecs = 0, all_recs = 0; bool started = false;      // all_recs: with the nested segments' (ncells includes them)
    uint32_t unit = NO_SLOT;      // the depth-1 instance (shard unit) this segment is or lies in
    int tmpl = -1; uint32_t inst = 0;
    long last_const_at = -1; uint64_t last_const_cell = 0; size_t last_const_tr = 0;      // the op emitted last is a static CONST1 (its tape position, its cell): a GLOP right behind it that takes it as operand A fuses with it
    uint32_t nglp = 0;                // fused permutations (DOP_GLPERM) of this segment
    uint32_t nbnp = 0; std::vector<uint64_t> bnp_cells;      // fused PoseidonBN254 permutations (DOP_BNPERM) of this segment: their first cells
};
// The tape lowered segment by segment: what a plan is assembled from.
struct Lowered {
    std::vector<SegInfo> segs; std::vector<ValInfo> vals; std::unordered_map<uint64_t, uint32_t> val_of;      // val_of: cell offset of a handle -> value
    std::vector<uint64_t> pool64; std::map<uint64_t, uint32_t> pool64_of; std::vector<fr_t> poolfr;
    std::vector<uint64_t> meta; uint64_t nrec = 0; std::string err;
    std::vector<int> op_seg;      // the segment every trace op lies in (a scope op: the segment current behind it)
    uint64_t n_select_parts = 0;  // parts of split selects (H2W_TRACE_SPLIT_SELECTS: tapefmt.h SELIND_*) over all segments; 0: nothing was split
};
constexpr int MAX_PERM_IO = GLPERM_IO;
enum { CANON_GL = 0, CANON_BN = 1, CANON_BN_ZERO = 2 };      // CANON_BN_ZERO: the PoseidonBN254 tape recorded on a fresh context (the load_zero cell inside its first mix)
// a stretch that matched a canonical tape in op codes, record templates, widths and dataflow; const_bad: on other constants; escaped: an interior value is read outside
struct Stretch { size_t tr0, tr1; int seg, canon, nio; TraceIn in[MAX_PERM_IO]; uint64_t out[MAX_PERM_IO]; uint64_t cell0, cell1; bool const_bad, escaped; };

// ---- the stages
// The stretches of the trace that ARE a permutation on `consts` and that nothing outside reads into (H2W_TRACE_FUSE_GL_PERMUTE, _BN_PERMUTE): fuse,
// by their first trace op; glp_meta: the record block of a Goldilocks one, (template, cell relative to the block), of glp_block_cells cells;
// n_candidates / n_bn_left: the stretches recognised and left interpreted.
struct Fusable { std::map<size_t, Stretch> fuse; std::vector<uint64_t> glp_meta; uint64_t glp_block_cells = 0, n_candidates = 0, n_bn_left = 0; };
// false: err holds the message (with the entry point's name)
// (split_selects: as lower_trace - the search lowers the tape once itself)
bool find_fusable(const Trace *tr, int L, TemplateTable &tt, const char *const *parallel_scopes, size_t n_scopes, const h2w_poseidon_consts_t *consts, bool gl, bool bn, bool split_selects, Fusable &F, std::string &err);
// segments (the instances of the parallel scopes + the root) and their tapes; F's stretches as ONE op each.  LW.err: why the trace does not lower
// split_selects (H2W_TRACE_SPLIT_SELECTS): a DOP_FR_SELIND whose fetched operands do not fit the ring becomes consecutive parts instead of a refusal
void lower_trace(const Trace *tr, int L, TemplateTable &tt, const char *const *parallel_scopes, size_t n_scopes, const Fusable &F, bool split_selects, Lowered &LW);
// Shard units: the depth-1 instances in tape order (unit q: the q-th; "verify_query_round" instance q of the standard trace, where the compiled
// plan's query block q starts: AbiBackend::query_begin).  Shardable (why_unshardable empty): the root's block [0, unit 0) and the units back to back
// to the end of the stream and of the records, units 1.. all of one size (the compiled plan's StrandTable: query 0, a later query).
struct ShardUnits {
    std::vector<int> units; std::string why_unshardable;      // units: their segments
    uint32_t num_queries = 1; uint64_t pro_ncell = 0, pro_nrec = 0, q_cell0[2] = {0, 0}, q_rec0[2] = {0, 0}, q_ncell[2] = {0, 0}, q_nrec[2] = {0, 0};      // the StrandTable's numbers (unshardable: one block)
};
ShardUnits shard_units(Lowered &LW, uint64_t total_cells);
// consecutive Goldilocks-level ops -> runs (DOP_GLOPRUN)
void pack_glop_runs(Lowered &LW, const TemplateTable &tt);
// What traceplan.cpp uploads.  Isomorphic instances (equal tapes, slot counts, table sizes) share one template; tapes back to back in `tape`.
struct LoweredPlan {
    std::vector<uint32_t> tape; std::vector<TmplD> tmpls; std::vector<InstD> insts; std::vector<ImpD> imps; std::vector<uint32_t> inputs;
    std::vector<uint64_t> pool64; std::vector<fr_t> poolfr; std::vector<uint64_t> meta; uint64_t nrec = 0;
    std::vector<TapeLimits> limits;          // per template: the counts of its segments that tape_check holds its tape against (slots, imports, inputs, list slots); the caller
                                             // adds the plan-wide limits and the pointer to the template's inputs (those of its first instance: inputs + insts[inst0].in0)
    std::vector<uint32_t> unit;              // the shard unit of every instance (InstD order)
    uint32_t nglp = 0; std::vector<uint32_t> glp_unit;      // fused Goldilocks-Poseidon permutations per proof; the shard unit of every list entry
    uint32_t nbnp = 0; std::vector<BnpD> bnp; std::vector<uint32_t> bnp0;      // fused PoseidonBN254 permutations per proof; the entries; per instance its first entry
    uint64_t total_slot_lanes = 0, n_segments = 0;
    uint64_t n_select_parts = 0;             // parts of split selects in the tapes (0: the plan launches the interpreter without them)
    const uint32_t *tmpl_tape(size_t t) const { return tape.data() + tmpls[t].tape0; }      // template t's tape and its words: up to the next template's
    size_t tmpl_tape_words(size_t t) const { return (t + 1 < tmpls.size() ? tmpls[t + 1].tape0 : tape.size()) - tmpls[t].tape0; }
};
// false: err ("more than MAX_TMPL distinct scope shapes").  Takes the pools and the record meta list out of LW.
bool group_templates(Lowered &LW, const ShardUnits &U, LoweredPlan &P, std::string &err);
// H2W_TRACE_OUTPUT_FORMS: the direct cells of the lowered plan - what the interpreter and the fused PoseidonBN254 emission write themselves - as the
// complement of the record ranges (P.meta: record i covers tt.ncells(template) cells from its offset), one bit per cell, padded to whole 64-word rows
// (batch.hip k_direct_to_montgomery).  false: err - a record beyond the stream, two records on one cell, or direct + record cells != ncells.
bool direct_cell_map(const LoweredPlan &P, const TemplateTable &tt, uint64_t ncells, std::vector<uint64_t> &direct, uint64_t &n_direct, std::string &err);
// ... and the map the ranged kernel works from when the fused PoseidonBN254 permutations' cells leave their own kernel converted: `direct` without
// [BnpD::cell0, + perm_cells) of every listed permutation.  false: err - one of those cells is not a direct cell.
bool ranged_cell_map(const LoweredPlan &P, uint64_t perm_cells, const std::vector<uint64_t> &direct, std::vector<uint64_t> &ranged, std::string &err);

// ---- the verdict stage (h2w_trace_verdict_batch): runs behind group_templates, reads what the stages above left and changes none of it.
// The recorded assert_equal calls (Trace::asserts) and the level-1 range checks of the tape as a per-template table of VEntD (verdictfmt.h); every
// side of an equality becomes an old-style ref through the lowering's own map from a handle's cell to (segment, slot, width) or a literal.  A value
// of an enclosing segment goes through the verdict's OWN import table (vimps: per instance, nvimp[template] entries from vimp0[instance]) - the
// witness plan's import tables stay what they are.  why non-empty: the plan has no verdict (an operand that is no op's result handle, an operand
// interior to a fused stretch, instances of a template whose tables differ in more than the site words) - the plan itself is built as before.
struct VerdictTables {
    std::string why;
    std::vector<VEntD> ents; std::vector<uint32_t> ent0;                                   // template t's entries: [ent0[t], ent0[t + 1])
    std::vector<ImpD> vimps; std::vector<uint32_t> vimp0, nvimp;                           // vimp0: per instance (InstD order); nvimp: per template
    std::vector<uint32_t> sites, site0;                                                    // the site word of every (instance, entry): instance i's from site0[i]
    uint64_t n_asserts = 0, n_eq_lanes = 0, n_range = 0, n_tmpl = 0;                       // recorded equalities; equalities over all instances; range sites over all instances; templates with entries
};
VerdictTables verdict_tables(const Trace *tr, const Lowered &LW, const Fusable &F, const LoweredPlan &P);

}  // namespace h2w
