// bnemit.h — the emission of a traced plan's fused PoseidonBN254 permutations (H2W_TRACE_FUSE_BN_PERMUTE): the arguments of replay.hip's
// k_bn_emit_traced (canonical cells) and of bnemit_mont.hip's k_bn_emit_traced_mont (H2W_FORM_MONTGOMERY), its twin line for line.
// One QUAD per listed PoseidonBN254 permutation of the launch: its 4,032 cells from the entry's input state, by the one-pass emitter the compiled plan's
// k_merkle_bn_fused runs (bnquad.h QuadSinkT::bn_emit_cells<false>: it walks the S-box chain itself; 64 contiguous bytes per quad and store).  The launch
// works from a dense list of items: every (proof, entry) pair, or - sharded - `items`, the pairs of this rank's blocks (the others' entries were never
// written).  The quads of a wavefront cooperate (cross-lane moves over the whole wavefront): none leaves early, tail quads redo the last item and write
// identical bytes.  WHERE a permutation's cells go is static (BnpD, checked against the entry: status 97 if the interpreter listed another cell); only
// the state comes from the list.  Both are launched by replay.hip traced_run; the plan's tables they read are traceplan.cpp's uploads.  LDS: the tables (34.7 KB) + 10 KB of value slots per wavefront, as k_merkle_bn_fused: two blocks per CU.
#pragma once
#include "plan.h"
#include "tracelower.h"
#include "bnquad.h"

namespace h2w {

struct BnEmitArgs {
    const fr_t *bn_tab; const uint64_t *list; const BnpD *bnp; const uint32_t *items; uint64_t nitems; uint32_t nbnp;
    fr_t *out; uint64_t cell_stride; ColMap cm; FrParams P; uint32_t *status;
    uint32_t sh_world, sh_rank, sh_compact, nq; uint64_t pro_ncell, q_slot;
};
// the Montgomery instantiation's: + the plan's table with its canonical half in Montgomery form (the cells the flushes read), mont_k() (montform.h)
struct BnEmitMontArgs : BnEmitArgs { const fr_t *bn_tab_mont; fr_t mont_k; };
int launch_bn_emit_traced_mont(const BnEmitMontArgs &E, bool cols, uint32_t nblk, hipStream_t stream);      // bnemit_mont.hip

}  // namespace h2w
