// traceverdict.h — what replay.hip (h2w_trace_verdict_batch: the host side) and traceverdict.hip (the kernels) share: the device tables of a traced
// plan's verdict and the launches.  The table entries themselves are verdictfmt.h's.
#pragma once
#include <hip/hip_runtime.h>
#include "verdictfmt.h"

namespace h2w {

// per instance (InstD order): its first entry in the verdict import table, its first input (InstD::in0), its shard unit (InstD::unit), its first site word
struct VInstD { uint32_t vimp0, in0, unit, site0; };
// a value of an enclosing segment: the producer's template, its instance, the value's first slot (ImpD, in whole 64-bit words)
struct VImpD { uint32_t tmpl, inst, slot, pad; };

struct TraceVerdictArgs {
    const VEntD *ents; const VInstD *vinst; const VImpD *vimps; const uint32_t *sites;      // sites: [instance][entry], from VInstD::site0
    const uint64_t *tinfo;                   // per template: {u64 elements per proof of the value stores before it, its instances}
    const uint32_t *inputs; const uint64_t *pool64; const fr_t *poolfr;      // the plan's own tables (replay.hip)
    const uint64_t *vals, *proofs; uint64_t proof_words;
    h2w_verdict_t *verdict; const uint32_t *status, *lflag;                  // status, lflag: the replay's words in the workspace (k_trace_verdict_finish)
    uint32_t nproofs, tmpl, inst0, ninst, ent0, nent; int L;                 // the launch's template: its first instance, its instances, its entries
};
// one lane per proof: the verdict's start value / the status word, in h2w_plan_status's order
void launch_trace_verdict_init(const TraceVerdictArgs &A, hipStream_t stream);
void launch_trace_verdict_finish(const TraceVerdictArgs &A, hipStream_t stream);
// one lane per (entry, proof, instance) of template A.tmpl; the caller has bounded nent * nproofs * ninst below 2^31
void launch_trace_verdict(const TraceVerdictArgs &A, hipStream_t stream);

}  // namespace h2w
