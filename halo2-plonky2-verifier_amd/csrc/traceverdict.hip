// traceverdict.hip - the kernels of h2w_trace_verdict_batch (include/h2w.h 2d): per-proof verdicts of a TRACED plan.
//
// The chips' assert_equal calls emit no cells and the replay computes both sides of every one of them anyway: h2w_constrain_equal records them beside
// the tape (trace.h Trace::asserts), the lowering turns them into a per-template table (tracelower.h verdict_tables, verdictfmt.h), and the call
// (replay.hip) runs the interpreter on quiet lanes - values only, into the per-proof value store - and then
//   k_trace_verdict_init    one lane per proof: the verdict's start value
//   k_trace_verdict         one lane per (table entry, proof, instance) of one template: both sides of an equality out of the value store (an enclosing
//                           segment's value through the verdict import table, a literal out of the plan's pools, a proof word), compared as 256-bit
//                           values; a range site's value against its bits.  No LDS; its only stores are the verdict words' atomics
//   k_trace_verdict_finish  one lane per proof: the replay's status word, status 4 where no chip reported a condition of its own (h2w_plan_status's order)
#include <hip/hip_runtime.h>
#include "traceverdict.h"

namespace h2w {

static_assert(sizeof(h2w_verdict_t) == 16 && sizeof(VEntD) == 24 && sizeof(VInstD) == 16 && sizeof(VImpD) == 16, "the tables are read in 64-bit words");
#if defined(__HIP_DEVICE_COMPILE__)
#define TV_GLOAD32(p) (*(const __attribute__((address_space(1))) unsigned int *)(p))
#else
#define TV_GLOAD32(p) (*(const unsigned int *)(p))
#endif

// word j of operand r of a lane: the value store's addressing (replay.hip slow_get64, on the verdict's tables).  own: the lane's own store at its place
// (vals + nproofs * prefix[t] + p * ninst + inst), Lt = nproofs * ninst its slot stride
HD uint64_t tv_get64(const TraceVerdictArgs &A, uint32_t r, uint32_t j, const uint64_t *own, uint64_t Lt, uint32_t p, uint32_t vimp0, uint32_t in0) {
    const uint32_t i = ref_idx(r); const int k = ref_kind(r);
    if (k == RK_LOCAL) return H2W_GLOAD64(own + (uint64_t)(i + j) * Lt);
    if (k == RK_INPUT) return H2W_GLOAD64(A.proofs + (uint64_t)p * A.proof_words + TV_GLOAD32(A.inputs + in0 + i) + j);
    if (k == RK_LIT64) return H2W_GLOAD64(A.pool64 + i + j);
    if (k == RK_LITFR) return H2W_GLOAD64(reinterpret_cast<const uint64_t *>(A.poolfr + i) + j);
    const uint64_t *d = reinterpret_cast<const uint64_t *>(A.vimps + vimp0 + i);      // RK_IMPORT (verdict_table_check admits nothing else)
    const uint64_t d0 = H2W_GLOAD64(d), d1 = H2W_GLOAD64(d + 1);
    const uint32_t dt = (uint32_t)d0, dinst = (uint32_t)(d0 >> 32), dslot = (uint32_t)d1;
    const uint64_t pre = H2W_GLOAD64(A.tinfo + 2 * dt), ni = H2W_GLOAD64(A.tinfo + 2 * dt + 1);
    return H2W_GLOAD64(A.vals + (uint64_t)A.nproofs * pre + (uint64_t)(dslot + j) * ((uint64_t)A.nproofs * ni) + (uint64_t)p * ni + dinst);
}

__global__ __launch_bounds__(256) void k_trace_verdict_init(TraceVerdictArgs A) {
    const unsigned p = blockIdx.x * 256 + threadIdx.x;
    if (p >= A.nproofs) return;
    h2w_verdict_t v; v.flags = 0; v.n_failed = 0; v.first_query = 0xFFFFFFFFu; v.status = 0;
    A.verdict[p] = v;
}

__global__ __launch_bounds__(256) void k_trace_verdict_finish(TraceVerdictArgs A) {
    const unsigned p = blockIdx.x * 256 + threadIdx.x;
    if (p >= A.nproofs) return;
    const uint32_t s = A.status[p];
    A.verdict[p].status = s ? s : A.lflag[p];      // (the chips' conditions come first: h2w_plan_status)
}

__global__ __launch_bounds__(256) void k_trace_verdict(TraceVerdictArgs A) {
    const uint64_t Lt = (uint64_t)A.nproofs * A.ninst, gidx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (gidx >= Lt * A.nent) return;
    // neighbouring lanes: the same entry on neighbouring (proof, instance) places - the value store is [slot][place]
    const uint32_t e = (uint32_t)(gidx / Lt), g = (uint32_t)(gidx % Lt), p = g / A.ninst, inst = g % A.ninst;
    const uint64_t *E = reinterpret_cast<const uint64_t *>(A.ents + A.ent0 + e);
    const uint64_t e0 = H2W_GLOAD64(E), e1 = H2W_GLOAD64(E + 1), aux = H2W_GLOAD64(E + 2);
    const uint32_t ra = (uint32_t)e0, rb = (uint32_t)(e0 >> 32), kind = (uint32_t)(e1 >> 32);
    const uint64_t *I = reinterpret_cast<const uint64_t *>(A.vinst + A.inst0 + inst);
    const uint64_t i0 = H2W_GLOAD64(I), i1 = H2W_GLOAD64(I + 1);
    const uint32_t vimp0 = (uint32_t)i0, in0 = (uint32_t)(i0 >> 32), unit = (uint32_t)i1;
    const uint32_t site = TV_GLOAD32(A.sites + (uint32_t)(i1 >> 32) + e);      // the instance's own word (isomorphic instances may stand at different sites)
    const uint64_t *own = A.vals + (uint64_t)A.nproofs * H2W_GLOAD64(A.tinfo + 2 * A.tmpl) + g;
    h2w_verdict_t *v = A.verdict + p;
    uint64_t a[4];      // (unrolled: the words stay in registers)
    const uint32_t na = vref_words(ra);
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) a[j] = j < na ? tv_get64(A, ra, j, own, Lt, p, vimp0, in0) : 0;
    if (kind == VK_EQUAL) {
        uint64_t b[4];
        const uint32_t nb = vref_words(rb);
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) b[j] = j < nb ? tv_get64(A, rb, j, own, Lt, p, vimp0, in0) : 0;
        if (((a[0] ^ b[0]) | (a[1] ^ b[1]) | (a[2] ^ b[2]) | (a[3] ^ b[3])) == 0) return;
        atomicAdd(&v->n_failed, 1u); if (site) atomicOr(&v->flags, site); if (unit != NO_SLOT) atomicMin(&v->first_query, unit);
        return;
    }
    // a range site.  RangeChip::range_check decomposes the value into n = ceil(bits / lookup_bits) limbs, looks every limb up (the last one shifted to the
    // table's width) and, with more than one limb, constrains their sum to equal the value: a value beyond its bits fails a lookup (the flag); one that
    // does not even fit the n limbs breaks that copy constraint too (counted, as k_verdict_init counts it for the PoW response)
    const uint64_t x = a[0]; const uint32_t L = (uint32_t)A.L;
    bool flag = false; uint32_t cnt = 0;
    if (kind == VK_RANGE) {
        const uint32_t bits = (uint32_t)aux, n = (bits + L - 1) / L;
        flag = bits != 0 && bits < 64 && (x >> bits) != 0;
        cnt = (n > 1 && n * L < 64 && (x >> (n * L)) != 0) ? 1u : 0u;
    } else {
        // check_less_than_safe(a, b): range_check(a, rb = n L bits, n = ceil(bit_length(b) / L)), then range_check(a + 2^rb - b, rb): with a >= b the
        // difference is 2^rb + (a - b), which no n limbs hold
        uint32_t bl = 0; for (uint64_t t = aux; t; t >>= 1) bl++;
        const uint32_t n = (bl + L - 1) / L, rbits = n * L;
        const bool fits = rbits >= 64 || (x >> rbits) == 0, lt = x < aux;
        flag = !fits || !lt;
        cnt = n > 1 ? (fits ? 0u : 1u) + (lt ? 0u : 1u) : 0u;
    }
    if (cnt) atomicAdd(&v->n_failed, cnt);
    if (flag) atomicOr(&v->flags, site | H2W_TRACE_VERDICT_RANGE);
}

void launch_trace_verdict_init(const TraceVerdictArgs &A, hipStream_t stream) { hipLaunchKernelGGL(k_trace_verdict_init, dim3((A.nproofs + 255) / 256), dim3(256), 0, stream, A); }
void launch_trace_verdict_finish(const TraceVerdictArgs &A, hipStream_t stream) { hipLaunchKernelGGL(k_trace_verdict_finish, dim3((A.nproofs + 255) / 256), dim3(256), 0, stream, A); }
void launch_trace_verdict(const TraceVerdictArgs &A, hipStream_t stream) {
    const uint64_t lanes = (uint64_t)A.nproofs * A.ninst * A.nent;
    if (lanes) hipLaunchKernelGGL(k_trace_verdict, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, stream, A);
}

}  // namespace h2w
