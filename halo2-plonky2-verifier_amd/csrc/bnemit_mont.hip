// bnemit_mont.hip — k_bn_emit_traced_mont: the Montgomery instantiation of a traced plan's PoseidonBN254 emission (bnemit.h; replay.hip traced_run
// launches it when the plan's output form is H2W_FORM_MONTGOMERY).  Each fused permutation's 4,032 cells are stored once, already as v * 2^256 mod r:
// the emitter is bnquad.h's one-pass form in its QUAD_FUSED_MONT mode - the flush code, the addresses (flat, columns, sharded, packed), the store
// pattern (64 contiguous bytes per quad and store) and the status-97 check are the canonical kernel's.  What differs is what the flushes read: the
// canonical half of the LDS table holds the plan's cell table in Montgomery form (host-built, uploaded when the form is first selected: traceplan.cpp traced_mont_tables), and every value
// slot is filled with fr_mont_mul(v, mont_k, ninv) - the product h2w_advice_to_montgomery and k_direct_to_montgomery apply, hence the same bytes.
// LDS: the tables (34.7 KB) + the canonical round constants the adds take (2.8 KB) + 10 KB of value slots per wavefront = 76.6 KB: two blocks per CU.
// A unit of its own: the LDS variables of a unit are laid out together, and replay.hip's interpreter keeps the layout - and the code - it has.
#include <hip/hip_runtime.h>
#include "bnemit.h"

namespace h2w {

template <bool COLS> __global__ __launch_bounds__(QUAD_BLOCK) H2W_QUAD_ATTR void k_bn_emit_traced_mont(BnEmitMontArgs A) {
    typedef QuadSinkT<COLS, QUAD_FUSED_MONT> Sink;
    stage_bn_canon_c(A.bn_tab, threadIdx.x, QUAD_BLOCK);
    stage_bn_consts(A.bn_tab_mont, threadIdx.x, QUAD_BLOCK);      // (block-wide barrier inside: before any wavefront leaves)
    if ((((uint64_t)blockIdx.x * QUAD_BLOCK + (threadIdx.x & ~63u)) >> 2) >= A.nitems) return;      // a whole wavefront past the last item
    uint64_t g = ((uint64_t)blockIdx.x * QUAD_BLOCK + threadIdx.x) >> 2;
    if (g >= A.nitems) g = A.nitems - 1;
    const uint64_t it = A.items ? (uint64_t)A.items[g] : g;      // proof * nbnp + entry
    const uint64_t p = it / A.nbnp; const uint32_t e = (uint32_t)(it % A.nbnp);
    const BnpD D = A.bnp[e];
    const uint64_t *ent = A.list + it * BNP_LIST_WORDS;
    fr_t *outb = A.out + p * A.cell_stride;
    if (A.sh_compact)           // the packed buffer: the permutation's block at its local start
        outb = A.out + packed_block_start(A.sh_world, A.sh_rank, A.nq, A.pro_ncell, A.q_slot, p, D.unit == NO_SLOT ? -1 : (int64_t)D.unit) - D.ucell0;
    if (g_load_u64(ent) != D.cell0 && (threadIdx.x & 3) == 0) atomicCAS(&A.status[p], 0u, 97u);
    fr_t st[BN_WIDTH];
#pragma unroll
    for (int i = 0; i < BN_WIDTH; i++) st[i] = g_load_fr(reinterpret_cast<const fr_t *>(ent + 2) + i);
    Sink sink; sink.recs = nullptr; sink.nrec = 0; sink.out = outb; sink.cell_off = D.cell0; sink.ncells = nullptr; sink.l4 = threadIdx.x & 3; sink.cc.init(A.cm);
    sink.ustate = nullptr; sink.sbx = nullptr; sink.mk = A.mont_k; sink.mninv = A.P.ninv;
    ValCfg cfg; cfg.proof = nullptr; cfg.mode = 1; cfg.L = 0; cfg.P = A.P; cfg.inv_pos = cfg.inv_neg = nullptr; cfg.st = nullptr; cfg.split = false; cfg.split_bn = true;
    cfg.load_items = nullptr; cfg.n_load_items = 0; cfg.load_nrec = cfg.load_ncell = 0; cfg.n_cap_items = 0; cfg.fri = nullptr;
    bool zc = true;             // (a stretch with the Context's load_zero cell in it is never fused)
    sink.template bn_emit_cells<false>(st, cfg, zc);
}

int launch_bn_emit_traced_mont(const BnEmitMontArgs &E, bool cols, uint32_t nblk, hipStream_t stream) {
    launch_cols(cols, k_bn_emit_traced_mont<true>, k_bn_emit_traced_mont<false>, dim3(nblk), dim3(QUAD_BLOCK), 0, stream, E);
    return 0;
}

}  // namespace h2w
