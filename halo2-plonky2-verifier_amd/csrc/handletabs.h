// handletabs.h — the derived tables every handle of the value backend needs, built and uploaded in ONE place (host code): the constructors of
// a compiled plan (plancompile.cpp), a traced plan (traceplan.cpp) and the batched chip ops (chipbatch.hip, chiphash.hip) call these.
#pragma once
#include "common.h"
#include "valbackend.h"
#include "glptab.h"
#include "bntab.h"

namespace h2w {

// [0, INV_TAB): 1 / k, [INV_TAB, 2 INV_TAB): -1 / k (ValCfg::inv_pos / inv_neg; entry 0 of each half is zero)
inline std::vector<fr_t> inverse_table(const FrParams &P) {
    std::vector<fr_t> inv(2 * INV_TAB, fr_zero());
    for (int k = 1; k < INV_TAB; k++) { inv[k] = fr_inv(fr_from_u64((uint64_t)k), P); inv[INV_TAB + k] = fr_neg(inv[k]); }
    return inv;
}
// cells per record of every template id (the device sinks' ncells)
inline int upload_tmpl_cells(DevBuf<uint16_t> &d, const TemplateTable &tt) {
    std::vector<uint16_t> nc(T_MAX, 0);
    for (size_t i = 0; i < tt.info.size(); i++) nc[i] = tt.info[i].ncells;
    return d.upload(nc);
}
// the Goldilocks-Poseidon constants, and behind them the derived tables of the values phase (glptab.h glp_aux_tables; glcoop.h stage_glp_consts reads them there)
struct GlpConsts : h2w_poseidon_consts_t { uint64_t aux[GLP_AUX_WORDS]; };
static_assert(sizeof(GlpConsts) == sizeof(h2w_poseidon_consts_t) + GLP_AUX_WORDS * sizeof(uint64_t), "the derived tables start where the constants end");
inline int upload_glp_consts(DevBuf<GlpConsts> &d, const h2w_poseidon_consts_t &k) {
    std::vector<GlpConsts> h(1);
    static_cast<h2w_poseidon_consts_t &>(h[0]) = k; glp_aux_tables(k, h[0].aux);
    return d.upload(h);
}
// the PoseidonBN254 tables, canonical and times R, per handle (two handles with different tables never share state); tab9: the values passes' limb-form copy
inline int upload_bn_tab(DevBuf<fr_t> &d, const h2w_poseidon_consts_t &k, const FrParams &P, DevBuf<uint32_t> *tab9 = nullptr) {
    std::vector<fr_t> tab(BK_ALL); bn_table_build(k, P, tab.data());
    if (d.upload(tab) != 0) return -1;
    if (!tab9) return 0;
    std::vector<uint32_t> t9((size_t)BK9_N * BK9_W); bn_table9_build(tab.data(), t9.data());
    return tab9->upload(t9);
}

}  // namespace h2w
