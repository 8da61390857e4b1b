// chipbatch.h - the handle of the batched chip operations (include/h2w.h 2c), shared by its two units: chipbatch.hip (the field chips' ops, and the
// entry points) and chiphash.hip (the hash and Merkle chips' ops: a handle with `hash` set is that unit's).
#pragma once
#include "handletabs.h"

namespace h2w { struct ChipHash; }

struct h2w_chipbatch {
    int op, L, device, nw; h2w::TemplateTable tt; h2w::DeviceTables dt; h2w::FrParams P;
    uint64_t nrec = 0, ncells = 0; h2w::DevBuf<uint64_t> d_meta; h2w::DevBuf<uint16_t> d_tmpl_cells;
    h2w::ChipHash *hash = nullptr;      // ops 9-13 (h2w_chipbatch_new_hash): parameters, tables and launch state of chiphash.hip
    explicit h2w_chipbatch(int L_) : tt(L_) {}
};

namespace h2w {
void chiphash_free(h2w_chipbatch *h);      // the ChipHash part only (its device tables are DevBufs: a delete)
int chiphash_run(h2w_chipbatch *h, const uint64_t *operands_dev, uint64_t n, void *advice_dev, uint32_t *status_dev, void *stream);      // chiphash.hip
}
