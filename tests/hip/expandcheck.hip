// Device harness of tests/test_gpu_expandcheck.py: runs the product's own expansion kernels (csrc/expand.hip, compiled next to this file as a second
// translation unit; nothing else of the library is linked) on records a test wrote by hand, through launch_expand, and writes the whole output buffer
// back.  No reference arithmetic lives here: the expected cells are Python integers (tests/expand_ref.py).
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I halo2-plonky2-verifier_amd/csrc -I include tests/hip/expandcheck.hip halo2-plonky2-verifier_amd/csrc/expand.hip -o expandcheck
//   expandcheck <case file> <result file>
// One process, one case file, one device context, ONE call of launch_expand.  Exit status 0: the launch ran and the result file is complete; anything
// else: a message on stdout, and nothing was launched after the first HIP error.
//
// Case file: raw little-endian 64-bit words (mirrored by expand_ref.pack_case)
//   [0] magic "EXPCHK01"   [1] lookup_bits   [2] nproofs   [3] nrec   [4] rec_stride (records)   [5] cell_stride (cells)   [6] grid_x   [7] roam_per_cu
//   [8] work counter: 0 = tile_ctr null, 1 = nproofs zeroed 32-bit words   [9] 1 = Montgomery form   [10] ncols (0: flat)   [11] k
//   [12] guard cells in front of cell 0 and behind the last cell (>= 64)   [13..15] 0
//   starts[ncols]   meta[nrec]   recs[nproofs][rec_stride] (4 words each)
// Result file: (guard + nproofs * cell_stride + guard) cells of 32 bytes, pre-filled with the byte SENTINEL; `out` is the pointer past the front guard.
// Every case is a well-formed launch: a record whose cells would leave [0, cell_stride) is refused here, before anything runs.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "common.h"
#include "montform.h"
using namespace h2w;
namespace h2w {
thread_local std::string g_last_error;
void set_error(const std::string &s) { g_last_error = s; }
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

constexpr uint64_t MAGIC = 0x31304b4843505845ull;      // "EXPCHK01"
constexpr int SENTINEL = 0xA5, HEADER = 16;

int main(int argc, char **argv) {
    if (argc != 3) { printf("usage: expandcheck <case file> <result file>\n"); return 2; }
    std::vector<uint64_t> in;
    {
        FILE *f = fopen(argv[1], "rb"); if (!f) { printf("cannot read %s\n", argv[1]); return 2; }
        fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
        if (bytes < 8 * HEADER || bytes % 8) { printf("case file: not whole 64-bit words\n"); fclose(f); return 2; }
        in.resize((size_t)bytes / 8);
        const size_t got = fread(in.data(), 8, in.size(), f); fclose(f);
        if (got != in.size()) { printf("short read\n"); return 2; }
    }
    if (in[0] != MAGIC) { printf("case file: bad magic\n"); return 2; }
    const int lookup_bits = (int)in[1];
    const uint64_t nproofs = in[2], nrec = in[3], rec_stride = in[4], cell_stride = in[5], grid_x = in[6], roam_per_cu = in[7], ctr = in[8], mont = in[9],
                   ncols = in[10], k = in[11], guard = in[12];
    if (lookup_bits < 2 || lookup_bits > 28 || nproofs < 1 || nproofs > 4096 || nrec < 1 || rec_stride < nrec || guard < 64 || ctr > 1 || mont > 1 || grid_x < 1 || grid_x > 65535 ||
        k > 30 || ncols > 4096 || cell_stride < 1 || cell_stride > (1ull << 32) - 64 || nproofs * cell_stride > (1ull << 23)) { printf("case file: header out of range\n"); return 2; }
    if (in.size() != (size_t)HEADER + ncols + nrec + nproofs * rec_stride * 4) { printf("case file: %zu words, expected %zu\n", in.size(), (size_t)(HEADER + ncols + nrec + nproofs * rec_stride * 4)); return 2; }
    const uint64_t *starts = &in[HEADER], *meta = starts + ncols;

    // a well-formed launch: fixed templates only, every record's cells inside its proof's slice of the buffer
    TemplateTable tt(lookup_bits);
    if (ncols) {
        if (starts[0] != 0 || (ncols << k) > cell_stride) { printf("case file: column map outside the buffer\n"); return 2; }
        for (uint64_t c = 1; c < ncols; c++) if (starts[c] <= starts[c - 1] || starts[c] - starts[c - 1] > (1ull << k)) { printf("case file: column %llu longer than 2^k\n", (unsigned long long)c - 1); return 2; }
    }
    for (uint64_t i = 0; i < nrec; i++) {
        const uint32_t t = meta_tmpl(meta[i]); const uint64_t off = meta_off(meta[i]);
        if (t >= T_LITERAL) { printf("record %llu: template %u is not a fixed one\n", (unsigned long long)i, t); return 2; }
        const uint64_t end = off + (uint64_t)tt.ncells((int)t);
        // (columns: cell i lives at (c << k) + i - starts[c]; every column but the last is at most 2^k long, checked above)
        const bool ok = ncols ? end <= starts[ncols - 1] || end - starts[ncols - 1] <= (1ull << k) : end <= cell_stride;
        if (!ok) { printf("record %llu: cells [%llu, %llu) leave the buffer\n", (unsigned long long)i, (unsigned long long)off, (unsigned long long)end); return 2; }
    }

    DeviceTables dt;
    if (dt.upload(tt) != 0) { printf("DeviceTables::upload: %s\n", g_last_error.c_str()); return 1; }
    MontForm K; montform_init(K, tt.rb);      // batch.hip h2w_plan_configure
    MontForm *d_mont = nullptr; uint64_t *d_in = nullptr; uint32_t *d_ctr = nullptr; unsigned char *d_buf = nullptr;
    CK(hipMalloc((void **)&d_mont, sizeof K)); CK(hipMemcpy(d_mont, &K, sizeof K, hipMemcpyHostToDevice));
    CK(hipMalloc((void **)&d_in, in.size() * 8)); CK(hipMemcpy(d_in, in.data(), in.size() * 8, hipMemcpyHostToDevice));
    if (ctr) { CK(hipMalloc((void **)&d_ctr, nproofs * sizeof(uint32_t))); CK(hipMemset(d_ctr, 0, nproofs * sizeof(uint32_t))); }
    const size_t cells = (size_t)(guard + nproofs * cell_stride + guard);
    CK(hipMalloc((void **)&d_buf, cells * 32)); CK(hipMemset(d_buf, SENTINEL, cells * 32));

    ExpandArgs A;      // eager.cpp ensure_expanded / batch.hip launch_plan_expand
    A.meta = d_in + HEADER + ncols; A.recs = reinterpret_cast<const rec_t *>(d_in + HEADER + ncols + nrec); A.nrec = nrec; A.rec_stride = rec_stride;
    A.out = reinterpret_cast<fr_t *>(d_buf) + guard; A.cell_stride = cell_stride; A.pool = nullptr;
    A.cm = ncols ? ColMap{d_in + HEADER, (uint32_t)ncols, (uint32_t)k} : ColMap{nullptr, 0, 0};
    expand_unsharded(A);
    dt.fill(A);
    A.tile_ctr = d_ctr; A.roam_per_cu = (uint32_t)roam_per_cu; A.mont = mont ? d_mont : nullptr; A.nproofs = (uint32_t)nproofs; A.roam = 0;
    // what launch_expand's choice of kernel depends on, as far as it shows here (units256: its work units per proof, 256 records each)
    printf("conditions: counter=%d lookup_bits=%d fast_bits=%d ncols=%llu cols_fit=%d units256=%llu roam_per_cu=%llu mont=%d nproofs=%llu\n", (int)ctr, lookup_bits,
           (int)(lookup_bits == 21 || lookup_bits == 13 || lookup_bits == 8), (unsigned long long)ncols, (int)(ncols <= 64), (unsigned long long)((nrec + 255) / 256),
           (unsigned long long)roam_per_cu, (int)mont, (unsigned long long)nproofs);
    if (launch_expand(A, nproofs, (int)grid_x, nullptr) != 0) { printf("launch_expand: %s\n", g_last_error.c_str()); return 1; }
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());

    std::vector<unsigned char> res(cells * 32);
    CK(hipMemcpy(res.data(), d_buf, res.size(), hipMemcpyDeviceToHost));
    FILE *f = fopen(argv[2], "wb"); if (!f) { printf("cannot write %s\n", argv[2]); return 2; }
    const size_t put = fwrite(res.data(), 32, cells, f);
    if (fclose(f) != 0 || put != cells) { printf("short write\n"); return 2; }
    printf("expandcheck: %llu proofs x %llu records, %zu cells out\n", (unsigned long long)nproofs, (unsigned long long)nrec, cells);
    return 0;
}
