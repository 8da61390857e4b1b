// advicetools.hip — what works on a FINISHED advice stream (no part of a witness call):
//   h2w_layout_columns, h2w_layout_lookup_columns   advice -> FlexGate columns / lookup advice columns (k_layout_columns, k_layout_lookup)
//   h2w_check_constraints, h2w_check_equalities     the MockProver's gate, lookup and copy checks restated on the device (k_check_*)
//   h2w_advice_digest                               a 256-bit digest of a stream (k_digest)
//   h2w_advice_to_montgomery                        canonical -> Montgomery form in place (k_to_montgomery)
#include <hip/hip_runtime.h>
#include <vector>
#include <algorithm>
#include "plan.h"

namespace h2w {
__global__ void k_digest(const ulonglong4 *cells, uint64_t n, unsigned long long *out4) {
    unsigned long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        ulonglong4 c = cells[i]; unsigned long long m = (i + 1) * 0x9E3779B97F4A7C15ULL | 1ULL;
        a0 += c.x * m; a1 += c.y * (m + 2); a2 += c.z * (m + 4); a3 += c.w * (m + 6);
    }
    for (int d = 32; d > 0; d >>= 1) { a0 += __shfl_down(a0, d, 64); a1 += __shfl_down(a1, d, 64); a2 += __shfl_down(a2, d, 64); a3 += __shfl_down(a3, d, 64); }
    if ((threadIdx.x & 63) == 0) { atomicAdd(&out4[0], a0); atomicAdd(&out4[1], a1); atomicAdd(&out4[2], a2); atomicAdd(&out4[3], a3); }
}
}  // namespace h2w

extern "C" {

// advice -> FlexGate columns on the device: columns[p][c][r], c < n_bp + 1, r < 2^k (unassigned rows zero), 32-byte cells
__global__ void k_layout_columns(const ulonglong2 *advice, uint64_t proof_stride, const uint64_t *starts, const uint64_t *lens, uint32_t ncols, uint32_t k, ulonglong2 *out) {
    const uint64_t rows2 = (uint64_t)2 << k;                      // 16-byte halves per column
    const uint32_t p = blockIdx.z, c = blockIdx.y;
    const uint64_t start = starts[c], len2 = lens[c] * 2;
    const ulonglong2 *src = advice + ((uint64_t)p * proof_stride + start) * 2;
    ulonglong2 *dst = out + ((uint64_t)p * ncols + c) * rows2;
    for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < rows2; h += (uint64_t)gridDim.x * blockDim.x)
        dst[h] = h < len2 ? src[h] : make_ulonglong2(0, 0);
}
int h2w_layout_columns(const void *advice_dev, uint64_t n_cells, uint64_t proof_stride_cells, uint64_t n_proofs, const uint64_t *break_points, uint64_t n_bp, int k, void *columns_dev, void *stream_) {
    if (!advice_dev || !columns_dev || (!break_points && n_bp) || k < 3 || k > 34) { set_error("h2w_layout_columns: bad argument"); return -1; }
    if (n_proofs == 0) return 0;
    const uint64_t ncols = n_bp + 1; std::vector<uint64_t> h(2 * ncols); uint64_t start = 0;
    for (uint64_t c = 0; c < ncols; c++) {      // column c holds cells [start, start + len); consecutive columns share their boundary cell
        // a break point is a row 1 .. 2^k - 1: a column that breaks holds its first cell and the breaking one at least, and bp + 1 cannot wrap
        if (c < n_bp && (break_points[c] == 0 || break_points[c] >= ((uint64_t)1 << k))) { set_error("h2w_layout_columns: break points do not fit the stream"); return -1; }
        const uint64_t len = c < n_bp ? break_points[c] + 1 : n_cells - start;
        if (start > n_cells || len > n_cells - start || len > ((uint64_t)1 << k)) { set_error("h2w_layout_columns: break points do not fit the stream"); return -1; }
        h[c] = start; h[ncols + c] = len; start += len - (c < n_bp ? 1 : 0);
    }
    if (ncols > 65535 || n_proofs > 65535) { set_error("h2w_layout_columns: too many columns / proofs per call"); return -1; }
    DeviceGuard dg(device_of(advice_dev));
    hipStream_t stream = (hipStream_t)stream_; uint64_t *d = nullptr;
    H2W_HIP(hipMallocAsync((void **)&d, h.size() * sizeof(uint64_t), stream));
    H2W_HIP(hipMemcpyAsync(d, h.data(), h.size() * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    H2W_HIP(hipStreamSynchronize(stream));      // h is a local
    const unsigned gx = (unsigned)std::min<uint64_t>((((uint64_t)2 << k) + 255) / 256, 4096);
    hipLaunchKernelGGL(k_layout_columns, dim3(gx, (unsigned)ncols, (unsigned)n_proofs), dim3(256), 0, stream, (const ulonglong2 *)advice_dev, proof_stride_cells, d, d + ncols, (uint32_t)ncols, (uint32_t)k, (ulonglong2 *)columns_dev);
    H2W_HIP(hipFreeAsync(d, stream));
    H2W_HIP(hipGetLastError());
    return 0;
}
// lookup advice: the looked-up cells, in registration order, down columns of max_rows rows [R]; out[p][c][r], r < 2^k
__global__ void k_layout_lookup(const ulonglong2 *advice, uint64_t proof_stride, const uint32_t *cells, uint64_t n_lookups, uint64_t max_rows, uint32_t ncols, uint32_t k, ulonglong2 *out) {
    const uint64_t rows = (uint64_t)1 << k, total2 = (uint64_t)ncols * rows * 2; const uint32_t p = blockIdx.y;
    for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < total2; h += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t cellpos = h >> 1, c = cellpos / rows, r = cellpos % rows, j = c * max_rows + r;
        ulonglong2 v = make_ulonglong2(0, 0);
        if (r < max_rows && j < n_lookups) v = advice[((uint64_t)p * proof_stride + cells[j]) * 2 + (h & 1)];
        out[(uint64_t)p * total2 + h] = v;
    }
}
static int ensure_lookup_cells(h2w_plan *p);
int h2w_layout_lookup_columns(h2w_plan *p, const void *advice_dev, uint64_t proof_stride_cells, uint64_t n_proofs, int k, int unusable_rows, void *out_dev, uint64_t *n_cols_out, void *stream_) {
    // the rule of h2w_break_points: a column keeps at least five usable rows (max_rows below is never zero and never wraps)
    if (!p || k < 3 || k > 34 || unusable_rows < 0 || ((uint64_t)1 << k) <= (uint64_t)unusable_rows + 4) { set_error("h2w_layout_lookup_columns: bad argument"); return -1; }
    if (h2w_plan_metadata(p) != 0) return -1;
    const uint64_t max_rows = ((uint64_t)1 << k) - (uint64_t)unusable_rows, ncols = (p->n_lookups + max_rows - 1) / max_rows;
    if (n_cols_out) *n_cols_out = ncols;
    if (!out_dev) return 0;                    // size query
    if (!advice_dev) { set_error("h2w_layout_lookup_columns: null advice"); return -1; }
    if (p->device < 0) { set_error("h2w_layout_lookup_columns: no HIP device"); return -1; }
    DeviceGuard dg(p->device);
    hipStream_t stream = (hipStream_t)stream_;
    if (ensure_lookup_cells(p) != 0) return -1;
    if (n_proofs == 0 || ncols == 0) return 0;
    hipLaunchKernelGGL(k_layout_lookup, dim3(4096, (unsigned)n_proofs), dim3(256), 0, stream, (const ulonglong2 *)advice_dev, proof_stride_cells, p->d_lookup_cells.get(), p->n_lookups, max_rows, (uint32_t)ncols, (uint32_t)k, (ulonglong2 *)out_dev);
    H2W_HIP(hipGetLastError());
    return 0;
}
// Device-side constraint check of an advice stream (the MockProver's gate and lookup checks, restated): every vertical gate
// a[i] + a[i+1]*a[i+2] = a[i+3] at a selector-enabled cell i, and every looked-up cell < 2^lookup_bits.  Size-independent: it
// covers every cell of a full-size stream without the CPU oracle.  Copy constraints are not checked (no equality lists yet).
__global__ void k_check_gates(const fr_t *advice, uint64_t proof_stride, uint64_t n_cells, const uint8_t *sel, FrParams P, unsigned long long *bad) {
    const uint32_t p = blockIdx.y; const fr_t *adv = advice + (uint64_t)p * proof_stride; unsigned long long nb = 0;
    for (uint64_t byte = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; byte < (n_cells + 7) / 8; byte += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t m = sel[byte];
        while (m) {
            const int b = __ffs((int)m) - 1; m &= m - 1; const uint64_t i = byte * 8 + (uint64_t)b;
            if (i + 3 >= n_cells) { nb++; continue; }
            const fr_t a = g_load_fr(adv + i), x = g_load_fr(adv + i + 1), y = g_load_fr(adv + i + 2), d = g_load_fr(adv + i + 3);
            // a, x, y >= r are no field elements: a + r or x + r would pass below (one conditional subtraction, a reduced product).  With the
            // three canonical the sum is canonical, so the bitwise compare refuses a d >= r by itself.
            if (fr_geq_mod(a) || fr_geq_mod(x) || fr_geq_mod(y) || !fr_eq(fr_add(a, fr_mul(x, y, P)), d)) nb++;
        }
    }
    if (nb) atomicAdd(bad, nb);
}
__global__ void k_check_lookups(const fr_t *advice, uint64_t proof_stride, const uint32_t *cells, uint64_t n_lookups, int lookup_bits, unsigned long long *bad) {
    const uint32_t p = blockIdx.y; const fr_t *adv = advice + (uint64_t)p * proof_stride; unsigned long long nb = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_lookups; j += (uint64_t)gridDim.x * blockDim.x) {
        const fr_t v = g_load_fr(adv + cells[j]);
        if ((v.l[1] | v.l[2] | v.l[3]) != 0 || (v.l[0] >> lookup_bits) != 0) nb++;
    }
    if (nb) atomicAdd(bad + 1, nb);
}
static int ensure_lookup_cells(h2w_plan *p) {
    if (p->d_lookup_cells.get() || !p->n_lookups) return 0;
    if (p->ncells >> 32) { set_error("lookup cells: stream longer than 2^32 cells"); return -1; }
    std::vector<uint32_t> h((size_t)p->n_lookups); uint64_t k2 = 0;
    for (uint64_t i = 0; i < p->ncells; i++) if (p->lk_bits[i / 8] >> (i & 7) & 1) h[k2++] = (uint32_t)i;
    return p->d_lookup_cells.upload(h);
}
int h2w_check_constraints(h2w_plan *p, const void *advice_dev, uint64_t proof_stride_cells, uint64_t n_proofs, uint64_t bad_out[2], void *stream_) {
    if (!p || !advice_dev || !bad_out) { set_error("h2w_check_constraints: null argument"); return -1; }
    if (p->device < 0) { set_error("h2w_check_constraints: no HIP device"); return -1; }
    DeviceGuard dg(p->device);
    if (h2w_plan_metadata(p) != 0 || ensure_lookup_cells(p) != 0) return -1;
    bad_out[0] = bad_out[1] = 0;
    if (n_proofs == 0) return 0;
    if (n_proofs > 65535) { set_error("h2w_check_constraints: too many proofs per call"); return -1; }
    hipStream_t stream = (hipStream_t)stream_;
    if (!p->d_sel_bits.get() && p->d_sel_bits.upload(p->sel_bits) != 0) return -1;
    unsigned long long *d_bad = nullptr;
    H2W_HIP(hipMallocAsync((void **)&d_bad, 16, stream));
    unsigned long long h[2] = {0, 0};
    auto run = [&]() -> int {
        H2W_HIP(hipMemsetAsync(d_bad, 0, 16, stream));
        hipLaunchKernelGGL(k_check_gates, dim3(2048, (unsigned)n_proofs), dim3(256), 0, stream, (const fr_t *)advice_dev, proof_stride_cells, p->ncells, p->d_sel_bits.get(), p->P, d_bad);
        if (p->n_lookups) hipLaunchKernelGGL(k_check_lookups, dim3(1024, (unsigned)n_proofs), dim3(256), 0, stream, (const fr_t *)advice_dev, proof_stride_cells, p->d_lookup_cells.get(), p->n_lookups, (int)p->shape.lookup_bits, d_bad);
        H2W_HIP(hipMemcpyAsync(h, d_bad, 16, hipMemcpyDeviceToHost, stream));
        H2W_HIP(hipStreamSynchronize(stream));
        return 0;
    };
    const int rc = run();
    (void)hipFreeAsync(d_bad, stream);
    if (rc != 0) return -1;
    bad_out[0] = h[0]; bad_out[1] = h[1];
    return 0;
}
// copy constraints and constant equalities over device advice streams (the rest of the restated MockProver): the lists are static
// per shape and come from an eager keygen context (h2w_ctx_equalities / h2w_ctx_const_equalities)
__global__ void k_check_equalities(const fr_t *advice, uint64_t proof_stride, const uint64_t *pairs, uint64_t n_pairs, const uint64_t *ccells, const fr_t *cvals, uint64_t n_const, unsigned long long *bad) {
    const uint32_t p = blockIdx.y; const fr_t *adv = advice + (uint64_t)p * proof_stride; unsigned long long b0 = 0, b1 = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_pairs + n_const; j += (uint64_t)gridDim.x * blockDim.x) {
        if (j < n_pairs) { if (!fr_eq(g_load_fr(adv + pairs[2 * j]), g_load_fr(adv + pairs[2 * j + 1]))) b0++; }
        else { const uint64_t t = j - n_pairs; if (!fr_eq(g_load_fr(adv + ccells[t]), g_load_fr(cvals + t))) b1++; }
    }
    if (b0) atomicAdd(bad, b0);
    if (b1) atomicAdd(bad + 1, b1);
}
int h2w_check_equalities(const void *advice_dev, uint64_t n_cells, uint64_t proof_stride_cells, uint64_t n_proofs, const uint64_t *pairs, uint64_t n_pairs,
                         const uint64_t *const_cells, const h2w_fr_t *const_values, uint64_t n_const, uint64_t bad_out[2], void *stream_) {
    if (!advice_dev || !bad_out || (n_pairs && !pairs) || (n_const && (!const_cells || !const_values))) { set_error("h2w_check_equalities: null argument"); return -1; }
    bad_out[0] = bad_out[1] = 0;
    if (n_proofs == 0 || n_pairs + n_const == 0) return 0;
    if (n_proofs > 65535) { set_error("h2w_check_equalities: too many proofs per call"); return -1; }
    for (uint64_t i = 0; i < 2 * n_pairs; i++) if (pairs[i] >= n_cells) { set_error("h2w_check_equalities: equality refers to a cell outside the stream"); return -1; }
    for (uint64_t i = 0; i < n_const; i++) if (const_cells[i] >= n_cells) { set_error("h2w_check_equalities: constant equality refers to a cell outside the stream"); return -1; }
    DeviceGuard dg(device_of(advice_dev));
    hipStream_t stream = (hipStream_t)stream_;
    // one stream-ordered allocation for the three lists and the counters: nothing to leak on an error path, nothing synchronous
    const size_t b_pairs = (n_pairs ? 2 * n_pairs : 1) * 8, b_cc = (n_const ? n_const : 1) * 8, b_cv = (n_const ? n_const : 1) * sizeof(fr_t);
    char *d = nullptr;
    H2W_HIP(hipMallocAsync((void **)&d, b_pairs + b_cc + b_cv + 16, stream));
    uint64_t *d_pairs = (uint64_t *)d, *d_cc = (uint64_t *)(d + b_pairs); fr_t *d_cv = (fr_t *)(d + b_pairs + b_cc); unsigned long long *d_bad = (unsigned long long *)(d + b_pairs + b_cc + b_cv);
    unsigned long long h[2] = {0, 0};
    auto run = [&]() -> int {
        if (n_pairs) H2W_HIP(hipMemcpyAsync(d_pairs, pairs, 2 * n_pairs * 8, hipMemcpyHostToDevice, stream));
        if (n_const) { H2W_HIP(hipMemcpyAsync(d_cc, const_cells, n_const * 8, hipMemcpyHostToDevice, stream)); H2W_HIP(hipMemcpyAsync(d_cv, const_values, n_const * sizeof(fr_t), hipMemcpyHostToDevice, stream)); }
        H2W_HIP(hipMemsetAsync(d_bad, 0, 16, stream));
        hipLaunchKernelGGL(k_check_equalities, dim3(1024, (unsigned)n_proofs), dim3(256), 0, stream, (const fr_t *)advice_dev, proof_stride_cells, d_pairs, n_pairs, d_cc, d_cv, n_const, d_bad);
        H2W_HIP(hipMemcpyAsync(h, d_bad, 16, hipMemcpyDeviceToHost, stream));
        H2W_HIP(hipStreamSynchronize(stream));
        return 0;
    };
    const int rc = run();
    (void)hipFreeAsync(d, stream);
    if (rc != 0) return -1;
    bad_out[0] = h[0]; bad_out[1] = h[1];
    return 0;
}
int h2w_advice_digest(const void *advice_dev, uint64_t n_cells, uint64_t *digest4_dev, void *stream_) {
    if (!advice_dev || !digest4_dev) { set_error("h2w_advice_digest: null argument"); return -1; }
    DeviceGuard dg(device_of(advice_dev));
    hipStream_t stream = (hipStream_t)stream_;
    H2W_HIP(hipMemsetAsync(digest4_dev, 0, 32, stream));
    if (n_cells) hipLaunchKernelGGL(k_digest, dim3(2048), dim3(256), 0, stream, (const ulonglong4 *)advice_dev, n_cells, (unsigned long long *)digest4_dev);
    H2W_HIP(hipGetLastError());
    return 0;
}
// canonical -> Montgomery form (halo2curves bn256::Fr in memory: v * 2^256 mod r, little-endian limbs), in place.  One Montgomery
// product per cell with the constant 2^(256+261) mod r (the device product divides by 2^261).
__global__ void k_to_montgomery(fr_t *cells, uint64_t n, fr_t kconst, uint64_t ninv) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        g_store_fr(cells + i, fr_mont_mul(g_load_fr(cells + i), kconst, ninv));
}
int h2w_advice_to_montgomery(void *cells_dev, uint64_t n_cells, void *stream_) {
    if (!cells_dev) { set_error("h2w_advice_to_montgomery: null argument"); return -1; }
    if (n_cells == 0) return 0;
    DeviceGuard dg(device_of(cells_dev));
    static const FrParams P = fr_params_init();
    hipLaunchKernelGGL(k_to_montgomery, dim3(4096), dim3(256), 0, (hipStream_t)stream_, (fr_t *)cells_dev, n_cells, mont_k(), P.ninv);
    H2W_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
