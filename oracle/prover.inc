/*
 * prover.inc — a native (value-domain, no cells) FRI prover for the oracle.  TEST INFRASTRUCTURE ONLY (see oracle.h).
 *
 * SURVEY §8(c)(iv) / §8(d) variant (A): produce a VALID FRI instance of a given shape, so that the restated verifier gadget can
 * be checked for self-consistency on something better than random bytes: on a valid proof every chip-level assert_equal of
 * the gadget (Merkle roots, FRI fold consistency, final-polynomial evaluation, proof of work) must hold, i.e. the restated
 * MockProver reports semantic_failed == 0.  That pins what cell counts cannot: index bit order, bit-reversed leaf order,
 * coset shifts, fold arity handling, barycentric interpolation, the challenger transcript order.
 *
 * It is written against plonky2's PROVER conventions (SURVEY App. B, all [R]; plonky2 itself is not on this box):
 *   - PolynomialBatch: LDE on the coset 7·<w>, |<w>| = 2^(degree_bits + rate_bits); Merkle leaves in bit-reversed order,
 *     leaf j = the values of every polynomial of the oracle at 7·w^rev(j); cap = the 2^cap_height subtree roots.
 *   - FRI batching: F(X) = sum over batches b of alpha^(shift) * (G_b(X) - G_b(z_b)) / (X - z_b), G_b = sum_i alpha^i f_{b,i},
 *     accumulated as the verifier does (sum = sum * alpha^{n_b} + quotient_b), no extra multiplication by X (fri/mod.rs:169-220).
 *   - commit phase: bit-reverse the coset evaluations, chunk by arity into leaves, observe the cap, beta, fold the COEFFICIENTS
 *     (chunks of arity reduced with powers of beta), shift <- shift^arity; final polynomial truncated by rate_bits.
 *   - proof of work: grind pow_witness until the challenge squeezed after observing it has pow_bits leading zero bits.
 * The STARK constraint/quotient identity is not part of the path (StarkChip::verify_proof_with_challenges never evaluates
 * constraints: stark/mod.rs:230-344), so the committed polynomials are random polynomials of degree < 2^degree_bits.
 *
 * Hashing / transcript use native value-domain twins (nv_*) of the gadget functions above; tests also compare the twins with
 * the gadgets' cell values on random inputs.
 */

/* ------------------------------------------------------------------ native Poseidon (GL, "fast" layout) — twin of pg_* */
static void nv_gl_permute(const oconsts_t *k, uint64_t *st) {
    int round_ctr = 0;
    for (int half = 0; half < 2; half++) {
        if (half == 1) {
            for (int i = 0; i < SPONGE_WIDTH; i++) st[i] = glf_add(st[i], k->fast_partial_first_round_constant[i]);
            uint64_t res[SPONGE_WIDTH] = {0}; res[0] = st[0];
            for (int r = 1; r < SPONGE_WIDTH; r++) for (int cc = 1; cc < SPONGE_WIDTH; cc++)
                res[cc] = glf_add(glf_mul(k->fast_partial_round_initial_matrix[r - 1][cc - 1], st[r]), res[cc]);
            memcpy(st, res, sizeof(res));
            for (int r = 0; r < N_PARTIAL_ROUNDS; r++) {
                uint64_t x = st[0], x2 = glf_mul(x, x), x4 = glf_mul(x2, x2), x6 = glf_mul(x4, x2);
                st[0] = glf_add(glf_mul(x6, x), k->fast_partial_round_constants[r]);
                uint64_t d = glf_mul(glf_add(k->mds_circ[0], k->mds_diag[0]), st[0]);
                for (int i = 1; i < SPONGE_WIDTH; i++) d = glf_add(glf_mul(k->fast_partial_round_w_hats[r][i - 1], st[i]), d);
                uint64_t nr[SPONGE_WIDTH]; nr[0] = d;
                for (int i = 1; i < SPONGE_WIDTH; i++) nr[i] = glf_add(glf_mul(k->fast_partial_round_vs[r][i - 1], st[0]), st[i]);
                memcpy(st, nr, sizeof(nr));
            }
            round_ctr += N_PARTIAL_ROUNDS;
        }
        for (int f = 0; f < HALF_N_FULL_ROUNDS; f++) {
            for (int i = 0; i < SPONGE_WIDTH; i++) {
                uint64_t x = glf_add(st[i], k->all_round_constants[i + SPONGE_WIDTH * round_ctr]);
                uint64_t x2 = glf_mul(x, x), x4 = glf_mul(x2, x2), x6 = glf_mul(x4, x2); st[i] = glf_mul(x6, x);
            }
            uint64_t res[SPONGE_WIDTH];
            for (int r = 0; r < SPONGE_WIDTH; r++) {
                uint64_t acc = 0;
                for (int i = 0; i < SPONGE_WIDTH; i++) acc = glf_add(glf_mul(k->mds_circ[i], st[(i + r) % SPONGE_WIDTH]), acc);
                res[r] = glf_add(glf_mul(k->mds_diag[r], st[r]), acc);
            }
            memcpy(st, res, sizeof(res)); round_ctr++;
        }
    }
}
/* ------------------------------------------------------------------ native PoseidonBN254 — twin of pb_* */
static ofr_t nv_fr_exp5(const ofr_t *x) { ofr_t x2 = fr_mul(x, x), x4 = fr_mul(&x2, &x2); return fr_mul(&x4, x); }
static void nv_bn_mix(ofr_t *st, const ofr_t m[4][4]) {
    ofr_t ns[4];
    for (int i = 0; i < 4; i++) { ns[i] = fr_from_u64(0); for (int j = 0; j < 4; j++) { ofr_t t = fr_mul(&m[j][i], &st[j]); ns[i] = fr_add(&ns[i], &t); } }
    memcpy(st, ns, sizeof(ns));
}
static void nv_bn_permute(const oconsts_t *k, ofr_t *st) {
    for (int i = 0; i < 4; i++) st[i] = fr_add(&st[i], &k->bn_c[i]);
    for (int half = 0; half < 2; half++) {
        if (half == 1) for (int r = 0; r < BN_PARTIAL_ROUNDS; r++) {
            st[0] = nv_fr_exp5(&st[0]); st[0] = fr_add(&st[0], &k->bn_c[(BN_FULL_ROUNDS / 2 + 1) * BN_WIDTH + r]);
            ofr_t ns0 = fr_from_u64(0);
            for (int j = 0; j < 4; j++) { ofr_t t = fr_mul(&k->bn_s[7 * r + j], &st[j]); ns0 = fr_add(&ns0, &t); }
            for (int kk = 1; kk < 4; kk++) { ofr_t t = fr_mul(&k->bn_s[7 * r + 4 + kk - 1], &st[0]); st[kk] = fr_add(&st[kk], &t); }
            st[0] = ns0;
        }
        for (int i = 0; i < BN_FULL_ROUNDS / 2 - 1; i++) {
            for (int j = 0; j < 4; j++) st[j] = nv_fr_exp5(&st[j]);
            int it = half == 0 ? (i + 1) * BN_WIDTH : (BN_FULL_ROUNDS / 2 + 1) * BN_WIDTH + BN_PARTIAL_ROUNDS + i * BN_WIDTH;
            for (int j = 0; j < 4; j++) st[j] = fr_add(&st[j], &k->bn_c[it + j]);
            nv_bn_mix(st, k->bn_m);
        }
        for (int j = 0; j < 4; j++) st[j] = nv_fr_exp5(&st[j]);
        if (half == 0) { for (int j = 0; j < 4; j++) st[j] = fr_add(&st[j], &k->bn_c[(BN_FULL_ROUNDS / 2) * BN_WIDTH + j]); nv_bn_mix(st, k->bn_p); }
        else nv_bn_mix(st, k->bn_m);
    }
}
/* ------------------------------------------------------------------ native hashers: a hash is 4 u64 words in both modes */
typedef struct { uint64_t w[4]; } nvh_t;
static ofr_t nv_limbs_to_fr(const uint64_t *in, int n) { ofr_t r = {{0, 0, 0, 0}}; for (int i = 0; i < n; i++) r.l[i] = in[i]; return r; } /* sum in[i] 2^(64 i), n <= 3 */
static nvh_t nv_hash_no_pad(const oconsts_t *k, int mode, const uint64_t *in, int n) {
    nvh_t h;
    if (mode == 0) {
        uint64_t st[SPONGE_WIDTH] = {0};
        for (int off = 0; off < n; off += SPONGE_RATE) { int len = n - off < SPONGE_RATE ? n - off : SPONGE_RATE; memcpy(st, in + off, (size_t)len * 8); nv_gl_permute(k, st); }
        memcpy(h.w, st, 32);
    } else {
        ofr_t st[4]; memset(st, 0, sizeof(st));
        for (int off = 0; off < n; off += 9) {
            int len = n - off < 9 ? n - off : 9;
            for (int j = 0, o = 0; o < len; j++, o += 3) st[j + 1] = nv_limbs_to_fr(in + off + o, len - o < 3 ? len - o : 3);
            nv_bn_permute(k, st);
        }
        memcpy(h.w, st[0].l, 32);
    }
    return h;
}
static nvh_t nv_hash_or_noop(const oconsts_t *k, int mode, const uint64_t *in, int n) {
    if (n > (mode == 0 ? 4 : 3)) return nv_hash_no_pad(k, mode, in, n);
    nvh_t h; memset(&h, 0, sizeof(h));
    for (int i = 0; i < n; i++) h.w[i] = in[i];      /* GL: zero-padded elements; BN254: limbs_to_num = the same words as an Fr */
    return h;
}
static nvh_t nv_two_to_one(const oconsts_t *k, int mode, nvh_t l, nvh_t r) {
    nvh_t h;
    if (mode == 0) { uint64_t st[SPONGE_WIDTH] = {0}; memcpy(st, l.w, 32); memcpy(st + 4, r.w, 32); nv_gl_permute(k, st); memcpy(h.w, st, 32); }
    else { ofr_t st[4]; memset(st, 0, sizeof(st)); memcpy(st[2].l, l.w, 32); memcpy(st[3].l, r.w, 32); nv_bn_permute(k, st); memcpy(h.w, st[0].l, 32); }
    return h;
}
static int nv_hash_to_goldilocks(int mode, nvh_t h, uint64_t *out) {
    if (mode == 0) { memcpy(out, h.w, 32); return 4; }
    ofr_t v; memcpy(v.l, h.w, 32);
    for (int i = 0; i < 5; i++) out[i] = fr_bits(&v, 56 * i, 56);
    return 5;
}
/* ------------------------------------------------------------------ native challenger — twin of ch_* */
typedef struct { const oconsts_t *k; uint64_t state[SPONGE_WIDTH]; uint64_t *in; int n_in, cap_in; uint64_t out[SPONGE_RATE]; int n_out; } nvchal_t;
static void nvc_observe(nvchal_t *ch, uint64_t v) {
    ch->n_out = 0;
    if (ch->n_in == ch->cap_in) { ch->cap_in = ch->cap_in ? ch->cap_in * 2 : 64; ch->in = (uint64_t *)realloc(ch->in, (size_t)ch->cap_in * 8); }
    ch->in[ch->n_in++] = v;
}
static void nvc_observe_cap(nvchal_t *ch, int mode, const nvh_t *cap, int n) { uint64_t v[5]; for (int i = 0; i < n; i++) { int m = nv_hash_to_goldilocks(mode, cap[i], v); for (int j = 0; j < m; j++) nvc_observe(ch, v[j]); } }
static void nvc_observe_ext(nvchal_t *ch, const gle_t *e, int n) { for (int i = 0; i < n; i++) { nvc_observe(ch, e[i].c[0]); nvc_observe(ch, e[i].c[1]); } }
static uint64_t nvc_challenge(nvchal_t *ch) {
    if (ch->n_in) {
        for (int off = 0; off < ch->n_in; off += SPONGE_RATE) { int len = ch->n_in - off < SPONGE_RATE ? ch->n_in - off : SPONGE_RATE; memcpy(ch->state, ch->in + off, (size_t)len * 8); nv_gl_permute(ch->k, ch->state); }
        memcpy(ch->out, ch->state, SPONGE_RATE * 8); ch->n_out = SPONGE_RATE; ch->n_in = 0;
    }
    if (ch->n_out == 0) { nv_gl_permute(ch->k, ch->state); memcpy(ch->out, ch->state, SPONGE_RATE * 8); ch->n_out = SPONGE_RATE; }
    return ch->out[--ch->n_out];
}
static gle_t nvc_ext_challenge(nvchal_t *ch) { gle_t r; r.c[0] = nvc_challenge(ch); r.c[1] = nvc_challenge(ch); return r; }
/* ------------------------------------------------------------------ polynomials */
static gle_t gle_add(gle_t a, gle_t b) { gle_t r = {{glf_add(a.c[0], b.c[0]), glf_add(a.c[1], b.c[1])}}; return r; }
static gle_t gle_sub(gle_t a, gle_t b) { gle_t r = {{glf_sub(a.c[0], b.c[0]), glf_sub(a.c[1], b.c[1])}}; return r; }
static gle_t gle_from(uint64_t a) { gle_t r = {{a, 0}}; return r; }
static int bitrev(int i, int bits) { int r = 0; for (int b = 0; b < bits; b++) if (i & (1 << b)) r |= 1 << (bits - 1 - b); return r; }
/* in-place radix-2 DIT NTT of size 2^bits: a[i] <- sum_j a[j] w^(ij), w = primitive_root_of_unity(bits) */
static void nv_ntt(uint64_t *a, int bits) {
    int n = 1 << bits;
    for (int i = 0; i < n; i++) { int r = bitrev(i, bits); if (r > i) { uint64_t t = a[i]; a[i] = a[r]; a[r] = t; } }
    for (int len = 2, lb = 1; len <= n; len <<= 1, lb++) {
        uint64_t wl = glf_primitive_root_of_unity(lb);
        for (int s = 0; s < n; s += len) { uint64_t w = 1; for (int j = 0; j < len / 2; j++) { uint64_t u = a[s + j], v = glf_mul(a[s + j + len / 2], w); a[s + j] = glf_add(u, v); a[s + j + len / 2] = glf_sub(u, v); w = glf_mul(w, wl); } }
    }
}
/* values of the polynomial with `nc` coefficients on the coset shift*<w>, |<w>| = 2^bits, natural order */
static void nv_coset_eval(const uint64_t *coef, int nc, uint64_t shift, int bits, uint64_t *out) {
    int n = 1 << bits; uint64_t s = 1;
    for (int i = 0; i < n; i++) { out[i] = i < nc ? glf_mul(coef[i], s) : 0; s = glf_mul(s, shift); }
    nv_ntt(out, bits);
}
static gle_t nv_eval_base_poly(const uint64_t *coef, int n, gle_t x) { gle_t acc = {{0, 0}}; for (int i = n - 1; i >= 0; i--) acc = gle_add(gle_mul(acc, x), gle_from(coef[i])); return acc; }
/* Merkle tree over 2^bits leaf hashes (heap layout: level 0 = leaves); returns all levels */
typedef struct { nvh_t **lvl; int bits; } nvtree_t;
static nvtree_t nv_tree_build(const oconsts_t *k, int mode, nvh_t *leaves, int bits) {
    nvtree_t t; t.bits = bits; t.lvl = (nvh_t **)calloc((size_t)bits + 1, sizeof(nvh_t *)); t.lvl[0] = leaves;
    for (int l = 1; l <= bits; l++) { int n = 1 << (bits - l); t.lvl[l] = (nvh_t *)malloc((size_t)n * sizeof(nvh_t)); for (int i = 0; i < n; i++) t.lvl[l][i] = nv_two_to_one(k, mode, t.lvl[l - 1][2 * i], t.lvl[l - 1][2 * i + 1]); }
    return t;
}
static void nv_tree_free(nvtree_t *t) { for (int l = 0; l <= t->bits; l++) free(t->lvl[l]); free(t->lvl); }
static void put_hash(uint64_t **w, nvh_t h) { memcpy(*w, h.w, 32); *w += 4; }

/* orc_prove_fri_coef: a valid proof of the given shape in the flat layout of orc_proof_words(), for the given committed
 * polynomials (coefs_in: [polynomial][2^degree_bits] coefficients).  pow_witness grinding: ~2^pow_bits
 * native permutations.  Intended for small shapes (cost ~ (polys + folds) * 2^lde_bits hashes). Returns 0, or -1 if the shape
 * is unsupported. */
int orc_prove_fri_coef(const oshape_t *sh, const oconsts_t *k, const uint64_t *coefs_in, const uint64_t *pis, uint64_t *words) {
    fr_init(); oderived_t d; derive(sh, &d);
    const int mode = sh->hash_mode, N = 1 << sh->degree_bits, lb = d.lde_bits, L = 1 << lb, capb = sh->cap_height;
    if (lb > 22 || capb > lb) return -1;
    int npoly[3], no = d.n_oracles; for (int o = 0; o < no; o++) npoly[o] = d.oracle_polys[o];
    size_t poly_no = 0;
    /* random polynomials, their LDEs, trees (leaves in bit-reversed order) */
    uint64_t **coef[3], **lde[3]; nvtree_t tree[3];
    for (int o = 0; o < no; o++) {
        coef[o] = (uint64_t **)malloc((size_t)npoly[o] * sizeof(uint64_t *)); lde[o] = (uint64_t **)malloc((size_t)npoly[o] * sizeof(uint64_t *));
        for (int p = 0; p < npoly[o]; p++) {
            coef[o][p] = (uint64_t *)malloc((size_t)N * 8); lde[o][p] = (uint64_t *)malloc((size_t)L * 8);
            memcpy(coef[o][p], coefs_in + (poly_no++) * (size_t)N, (size_t)N * 8);
            nv_coset_eval(coef[o][p], N, 7, lb, lde[o][p]);
        }
        nvh_t *leaves = (nvh_t *)malloc((size_t)L * sizeof(nvh_t)); uint64_t buf[16];
        for (int j = 0; j < L; j++) { int x = bitrev(j, lb); for (int p = 0; p < npoly[o]; p++) buf[p] = lde[o][p][x]; leaves[j] = nv_hash_or_noop(k, mode, buf, npoly[o]); }
        tree[o] = nv_tree_build(k, mode, leaves, lb);
    }
    const int o_trace = 0, o_perm = sh->n_perm_z > 0 ? 1 : -1, o_quot = no - 1;
    const int cs = d.cap_size; nvh_t *cap[3] = {NULL, NULL, NULL}; for (int o = 0; o < no; o++) cap[o] = tree[o].lvl[lb - capb];
    /* transcript (challenger/mod.rs:167-222 as restated in orc_verify_stark) */
    nvchal_t ch; memset(&ch, 0, sizeof(ch)); ch.k = k;
    nvc_observe_cap(&ch, mode, cap[o_trace], cs);
    if (o_perm >= 0) { for (int set = 0; set < sh->perm_batch_size; set++) for (int i = 0; i < sh->num_challenges; i++) { nvc_challenge(&ch); nvc_challenge(&ch); } nvc_observe_cap(&ch, mode, cap[o_perm], cs); }
    for (int i = 0; i < sh->num_challenges; i++) nvc_challenge(&ch);
    nvc_observe_cap(&ch, mode, cap[o_quot], cs);
    gle_t zeta = nvc_ext_challenge(&ch), gzeta = gle_mul(gle_from(glf_primitive_root_of_unity(sh->degree_bits)), zeta);
    /* openings; batch 0 = every polynomial at zeta (trace, perm Z, quotient), batch 1 = trace and perm Z at g*zeta */
    int nz = 0, nzn = 0; const uint64_t *bpoly[2][16]; gle_t open[2][16];
    for (int o = 0; o < no; o++) for (int p = 0; p < npoly[o]; p++) { bpoly[0][nz] = coef[o][p]; open[0][nz] = nv_eval_base_poly(coef[o][p], N, zeta); nz++; }
    for (int o = 0; o < no; o++) if (o != o_quot) for (int p = 0; p < npoly[o]; p++) { bpoly[1][nzn] = coef[o][p]; open[1][nzn] = nv_eval_base_poly(coef[o][p], N, gzeta); nzn++; }
    nvc_observe_ext(&ch, open[0], nz); nvc_observe_ext(&ch, open[1], nzn);
    gle_t alpha = nvc_ext_challenge(&ch);
    /* F = (G_0 - G_0(zeta))/(X - zeta) * alpha^{n_1} + (G_1 - G_1(g zeta))/(X - g zeta), coefficients over the extension */
    gle_t *F = (gle_t *)calloc((size_t)L, sizeof(gle_t));
    for (int b = 0; b < 2; b++) {
        int nb = b == 0 ? nz : nzn; gle_t z = b == 0 ? zeta : gzeta;
        gle_t *G = (gle_t *)calloc((size_t)N, sizeof(gle_t)); gle_t ap = gle_from(1), gz = {{0, 0}};
        for (int i = 0; i < nb; i++) { for (int j = 0; j < N; j++) G[j] = gle_add(G[j], gle_mul(ap, gle_from(bpoly[b][i][j]))); gz = gle_add(gz, gle_mul(ap, open[b][i])); ap = gle_mul(ap, alpha); }
        G[0] = gle_sub(G[0], gz);
        /* synthetic division by (X - z): q[N-2..0]; the remainder is zero by construction */
        gle_t *Q = (gle_t *)calloc((size_t)N, sizeof(gle_t)); gle_t carry = {{0, 0}};
        for (int j = N - 1; j >= 1; j--) { carry = gle_add(G[j], gle_mul(carry, z)); Q[j - 1] = carry; }
        gle_t an = gle_from(1); for (int i = 0; i < nb; i++) an = gle_mul(an, alpha);          /* alpha^{n_b}: the verifier's alpha_shift */
        for (int j = 0; j < N; j++) F[j] = gle_add(gle_mul(F[j], an), Q[j]);
        free(G); free(Q);
    }
    /* commit phase */
    uint64_t shift = 7; int cur_bits = lb; nvtree_t ftree[MAX_STEPS]; gle_t **fvals = (gle_t **)calloc(MAX_STEPS, sizeof(gle_t *)); gle_t betas[MAX_STEPS];
    for (int st = 0; st < d.n_steps; st++) {
        int ab = d.arity[st], ar = 1 << ab, n = 1 << cur_bits;
        uint64_t *c0 = (uint64_t *)malloc((size_t)n * 8), *c1 = (uint64_t *)malloc((size_t)n * 8), *v0 = (uint64_t *)malloc((size_t)n * 8), *v1 = (uint64_t *)malloc((size_t)n * 8);
        for (int i = 0; i < n; i++) { c0[i] = F[i].c[0]; c1[i] = F[i].c[1]; }
        nv_coset_eval(c0, n, shift, cur_bits, v0); nv_coset_eval(c1, n, shift, cur_bits, v1);      /* componentwise: the domain is in the base field */
        fvals[st] = (gle_t *)malloc((size_t)n * sizeof(gle_t));
        for (int j = 0; j < n; j++) { int x = bitrev(j, cur_bits); fvals[st][j].c[0] = v0[x]; fvals[st][j].c[1] = v1[x]; }   /* bit-reversed order */
        int nl = n >> ab; nvh_t *leaves = (nvh_t *)malloc((size_t)nl * sizeof(nvh_t)); uint64_t buf[128];
        for (int j = 0; j < nl; j++) { for (int t = 0; t < ar; t++) { buf[2 * t] = fvals[st][j * ar + t].c[0]; buf[2 * t + 1] = fvals[st][j * ar + t].c[1]; } leaves[j] = nv_hash_or_noop(k, mode, buf, 2 * ar); }
        ftree[st] = nv_tree_build(k, mode, leaves, cur_bits - ab);
        nvc_observe_cap(&ch, mode, ftree[st].lvl[cur_bits - ab - capb], cs);
        gle_t beta = nvc_ext_challenge(&ch); betas[st] = beta;
        for (int j = 0; j < nl; j++) { gle_t acc = {{0, 0}}; for (int t = ar - 1; t >= 0; t--) acc = gle_add(gle_mul(acc, beta), F[j * ar + t]); F[j] = acc; }
        shift = glf_exp(shift, (uint64_t)ar); cur_bits -= ab;
        free(c0); free(c1); free(v0); free(v1);
    }
    (void)betas;
    const int fl = d.final_poly_len;                 /* = 2^cur_bits >> rate_bits; the dropped coefficients are zero */
    nvc_observe_ext(&ch, F, fl);
    /* proof of work */
    /* the challenge squeezed after observing a candidate is nvc_challenge() of the pending inputs + the candidate: the complete rate
     * blocks of the pending inputs (the final polynomial) are the same for every candidate and are absorbed once; a candidate costs the
     * one permutation of the last block.  The witness found goes through nvc_observe / nvc_challenge itself below, and must give the same word. */
    uint64_t pow_witness = 0, pow_response;
    {
        const int full = ch.n_in - ch.n_in % SPONGE_RATE, tail = ch.n_in - full;
        uint64_t base[SPONGE_WIDTH]; memcpy(base, ch.state, sizeof(base));
        for (int off = 0; off < full; off += SPONGE_RATE) { memcpy(base, ch.in + off, SPONGE_RATE * 8); nv_gl_permute(k, base); }
        for (;; pow_witness++) {
            uint64_t st[SPONGE_WIDTH]; memcpy(st, base, sizeof(st));
            memcpy(st, ch.in + full, (size_t)tail * 8); st[tail] = pow_witness;
            nv_gl_permute(k, st); pow_response = st[SPONGE_RATE - 1];
            if (sh->pow_bits == 0 || (pow_response >> (64 - sh->pow_bits)) == 0) break;
        }
    }
    nvc_observe(&ch, pow_witness);
    const int pow_ok = nvc_challenge(&ch) == pow_response;      /* (the proof is refused below if the shortcut above is wrong) */
    /* write the proof */
    uint64_t *w = words;
    for (int i = 0; i < cs; i++) put_hash(&w, cap[o_trace][i]);
    for (int i = 0; i < cs; i++) put_hash(&w, cap[o_quot][i]);
    {   /* local_values, next_values, perm_zs, perm_zs_next, quotient_polys */
        int nc = sh->n_cols, np = sh->n_perm_z, nq = sh->n_quotient;
        for (int i = 0; i < nc; i++) { *w++ = open[0][i].c[0]; *w++ = open[0][i].c[1]; }
        for (int i = 0; i < nc; i++) { *w++ = open[1][i].c[0]; *w++ = open[1][i].c[1]; }
        for (int i = 0; i < np; i++) { *w++ = open[0][nc + i].c[0]; *w++ = open[0][nc + i].c[1]; }
        for (int i = 0; i < np; i++) { *w++ = open[1][nc + i].c[0]; *w++ = open[1][nc + i].c[1]; }
        for (int i = 0; i < nq; i++) { *w++ = open[0][nc + np + i].c[0]; *w++ = open[0][nc + np + i].c[1]; }
    }
    if (o_perm >= 0) for (int i = 0; i < cs; i++) put_hash(&w, cap[o_perm][i]);
    *w++ = pow_witness;
    for (int i = 0; i < fl; i++) { *w++ = F[i].c[0]; *w++ = F[i].c[1]; }
    { int bits = lb; for (int st = 0; st < d.n_steps; st++) { bits -= d.arity[st]; for (int i = 0; i < cs; i++) put_hash(&w, ftree[st].lvl[bits - capb][i]); } }
    for (int q = 0; q < sh->num_queries; q++) {
        uint64_t x_index = nvc_challenge(&ch) & ((uint64_t)L - 1);
        for (int o = 0; o < no; o++) {
            int x = bitrev((int)x_index, lb);
            for (int p = 0; p < npoly[o]; p++) *w++ = lde[o][p][x];
            for (int l = 0; l < lb - capb; l++) put_hash(&w, tree[o].lvl[l][(x_index >> l) ^ 1]);
        }
        uint64_t idx = x_index; int bits = lb;
        for (int st = 0; st < d.n_steps; st++) {
            int ab = d.arity[st], ar = 1 << ab; uint64_t coset = idx >> ab; bits -= ab;
            for (int t = 0; t < ar; t++) { *w++ = fvals[st][coset * ar + t].c[0]; *w++ = fvals[st][coset * ar + t].c[1]; }
            for (int l = 0; l < bits - capb; l++) put_hash(&w, ftree[st].lvl[l][(coset >> l) ^ 1]);
            idx = coset;
        }
    }
    for (int i = 0; i < sh->n_pis; i++) *w++ = pis[i];
    int rc = pow_ok && (size_t)(w - words) == orc_proof_words(sh) ? 0 : -1;
    for (int o = 0; o < no; o++) { for (int p = 0; p < npoly[o]; p++) { free(coef[o][p]); free(lde[o][p]); } free(coef[o]); free(lde[o]); nv_tree_free(&tree[o]); }
    for (int st = 0; st < d.n_steps; st++) { nv_tree_free(&ftree[st]); free(fvals[st]); }
    free(fvals); free(F); free(ch.in);
    return rc;
}
/* the committed polynomials are random: coefficients (oracle by oracle, polynomial by polynomial), then the public inputs, from
 * one splitmix64 stream */
size_t orc_prove_fri_inputs(const oshape_t *sh, uint64_t seed, uint64_t *coefs, uint64_t *pis) {
    oderived_t d; derive(sh, &d); size_t np = 0; for (int o = 0; o < d.n_oracles; o++) np += (size_t)d.oracle_polys[o];
    const size_t n = np << sh->degree_bits;
    if (coefs) { uint64_t rs = seed; for (size_t i = 0; i < n; i++) coefs[i] = rand_gl(&rs); for (int i = 0; i < sh->n_pis; i++) pis[i] = rand_gl(&rs); }
    return n;
}
int orc_prove_fri(const oshape_t *sh, const oconsts_t *k, uint64_t seed, uint64_t *words) {
    size_t n = orc_prove_fri_inputs(sh, seed, NULL, NULL);
    uint64_t *coefs = (uint64_t *)malloc(n * 8), pis[64];
    if (sh->n_pis > 64) { free(coefs); return -1; }
    orc_prove_fri_inputs(sh, seed, coefs, pis);
    int rc = orc_prove_fri_coef(sh, k, coefs, pis, words);
    free(coefs); return rc;
}
/* native twins exposed so tests can compare them with the gadgets' cell values */
void orc_nv_gl_permute(const oconsts_t *k, uint64_t st[12]) { nv_gl_permute(k, st); }
void orc_nv_bn_permute(const oconsts_t *k, ofr_t st[4]) { fr_init(); nv_bn_permute(k, st); }
void orc_nv_hash_or_noop(const oconsts_t *k, int mode, const uint64_t *in, int n, uint64_t out[4]) { fr_init(); nvh_t h = nv_hash_or_noop(k, mode, in, n); memcpy(out, h.w, 32); }
