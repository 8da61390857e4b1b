/*
 * h2w.h — C ABI of the MI355X-native halo2 witness-generation engine for the plonky2/starky
 * FRI-verifier gadget (drop-in for ONE hot path of shuklaayush/halo2-plonky2-verifier).
 *
 * The boundary sits below the reference's NativeChip (verifier/src/field/native.rs:11-194) /
 * ContextWrapper.ctx (verifier/src/util/context_wrapper.rs:11-26), i.e. where the Rust code calls
 * halo2-base Context / GateChip / RangeChip.  Three API levels, all producing the SAME advice stream:
 *
 *   1. eager NativeChip level  (h2w_load_*, h2w_add ... h2w_range_check)   — 1:1 with field/native.rs
 *   2. fused Goldilocks level  (h2w_gl_*)                                  — field/goldilocks/base.rs ops
 *      (hints — u128 divmod, GL inverse — run inside the library)
 *   3. batched hot path        (h2w_plan_* / h2w_fri_witness_batch)        — whole
 *      load_proof_with_pis + StarkChip::verify_proof (stark/mod.rs:483-508) for a batch of proofs,
 *      values and cells computed on the GPU.
 *
 * Plain C: pointers and sizes only, no C++/torch types.  All functions returning int return 0 on
 * success; on failure h2w_last_error() describes it (the reference panics instead; the Rust shim
 * in INTEGRATION.md converts non-zero to panic!).  Handles are not thread-safe; distinct handles
 * are independent (the reference is single-threaded: one &mut Context) and carry their device: a call
 * makes the handle's device current for its own duration (functions without a handle use the device their
 * device pointer lives on), so one thread can drive plans on several GPUs.
 *
 * Advice cells are BN254 Fr values, 32 bytes each, canonical little-endian (4 x u64 limbs).
 */
#ifndef H2W_H
#define H2W_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define H2W_ABI_VERSION 1

typedef struct { uint64_t l[4]; } h2w_fr_t;

/* mirrors halo2-base AssignedValue{value, cell: Option<ContextCell{context_id, offset}>} */
typedef struct {
    h2w_fr_t value;
    uint64_t offset;     /* row in Context::advice */
    uint32_t ctx_id;
    uint32_t has_cell;   /* 0 = value only (QuantumCell::Witness/Constant not yet assigned) */
} h2w_assigned_t;

/* STARK / FRI shape: starky StarkConfig + the Stark trait facts the verifier needs
 * (stark/mod.rs:145-200, challenger/mod.rs:168-222, fri/mod.rs:447-502).
 * Limit: at most 8 FRI fold steps.  ConstantArityBits folds by arity_bits while degree_bits > final_poly_bits and
 * degree_bits + rate_bits - arity_bits >= cap_height, without a bound; a shape that would fold a ninth time is refused ("unsupported
 * shape") by every entry point that takes one (h2w_plan_compile, h2w_chip_verify_stark, h2w_prover_new): raise final_poly_bits or arity_bits. */
typedef struct {
    int32_t degree_bits, rate_bits, cap_height, num_queries, pow_bits, num_challenges;
    int32_t arity_bits, final_poly_bits;          /* FriReductionStrategy::ConstantArityBits */
    int32_t n_cols, n_perm_z, n_quotient, n_pis;  /* Fibonacci: 4, 2, 2, 3 */
    int32_t perm_batch_size;
    int32_t hash_mode;                            /* 0 = Goldilocks Poseidon Merkle, 1 = PoseidonBN254 Merkle */
    int32_t lookup_bits;                          /* RangeChip lookup_bits (= k-1) */
    int32_t witness_load_range_check;             /* 1 = witness/mod.rs:49-51 (28 cells / GL element) */
} h2w_shape_t;

/* Poseidon constants are caller inputs (plonky2 `hash::poseidon`, plonky2x `poseidon_bn128_constants`);
 * indexing as hash/poseidon/permutation.rs:55-68,97-104,120-130,143-171,184-192,229-235 and
 * hash/poseidon_bn254/permutation.rs:86-109,138-159,163-170. */
typedef struct {
    uint64_t all_round_constants[360];
    uint64_t mds_circ[12];
    uint64_t mds_diag[12];
    uint64_t fast_partial_first_round_constant[12];
    uint64_t fast_partial_round_constants[22];
    uint64_t fast_partial_round_initial_matrix[11][11];
    uint64_t fast_partial_round_w_hats[22][11];
    uint64_t fast_partial_round_vs[22][11];
    h2w_fr_t bn_c[88];
    h2w_fr_t bn_s[392];
    h2w_fr_t bn_m[4][4];
    h2w_fr_t bn_p[4][4];
} h2w_poseidon_consts_t;

typedef struct h2w_ctx h2w_ctx;
typedef struct h2w_plan h2w_plan;

/* ------------------------------------------------------------------ library */
int         h2w_abi_version(void);
const char *h2w_last_error(void);
int         h2w_device_count(void);              /* number of visible HIP devices (0 = none: every compute call fails) */
/* The published parameter sets the reference links in from its dependencies: plonky2's Goldilocks Poseidon (width 12:
 * ALL_ROUND_CONSTANTS, MDS_MATRIX_CIRC/_DIAG, FAST_PARTIAL_*; hash/poseidon/permutation.rs:2-7) and plonky2x's
 * circomlib t = 4 PoseidonBN254 tables C/S/M/P (hash/poseidon_bn254/permutation.rs:7-11).  Pure data (no device needed);
 * a caller may pass any other tables of the same layout instead. */
int         h2w_poseidon_published(h2w_poseidon_consts_t *out);

/* ------------------------------------------------------------------ 1. eager NativeChip level
 * replaces halo2-base Context + GateChip + RangeChip as used by field/native.rs.
 * Values are computed on the host at call time (the reference reads AssignedValue::value() for hints:
 * base.rs:27-35,349,382); cells are materialised on the GPU from compact records when the advice is
 * requested (h2w_ctx_advice_device / h2w_ctx_download). */
h2w_ctx *h2w_ctx_new(int lookup_bits, int witness_gen_only, int device_id);   /* base_test().k(k): lookup_bits = k-1 */
void     h2w_ctx_free(h2w_ctx *);
int      h2w_ctx_reset(h2w_ctx *);                                              /* the context as new, its host memory kept (the next proof's run does not fault its pages in again) */
int      h2w_ctx_footprint(const h2w_ctx *, uint64_t out[2]);                    /* what the run so far appended: out[0] block records, out[1] literal cells (32 B each) */
int      h2w_ctx_reserve(h2w_ctx *, uint64_t n_records, uint64_t n_literal_cells); /* Vec::with_capacity for a NEW context: its host vectors sized and mapped ahead (a cfg-3 PoseidonBN254
                                                                                  * proof appends 350 MB; on a fresh context two thirds of a level-1 run are first-touch faults and
                                                                                  * reallocation copies).  Sizes: h2w_ctx_footprint of an earlier run of the same shape */
uint64_t h2w_num_cells(const h2w_ctx *);                                        /* util/context_wrapper.rs:24-26 */
int      h2w_ctx_error(const h2w_ctx *);                                        /* sticky error flag of the context */
/* scoped cell counters: what the reference's #[count] proc-macro (macro/src/lib.rs:9-61) drives through
 * ContextWrapper::push_context / pop_context (util/context_wrapper.rs:28-34, util/context_tree.rs) */
int      h2w_push_context(h2w_ctx *, const char *name);
int      h2w_pop_context(h2w_ctx *);
size_t   h2w_context_dump(const h2w_ctx *, char *buf, size_t cap);              /* "a;b;c <inclusive cells>\n" lines; returns bytes needed */
/* field/native.rs:28-46 */
int h2w_load_constant(h2w_ctx *, const h2w_fr_t *c, h2w_assigned_t *out);
int h2w_load_zero(h2w_ctx *, h2w_assigned_t *out);
int h2w_load_constants(h2w_ctx *, const h2w_fr_t *c, size_t n, h2w_assigned_t *out);
int h2w_load_witness(h2w_ctx *, const h2w_fr_t *w, h2w_assigned_t *out);
/* field/native.rs:48-92 */
int h2w_add(h2w_ctx *, const h2w_assigned_t *a, const h2w_assigned_t *b, h2w_assigned_t *out);
int h2w_mul(h2w_ctx *, const h2w_assigned_t *a, const h2w_assigned_t *b, h2w_assigned_t *out);
int h2w_mul_add(h2w_ctx *, const h2w_assigned_t *a, const h2w_assigned_t *b, const h2w_assigned_t *c, h2w_assigned_t *out);
int h2w_select(h2w_ctx *, const h2w_assigned_t *a, const h2w_assigned_t *b, const h2w_assigned_t *sel, h2w_assigned_t *out);
/* field/native.rs:95-148 */
int h2w_select_from_idx(h2w_ctx *, const h2w_assigned_t *arr, size_t n, const h2w_assigned_t *idx, h2w_assigned_t *out);
int h2w_select_array_by_indicator(h2w_ctx *, const h2w_assigned_t *array2d /* [len][w] row-major */, size_t len, size_t w,
                                  const h2w_assigned_t *indicator, h2w_assigned_t *out /* [w] */);
int h2w_idx_to_indicator(h2w_ctx *, const h2w_assigned_t *idx, size_t len, h2w_assigned_t *out);
int h2w_num_to_bits(h2w_ctx *, const h2w_assigned_t *a, size_t range_bits, h2w_assigned_t *out);
int h2w_bits_to_num(h2w_ctx *, const h2w_assigned_t *bits, size_t n, h2w_assigned_t *out);
/* field/native.rs:150-193 */
int h2w_decompose_le(h2w_ctx *, const h2w_assigned_t *num, size_t limb_bits, size_t num_limbs, h2w_assigned_t *out);
int h2w_limbs_to_num(h2w_ctx *, const h2w_assigned_t *limbs, size_t n, size_t limb_bits, h2w_assigned_t *out);
int h2w_check_less_than_safe(h2w_ctx *, const h2w_assigned_t *a, uint64_t b);
int h2w_range_check(h2w_ctx *, const h2w_assigned_t *a, size_t range_bits);
int h2w_constrain_equal(h2w_ctx *, const h2w_assigned_t *a, const h2w_assigned_t *b); /* Context::constrain_equal: no cells */

/* ------------------------------------------------------------------ 2. fused Goldilocks level
 * field/goldilocks/base.rs: one call = the whole cell block of the op, hint included. */
int h2w_gl_load_constant(h2w_ctx *, uint64_t a, h2w_assigned_t *out);            /* base.rs:61-70   (1 cell)  */
int h2w_gl_load_witness(h2w_ctx *, uint64_t a, h2w_assigned_t *out);             /* base.rs:107-119 (28 @L=21) */
int h2w_gl_reduce(h2w_ctx *, const h2w_assigned_t *a, h2w_assigned_t *out);      /* base.rs:346-368 (61) */
int h2w_gl_add(h2w_ctx *, const h2w_assigned_t *a, const h2w_assigned_t *b, h2w_assigned_t *out);     /* :251-260 (65) */
int h2w_gl_sub(h2w_ctx *, const h2w_assigned_t *a, const h2w_assigned_t *b, h2w_assigned_t *out);     /* :274-283 (66) */
int h2w_gl_mul(h2w_ctx *, const h2w_assigned_t *a, const h2w_assigned_t *b, h2w_assigned_t *out);     /* :296-305 (65) */
int h2w_gl_mul_add(h2w_ctx *, const h2w_assigned_t *a, const h2w_assigned_t *b, const h2w_assigned_t *c, h2w_assigned_t *out); /* :319-329 */
int h2w_gl_div(h2w_ctx *, const h2w_assigned_t *a, const h2w_assigned_t *b, h2w_assigned_t *out);     /* :371-393 (93); error if b == 0 (:379) */
int h2w_gl_inv(h2w_ctx *, const h2w_assigned_t *a, h2w_assigned_t *out);                              /* :395-399 (94) */
int h2w_gl_mul_sub(h2w_ctx *, const h2w_assigned_t *a, const h2w_assigned_t *b, const h2w_assigned_t *c, h2w_assigned_t *out); /* :332-343 (70) */
int h2w_gl_neg(h2w_ctx *, const h2w_assigned_t *a, h2w_assigned_t *out);                              /* :234-238 (1 + 65) */
int h2w_gl_square(h2w_ctx *, const h2w_assigned_t *a, h2w_assigned_t *out);                           /* :401-404 (65) */
int h2w_gl_exp_power_of_2(h2w_ctx *, const h2w_assigned_t *base, size_t power_log, h2w_assigned_t *out); /* :433-445 (65 * power_log) */
/* The hint of GoldilocksQuadExtChip::inv (field/goldilocks/extension.rs:320-340: `a.value().inverse()` loaded as two witnesses, 56 cells at
 * lookup_bits 21): the inverse of a[0] + a[1] X is computed inside; the caller goes on with mul(a, out) and the assert_equal.  Error if a == 0 (:327). */
int h2w_gl_ext_inv_witness(h2w_ctx *, const h2w_assigned_t a[2], h2w_assigned_t out[2]);

/* ------------------------------------------------------------------ 2b. the reference's higher chips over the eager boundary
 * (host side above the C-ABI: csrc/chips.h + csrc/verifier.h instantiated on a backend that only calls the functions above).
 * Hash wires are 4 assigned values (hash_mode 0: PoseidonHashWire.elements) or 1 (hash_mode 1: PoseidonBN254HashWire.value;
 * outputs replicate it 4x). */
int h2w_chip_ext_op(h2w_ctx *, int op, const h2w_assigned_t a[2], const h2w_assigned_t b[2], const h2w_assigned_t c[2], h2w_assigned_t out[2]); /* field/goldilocks/extension.rs: 0 add 1 sub 2 mul 3 square 4 inv 5 div 6 mul_add 7 scalar_mul 8 scalar_div */
int h2w_chip_gl_exp_from_bits_const_base(h2w_ctx *, uint64_t base, const h2w_assigned_t *bits, size_t n, h2w_assigned_t *out);                 /* base.rs:407-430 */
int h2w_chip_gl_poseidon_permute(h2w_ctx *, const h2w_poseidon_consts_t *, const h2w_assigned_t in[12], h2w_assigned_t out[12]);             /* hash/poseidon/permutation.rs:270-284 */
int h2w_chip_bn_poseidon_permute(h2w_ctx *, const h2w_poseidon_consts_t *, const h2w_assigned_t in[4], h2w_assigned_t out[4]);               /* hash/poseidon_bn254/permutation.rs:190-203 */
int h2w_chip_hash_no_pad(h2w_ctx *, const h2w_poseidon_consts_t *, int hash_mode, const h2w_assigned_t *in, size_t n, h2w_assigned_t out[4]); /* HasherChip::hash_no_pad */
int h2w_chip_two_to_one(h2w_ctx *, const h2w_poseidon_consts_t *, int hash_mode, const h2w_assigned_t l[4], const h2w_assigned_t r[4], h2w_assigned_t out[4]); /* HasherChip::two_to_one */
int h2w_chip_merkle_verify(h2w_ctx *, const h2w_poseidon_consts_t *, int hash_mode, const h2w_assigned_t *leaf, size_t n_leaf,
                           const h2w_assigned_t *index_bits, size_t n_bits, const h2w_assigned_t *cap_index,
                           const h2w_assigned_t *cap, size_t n_cap, const h2w_assigned_t *siblings, size_t n_sib);                               /* merkle/mod.rs:57-78 */
int h2w_chip_verify_stark(h2w_ctx *, const h2w_shape_t *, const h2w_poseidon_consts_t *, const uint64_t *proof_words);                         /* stark/mod.rs:483-508 */

/* ------------------------------------------------------------------ 2d. record and replay: the operator API served at GPU speed
 * A context in trace mode records the tape of ONE run driven through nothing but the level-1 / level-2 calls above (for the reference: its unchanged
 * chips over the NativeChip shim); h2w_plan_from_trace lowers the tape to a device program, and h2w_fri_witness_batch replays it on any batch of proofs
 * of the same shape - bit-identical to running the calls on each of them, for every proof whose status is 0.  The replay works at the widths the
 * lowering assigned on the traced proof and has no host call that could refuse a value: a proof in which a selector of h2w_select, an indicator of
 * h2w_select_array_by_indicator - in every part of a split one - or an operand of h2w_bits_to_num is above 1, in which more than one indicator of a
 * select on one-word entries is set (their sum need not be one word), or in which the operand of h2w_gl_reduce - the one inside
 * h2w_gl_mul_sub too - is 2^128 or more (where the eager calls fail) has status 5: decided on the operand, whether or not the result would come out
 * right.  Among 1, 2 and 5 the first op in program order wins, and all win over 4.  The cells in front of the first cell of the first such op are
 * those of the calls; the cells from there on are unspecified; no other proof of the batch changes.  What makes a run replayable:
 *   - control flow does not depend on values (true of the reference's gadgets: SURVEY 7);
 *   - a value that depends on the proof enters as a TAGGED proof word: h2w_trace_input(ctx, word, n) just before the h2w_load_witness /
 *     h2w_gl_load_witness / h2w_load_constant / h2w_gl_load_constant that loads it (n = 1: a Goldilocks element, 4: a BN254 hash);
 *   - hints are computed by the library: the two sites where the reference reads AssignedValue::value() for one (base.rs:382, extension.rs:327)
 *     are h2w_gl_div and h2w_gl_ext_inv_witness;  an untagged witness is an error at h2w_plan_from_trace.
 * parallel_scopes: names of h2w_push_context scopes whose instances do not depend on one another (the reference's #[count] scopes
 * "verify_query_round", fri/mod.rs:488-501, and "verify_proof_to_cap_with_cap_index", merkle/mod.rs:57-78): each instance becomes a lane of the
 * device program.  The library VERIFIES the claim on the tape (an instance may read what its enclosing scopes computed before it and nothing else;
 * nothing outside reads what it computes) and fails otherwise.  The plan supports h2w_plan_num_cells / _proof_words / _num_records /
 * _workspace_bytes / _status (4: a proof word outside its field, as a compiled plan reports it), h2w_fri_witness_batch, h2w_fri_witness_batch_columns
 * and h2w_plan_free, and:
 *   - (proof, query) sharding: the shard units are the instances of the parallel scopes at depth 1 ("verify_query_round": unit q = the q-th
 *     instance in tape order, where the compiled plan's query block q starts), the prologue block is the root's.  h2w_plan_strand_layout /
 *     _shard_cells / _shard_block / _shard_workspace_bytes, h2w_fri_witness_batch_shard and h2w_fri_witness_batch_shard_compact (world >= 2) work
 *     as on the compiled plan of the shape, with its layout.  A plan whose depth-1 instances do not tile the stream behind the root's block (none,
 *     or only "verify_proof_to_cap_with_cap_index" parallel) refuses every shard call, saying why; so does the packed call with world 1.
 *   - keygen metadata, when the tracing context was created with witness_gen_only = 0 (the lists it recorded): h2w_plan_num_gates / _num_lookups /
 *     _selectors / _lookup_cells / _num_equalities / _equalities / _num_const_equalities / _const_equalities (the proof-word constants of
 *     Goldilocks-Poseidon caps taken from the proof passed in), and so h2w_check_constraints and h2w_layout_lookup_columns.  A plan traced with
 *     witness_gen_only != 0 refuses them. */
int h2w_ctx_trace_begin(h2w_ctx *);                                   /* on a fresh context */
int h2w_trace_input(h2w_ctx *, uint64_t word, uint32_t n_words);      /* no-op on a context that is not tracing */
h2w_plan *h2w_plan_from_trace(h2w_ctx *, uint64_t proof_words, const char *const *parallel_scopes, size_t n_scopes, int device_id);
/* h2w_plan_from_trace with options (flags == 0: exactly h2w_plan_from_trace; consts may then be null).
 * H2W_TRACE_FUSE_GL_PERMUTE: stretches of the tape that ARE a Goldilocks-Poseidon permutation on `consts` run as one device op each instead of
 * ~2,600 interpreted ones.  The library records its own PoseidonChip::permute (h2w_chip_gl_poseidon_permute) on `consts` once, lowers it like the
 * caller's tape, and fuses a stretch only if it equals that canonical tape word for word - op codes, record templates, constant values, dataflow -
 * with its 12 inputs abstracted, lies in one segment, and nothing outside it reads a value it computes other than its 12 outputs.  Scope names play
 * no part, traced values neither.  Everything else - a permutation on other tables, a hand-driven variant, a stretch with a value that escapes - stays
 * interpreted: the stream is the same either way.  The lane computes the permutation's values (plonky2's fast form) and lists {first record,
 * input state}; one wavefront per listed permutation writes its records before the expansion.  The plan needs 104 more bytes of workspace per
 * fused permutation and proof; every call that works on a traced plan works on it.
 * h2w_plan_trace_info: out = {ops of the trace, segments, templates, fused permutations, permutation-shaped stretches left interpreted (other
 * constants, or an interior value read outside), list entries per proof}.
 * h2w_plan_trace_timing (a traced plan on a device): the first call switches event timing on and returns 0; later calls wait for the plan's last
 * witness call and fill ms[] with the time of each of its kernels in launch order - k_replay depth by depth, the permutation records' kernel (0
 * without fused permutations), the expansion - and return how many (at most cap).
 * H2W_TRACE_FUSE_BN_PERMUTE (may be combined with H2W_TRACE_FUSE_GL_PERMUTE; `consts` is required when either is set): the same for PoseidonBN254.
 * The canonical tape is the library's own PoseidonBN254PermutationChip::permute (h2w_chip_bn_poseidon_permute) on `consts`' bn_c / bn_s / bn_m / bn_p
 * with its 4 inputs abstracted - an input may be whatever the caller's tape has there: a computed value of any width, a value of an enclosing scope, a
 * proof hash, a literal such as the sponge's zero capacity element.  A fused stretch is ONE device op instead of ~700: the lane computes the four
 * outputs (state times R, one Montgomery product per multiplication, x^5 in three) and lists {first cell of the permutation in the proof's stream,
 * zero-cell flag, the 4 x 32-byte input state}; a second kernel, one quad of lanes per listed permutation, writes its 4,032 cells from that state
 * (64 contiguous bytes per quad and store) after the interpreter and beside nothing it depends on.  halo2-base caches the first load_zero cell of a
 * context, so the first PoseidonBN254 permutation to run may hold that one extra cell inside its first mix: such a stretch is recognised (the
 * canonical tape is recorded in both variants) and left interpreted - at most one per trace.  The plan needs 144 more bytes of workspace per fused
 * PoseidonBN254 permutation and proof (the list entry: 18 u64 words, behind the value store and the Goldilocks list); h2w_plan_workspace_bytes changes
 * for plans built with this flag only (the value store loses the fused stretches' interior values: the total is usually smaller).  Every call that works on a traced plan works on it (flat, _columns, _shard, _shard_compact, _status, the
 * keygen metadata); flags 0 and 1 are exactly as before.
 * h2w_plan_trace_info_bn: out = {fused PoseidonBN254 permutations, PoseidonBN254-shaped stretches left interpreted (other constants, an interior
 * value read outside, the zero-cell variant), list entries per proof}; h2w_plan_trace_info's counts stay the Goldilocks ones.
 * h2w_plan_trace_timing of a plan built with H2W_TRACE_FUSE_BN_PERMUTE reports one more kernel: the PoseidonBN254 emission, behind the Goldilocks
 * record kernel's slot and in front of the expansion (0 when nothing was fused).
 * h2w_plan_trace_op_counts: what the device program consists of, counted on the host when the plan was lowered, over the final tapes of all its
 * templates: out[op] = how many ops of device op code `op` (csrc/tapefmt.h DOP_*: op < DOP_COUNT), then out[DOP_COUNT + k] = the DOP_FETCH ops whose
 * operand is of reference kind k (RK_LOCAL .. RK_LITFR: a value of the lane more than 256 slots back, a value of an enclosing scope, a 64-bit
 * constant beyond the 2,048 kept at hand, a proof word, a wide constant beyond the 472 kept at hand), then the longest DOP_GLOPRUN.  At most n_out
 * entries are written (the rest of out is zeroed); returns how many there are, -1 on a plan that was not traced.
 * One op's operands: an operand that is not at hand (above) is fetched into the lane's 256 value slots in front of the op.  An op whose fetched
 * operands need more than 256 slots is refused by h2w_plan_from_trace, by name and with the count: in practice h2w_select_array_by_indicator /
 * h2w_select_from_idx on 52 to 64 wide (four-word) entries, whose 4 n + n operand words cannot all be at hand - a traced PoseidonBN254 verifier
 * with cap_height 6 (64 cap entries) is such a run; up to 51 wide entries (cap_height 5) replay, and so does any
 * length up to 64 of one-word entries.
 * H2W_TRACE_SPLIT_SELECTS (combines freely with the other flags; alone, `consts` may be null) lifts that refusal for the wide select: where its
 * fetched operands need more than the 256 slots, the lowering cuts it at entry boundaries into as few consecutive parts as the 256 slots allow, each
 * with its own fetches in front of it; the running sum passes from part to part in the lane's registers (no value slot, no workspace), the last part
 * stores the result.  The cells - the leading zero, then entry, indicator, sum per entry -, the gates, the status words and the stream are those of
 * the select as one op; h2w_plan_trace_op_counts counts every part as one wide select.  Every call that works on a traced plan works on one with
 * parts (flat, _columns, _shard, _shard_compact, _status, the keygen metadata, H2W_OPT_OUTPUT_FORM with H2W_TRACE_OUTPUT_FORMS,
 * h2w_trace_verdict_batch).  A plan in which nothing had to be split is the plan lowered without the flag, and runs the same kernels; any other op
 * whose fetched operands need more than 256 slots is refused as before, and so is everything else the lowering refuses.
 * H2W_TRACE_OUTPUT_FORMS (combines freely with the fuse flags; alone, `consts` may be null): the lowering also builds, on the host, the map of the
 * plan's direct cells - the cells the expansion kernel does not write: the interpreter's own and, with H2W_TRACE_FUSE_BN_PERMUTE, the 4,032 of every
 * fused PoseidonBN254 permutation - as the complement of the record ranges, and checks that direct cells + record cells are the cells of the stream.
 * Such a plan accepts H2W_OPT_OUTPUT_FORM as a compiled plan does (below: canonical by default, the form may change between calls, constants and
 * bitmap uploaded when the Montgomery form is first selected), in every call that works on a traced plan (flat, _columns, _shard, _shard_compact), and
 * answers h2w_plan_direct_cells / h2w_plan_record_ranges.  In Montgomery form the record cells leave the expansion kernel converted, the fused
 * PoseidonBN254 permutations' cells leave their emission kernel converted (stored once: a Montgomery instantiation of that kernel, on a Montgomery copy
 * of the plan's cell table), and one ranged kernel converts the remaining direct cells in place.  Its h2w_plan_trace_timing reports one more entry, the direct cells' conversion, between
 * the PoseidonBN254 emission's slot and the expansion (0 in canonical form).  Sizes, status words and the stream in canonical form are those of the
 * plan without the flag; a plan lowered without it is exactly as before.  (Flag values 4 and 16 are unassigned and refused.) */
#define H2W_TRACE_FUSE_GL_PERMUTE 1
#define H2W_TRACE_FUSE_BN_PERMUTE 2
#define H2W_TRACE_OUTPUT_FORMS 8
#define H2W_TRACE_SPLIT_SELECTS 32
h2w_plan *h2w_plan_from_trace_ex(h2w_ctx *, uint64_t proof_words, const char *const *parallel_scopes, size_t n_scopes, int device_id,
                                 const h2w_poseidon_consts_t *consts, uint32_t flags);
int h2w_plan_trace_info(const h2w_plan *, uint64_t out[6]);
int h2w_plan_trace_info_bn(const h2w_plan *, uint64_t out[3]);
int h2w_plan_trace_op_counts(const h2w_plan *, uint64_t *out, size_t n_out);
int h2w_plan_trace_timing(h2w_plan *, float *ms, uint32_t cap);
/* ---- per-proof verdicts of a TRACED plan (3b below is the compiled plan's call; h2w_fri_verdict_batch refuses a traced plan).
 * While a context records a trace, every h2w_constrain_equal(a, b) - and the assert_equal inside h2w_gl_div - is kept beside the tape: its two handles'
 * cells, its place, and the SITE WORD in force.  h2w_trace_site(ctx, flag_bits) sets that word (0 at h2w_ctx_trace_begin; a no-op returning 0 on a
 * context that is not tracing): call it where a protocol check begins, with the bits its failing equalities shall raise - h2w_chip_verify_stark calls it
 * with the H2W_VERDICT_* bit of every Merkle / fold / final-polynomial site and with 0 where a query round begins.  The word also goes with every
 * h2w_range_check / h2w_check_less_than_safe recorded after it (a range site).  Recording changes nothing of the tape or of the plan lowered from it.
 * h2w_plan_from_trace lowers the recorded checks to a per-template table once the witness plan is final; where it cannot - a handle that is no traced
 * call's result, a value interior to a fused permutation (no longer in the value store), instances of one template whose checks differ - the plan is
 * built as before and only its verdict is unavailable; the reason is h2w_last_error() after the two calls below.
 * h2w_trace_verdict_batch runs the replay's interpreter on quiet lanes (values into the workspace's value store; no record, no cell, no list entry; no
 * emission kernel, no expansion) and one kernel that compares both sides of every recorded equality, as 256-bit values zero-extended from their widths:
 *   flags        OR of the site words of the failing equalities and range sites, | H2W_TRACE_VERDICT_RANGE for a failing range site (a value beyond its
 *                range_bits; for check_less_than_safe a value >= the bound)
 *   n_failed     failing equalities, + 1 for a range site whose value does not fit the ceil(bits / lookup_bits) limbs RangeChip::range_check decomposes
 *                it into (more than one limb: the copy constraint on the limb sum, as 3b counts it for the PoW response); check_less_than_safe(a, b) is
 *                range_check(a, n limbs) and range_check(a + 2^(n lookup_bits) - b, n limbs): a >= b breaks the second limb sum (+ 1 with n > 1)
 *   first_query  the lowest shard unit (the depth-1 parallel instance an equality's scope is or lies in) that owns a failing equality; 0xFFFFFFFF: none
 *                fails, or only the root's, or the plan has no units.  Range sites do not count here
 *   status       the word h2w_plan_status reports after a witness call of the plan on the same proofs (1, 2: the hint ops; 5: a value outside its op's domain; 4: a proof word outside its field)
 * A proof is accepted iff flags == 0 && n_failed == 0 && status == 0.  On a trace of h2w_chip_verify_stark the first three words are those of 3b's call
 * on the compiled plan of the shape (the hint checks in the prologue, which 3b's kernels do not judge, can only fail beside status 1 / 2).
 * workspace_dev: h2w_plan_workspace_bytes(n_proofs) bytes, the witness call's (the value store and the status words live there; whoever runs next on it
 * re-zeroes its status words).  Stream-ordered; the first call of a batch size uploads a lane table (one device synchronisation, as the first sharded
 * call); the plan's device is current for the call only; n_proofs == 0: 0; whole proofs only; nothing but the workspace and verdict_dev is written.
 * -1 before any device work, the reason in h2w_last_error(): a null plan or buffer, a plan of h2w_plan_compile, a plan whose verdict is unavailable,
 * no device, more than 65,535 proofs or 2^31 lanes.
 * h2w_plan_trace_verdict_info: out = {equalities recorded, equalities in the device tables summed over instances, range sites, 1 if the verdict call
 * is available (else 0, the reason in h2w_last_error()), templates with a table, 0}.  No device needed.  -1 for a plan of h2w_plan_compile. */
int h2w_trace_site(h2w_ctx *, uint32_t flag_bits);
int h2w_plan_trace_verdict_info(const h2w_plan *, uint64_t out[6]);

/* ------------------------------------------------------------------ advice hand-off (eager contexts) */
/* Expands all pending records on the GPU; *dev_ptr receives a device pointer to num_cells*32 bytes
 * owned by the context (valid until the next h2w_* call on it). */
int h2w_ctx_advice_device(h2w_ctx *, void **dev_ptr);
/* Copies cells [first, first+count) to host memory (expanding on the GPU first). */
int h2w_ctx_download(h2w_ctx *, uint64_t first, uint64_t count, h2w_fr_t *host_dst);

/* ------------------------------------------------------------------ 3. batched hot path */
/* Shape compile: replays the gadget once (host) to lay out every cell block of
 * load_proof_with_pis + verify_proof for this shape; uploads tables + constants to `device_id`. */
h2w_plan *h2w_plan_compile(const h2w_shape_t *, const h2w_poseidon_consts_t *, int device_id);
void      h2w_plan_free(h2w_plan *);
uint64_t  h2w_plan_num_cells(const h2w_plan *);         /* advice cells per proof */
uint64_t  h2w_plan_proof_words(const h2w_plan *);       /* u64 words per flat proof (layout: INTEGRATION.md) */
uint64_t  h2w_plan_num_records(const h2w_plan *);
/* Scratch bytes the batch call needs on the device for n_proofs (records, challenge blocks, traces). */
uint64_t  h2w_plan_workspace_bytes(const h2w_plan *, uint64_t n_proofs);
/* proofs_dev:  n_proofs * proof_words u64, device memory.
 * advice_dev:  n_proofs * num_cells * 32 bytes, device memory (canonical LE Fr).
 * workspace_dev: h2w_plan_workspace_bytes bytes, device memory.
 * stream: hipStream_t (NULL = default stream).  Asynchronous: returns after enqueueing. */
int h2w_fri_witness_batch(h2w_plan *, const uint64_t *proofs_dev, uint64_t n_proofs,
                          void *advice_dev, void *workspace_dev, void *stream);
/* Same, with the HBM-bound expansion kernel issued on `emit_stream` (ordered after the value strands by an event; `stream`
 * waits for it).  Lets a caller give the latency-bound value strands and the streaming kernel differently CU-masked streams. */
int h2w_fri_witness_batch2(h2w_plan *, const uint64_t *proofs_dev, uint64_t n_proofs,
                           void *advice_dev, void *workspace_dev, void *stream, void *emit_stream);
/* The expansion kernel alone: re-expands the block records a previous h2w_fri_witness_batch* call (same n_proofs) left in
 * workspace_dev into advice_dev (flat layout).  Cells the value kernels write directly are not touched.  For measurement. */
int h2w_fri_expand_records(h2w_plan *, uint64_t n_proofs, void *advice_dev, void *workspace_dev, void *stream);
/* ---- keygen-side bookkeeping of an eager context created with witness_gen_only == 0 (halo2-base Context when
 * witness_gen_only is false; semantics [R]): gate cells (selector on), range-lookup registrations (in order),
 * copy constraints (advice_equalities: pairs of cell offsets) and constant equalities (cell, constant). */
uint64_t h2w_ctx_num_gates(h2w_ctx *);           int h2w_ctx_gate_cells(h2w_ctx *, uint64_t *cells);
uint64_t h2w_ctx_num_lookups(h2w_ctx *);         int h2w_ctx_lookup_cells(h2w_ctx *, uint64_t *cells);
uint64_t h2w_ctx_num_equalities(h2w_ctx *);      int h2w_ctx_equalities(h2w_ctx *, uint64_t *pairs /* 2 per equality */);
uint64_t h2w_ctx_num_const_equalities(h2w_ctx *); int h2w_ctx_const_equalities(h2w_ctx *, uint64_t *cells, h2w_fr_t *values);

/* ---- the consumer-side format of the advice stream -------------------------------------------
 * The cell stream of a shape is static, so its keygen metadata is too.  Restates (halo2-lib `community-edition`, not in
 * /root/reference; semantics [R]): Context::selector (one bit per cell: a vertical gate starts there),
 * the range-lookup registrations (RangeChip::range_check -> cells_to_lookup, in registration order), the FlexGate
 * break points (gates/flex_gate/threads: assign_with_constraints) and the column assignment of the witness
 * (assign_witnesses) incl. the lookup-advice columns, and the copy manager's lists (advice_equalities, constant_equalities). */
uint64_t h2w_plan_num_gates(h2w_plan *);
uint64_t h2w_plan_num_lookups(h2w_plan *);
int h2w_plan_selectors(h2w_plan *, uint8_t *bitmap /* (num_cells + 7) / 8 bytes, bit i = cell i */);
int h2w_plan_lookup_cells(h2w_plan *, uint64_t *cells /* num_lookups */);
/* Copy constraints (pairs of cell offsets: Context::constrain_equal and the copies of Existing cells into gates, field/native.rs:185-193)
 * and constant equalities (cell, constant) of the plan's cell stream - what the halo2-base Context the reference hands to MockProver
 * carries (stark/mod.rs:483-518).  Built on first use by replaying the shape through an eager keygen context on the host. */
uint64_t h2w_plan_num_equalities(h2w_plan *);
uint64_t h2w_plan_num_const_equalities(h2w_plan *);
int h2w_plan_equalities(h2w_plan *, uint64_t *pairs /* 2 per equality */);
/* proof_words (host, h2w_plan_proof_words of them) may be NULL with PoseidonBN254 caps; with Goldilocks-Poseidon caps the reference loads
 * every hash wire of the proof as a CONSTANT (hash/poseidon/hash.rs:86-96), so those constants are the proof's own words. */
int h2w_plan_const_equalities(h2w_plan *, const uint64_t *proof_words, uint64_t *cells, h2w_fr_t *values);
/* break_points[c] = last used row of column c (the cell there is repeated at row 0 of column c + 1); max_rows = 2^k - unusable_rows.
 * out may be NULL to query *n_out. */
int h2w_break_points(const uint8_t *selectors, uint64_t n_cells, int k, int unusable_rows,
                     uint64_t *out, uint64_t cap, uint64_t *n_out);
/* flat advice (device) -> columns[n_proofs][n_bp + 1][2^k] (device, 32-byte canonical Fr, unassigned rows zero).  Every break point
 * is a row 1 .. 2^k - 1 and the columns must fit n_cells (the last one takes the rest, at most 2^k cells): anything else is -1. */
int h2w_layout_columns(const void *advice_dev, uint64_t n_cells, uint64_t proof_stride_cells, uint64_t n_proofs,
                       const uint64_t *break_points, uint64_t n_bp, int k, void *columns_dev, void *stream);
/* The same result as h2w_fri_witness_batch + h2w_layout_columns without materialising the flat stream: every kernel writes its
 * cells straight to columns_dev[n_proofs][n_bp + 1][2^k] (a piecewise-constant address shift per column; a small fix-up kernel repeats
 * the boundary cells and zeroes the unused rows).  k >= 12.  Workspace as for h2w_fri_witness_batch. */
int h2w_fri_witness_batch_columns(h2w_plan *, const uint64_t *proofs_dev, uint64_t n_proofs, const uint64_t *break_points, uint64_t n_bp,
                                  int k, void *columns_dev, void *workspace_dev, void *stream);
/* lookup advice columns: out[n_proofs][*n_cols_out][2^k]; out_dev may be NULL to query *n_cols_out.  unusable_rows as for
 * h2w_break_points: 2^k > unusable_rows + 4, or -1. */
int h2w_layout_lookup_columns(h2w_plan *, const void *advice_dev, uint64_t proof_stride_cells, uint64_t n_proofs,
                              int k, int unusable_rows, void *out_dev, uint64_t *n_cols_out, void *stream);

/* Device-side constraint check of advice streams (restated MockProver gate + lookup checks): bad[0] = vertical
 * gates a[i] + a[i+1]*a[i+2] != a[i+3] over the selector-enabled cells, bad[1] = looked-up cells >= 2^lookup_bits, summed over
 * the n_proofs streams.  A gate also counts as failed when one of its four cells is not a field element (>= r: the unreduced
 * cells of a status-4 stream), whatever it is congruent to, and when it starts in the last three cells of the stream.
 * Synchronises the stream.  Covers every cell of full-size streams without the CPU oracle. */
int h2w_check_constraints(h2w_plan *, const void *advice_dev, uint64_t proof_stride_cells, uint64_t n_proofs,
                          uint64_t bad[2], void *stream);

/* (proof, query) sharding across the GPUs of a node (north star: "independent FRI queries and Merkle paths sharded across
 * the 8 GPUs"; the loop being dealt out is fri/mod.rs:488-501): rank r of `world` generates, at their global offsets in its own
 * advice_dev[n_proofs][num_cells], the prologue block of the proofs it owns (proof % world == r: witness load, challenger, PoW, reduced
 * openings) and the query blocks of the units (proof * num_queries + query) % world == r; the other blocks are not touched.  A rank
 * LAUNCHES only what it owns: its strand kernels run over its own units, its expansion kernel walks its own record ranges, so the
 * chain / glue / expansion time of a rank is 1 / world of the unsharded launch's.  The one exception is the values of the prologues
 * (one wavefront per proof, a fixed latency whatever the number of proofs): every rank needs every proof's challenges and computes
 * them itself - cheaper than a collective in the middle of the call; only the owner writes the block.  No collective on the data path:
 * every rank needs the proofs (one broadcast) and nothing else.  The ranks' blocks are disjoint and their union is the full stream. */
int h2w_fri_witness_batch_shard(h2w_plan *, const uint64_t *proofs_dev, uint64_t n_proofs, void *advice_dev, void *workspace_dev,
                                void *stream, int rank, int world);
/* The same blocks PACKED: shard_advice_dev holds only this rank's blocks, h2w_plan_shard_cells(plan, n_proofs, rank, world) cells, back to
 * back in (proof, block) order (prologue block first, then the owned query blocks by query number; every query block takes a slot of the
 * larger of the two query block sizes) - a rank's buffer is 1 / world of the stream, so the batch that fits a GPU grows with the world.
 * h2w_plan_shard_block: where a block lies - *local_cell in the packed buffer, *n_cells long, *global_cell its offset inside its proof's
 * flat stream; query < 0: the prologue block.  Returns 1 (and writes nothing) when the block belongs to another rank. */
uint64_t h2w_plan_shard_cells(const h2w_plan *, uint64_t n_proofs, int rank, int world);
/* Scratch bytes a sharded call (either form) of this rank needs for n_proofs: the per-proof pieces of h2w_plan_workspace_bytes plus the
 * PoseidonBN254 unit buffers of the rank's own (proof, query) units only (1 / world of them).  A workspace of h2w_plan_workspace_bytes(n_proofs)
 * bytes is always large enough. */
uint64_t h2w_plan_shard_workspace_bytes(const h2w_plan *, uint64_t n_proofs, int rank, int world);
int h2w_plan_shard_block(const h2w_plan *, int rank, int world, uint64_t proof, int query, uint64_t *local_cell, uint64_t *n_cells, uint64_t *global_cell);
int h2w_fri_witness_batch_shard_compact(h2w_plan *, const uint64_t *proofs_dev, uint64_t n_proofs, void *shard_advice_dev, void *workspace_dev,
                                        void *stream, int rank, int world);
/* The block structure of a proof's cell stream that the sharding above follows (static per shape; no device needed):
 * out[0] = cells of the prologue block [0, out[0]); out[1] = cells of query block 0 (it holds the Context's one cached load_zero
 * cell when that falls into a query); out[2] = cells of every later query block; out[3] = cells per proof
 * (= out[0] + out[1] + (num_queries - 1) * out[2]). */
int h2w_plan_strand_layout(const h2w_plan *, uint64_t out[4]);
/* The rest of the restated MockProver: copy constraints (bad[0] = pairs whose two cells differ) and constant equalities (bad[1])
 * over device advice streams.  The lists are static per shape: h2w_plan_equalities / h2w_plan_const_equalities (or an eager keygen
 * context of the same shape: h2w_ctx_equalities / h2w_ctx_const_equalities).  Synchronises the stream. */
int h2w_check_equalities(const void *advice_dev, uint64_t n_cells, uint64_t proof_stride_cells, uint64_t n_proofs,
                         const uint64_t *pairs, uint64_t n_pairs, const uint64_t *const_cells, const h2w_fr_t *const_values,
                         uint64_t n_const, uint64_t bad[2], void *stream);

/* Per-proof device status words.  0 = ok.  1 = GoldilocksChip::div by zero (reference asserts, base.rs:379), 2 = extension
 * inverse of zero (extension.rs:327), 3 = challenger input buffer overflow, 4 = the proof holds a word outside its field's
 * canonical range (a Goldilocks word >= p or a BN254 hash >= r: not representable by the reference's types; the cells are
 * still produced — identical to the reference's arithmetic for Goldilocks words, unreduced for the hash), 5 = a traced
 * plan only (2d): a replayed value left the domain its op was lowered for (a selector, indicator or bit above 1, a second
 * indicator set on one-word entries, 2^128 or more in front of GoldilocksChip::reduce); the cells from that op on are
 * unspecified.  The first condition met wins. */
int h2w_plan_status(h2w_plan *, const void *workspace_dev, uint64_t n_proofs, uint32_t *host_status, void *stream);
/* 32-byte checksum of n_cells cells (for streamed configurations, whose advice buffers are re-used before anything could read them
 * back): digest[j] = sum over cells i of limb_j(cell i) * ((((i + 1) * 0x9E3779B97F4A7C15) | 1) + 2 j)  mod 2^64 - position-dependent,
 * order-independent in its evaluation.  digest4_dev: 4 x u64, device.  One call per proof. */
int h2w_advice_digest(const void *advice_dev, uint64_t n_cells, uint64_t *digest4_dev, void *stream);
/* ---- Multi-GPU ingest: one process per GPU, no data-path collective.  The only exchange is ONE broadcast of the flat proof block
 * from the ingest rank (RCCL over xGMI); after it every rank runs h2w_fri_witness_batch on its own proofs or h2w_fri_witness_batch_shard on
 * its (proof, query) units.  Optionally the ranks gather each other's h2w_advice_digest words.  RCCL is loaded at the first call here
 * (dlopen), so the rest of the library works without it.  Replaces, for a caller without torch.distributed, what bench.py does with
 * dist.broadcast; the reference has no counterpart (single process, fri/mod.rs:488-501 is the loop being sharded).
 * id: H2W_COMM_ID_BYTES bytes made by h2w_comm_unique_id on one rank and handed to the others by any out-of-band channel. */
#define H2W_COMM_ID_BYTES 128
typedef struct h2w_comm h2w_comm;
int h2w_comm_unique_id(void *id128);
h2w_comm *h2w_comm_init(const void *id128, int rank, int world, int device_id);      /* collective: every rank calls it */
void h2w_comm_free(h2w_comm *);
int h2w_comm_rank(const h2w_comm *);
int h2w_comm_world(const h2w_comm *);
int h2w_comm_broadcast_proofs(h2w_comm *, uint64_t *proofs_dev, uint64_t n_words, int root, void *stream);      /* in place */
int h2w_comm_allgather_digests(h2w_comm *, const uint64_t *digest4_dev, uint64_t *all_dev /* [world][4] */, void *stream);
/* Output format: the stream is canonical little-endian Fr (what Fr::from_repr / to_repr use).  For a consumer that copies cells into
 * halo2curves' in-memory representation (Montgomery form, R = 2^256) this converts n_cells cells in place on the device. */
int h2w_advice_to_montgomery(void *cells_dev, uint64_t n_cells, void *stream);
/* H2W_OPT_OUTPUT_FORM (default H2W_FORM_CANONICAL): the form of every cell that h2w_fri_witness_batch, _batch2, _columns, _shard and _shard_compact
 * (and h2w_fri_expand_records) write for this plan.  H2W_FORM_MONTGOMERY: every cell holds v * 2^256 mod r, four little-endian u64 limbs - halo2curves'
 * bn256::Fr as it lies in memory, so a consumer fills Context::advice with a plain copy - without a second pass over the stream: the expansion kernel
 * converts its cells in registers as it writes them (by their width: they are values below 2^128), and one ranged kernel converts the cells the value
 * kernels wrote themselves (h2w_plan_direct_cells) in place before the call completes.  Column layouts (boundary cells repeated, unused rows zero) and
 * sharded calls (only this rank's blocks are touched) hold as in the canonical form.  Status words, workspace sizes, cell counts, layouts and the
 * keygen metadata do not depend on the form.  h2w_advice_digest, h2w_check_constraints, h2w_check_equalities, h2w_layout_columns and
 * h2w_layout_lookup_columns read cells as canonical values: they are meant for canonical streams (the layouts only move cells and work on either).
 * A traced plan takes the option when it was lowered with H2W_TRACE_OUTPUT_FORMS (h2w_plan_from_trace_ex, 2d): its record cells leave the expansion
 * kernel converted, so do the fused PoseidonBN254 permutations' cells their emission kernel, and the ranged kernel converts the other direct cells
 * - the interpreter's - behind their writers and in front of the expansion, on the call's stream.  A plan made by h2w_plan_from_trace, or by h2w_plan_from_trace_ex without that flag,
 * refuses H2W_FORM_MONTGOMERY (-1): its stream is canonical; convert it with h2w_advice_to_montgomery.
 * Any other value: -1.  The form may be changed between calls. */
#define H2W_OPT_OUTPUT_FORM 5
#define H2W_FORM_CANONICAL 0
#define H2W_FORM_MONTGOMERY 1
/* The cells of a proof's stream that value kernels write themselves (PoseidonBN254 permutation units, selects, inverses, ...): bit i of the bitmap
 * ((num_cells + 7) / 8 bytes) = cell i; the others - h2w_plan_num_record_cells of them - are written by the expansion kernel, record by record:
 * ranges[2 i] = first cell of record i, ranges[2 i + 1] = its cells (h2w_plan_num_records records).  Static per shape, no device needed.  Of
 * traced plans, those lowered with H2W_TRACE_OUTPUT_FORMS answer (the others: -1). */
int h2w_plan_direct_cells(const h2w_plan *, uint8_t *bitmap);
int h2w_plan_record_ranges(const h2w_plan *, uint64_t *ranges);
/* Scheduling options of a plan.  H2W_OPT_FORK_CHAINS (default 1): with PoseidonBN254 Merkle caps the chain kernel of a batch call
 * runs on a library-owned side stream beside the query-glue and expansion kernels of the same call (they depend on the prologue
 * only); the caller's stream still completes when the whole advice is written.  0: every kernel on the caller's stream. */
#define H2W_OPT_FORK_CHAINS 1
/* H2W_OPT_SERIAL_EXPAND (default 1): the expansion kernel of a batch call
 * waits for the expansion kernel of the plan's previous batch call, whatever stream that was issued on, so that the latency-bound
 * strands of the other calls in flight find free CUs; the cells written are the same either way. */
#define H2W_OPT_SERIAL_EXPAND 2
/* H2W_OPT_CHAIN_PASSES (PoseidonBN254 caps): how the Merkle paths (merkle/mod.rs:57-78) are generated.
 * 1: one quad per path walks it and emits as it goes - the least arithmetic per cell, serial in the path's depth (18 permutations at 2^20
 *    rows, ~7 ms): right when many paths are in flight (large batches, several launches pipelined), which hide that latency.
 * 2: a values pass walks every path serially, then one quad per permutation emits its cells - all levels of all paths side by side.  The
 *    emission is a streaming kernel whose time is proportional to the work (1 / world of it in a sharded launch), at the price of evaluating
 *    every permutation twice: right for small or sharded launches, which the depth of a path would otherwise bound.
 * 0 (default): 2 for launches of at most 512 (proof, query) units of this rank, else 1.  The cells are the same either way. */
#define H2W_OPT_CHAIN_PASSES 3
/* H2W_OPT_VALUES_FORM (PoseidonBN254 caps, two-pass paths): how the values pass walks a path.  1: four lanes per path (a Montgomery product on one
 * lane); 2: one wavefront per path, a product spread over the 16 lanes of a row, one 29-bit limb per lane (a path in less than half the time, six
 * times the instructions per path: right while there is a SIMD for nearly every path).  0 (default): 2 for launches of at most 784 paths of this
 * rank (4 proofs of 2^20 rows x 28 queries), else 1: alone on the chip form 2 wins up to ~2,500 paths (profiles/r04_values_forms.jsonl), with other launches
 * in flight its instructions are not free - a caller that runs one launch at a time sets 2.  The cells are the same either way. */
#define H2W_OPT_VALUES_FORM 4
int h2w_plan_configure(h2w_plan *, int option, int value);
/* Kernel timing of a batch call, in ms, from HIP events the library records on the streams it launches on:
 * ms[0] = prologue strands (values; with PoseidonBN254 caps also the records of their permutations), ms[1] = query glue strands (with
 * Goldilocks-Poseidon caps also the Merkle strands' values and the records of every listed permutation), ms[2] = PoseidonBN254 Merkle
 * chains, values + emission (0 with Goldilocks-Poseidon caps), ms[3] = expansion kernel, ms[4] = whole call.
 * `back` = how many batch calls before the last one (a ring of the last 64 is kept).  Blocks until that batch finished. */
int h2w_plan_timing(h2w_plan *, uint64_t back, float ms[5]);
/* The same per kernel: ms[0] k_prologue_values (alone: the witness-load kernel k_prologue_load runs BEHIND it, beside the Merkle chains - nothing waits for its
 * cells - and is part of ms[6] only), ms[1] k_glp_emit (records of the listed Goldilocks-Poseidon permutations), ms[2] k_strands
 * (+ k_merkle_gl_values), ms[3] k_merkle_bn_values (one pass: k_merkle_bn_fused), ms[4] k_merkle_bn_emit, ms[5] expansion kernel, ms[6] whole call,
 * ms[7] = the H2W_OPT_CHAIN_PASSES the call ran with (PoseidonBN254 caps; else 0). */
int h2w_plan_timing_ex(h2w_plan *, uint64_t back, float ms[8]);
int h2w_plan_last_timing(h2w_plan *, float ms[5]);
/* Elapsed ms from event `which_a` of the batch call `back_a` calls before the last one to event `which_b` of the call `back_b` before
 * the last one (negative when b came first): how the kernels of different calls lie against each other on the device. */
#define H2W_EV_CALL_START 0
#define H2W_EV_PROLOGUE_END 1
#define H2W_EV_GLUE_START 2
#define H2W_EV_GLUE_END 3
#define H2W_EV_CHAINS_START 4
#define H2W_EV_CHAINS_END 5
#define H2W_EV_EXPAND_START 6
#define H2W_EV_EXPAND_END 7
#define H2W_EV_CALL_END 8
#define H2W_EV_COUNT 9
int h2w_plan_event_gap(h2w_plan *, uint64_t back_a, int which_a, uint64_t back_b, int which_b, float *ms);
/* Advice cells per proof written by the expansion kernel (the rest are written directly by the value kernels). */
uint64_t h2w_plan_num_record_cells(const h2w_plan *);
/* Advice cells per proof of the MerkleTreeChip::verify_proof_to_cap_with_cap_index calls (merkle/mod.rs:57-78): with PoseidonBN254
 * caps these are the cells the chain kernel writes itself (its permutations' 4,032 cells each, the selects, the cap lookup). */
uint64_t h2w_plan_num_chain_cells(const h2w_plan *);

/* ------------------------------------------------------------------ 3b. per-proof verdicts without a witness
 * The verifier gadget's protocol checks are assert_equal copy constraints: they emit no cells, so the stream of a proof the circuit will reject
 * looks like any other (only the proof-of-work range check shows in it, as a failing lookup).  h2w_fri_verdict_batch runs the VALUES of
 * StarkChip::verify_proof alone - the Fiat-Shamir prologue, the query glue, the Merkle paths - and stores nothing but one verdict per proof:
 * what a service runs in front of h2w_fri_witness_batch to drop the proofs that would waste a prover.
 *   flags        H2W_VERDICT_* bits of the checks that fail
 *   n_failed     chip-level assert_equal / assert_equal_fr calls of the proof's verify_proof whose two sides differ (a Goldilocks-Poseidon root counts
 *                four times, hash/poseidon/hash.rs:148-159; a PoseidonBN254 root once; an extension element twice; the hint checks of
 *                GoldilocksChip::div and the extension inverse count like any other and never fail; the PoW range check is in flags only - but
 *                RangeChip::range_check also constrains the response to equal the sum of the ceil((64 - pow_bits) / lookup_bits) limbs it is
 *                decomposed into, and a response that does not fit those limbs breaks that one copy constraint too: it is counted, and no query owns it)
 *   first_query  the lowest query index that owns a failing equality, 0xFFFFFFFF if there is none
 *   status       the word h2w_plan_status reports after h2w_fri_witness_batch on the same proofs
 * A proof is accepted iff flags == 0 && status == 0.  Without permutation Zs (n_perm_z == 0) initial oracle 1 is the quotient tree.
 * Stream-ordered, no synchronisation; whole proofs only (no sharded form); the call's workspace (challenge blocks) is a stream-ordered allocation
 * inside it; the result depends on no h2w_plan_configure option; the plan's device is current for the duration of the call only.
 * verdict_dev: [n_proofs], device.  n_proofs == 0: 0.  A plan of h2w_plan_from_trace: -1 (its call is h2w_trace_verdict_batch, 2d).  Without a device: -1 ("no HIP device"). */
typedef struct { uint32_t flags, n_failed, first_query, status; } h2w_verdict_t;
#define H2W_VERDICT_POW              1   /* pow_response does not fit 64 - pow_bits bits (fri/mod.rs:130-145) */
#define H2W_VERDICT_MERKLE_TRACE     2   /* a root != cap entry, per tree (merkle/mod.rs:57-78) */
#define H2W_VERDICT_MERKLE_PERM_Z    4
#define H2W_VERDICT_MERKLE_QUOTIENT  8
#define H2W_VERDICT_MERKLE_STEP     16   /* a commit-phase tree */
#define H2W_VERDICT_FOLD            32   /* fri/mod.rs:403-438, the consistency check of a fold step */
#define H2W_VERDICT_FINAL           64   /* final-polynomial evaluation */
int h2w_fri_verdict_batch(h2w_plan *, const uint64_t *proofs_dev, uint64_t n_proofs, h2w_verdict_t *verdict_dev, void *stream);
#define H2W_TRACE_VERDICT_RANGE 1u   /* = H2W_VERDICT_POW: set by a failing range site, beside the site word in force at it (2d) */
int h2w_trace_verdict_batch(h2w_plan *, const uint64_t *proofs_dev, uint64_t n_proofs,
                            h2w_verdict_t *verdict_dev, void *workspace_dev, void *stream);      /* 2d: the verdict call of a traced plan */
/* The same verdict words from other kernels and streams: `flags` = one H2W_VERDICT_FORM_*, optionally | H2W_VERDICT_FORK.  Every accepted value gives the
 * words h2w_fri_verdict_batch gives; flags == H2W_VERDICT_FORM_QUAD enqueues exactly what it enqueues.
 *   FORM_ROW   PoseidonBN254 caps only: one wavefront per Merkle path (the four rows of the wavefront hold the four state elements) instead of four lanes -
 *              a path's 18 dependent permutations in half the time with sixteen times the lanes: the form for a caller that judges a proof as it arrives
 *   FORM_AUTO  FORM_ROW while n_proofs x num_queries x (n_oracles + n_steps) is at most the crossover the library keeps (h2w_plan_verdict_form reports the
 *              choice), FORM_QUAD beyond it and always with hash_mode 0 (whose one Merkle kernel is a wavefront per path already)
 *   FORK       the query-glue kernel runs on a side stream of the plan beside the Merkle kernel (either hash mode) and the caller's stream waits for it before
 *              the verdicts are final and the call's workspace is released: still stream-ordered for the caller, no synchronisation.  The side stream is the
 *              one h2w_fri_witness_batch forks its chain kernels to from the same caller stream (work of the two is ordered on it); a plan serves at most 16
 *              caller streams with side streams - a further one runs the call unforked.
 * -1 before any device work, the reason in h2w_last_error(): a bit outside FORM_MASK | FORK, a form above FORM_ROW, FORM_ROW on a plan with hash_mode 0, a
 * plan of h2w_plan_from_trace.  Everything else as h2w_fri_verdict_batch. */
#define H2W_VERDICT_FORM_AUTO 0u      /* the library picks by the number of Merkle paths of the call */
#define H2W_VERDICT_FORM_QUAD 1u      /* the Merkle kernels of h2w_fri_verdict_batch */
#define H2W_VERDICT_FORM_ROW  2u      /* PoseidonBN254 caps: one wavefront per (proof, query, tree) */
#define H2W_VERDICT_FORM_MASK 0xFFu
#define H2W_VERDICT_FORK      0x100u  /* k_verdict_glue on a side stream of the plan, beside the Merkle kernel */
int h2w_fri_verdict_batch_ex(h2w_plan *, const uint64_t *proofs_dev, uint64_t n_proofs, h2w_verdict_t *verdict_dev, void *stream, uint32_t flags);
/* What FORM_AUTO resolves to for n_proofs of this plan's shape: H2W_VERDICT_FORM_QUAD or _ROW.  No device needed.  -1 for a traced plan. */
int h2w_plan_verdict_form(const h2w_plan *, uint64_t n_proofs);
/* The flat proof layout of the plan's shape (WitnessChip load order, witness/mod.rs:236-294; every hash is 4 words), in u64 words:
 *   out[0..11]  trace_cap, quotient_cap, openings, perm_cap, pow_witness, final_poly, commit_caps, queries (start of query 0), query_words (words per
 *               query), pis, total, cap_size (hashes per cap)
 *   out[12]     n_oracles, then per initial oracle o three words: init_off (start of its leaf within a query; its siblings follow the leaf), the leaf's
 *               length, init_sibs (siblings, 4 words each)
 *   then        n_steps, then per fold step i three words: step_off, the leaf's length (2 words per evaluation), step_sibs
 * so sibling j of tree t of query q starts at queries + q * query_words + off_t + len_t + 4 j.  Returns the number of words (14 + 3 n_oracles + 3 n_steps);
 * out == NULL: that number alone.  No device needed.  Not for traced plans (-1). */
int h2w_plan_proof_layout(const h2w_plan *, uint64_t *out, size_t n_out);

/* ------------------------------------------------------------------ 2c. batched chip ops on the device
 * n independent instances of ONE GoldilocksChip / GoldilocksQuadExtChip operation, each in a fresh Context: the operands are loaded
 * as witnesses (GoldilocksChip::load_witness, 28 cells each at lookup_bits 21; extension elements as two), then the op - the shape
 * of the reference's chip tests (field/goldilocks/base.rs:476-495, extension.rs:473-493).  One lane per instance computes the
 * values, the expansion kernel writes advice_dev[n][num_cells].  status_dev[i] = 0, or 1 / 2 where the reference panics
 * (GoldilocksChip::div by zero, base.rs:379; extension inverse of zero, extension.rs:327: the cells are then those of the op on
 * the substituted operand 1, as in the batched verifier path).  operands_dev: [n][num_operands] canonical Goldilocks words. */
#define H2W_OP_GL_ADD 0      /* a, b       base.rs:251-260 */
#define H2W_OP_GL_SUB 1      /* a, b       base.rs:274-283 */
#define H2W_OP_GL_MUL 2      /* a, b       base.rs:296-305 */
#define H2W_OP_GL_MUL_ADD 3  /* a, b, c    base.rs:319-329 */
#define H2W_OP_GL_DIV 4      /* a, b       base.rs:371-393 */
#define H2W_OP_GL_INV 5      /* a          base.rs:395-399 */
#define H2W_OP_EXT_MUL 6     /* a0 a1 b0 b1  extension.rs:211-234 */
#define H2W_OP_EXT_INV 7     /* a0 a1        extension.rs:320-340 */
#define H2W_OP_EXT_DIV 8     /* a0 a1 b0 b1  extension.rs:237-246 */
typedef struct h2w_chipbatch h2w_chipbatch;
h2w_chipbatch *h2w_chipbatch_new(int op, int lookup_bits, int device_id);
void           h2w_chipbatch_free(h2w_chipbatch *);
uint64_t       h2w_chipbatch_num_operands(const h2w_chipbatch *);   /* u64 words per instance */
uint64_t       h2w_chipbatch_num_cells(const h2w_chipbatch *);      /* advice cells per instance */
int            h2w_chipbatch_run(h2w_chipbatch *, const uint64_t *operands_dev, uint64_t n, void *advice_dev, uint32_t *status_dev, void *stream);
/* The hash and Merkle chips, batched the same way (csrc/chiphash.hip): every instance a fresh Context, its operands loaded the way the
 * verifier's WitnessChip loads them, then the op.  Created by h2w_chipbatch_new_hash (h2w_chipbatch_new refuses these ops, and
 * h2w_chipbatch_new_hash refuses ops 0-8); num_operands / num_cells / run / free are the calls above.  Operand words per instance, in
 * this order:
 *   GL_PERMUTE     12 Goldilocks words                          GoldilocksChip::load_witness each, then permute (hash_mode ignored)
 *   BN_PERMUTE     4 x 4 words (little-endian Fr)               NativeChip::load_witness each, then permute
 *   HASH_NO_PAD    n_in Goldilocks words                        load_witness each, then hash_no_pad
 *   TWO_TO_ONE     2 hashes x 4 words                           HasherChip::load_witness each, then two_to_one
 *   MERKLE_VERIFY  leaf[n_in], leaf_index, cap[2^cap_height][4], siblings[depth - cap_height][4]:
 *                  the leaf by load_witness; the index by load_witness, then num_to_bits(index, depth); the cap, then the siblings, by
 *                  HasherChip::load_witness; cap_index = bits_to_num(bits[depth - cap_height ..]); verify_proof_to_cap_with_cap_index
 * A hash is four words in both modes: four Goldilocks words loaded as CONSTANTS (hash_mode 0, poseidon/hash.rs:86-96) or one Fr loaded as
 * a native witness (hash_mode 1).  Parameters an op does not use must be 0.  n_in >= 1 (ops 11, 13), at most H2W_CHIPBATCH_MAX_N_IN;
 * 1 <= depth <= 32; cap_height <= min(depth, 6).
 * status_dev[i]: 0, or 4 where an operand word is outside its field (a Goldilocks word >= p, an Fr >= r: the cells are still produced,
 * from the raw value, as h2w_plan_status defines 4) or the leaf index is >= 2^depth (the cells of that instance are unspecified).
 * The chips' assert_equal emits no cells: a Merkle verdict is not part of the stream (h2w_chipbatch_values below gives it, and the op's
 * results; for whole proofs, h2w_fri_verdict_batch).
 * hash_mode 0 and GL_PERMUTE: one wavefront per instance, its permutations' records written by one wavefront per permutation;
 * hash_mode 1 and BN_PERMUTE: four lanes per instance, which emit every permutation's 4,032 cells themselves. */
#define H2W_OP_GL_PERMUTE     9   /* PoseidonPermutationChip::permute           hash/poseidon/permutation.rs:270-284 */
#define H2W_OP_BN_PERMUTE    10   /* PoseidonBN254PermutationChip::permute      hash/poseidon_bn254/permutation.rs:190-203 */
#define H2W_OP_HASH_NO_PAD   11   /* HasherChip::hash_no_pad                    poseidon/hash.rs:161-184, poseidon_bn254/hash.rs:156-179 */
#define H2W_OP_TWO_TO_ONE    12   /* HasherChip::two_to_one                     poseidon/hash.rs:187-214, poseidon_bn254/hash.rs:182-209 */
#define H2W_OP_MERKLE_VERIFY 13   /* MerkleTreeChip::verify_proof_to_cap        merkle/mod.rs:80-102 */
#define H2W_CHIPBATCH_MAX_N_IN 4096   /* largest n_in of HASH_NO_PAD / MERKLE_VERIFY */
h2w_chipbatch *h2w_chipbatch_new_hash(int op, const h2w_poseidon_consts_t *, int hash_mode, uint32_t n_in, uint32_t depth, uint32_t cap_height,
                                      int lookup_bits, int device_id);
/* H2W_CHIPBATCH_OPT_CHUNK: instances per internal launch of a handle made by h2w_chipbatch_new_hash (1 .. 32768; the default keeps the
 * call's internal workspace - records, permutation lists - under a fixed number of bytes). */
#define H2W_CHIPBATCH_OPT_CHUNK 1
int            h2w_chipbatch_configure(h2w_chipbatch *, int option, uint64_t value);
/* The same ops on VALUES (csrc/chipvalues.hip): what the op computed and, for MERKLE_VERIFY, whether the opening holds - without the advice stream.
 * A handle of h2w_chipbatch_new_hash only; a handle of h2w_chipbatch_new is refused.  operands_dev as for h2w_chipbatch_run.
 *   results_dev[n][num_results]   the op's output wires as canonical values:
 *       GL_PERMUTE               12 Goldilocks words (the permuted state)
 *       BN_PERMUTE               16 words: four little-endian Fr, each below r
 *       HASH_NO_PAD, TWO_TO_ONE  4 words: the four Goldilocks words of the hash (hash_mode 0), one little-endian Fr (hash_mode 1)
 *       MERKLE_VERIFY            0 words (results_dev may be null): the computed cap-level node is not handed out by MerkleTreeChip
 *   verdict_dev[n]   status    the word h2w_chipbatch_run stores for the same operands: 0, or 4 from the same item check
 *                    n_failed  chip-level assert_equal / assert_equal_fr calls of the op whose two sides differ, counted as h2w_verdict_t.n_failed
 *                              counts them: the root check of MERKLE_VERIFY is four comparisons with Goldilocks hashes, one with PoseidonBN254; ops 9-12
 *                              hold none (0).  An opening holds iff status == 0 && n_failed == 0.
 * An instance with status 4 has unspecified results and n_failed; it changes no other instance.
 * form: with hash_mode 1 and BN_PERMUTE, which kernel walks the instances - FORM_QUAD four lanes per instance, FORM_ROW one wavefront per instance
 * (a permutation in under half the time on sixteen times the lanes: for few instances); FORM_AUTO is FORM_ROW while n is at most the crossover the
 * library keeps (2,048 instances: measured, a call alone on the chip, on MERKLE_VERIFY at depth 20) and FORM_QUAD beyond it.  With hash_mode 0 and GL_PERMUTE there is one kernel (a wavefront per instance): FORM_QUAD and FORM_AUTO name it, FORM_ROW is
 * refused.  The words stored do not depend on the form, on lookup_bits or on any option.
 * Stream-ordered, no synchronisation, no device allocation: the kernels keep no records and no lists, so the call has no workspace and runs its n
 * instances as ONE launch - H2W_CHIPBATCH_OPT_CHUNK is not looked at.  n == 0: 0.  n above 2^26: -1 ("batch too large").
 * -1 before any device work, the reason in h2w_last_error(): a null handle, a handle of h2w_chipbatch_new, a form above FORM_ROW, FORM_ROW without
 * PoseidonBN254, a null operands_dev / verdict_dev (results_dev: null only where num_results is 0).  Without a device: -1 ("no HIP device"). */
typedef struct { uint32_t status, n_failed; } h2w_chipbatch_verdict_t;   /* 8 bytes */
uint64_t       h2w_chipbatch_num_results(const h2w_chipbatch *);   /* u64 words per instance of results_dev; needs no device (0 and an error for a handle of h2w_chipbatch_new) */
#define H2W_CHIPBATCH_FORM_AUTO 0
#define H2W_CHIPBATCH_FORM_QUAD 1   /* hash_mode 1: four lanes per instance;  hash_mode 0: its one kernel */
#define H2W_CHIPBATCH_FORM_ROW  2   /* hash_mode 1 / BN_PERMUTE only: one wavefront per instance (rowfr.h / rowperm.h) */
int            h2w_chipbatch_values(h2w_chipbatch *, const uint64_t *operands_dev, uint64_t n,
                                    uint64_t *results_dev, h2w_chipbatch_verdict_t *verdict_dev,
                                    unsigned form, void *stream);

/* ------------------------------------------------------------------ 2e. Merkle trees on the device: build, caps and openings
 * The producer side of H2W_OP_MERKLE_VERIFY (csrc/merkletree.hip): plonky2's MerkleTree::new(leaves, cap_height) and tree.prove(i) in both hash
 * modes, so that the reference's own chip test (merkle/mod.rs:137-230: build a tree, open a leaf, verify_proof_to_cap) runs on the device end to end.
 *   leaf digest   hash_or_noop(leaf): hash_mode 0 copies up to four words (zero-padded) and hashes longer leaves with the Goldilocks sponge at rate 8;
 *                 hash_mode 1 copies up to three words as the limbs of one Fr and hashes longer leaves nine words a PoseidonBN254 permutation
 *                 (three Fr of three words each)
 *   inner node    two_to_one(left, right); a hash is four words in both modes
 *   levels        0 (the 2^depth leaf digests) .. depth - cap_height (the cap, 2^cap_height hashes); nothing above the cap is computed
 *   hash store    one tree = tree_words = 4 (2^(depth+1) - 2^cap_height) u64 words, the levels from the leaves upward: level l starts at word
 *                 4 (2^(depth+1) - 2^(depth-l+1)), node i of it at 4 i behind that; the cap is the last 4 2^cap_height words.  The layout is public:
 *                 a caller reads caps and nodes out of trees_dev without a further call
 *   opening row   leaf[n_in], leaf_index, cap[2^cap_height][4], siblings[depth - cap_height][4], sibling j = node (index >> j) ^ 1 of level j:
 *                 the operand words of a MERKLE_VERIFY instance (2c), num_operands = h2w_chipbatch_num_operands of such a handle with the same
 *                 parameters - the rows of h2w_merkle_open go into h2w_chipbatch_run / h2w_chipbatch_values as they are
 * Limits: 1 <= n_in <= H2W_CHIPBATCH_MAX_N_IN, 1 <= depth <= 24 (the prover's LDE bound), cap_height <= min(depth, 6), hash_mode 0 or 1 - every tree
 * that can be built can be verified by the chip.  h2w_merkle_new names the reason of a refusal before it looks for a device; without a device it
 * returns a handle whose layout queries work and whose compute calls fail ("no HIP device").  The handle carries its device like every other.
 * h2w_merkle_layout: out[0] = n_levels = depth - cap_height + 1, out[1 .. n_levels] = the word offset of levels 0 .. n_levels - 1, then the cap's
 * word offset (the last level's), then num_operands of an opening row.  Returns the number of words (n_levels + 3); out == NULL: that number alone;
 * n_out below it: -1.
 * h2w_merkle_build: leaves_dev [n_trees][2^depth][n_in] canonical Goldilocks words -> trees_dev [n_trees][tree_words].  status_dev[t] = 0, or 4
 * when a leaf word of tree t is >= p (that tree's hashes are then unspecified; no other tree changes).
 * h2w_merkle_open: queries_dev [n][2] = {tree, leaf index} -> operands_dev [n][num_operands], from the leaves and the trees of a build.
 * status_dev[i] = 0, or 4 when the tree index is >= n_trees or the leaf index >= 2^depth (that row is then unspecified: it is not written).
 * Both calls are stream-ordered, synchronise nothing, allocate nothing on the device and touch nothing outside the caller's buffers.  n_trees == 0
 * and n == 0: 0.  A call of more than 2^30 leaves in all, more than 65,535 trees or more than 2^26 queries: -1 ("batch too large").
 * H2W_MERKLE_OPT_CROWN_BITS: the levels of at most 2^value nodes per tree (the crown; the leaf digests aside, which are always the leaf kernel's)
 * are built by one wavefront per node - the wavefront-cooperative permutations of the values calls, four levels a launch, handed over inside a
 * workgroup through LDS - instead of one lane per node and one launch per level.  value: 0 .. depth, H2W_MERKLE_CROWN_NONE (every level one lane per
 * node) or H2W_MERKLE_CROWN_AUTO (the default): the largest value with n_trees x 2^value at most the crossover the library keeps per hash mode.
 * The crossover: 16,384 nodes with hash_mode 0, 8,192 with hash_mode 1 - measured, a call alone on the chip: the build time falls with every level the
 * crown takes up to these counts and rises beyond them, at depth 12, 16 and 20, leaves of 5 and 20 words, 1, 8 and 64 trees (tools/bench_merkle.py
 * --crossover, profiles/merkle_tree_forms.jsonl).  A caller that keeps other launches in flight names its value itself.
 * h2w_merkle_crown_bits reports what a build of n_trees trees runs with: 0 .. depth or H2W_MERKLE_CROWN_NONE; no device needed.  The words stored do
 * not depend on the option. */
typedef struct h2w_merkle h2w_merkle;
#define H2W_MERKLE_OPT_CROWN_BITS 1
#define H2W_MERKLE_CROWN_NONE 254
#define H2W_MERKLE_CROWN_AUTO 255
h2w_merkle *h2w_merkle_new(const h2w_poseidon_consts_t *, int hash_mode, uint32_t n_in, uint32_t depth, uint32_t cap_height, int device_id);
void        h2w_merkle_free(h2w_merkle *);
uint64_t    h2w_merkle_tree_words(const h2w_merkle *);      /* u64 words of one tree's hash store */
int         h2w_merkle_layout(const h2w_merkle *, uint64_t *out, size_t n_out);
int         h2w_merkle_build(h2w_merkle *, const uint64_t *leaves_dev, uint64_t n_trees, uint64_t *trees_dev, uint32_t *status_dev, void *stream);
int         h2w_merkle_open(h2w_merkle *, const uint64_t *leaves_dev, const uint64_t *trees_dev, uint64_t n_trees,
                            const uint64_t *queries_dev, uint64_t n, uint64_t *operands_dev, uint32_t *status_dev, void *stream);
int         h2w_merkle_configure(h2w_merkle *, int option, uint64_t value);
int         h2w_merkle_crown_bits(const h2w_merkle *, uint64_t n_trees);

/* ------------------------------------------------------------------ the step BEFORE the path
 * Synthetic VALID FRI instances generated on the GPU (SURVEY 8(d) variant (A)): low-degree extension (Goldilocks NTT on the coset
 * 7<w>), Merkle commitments with the selected hash, the starky / plonky2 Fiat-Shamir transcript (stark/mod.rs:167-222 order, as
 * ChallengerChip replays it: challenger/mod.rs:168-222), openings at zeta and g*zeta, the alpha-batched quotient, the FRI commit
 * phase (arity 2^arity_bits coefficient folding), proof-of-work grinding and the query openings - written in the flat proof layout
 * h2w_fri_witness_batch consumes, so proofs never visit the host.  The reference obtains such proofs from starky's
 * prover (stark/mod.rs:405-426, test_util/fibonacci_stark.rs); as there, the committed polynomials are inputs: the STARK constraint
 * identity is not part of the verifier gadget (stark/mod.rs:243-321 is commented out), any polynomials of degree < 2^degree_bits do.
 * The serial sponge runs on the host between device phases (a few dozen permutations per proof).
 * h2w_prover_new accepts the shapes h2w_plan_compile accepts, with degree_bits + rate_bits in [1, 24] and n_pis <= 64; it refuses any
 * other with "unsupported shape: <reason>" before it looks for a device.  That is stricter than its own earlier check: num_queries in
 * [1, 128] (was up to 4096), a final polynomial of at most 128 coefficients (was 2048), lookup_bits in [2, 28], hash_mode 0 or 1,
 * cap_height in [0, 6], pow_bits <= 63, at most 8 fold steps - what the witness generator takes, so every proof made can be witnessed.
 * The handle carries its device like every other: device_id must be below h2w_device_count() ("device_id out of range" otherwise), and
 * h2w_prover_new, h2w_prove_fri(_batch) and h2w_prover_free make it current for their own duration only. */
typedef struct h2w_prover h2w_prover;
h2w_prover *h2w_prover_new(const h2w_shape_t *, const h2w_poseidon_consts_t *, int device_id);
void        h2w_prover_free(h2w_prover *);
uint64_t    h2w_prover_num_polys(const h2w_prover *);      /* n_cols + n_perm_z + n_quotient */
uint64_t    h2w_prover_proof_words(const h2w_prover *);    /* = h2w_plan_proof_words of the same shape */
/* coeffs_dev: [num_polys][2^degree_bits] canonical Goldilocks coefficients (trace columns, permutation Zs, quotient polynomials), device.
 * public_inputs: n_pis words, host.  proof_dev: proof_words u64, device.  Synchronises `stream` several times (transcript). */
int h2w_prove_fri(h2w_prover *, const uint64_t *coeffs_dev, const uint64_t *public_inputs, uint64_t *proof_dev, void *stream);
/* n_proofs (<= 2048) instances in lockstep: coeffs_dev [n_proofs][num_polys][2^degree_bits], public_inputs [n_proofs][n_pis] (host),
 * proofs_dev [n_proofs][proof_words].  Every kernel covers the whole batch and the host transcript serves all proofs at each of its
 * round trips, so the latency-bound pieces (upper tree levels, small fold steps) are paid once per batch.  Device scratch is
 * (re)allocated inside the handle for the largest batch seen (cfg 3: about 0.65 GB per proof). */
int h2w_prove_fri_batch(h2w_prover *, const uint64_t *coeffs_dev, const uint64_t *public_inputs, uint64_t *proofs_dev, uint64_t n_proofs, void *stream);
/* ms[0] = LDE (NTTs), ms[1] = Merkle commitments of the oracles, ms[2] = openings + batched quotient, ms[3] = FRI commit phase,
 * ms[4] = proof of work, ms[5] = query openings, ms[6] = whole call (wall clock incl. the host transcript) of the last h2w_prove_fri / h2w_prove_fri_batch */
int h2w_prover_timing(h2w_prover *, float ms[7]);

#ifdef __cplusplus
}
#endif
#endif
