// replay_lane.h — the interpreter of a traced plan: the body of the kernels k_replay<BN> and k_replay_parts<BN> (replay.hip), which include this text
// between their braces with H2W_REPLAY_PARTS defined as 0 or 1 - no include guard, nothing of its own to include.  R: the kernel's argument, ReplayArgsT<BN>.
// What stands under H2W_REPLAY_PARTS is the whole difference between the two kernels.
    const uint32_t lane = threadIdx.x;
    if (lane < T_MAX) s_nc[lane] = R.ncells[lane];
    if (lane == 0) { s_cx.gvals = R.vals; s_cx.tm = R.tm; s_cx.prefix = R.prefix; s_cx.imps = R.imps; s_cx.inputs = R.inputs; s_cx.pool64 = R.pool64; s_cx.poolfr = R.poolfr; s_cx.nproofs = R.nproofs; }
    for (uint32_t i = lane; i < R.npool64 && i < POOL64_CAP; i += 64) s_lds[LDS_POOL64 / 8 + i] = g_load_u64(R.pool64 + i);
    for (uint32_t i = lane; i < 4 * R.npoolfr && i < 4 * POOLFR_CAP; i += 64) s_lds[LDS_POOLFR / 8 + i] = g_load_u64(reinterpret_cast<const uint64_t *>(R.poolfr) + i);
    __syncthreads();
    // which template this block runs (the templates of one depth share a launch: they do not depend on one another)
    uint32_t t = 0;
#pragma unroll 1
    for (uint32_t i = 0; i < R.ntmpl; i++) if (R.tm[i].depth == R.depth && blockIdx.x >= R.blk0[i]) t = i;
    // (a value loaded from global memory is "divergent" to the compiler even at a uniform address: without the readfirstlane the tape pointer is a
    //  vector register, every tape word a VECTOR load - behind the record stores in flight, 2.5 us per op - and every branch of the interpreter a lane mask)
    t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
    const TmplD T = R.tm[t];
    const uint32_t ninst = (uint32_t)__builtin_amdgcn_readfirstlane((int)T.ninst), tape0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)T.tape0), inst0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)T.inst0);
    const uint32_t gl = (blockIdx.x - R.blk0[t]) * 64 + lane;
    uint32_t g, emit = 1u;      // g = p * ninst + inst: the lane's place in the value store
    if (R.lanes) {              // sharded: the lanes this rank owns; bit 31: a root lane of a proof it does not own; NO_SLOT: padding
        const uint32_t base = R.lane0[t];
        if (gl >= R.lane0[t + 1] - base) return;
        const uint32_t e = R.lanes[base + gl];
        if (e == NO_SLOT) return;
        g = e & 0x7fffffffu; emit = (uint32_t)__builtin_amdgcn_readfirstlane((int)((e >> 31) ^ 1u));
    } else { g = gl; if (g >= R.nproofs * ninst) return; }
    const uint32_t p = g / ninst, inst = g % ninst;
    const InstD *const I = R.insts + inst0 + inst;
    const uint32_t imp0 = I->imp0, in0 = I->in0, glp0 = I->glp0;
    [[maybe_unused]] uint32_t bnp0 = 0; if constexpr (BN) bnp0 = R.bnp0[inst0 + inst];
    fr_t *outb = R.out + (uint64_t)p * R.cell_stride;
    if (R.sh_compact) {         // the packed buffer: the lane's block (the root's: the prologue block) at its local start, its cells at their global offsets
        // (shardmap.h packed_block_start, written out: the call moves the interpreter loop below by three instructions, and the root lane of an unfused plan measured 1.5 % slower: profiles/replay_split_bench.json.  The packed tests hold this copy to h2w_plan_shard_block, which calls the function)
        const uint64_t W = R.sh_world, r = R.sh_rank, u0 = (uint64_t)p * R.nq, unit = I->unit;
        const uint64_t units_before = (u0 + W - 1 - r) / W;
        uint64_t local = (((uint64_t)p + W - 1 - r) / W) * R.pro_ncell + units_before * R.q_slot;
        if (unit != NO_SLOT) local += ((uint64_t)p % W == r ? R.pro_ncell : 0) + ((u0 + unit + W - 1 - r) / W - units_before) * R.q_slot;
        outb = R.out + local - I->ucell0;
    }
    ReplaySink sink; sink.recs = R.recs + (uint64_t)p * R.rec_stride; sink.out = outb; sink.ncells = s_nc; sink.cc.init(R.cm); sink.emit = emit;
    sink.nrec = I->rec0; sink.cell_off = I->cell0;
    ValCfg cfg; cfg.proof = R.proofs + (uint64_t)p * R.proof_words; cfg.mode = 1; cfg.L = R.L; cfg.P = R.P; cfg.inv_pos = R.inv_pos; cfg.inv_neg = R.inv_neg; cfg.st = nullptr;
    cfg.split = false; cfg.split_bn = false; cfg.load_items = nullptr; cfg.n_load_items = 0; cfg.load_nrec = cfg.load_ncell = 0; cfg.n_cap_items = 0; cfg.fri = nullptr;
    RB be(sink, cfg, true);
    const uint64_t Lt = (uint64_t)R.nproofs * ninst;
    const uint64_t pre = R.prefix[t];
    uint64_t *const vals_g = R.vals + (uint64_t)R.nproofs * (((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(pre >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)pre)) + g;
    const uint64_t *const proof = cfg.proof; const uint32_t *const tape = R.tape;
    const uint32_t lane8 = lane * 8;
    const char *const lds = reinterpret_cast<const char *>(s_lds);
    // word j of an operand: the ring or a pool entry, both in LDS, no branch (the ref says which: fastref_*)
    auto get64 = [&](uint32_t r, uint32_t j) -> uint64_t {
        const bool ring = (r >> 31) != 0;
        const uint32_t off = ring ? (((r + j) & (RING_K - 1)) << 9) : ((r & 0x3ffffu) + (j << 3));
        return *reinterpret_cast<const uint64_t *>(lds + off + (ring ? lane8 : 0u));
    };
    auto getfr = [&](uint32_t r) -> fr_t {
        const uint32_t w = (r >> 27) & 3u;      // W64, W128, WFR
        const uint64_t a = get64(r, 0), b = w != W64 ? get64(r, 1) : 0, c = w == WFR ? get64(r, 2) : 0, d = w == WFR ? get64(r, 3) : 0;
        fr_t v; v.l[0] = a; v.l[1] = b; v.l[2] = c; v.l[3] = d; return v;
    };
    auto ring_put = [&](uint32_t slot, uint64_t v) { s_lds[(slot & (RING_K - 1)) * 64 + lane] = v; };
    auto st1 = [&](uint32_t slot, uint64_t v) { ring_put(slot, v); H2W_GSTORE64(vals_g + (uint64_t)slot * Lt, v); };
    auto put64 = [&](uint32_t slot, uint64_t v) { if (slot != NO_SLOT) st1(slot, v); };
    auto putfr = [&](uint32_t slot, const fr_t &v) { if (slot != NO_SLOT) { st1(slot, v.l[0]); st1(slot + 1, v.l[1]); st1(slot + 2, v.l[2]); st1(slot + 3, v.l[3]); } };
    uint64_t ta[64], tb[64];
    bool bad_word = false;
#if H2W_REPLAY_PARTS
    fr_t carry = fr_zero();      // the running sum of a split select between a "continued" part and the "continues" part behind it: registers (the kernel's LDS is taken)
#endif
    // The op at pc sits in eight scalar registers (a window of the tape); the window of the NEXT op is requested before this one runs: a scalar load
    // waited for where it is used was ~200 cycles, five times per op.  (Ops with operand lists read the words beyond the window themselves.)
    uint32_t pc = tape0;
    uint32_t w0 = tw(tape, pc), w1 = tw(tape, pc + 1u), w2 = tw(tape, pc + 2u), w3 = tw(tape, pc + 3u), w4 = tw(tape, pc + 4u);
#pragma unroll 1
    for (;;) {
        const uint32_t h = w0; const uint32_t op = h & 0xff, n = (h >> 8) & 0xff, aux = (h >> 16) & 0xff;
        if (op == DOP_END) break;
        const uint32_t pcn = pc + (op == DOP_GLOPRUN ? 2u + 4u * n : (h >> 24));
        const uint32_t n0 = tw(tape, pcn), n1 = tw(tape, pcn + 1), n2 = tw(tape, pcn + 2), n3 = tw(tape, pcn + 3), n4 = tw(tape, pcn + 4);
        if constexpr (BN) {
            if (op == DOP_BNPERM) {     // (in front of the switch: the instantiation without it keeps its code)  The lane keeps the VALUES of the permutation (bnpval.h); its cells are k_bn_emit_traced's, from the listed input state
                fr_t st[BN_WIDTH];
                st[0] = getfr(w1); st[1] = getfr(w2); st[2] = getfr(w3); st[3] = getfr(w4);
                const uint32_t o = tw(tape, pc + 5), ls = tw(tape, pc + 6), nc = tw(tape, pc + 7);
                if (sink.emit) {
                    uint64_t *e = R.blist + ((uint64_t)p * R.nbnp + bnp0 + ls) * BNP_LIST_WORDS;
                    H2W_GSTORE64(e, sink.cell_off); H2W_GSTORE64(e + 1, 1ull);
#pragma unroll
                    for (int i = 0; i < BN_WIDTH; i++) { H2W_GSTORE64(e + 2 + 4 * i, st[i].l[0]); H2W_GSTORE64(e + 3 + 4 * i, st[i].l[1]); H2W_GSTORE64(e + 4 + 4 * i, st[i].l[2]); H2W_GSTORE64(e + 5 + 4 * i, st[i].l[3]); }
                }
                const unsigned long long *const bk = reinterpret_cast<const unsigned long long *>(R.bnk);
                bn_permute_values(st, R.P, [&](int i) -> fr_t { fr_t v; v.l[0] = H2W_CLOAD64(bk + 4 * i); v.l[1] = H2W_CLOAD64(bk + 4 * i + 1); v.l[2] = H2W_CLOAD64(bk + 4 * i + 2); v.l[3] = H2W_CLOAD64(bk + 4 * i + 3); return v; });
                putfr(o, st[0]); putfr(o + 4, st[1]); putfr(o + 8, st[2]); putfr(o + 12, st[3]);
                sink.skip(0, nc);
                pc = pcn; w0 = n0; w1 = n1; w2 = n2; w3 = n3; w4 = n4;
                continue;
            }
        }
#if H2W_REPLAY_PARTS
        if (op == DOP_FR_SELIND && aux != 0) {      // (in front of the switch, as DOP_BNPERM)  A part of a split select (tapefmt.h SELIND_*): the cells of its entries, where the
            // whole op puts them - the zero cell with the first part, a gate before every sum cell but the select's last.  The sum arrives from and leaves to the neighbouring
            // part in `carry`: only DOP_FETCH ops run in between, which touch the ring alone.  The result (the last part's: the others carry NO_SLOT) is stored behind the last read.
            fr_t sum = carry; uint64_t any = 0;
            if (!(aux & SELIND_CONTINUES)) { sum = fr_zero(); be.G(); be.cell64(0); }
            for (uint32_t i = 0; i < n; i++) { const fr_t a = getfr(tw(tape, pc + 1 + i)); const uint64_t ind = get64(tw(tape, pc + 1 + n + i), 0); any |= ind; if (ind) sum = h2w::fr_add(sum, a); be.cell(a); be.cell64(ind); if (i + 1 < n || (aux & SELIND_CONTINUED)) be.G(); be.cell(sum); }
            if (any > 1) be.fail(5);      // an indicator that is no bit, in this part (status 5, below)
            carry = sum; putfr(tw(tape, pc + 1 + 2 * n), sum);
            pc = pcn; w0 = n0; w1 = n1; w2 = n2; w3 = n3; w4 = n4;
            continue;
        }
#endif
        // Every case reads ALL its operands (into registers, ta / tb) before its first st1 / putfr: the lowering lets an op's result slots alias the ring
        // slots of its fetched operands (tracelower.cpp bounds the fetched slots alone by RING_K; tape_check the same).  A case that stores before its last read breaks that.
        // Status 5 (include/h2w.h 2d): an operand outside the domain its op was lowered for - a selector, an indicator or a bit above 1, a second indicator set
        // where the sum is kept in one word, 2^128 or more in front of a reduce.  The eager call of proof A did the field's arithmetic on such a value or refused
        // it; the templates of the value backend (shared with the compiled plan's kernels, where these are bits by construction) do neither.  Decided on the
        // operand, once per op (the words ORed), whether or not the result happens to come out right; the op's cells are written as before and are unspecified.
        switch (op) {
            case DOP_SKIP: { const uint64_t nr = ((uint64_t)w2 << 32) | w1, nc = ((uint64_t)w4 << 32) | w3; sink.skip(nr, nc); break; }
            case DOP_CONST1: { const uint64_t v = get64(w1, 0); sink.rec(T_CONST1, v, 0, 0, 0); put64(w2, v); break; }
            case DOP_FRCELL: { const fr_t v = getfr(w1); be.cell(v); putfr(w2, v); break; }
            case DOP_LOADW: { const uint64_t v = get64(w1, 0); sink.rec(T_LOADW, v, 0, 0, 0); put64(w2, v); break; }
            case DOP_LOADW_DIV: {      // the hint of GoldilocksChip::div (base.rs:371-393): a / b; b == 0: status 1, the cells of the op on 1
                const uint64_t a = get64(w1, 0); uint64_t b = get64(w2, 0);
                if (b == 0) { be.fail(1); b = 1; }
                const uint64_t v = gl_mul(a, gl_inv(b)); sink.rec(T_LOADW, v, 0, 0, 0); put64(w3, v); break;
            }
            case DOP_LOADW_EXTINV: {   // extension.rs:320-340
                gle_t a; a.c[0] = get64(w1, 0); a.c[1] = get64(w2, 0);
                if (a.c[0] == 0 && a.c[1] == 0) { be.fail(2); a.c[0] = 1; }
                const gle_t iv = gle_inv(a); const uint64_t v = (aux & 1) ? iv.c[1] : iv.c[0]; sink.rec(T_LOADW, v, 0, 0, 0); put64(w3, v); break;
            }
            case DOP_GLOP: { const uint64_t A = get64(w1, 0), B = get64(w2, 0), C = get64(w3, 0); sink.rec((int)aux, A, B, C, 0); put64(w4, gl_reduce128((u128)A * B + C)); break; }
            case DOP_GATE: { const uint64_t A = get64(w1, 0), B = get64(w2, 0), C = get64(w3, 0); sink.rec((int)aux, A, B, C, 0);
                             const u128 v = (u128)A * B + C; const uint32_t o = w4; if (o != NO_SLOT) { st1(o, (uint64_t)v); st1(o + 1, (uint64_t)(v >> 64)); } break; }
            case DOP_REDUCE: { const uint32_t r = w1; const uint64_t lo = get64(r, 0), hi = get64(r, 1);
                               if (((r >> 27) & 3u) == WFR && (get64(r, 2) | get64(r, 3)) != 0) be.fail(5);      // a four-slot operand (mul_sub: a b + c (p - 1)): beyond the range of GoldilocksChip::reduce, where h2w_gl_reduce fails
                               sink.rec(T_REDUCE, lo, hi, 0, 0); put64(w2, gl_reduce128(((u128)hi << 64) | lo)); break; }
            case DOP_CLT: { sink.rec(T_CLT_SAFE, get64(w1, 0), 0, 0, 0); break; }
            case DOP_FR_ADD: { const fr_t v = be.fr_add(getfr(w1), getfr(w2)); putfr(w3, v); break; }
            case DOP_FR_MUL: { const fr_t v = be.fr_mul(getfr(w1), getfr(w2)); putfr(w3, v); break; }
            case DOP_FR_MULADD: { const fr_t v = be.fr_mul_add(getfr(w1), getfr(w2), getfr(w3)); putfr(w4, v); break; }
            case DOP_SELECT: { const uint64_t sel = get64(w3, 0); if (sel > 1) be.fail(5); const uint64_t v = be.select(get64(w1, 0), get64(w2, 0), sel); put64(w4, v); break; }
            case DOP_FR_SELECT: { const uint64_t sel = get64(w3, 0); if (sel > 1) be.fail(5); const fr_t v = be.fr_select(getfr(w1), getfr(w2), sel); putfr(w4, v); break; }
            case DOP_IDX2IND: { be.idx_to_indicator(get64(w1, 0), (int)n, ta); const uint32_t o = w2; for (uint32_t i = 0; i < n; i++) st1(o + i, ta[i]); break; }
            case DOP_SELIND: { uint64_t any = 0, set = 0;      // (set: exact while every indicator is a bit; two entries of one word need not sum to one word)
                               for (uint32_t i = 0; i < n; i++) { ta[i] = get64(tw(tape, pc + 1 + i), 0); tb[i] = get64(tw(tape, pc + 1 + n + i), 0); any |= tb[i]; set += tb[i]; }
                               if ((any | set) > 1) be.fail(5);
                               put64(tw(tape, pc + 1 + 2 * n), be.select_by_indicator(ta, 1, tb, (int)n)); break; }
            case DOP_FR_SELIND: {      // GateChip::select_by_indicator on native values: [0, a0, ind0, s0, a1, ind1, s1, ...] (gates at 3 i)
                fr_t sum = fr_zero(); uint64_t any = 0; if (n > 0) be.G(); be.cell64(0);
                for (uint32_t i = 0; i < n; i++) { const fr_t a = getfr(tw(tape, pc + 1 + i)); const uint64_t ind = get64(tw(tape, pc + 1 + n + i), 0); any |= ind; if (ind) sum = h2w::fr_add(sum, a); be.cell(a); be.cell64(ind); if (i + 1 < n) be.G(); be.cell(sum); }
                if (any > 1) be.fail(5);
                putfr(tw(tape, pc + 1 + 2 * n), sum); break;
            }
            case DOP_NUM2BITS: { be.num_to_bits(get64(w1, 0), (int)n, ta); const uint32_t o = w2; for (uint32_t i = 0; i < n; i++) st1(o + i, ta[i]); break; }
            case DOP_BITS2NUM: { uint64_t any = 0; for (uint32_t i = 0; i < n; i++) { ta[i] = get64(tw(tape, pc + 1 + i), 0); any |= ta[i]; } if (any > 1) be.fail(5); put64(tw(tape, pc + 1 + n), be.bits_to_num(ta, (int)n)); break; }
            case DOP_DECOMP565: { be.decompose_le_56_5(getfr(w1), ta); const uint32_t o = w2; for (int i = 0; i < 5; i++) st1(o + i, ta[i]); break; }
            case DOP_LIMBS2NUM: { for (uint32_t i = 0; i < n; i++) ta[i] = get64(tw(tape, pc + 1 + i), 0); putfr(tw(tape, pc + 1 + n), n == 4 ? be.limbs_to_num4(ta) : be.limbs_to_num(ta, (int)n)); break; }
            case DOP_RANGE: { be.range_check(get64(w1, 0), (int)aux); break; }
            case DOP_GLOPRUN: {      // the Goldilocks-level ops of a gadget come in runs (a Poseidon round: hash/poseidon/permutation.rs:43-239): no dispatch between them, the next op's words requested before this one is computed
                uint32_t q = pc + 2; uint32_t a = w2, b = w3, c = w4, o = tw(tape, pc + 5);
                rec_t *rp = sink.recs + sink.nrec;      // (the cell cursor is only needed by direct cells: it moves by the run's total, from the tape, once)
#pragma unroll 1
                for (uint32_t i = 0; i < n; i++) {
                    q += 4;
                    const uint32_t na = tw(tape, q), nb = tw(tape, q + 1), nc = tw(tape, q + 2), no = tw(tape, q + 3);      // (past the last op: the next op's first words, unused)
                    const uint64_t A = get64(a, 0), B = get64(b, 0), C = get64(c, 0);
                    if (sink.emit) g_store_rec(rp, A, B, C, 0);
                    rp++; st1(o & 0xffffffu, gl_reduce128((u128)A * B + C));
                    a = na; b = nb; c = nc; o = no;
                }
                sink.nrec += n; sink.cell_off += w1;
                break;
            }
            case DOP_GLPERM: {     // the lane keeps the VALUES of the permutation; its records are k_glp_emit_traced's, from the listed input state
                uint64_t st[SPONGE_WIDTH];
#pragma unroll
                for (uint32_t i = 0; i < (uint32_t)SPONGE_WIDTH; i++) st[i] = get64(tw(tape, pc + 1 + i), 0);
                const uint32_t o = tw(tape, pc + 13), ls = tw(tape, pc + 14), nc = tw(tape, pc + 15);
                if (sink.emit) {
                    uint64_t *e = R.glist + ((uint64_t)p * R.nglp + glp0 + ls) * GLP_LIST_WORDS;
                    H2W_GSTORE64(e, sink.nrec);
#pragma unroll
                    for (int i = 0; i < SPONGE_WIDTH; i++) H2W_GSTORE64(e + 1 + i, st[i]);
                }
                const uint64_t *const glk = R.glk;
                glp_permute_values(st, [&](int i) -> uint64_t { return H2W_CLOAD64(glk + i); });
#pragma unroll
                for (uint32_t i = 0; i < (uint32_t)SPONGE_WIDTH; i++) st1(o + i, st[i]);
                sink.skip(GLP_RECS, nc);
                break;
            }
            case DOP_FETCH: {      // a far operand into the ring (no write-through: a copy)
                bool ge = true;        // a proof word (every one enters here): at least the modulus of its field (one word: Goldilocks, four: BN254)?
                for (uint32_t j = 0; j < n; j++) {
                    const uint64_t x = slow_get64(w1, j, vals_g, Lt, p, imp0, in0, proof), m = n == 1 ? GL_P : fr_mod_limb((int)j);
                    ring_put(w2 + j, x); ge = x > m || (x == m && ge);
                }
                if (ref_kind(w1) == RK_INPUT && ge) bad_word = true;      // status 4 (as k_prologue_load); the cells still come from the raw value
                break;
            }
            default: be.fail(99); break;      // (unreachable: the lowering emits nothing else)
        }
        pc = pcn; w0 = n0; w1 = n1; w2 = n2; w3 = n3; w4 = n4;
    }
    if (be.status) atomicCAS(&R.status[p], 0u, be.status);
    if (bad_word) atomicOr(&R.lflag[p], 4u);
