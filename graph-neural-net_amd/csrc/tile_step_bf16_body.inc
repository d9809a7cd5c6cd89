// tile_step_bf16_body.inc -- the body of tile_step_bf16_kernel (tile_step_kernel.h), included INSIDE the kernels that run it:
// the single-net kernel and its grouped twin (group_kernels.h).  In scope: the kernel argument `p` (TileStepParams),
// the template parameters GSRC / GDST / FWD, TS_HEAD_PROLOGUE / TS_HEAD (tile_step_kernel.h), and nine macros that say who the kernel works for:
// TS_BID (the workgroup's index in the tile map), TS_REL(ptr) (the net's copy of a pointer of `p`), TS_REL_LAYER(L) (the same
// for a layer descriptor), TS_STEP_OVER_B and TS_MOMENTUM, and the four row counts TS_K / TS_K_TRUE (the current batch, padded /
// live) and TS_NEXT_K / TS_NEXT_ROWS (the next one).  The single-net kernels define them as the plain expressions
// they replace (tile_step_kernel.h), the grouped twins as member k's (group_kernels.h): block-uniform either way.  Text the kernels include, not a function
// they call, so that the single-net kernels read `p` straight from their argument segment and compile to exactly the code
// they had before the grouped twins existed.
    constexpr int LDA = TS_TM + 16;  // [k][m] bf16 image: 160-B rows (32*odd)
    constexpr int LDD = TS_TN;       // [k][n] bf16 image: 32-B rows
    __shared__ __attribute__((aligned(16))) __bf16 sA[TS_KC * LDA];
    __shared__ __attribute__((aligned(16))) __bf16 sD[TS_KC * LDD];
    __shared__ __attribute__((aligned(16))) __bf16 sW[TS_TM * TS_TN]; // the tile's (new) weights [m][n], 32-B rows
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int fr = lane & 15, fg = lane >> 4;

    // by value: one batch of scalar loads, not one round trip per field as it is first used; layer 0's descriptor (nine of
    // ten workgroups) is requested at once, beside the map entry that names the tile, not behind it
    int li, tm, tn;
    GradLayer L = p.layer[0];
#if TS_HEAD_PROLOGUE
    // (as in tile_step_body.inc: a regular slot takes its tile from the workgroup's id and its first loads' addresses from the
    //  preloaded head arguments; the first two pointer slots carry the bf16 A and D of layer 0)
    const bool regular = TS_HEAD && ts_head_tile(hd_geo, hd_kx, (int)TS_BID, tm, tn); // (block-uniform)
    if (regular) {
        li = 0;
        L.W = hd_W; L.V = hd_V; L.lda = hd_lda; L.ldd = hd_ldd; L.M = hd_M;
    } else
#endif
    if (p.map_in_args) {
        const uint32_t w = p.map_words[TS_BID >> 1], e = (TS_BID & 1) ? w >> 16 : w & 0xffffu;
        if (e == 0xffffu) return;
        li = (int)(e & 7u); tm = (int)((e >> 3) & 63u); tn = (int)(e >> 9);
    } else {
        const uint32_t e = p.tile_map[TS_BID];
        if (e == ~0u) return;
        li = (int)(e & 15u); tm = (int)((e >> 4) & 0x3fffu); tn = (int)(e >> 18);
    }
    if (li != 0) L = p.layer[li];
    TS_REL_LAYER(L);
    const int m0 = tm * TS_TM, n0 = tn * TS_TN;
    const bool fwd = FWD && li == 0;
#if TS_HEAD_PROLOGUE
    const __bf16 *Ab = regular ? reinterpret_cast<const __bf16 *>(hd_A) : p.Ab[li], *Db = regular ? reinterpret_cast<const __bf16 *>(hd_D) : p.Db[li];
#else
    const __bf16 *Ab = TS_REL(p.Ab[li]), *Db = TS_REL(p.Db[li]);
#endif
    const int stage_cols = (TS_STAGE_N / TS_TN) < 8 ? (TS_STAGE_N / TS_TN) : 8; // tile columns that share the staging copy's 16-row groups (read with fwd only: layer 0)

    const int er = (t >> 6) * 16 + fr, eq = fg; // (as in tile_step_kernel: the accumulator layout of the transposed product)
    const bool e_ok = t < 256 && (m0 + er < L.M);
    const size_t e_off = (size_t)(m0 + er) * L.ldd + n0 + eq * 4;

    // ---- loads: gradient operands of the first K chunk, the tile's masters, then the next batch's rows ----
    bf16x8 va[2], vd;
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    auto load_grad = [&](int k0, int kc) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int idx = t + i * TS_THREADS, k = idx >> 3, q = idx & 7; // 8 chunks of 8 bf16 per row
            va[i] = zero8;
            if (k < kc && m0 + q * 8 < L.M) {
                size_t a_row = (size_t)(k0 + k);
                bool live = true;
                if (li == 0 && TS_HAS_ROW_IDX) { live = k0 + k < TS_K_TRUE; a_row = live ? (size_t)TS_REL(p.row_idx)[k0 + k] : 0; }
                if (live) va[i] = *reinterpret_cast<const bf16x8 *>(Ab + a_row * L.lda + m0 + q * 8);
            }
        }
        vd = zero8;
        if (t < 256) {
            const int k = t >> 1, q = t & 1;
            if (k < kc) vd = *reinterpret_cast<const bf16x8 *>(Db + (size_t)(k0 + k) * L.ldd + n0 + q * 8);
        }
    };
    const int kc0 = (TS_K < TS_KC) ? TS_K : TS_KC;
    if (GSRC == 1) load_grad(0, kc0);
    float4 w_old = make_float4(0.f, 0.f, 0.f, 0.f), v_old = w_old, g_in = w_old;
    if (e_ok) {
        if (GDST == 2 || FWD) w_old = *reinterpret_cast<const float4 *>(L.W + e_off);
        if (GDST == 2) v_old = *reinterpret_cast<const float4 *>(L.V + e_off);
    }
    if (GSRC >= 2) g_in = ts_gradient_in<GSRC>(p, L, e_off, e_ok);
    // next batch: lane (fr, fg) of wave w -> row 16w + fr; per 32-wide k block the inputs 4fg..4fg+3 and 16+4fg..+3
    s16x4 vn[2][2];
    int next_row0 = wave * 16 + fr; // (as in tile_step_kernel: the index of a sampled next batch's row is fetched ahead)
    if (fwd && TS_REL(p.next_idx) && next_row0 < TS_NEXT_ROWS) next_row0 = TS_REL(p.next_idx)[next_row0];
    auto load_next = [&](int b0) {
        const int b = b0 + wave * 16 + fr;
        const bool live = b < TS_NEXT_ROWS;
        const size_t row = live ? (b0 == 0 ? (size_t)next_row0 : TS_REL(p.next_idx) ? (size_t)TS_REL(p.next_idx)[b] : (size_t)b) : 0;
        const __bf16 *src = TS_REL(p.Anb) + row * p.ldan + m0 + 4 * fg;
#pragma unroll
        for (int kb = 0; kb < 2; kb++)
#pragma unroll
            for (int hh = 0; hh < 2; hh++) {
                vn[kb][hh] = (s16x4){0, 0, 0, 0};
                if (live && m0 + kb * 32 + hh * 16 + 4 * fg < L.M) vn[kb][hh] = *reinterpret_cast<const s16x4 *>(src + kb * 32 + hh * 16);
            }
    };
    if (fwd) load_next(0);

    // ---- gradient tile ------------------------------------------------------------------------------
    float4 g = g_in;
    if (GSRC == 1) {
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < TS_K; k0 += TS_KC) {
            const int kc = (TS_K - k0 < TS_KC) ? TS_K - k0 : TS_KC;
            if (k0) { __syncthreads(); load_grad(k0, kc); }
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const int idx = t + i * TS_THREADS, k = idx >> 3, q = idx & 7;
                *reinterpret_cast<bf16x8 *>(&sA[k * LDA + q * 8]) = va[i];
            }
            if (t < 256) *reinterpret_cast<bf16x8 *>(&sD[(t >> 1) * LDD + (t & 1) * 8]) = vd;
            __syncthreads();
            // waves 0..3: G^T[n][m] over the chunk's 32-wide k blocks (rows past kc were staged as zeros)
            if (wave < 4) {
                for (int kk = 0; kk < kc; kk += 64) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(sD, LDD, 0, kk, lane), tr_frag(sA, LDA, wave * 16, kk, lane), acc0, 0, 0, 0);
                    if (kk + 32 < kc)
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(sD, LDD, 0, kk + 32, lane), tr_frag(sA, LDA, wave * 16, kk + 32, lane), acc1, 0, 0, 0);
                }
            }
        }
        const f32x4 acc = acc0 + acc1; // rows n = 4 fg + r, column m = 16 wave + fr
        g = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }

    float4 w_new = w_old;
    if (GDST == 1) {
        if (e_ok) *reinterpret_cast<float4 *>(L.G + e_off) = g;
    } else if (GDST == 2) {
        float4 adj; // ((step*G)/B) + (momentum*prev), SCE:333, on the f32 masters
        adj.x = sgd_adj(TS_STEP_OVER_B, g.x, TS_MOMENTUM, v_old.x);
        adj.y = sgd_adj(TS_STEP_OVER_B, g.y, TS_MOMENTUM, v_old.y);
        adj.z = sgd_adj(TS_STEP_OVER_B, g.z, TS_MOMENTUM, v_old.z);
        adj.w = sgd_adj(TS_STEP_OVER_B, g.w, TS_MOMENTUM, v_old.w);
        w_new = make_float4(w_old.x - adj.x, w_old.y - adj.y, w_old.z - adj.z, w_old.w - adj.w);
        if (e_ok) {
            ts_store16(L.W + e_off, (f32x4){w_new.x, w_new.y, w_new.z, w_new.w}); // (write-through: see ts_store16)
            ts_store16(L.V + e_off, (f32x4){adj.x, adj.y, adj.z, adj.w});
            *reinterpret_cast<bf16x4 *>(TS_REL(p.Wb[li]) + e_off) = (bf16x4){(__bf16)w_new.x, (__bf16)w_new.y, (__bf16)w_new.z, (__bf16)w_new.w};
        }
    }
    if (!fwd) return;

    // ---- next batch's first-layer sums over this tile's 64 inputs, transposed: Zp^T[n][b] = sum_m W[m][n] A'[b][m] ----
    if (t < 256) {
        const float4 w = e_ok ? w_new : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<bf16x4 *>(&sW[er * TS_TN + eq * 4]) = (bf16x4){(__bf16)w.x, (__bf16)w.y, (__bf16)w.z, (__bf16)w.w};
    }
    __syncthreads();
    float *slab = TS_REL(p.slabs) + (size_t)tm * p.slab_rows * p.ldz;
    const bf16x8 w0 = tr_frag(sW, TS_TN, 0, 0, lane), w1 = tr_frag(sW, TS_TN, 0, 32, lane); // A operand: rows n, k = m
    for (int b0 = 0; b0 < TS_NEXT_K; b0 += TS_KC) {
        if (b0) load_next(b0);
        if (TS_REL(p.stage_out_b) && tn < stage_cols && (((b0 + wave * 16) >> 4) % stage_cols) == tn && b0 + wave * 16 < TS_NEXT_K) { // (as in tile_step_kernel)
            __bf16 *dst = TS_REL(p.stage_out_b) + (size_t)(b0 + wave * 16 + fr) * p.ldan + m0 + 4 * fg;
#pragma unroll
            for (int kb = 0; kb < 2; kb++)
#pragma unroll
                for (int hh = 0; hh < 2; hh++)
                    if (m0 + kb * 32 + hh * 16 + 4 * fg < L.M) *reinterpret_cast<s16x4 *>(dst + kb * 32 + hh * 16) = vn[kb][hh];
        }
        if (b0 + wave * 16 < TS_NEXT_K) { // wave-uniform
            f32x4 z = {0.f, 0.f, 0.f, 0.f};
            z = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, join8(vn[0][0], vn[0][1]), z, 0, 0, 0);
            z = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, join8(vn[1][0], vn[1][1]), z, 0, 0, 0);
            ts_mfma_result(z);
            ts_store16(slab + (size_t)(b0 + wave * 16 + fr) * p.ldz + n0 + 4 * fg, z); // rows n = 4fg + r, column b = fr
        }
    }
