// tile_step_body.inc -- the body of tile_step_kernel (tile_step_kernel.h), included INSIDE the kernels that run it:
// the single-net kernel and its grouped twin (group_kernels.h).  In scope: the kernel argument `p` (TileStepParams),
// the template parameters GSRC / GDST / FWD, TS_HEAD_PROLOGUE / TS_HEAD / TS_DEFER_WV / TS_LOOKUP1 / TS_HAS_ROW_IDX (tile_step_kernel.h), TS_MERGE_KINDS (and, where it is 1, TS_MERGE: the
// workgroup kinds of the merged map, in one single-net instance; 0 in the grouped twins), and nine macros that say who the kernel works for:
// TS_BID (the workgroup's index in the tile map), TS_REL(ptr) (the net's copy of a pointer of `p`), TS_REL_LAYER(L) (the same
// for a layer descriptor), TS_STEP_OVER_B and TS_MOMENTUM, and the four row counts TS_K / TS_K_TRUE (the current batch, padded /
// live) and TS_NEXT_K / TS_NEXT_ROWS (the next one).  The single-net kernels define them as the plain expressions
// they replace (tile_step_kernel.h), the grouped twins as member k's (group_kernels.h): block-uniform either way.  Text the kernels include, not a function
// they call, so that the single-net kernels read `p` straight from their argument segment and compile to exactly the code
// they had before the grouped twins existed.
    constexpr int NW = TS_THREADS / 64, NT = TS_THREADS, RPW = 1; // waves; threads; 16-row groups of a 128-row chunk per wave
    constexpr int LDA = TS_TM + 16;  // gradient A image [k][m]: row stride = 16 (mod 32) floats
    constexpr int LDD = TS_TN;       // delta image [k][n]: 16 floats (lanes 16-31 land on banks 16-31)
    constexpr int LDW = TS_TN + 4;   // weight tile / partial tiles [m][n]
    __shared__ __attribute__((aligned(16))) float sA[TS_KC * LDA];       // A chunk [128][64]
#if TS_MERGE_KINDS
    constexpr int SD_IMAGES = TS_MERGE ? 2 : 1; // (the merged kinds below keep two [128][16] images side by side: +8 KB)
#else
    constexpr int SD_IMAGES = 1;
#endif
    __shared__ __attribute__((aligned(16))) float sD[SD_IMAGES * TS_KC * LDD]; // delta chunk [128][16]
    __shared__ __attribute__((aligned(16))) float sW[TS_TM * LDW];       // the tile's (new) weights (53 KB in all)
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    TS_STAMP(0);

    // by value: one batch of scalar loads, not one round trip per field as it is first used; layer 0's descriptor (nine of
    // ten workgroups) is requested at once, beside the map entry that names the tile, not behind it
    int li, tm, tn;
    GradLayer L = p.layer[0];
#if TS_HEAD_PROLOGUE
    // a regular slot (tile_step_kernel.h, ts_head_tile: the full layer-0 tiles) takes its tile from the workgroup's id and
    // everything its first vector loads and the `interior` test need from the preloaded head arguments: no scalar load
    // stands in front of them.  Of the struct's descriptor only G is read then (the forms that store or fetch a gradient).
    const bool regular = TS_HEAD && ts_head_tile(hd_geo, hd_kx, (int)TS_BID, tm, tn); // (block-uniform)
    bool have_L = false; // the descriptor of a later layer's tile is in L already
    if (regular) {
        li = 0;
        L.A = hd_A; L.D = hd_D; L.W = hd_W; L.V = hd_V; L.lda = hd_lda; L.ldd = hd_ldd; L.M = hd_M;
    } else if (TS_HEAD && TS_LOOKUP1) {
        // A slot that keeps the lookup (a later layer's tile, layer 0's partial last tile row) had up to four DEPENDENT scalar
        // round trips in front of its first vector load: map_in_args, then the map word, then -- twice, the compiler waits
        // between two loads into registers still in flight -- the descriptor the word names.  Here everything such a slot can
        // need is requested in ONE batch: the flag, the word of this workgroup (its index clamped into the struct: the flag may
        // say that the map is not there) and layer 1's descriptor (inside the struct whatever n_layers is); layer 0's is the head arguments' in every
        // slot.  Only a tile of layer 2 or later, or a map that does not fit the arguments, pays a second trip.
        const unsigned wi = (unsigned)(TS_BID >> 1) < (unsigned)(TS_MAP_ARGS / 2) ? (unsigned)(TS_BID >> 1) : (unsigned)(TS_MAP_ARGS / 2 - 1); // (clamped: a grid the words do not hold reads the table below)
        const uint32_t w = p.map_words[wi];
        const int in_args = p.map_in_args;
        GradLayer L1 = p.layer[1];
        // (an empty statement that "reads" them: left alone, the compiler sinks the descriptor's loads into the branch that
        //  uses them, behind the wait for the word -- the second trip again)
        asm volatile("" ::"s"(w), "s"(in_args), "s"(L1.A), "s"(L1.D), "s"(L1.W), "s"(L1.V), "s"(L1.lda), "s"(L1.ldd), "s"(L1.M));
        if (GSRC >= 2 || GDST == 1) asm volatile("" ::"s"(L1.G));
#if TS_MERGE_KINDS
        if (TS_MERGE) asm volatile("" ::"s"(L1.N), "s"(L.N)); // (the merged kinds clip their columns at the layer's width)
#endif
        uint32_t e = (TS_BID & 1) ? w >> 16 : w & 0xffffu;
        li = (int)(e & 7u); tm = (int)((e >> 3) & 63u); tn = (int)(e >> 9);
        bool idle = e == 0xffffu;
        if (!in_args) {
            e = p.tile_map[TS_BID];
            idle = e == ~0u;
            li = (int)(e & 15u); tm = (int)((e >> 4) & 0x3fffu); tn = (int)(e >> 18);
        }
        if (idle) return;
        L.A = hd_A; L.D = hd_D; L.W = hd_W; L.V = hd_V; L.lda = hd_lda; L.ldd = hd_ldd; L.M = hd_M;
        if (li == 1) L = L1;
        else if (li != 0) L = p.layer[li];
        have_L = true;
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
#if TS_HEAD_PROLOGUE
    if (li != 0 && !have_L) L = p.layer[li];
#else
    if (li != 0) L = p.layer[li];
#endif
    TS_REL_LAYER(L);
    const int m0 = tm * TS_TM, n0 = tn * TS_TN;
    const bool fwd = FWD && li == 0; // block-uniform

#if TS_MERGE_KINDS
    // ---- the workgroup kinds of make_merged_tile_map (tile_step_kernel.h): several light tiles in one workgroup ------------
    // Every tile's sums are the ones it has on the path below, operation for operation: the same MFMAs on acc0 / acc1 over the
    // same trips, the same update, the same z0 + z1 of a slab piece (the MFMAs a partial-row tile spends on its zero padding are
    // not issued: they add +0 to sums that start at +0).  Only who computes a tile changes.  A whole layer-0 tile goes on below.
    static_assert(!TS_MERGE || (GSRC == 1 && GDST == 2 && FWD && TS_HEAD && TS_DEFER_WV), "the merged kinds exist for the training form only");
    if (TS_MERGE && (li != 0 || L.M - m0 <= TS_TM / 2)) {
        constexpr int SDI = TS_KC * LDD; // floats of one [128][16] image in sD
        const int tiles_n = L.N / TS_TN, kc0 = (TS_K < TS_KC) ? TS_K : TS_KC;
        // the gradient loop of the path below on two operand images: x the delta operand, y the A operand
        auto grad_loop = [&](const float *xp, const int ldx, const float *yp, const int ldy, const int kc, f32x4 &acc0, f32x4 &acc1) __attribute__((always_inline)) {
            int kk = 0;
            if (kc == TS_KC) {
                float x[2][8], y[2][8];
#pragma unroll
                for (int j = 0; j < 8; j++) { x[0][j] = xp[(4 * j) * ldx]; y[0][j] = yp[(4 * j) * ldy]; }
#pragma unroll
                for (int trip = 0; trip < TS_KC / 32; trip++) {
                    const int cur = trip & 1;
                    if (trip + 1 < TS_KC / 32) {
#pragma unroll
                        for (int j = 0; j < 8; j++) { x[cur ^ 1][j] = xp[(32 * (trip + 1) + 4 * j) * ldx]; y[cur ^ 1][j] = yp[(32 * (trip + 1) + 4 * j) * ldy]; }
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int j = 0; j < 8; j += 2) {
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x[cur][j], y[cur][j], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x[cur][j + 1], y[cur][j + 1], acc1, 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                kk = TS_KC;
            }
            for (; kk + 32 <= kc; kk += 32) {
                float x[8], y[8];
#pragma unroll
                for (int j = 0; j < 8; j++) { x[j] = xp[(kk + 4 * j) * ldx]; y[j] = yp[(kk + 4 * j) * ldy]; }
#pragma unroll
                for (int j = 0; j < 8; j += 2) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j], y[j], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j + 1], y[j + 1], acc1, 0, 0, 0);
                }
            }
            for (; kk < kc; kk += 4)
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xp[kk * ldx], yp[kk * ldy], acc0, 0, 0, 0);
        };
        auto update = [&](const f32x4 acc, const float4 w_old, const float4 v_old, const size_t e_off, const bool e_ok) __attribute__((always_inline)) {
            float4 adj;
            adj.x = sgd_adj(TS_STEP_OVER_B, acc[0], TS_MOMENTUM, v_old.x);
            adj.y = sgd_adj(TS_STEP_OVER_B, acc[1], TS_MOMENTUM, v_old.y);
            adj.z = sgd_adj(TS_STEP_OVER_B, acc[2], TS_MOMENTUM, v_old.z);
            adj.w = sgd_adj(TS_STEP_OVER_B, acc[3], TS_MOMENTUM, v_old.w);
            const float4 w_new = make_float4(w_old.x - adj.x, w_old.y - adj.y, w_old.z - adj.z, w_old.w - adj.w);
            if (e_ok) {
                ts_store16(L.W + e_off, (f32x4){w_new.x, w_new.y, w_new.z, w_new.w});
                ts_store16(L.V + e_off, (f32x4){adj.x, adj.y, adj.z, adj.w});
            }
            return w_new;
        };
        const bool wide = (unsigned long long)TS_KC * (unsigned)(L.lda > L.ldd ? L.lda : L.ldd) >= 0xffffffffull; // no 32-bit offsets

        if (li != 0) {
            // -- a pair of a later layer: columns tn and tn + 1 of one tile row.  The A chunk is loaded and staged once; waves
            //    0..3 run the gradient loop on column tn, waves 4..7 on column tn + 1 (the second image of sD); all 512 threads
            //    update 16 B of W / V.  No forward half.
            const int ncol = ts_merged_columns(li, 0, tn, tiles_n); // 2, or 1 at the end of an odd row
            const int half = wave >> 2, er = (wave & 3) * 16 + fr;
            const bool e_ok = m0 + er < L.M && half < ncol;
            const size_t e_off = (size_t)(m0 + er) * L.ldd + n0 + half * TS_TN + fq * 4;
            float4 va[4], vd[2];
            auto load_ops = [&](const int k0, const int kc, const bool plain) __attribute__((always_inline)) {
                if (plain) { // (block-uniform) a whole chunk of a whole tile, both columns: no bounds tests
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int idx = t + i * NT, k = idx >> 4, q = idx & 15;
                        va[i] = *reinterpret_cast<const float4 *>(L.A + ((unsigned)k * (unsigned)L.lda + m0 + q * 4));
                    }
#pragma unroll
                    for (int c = 0; c < 2; c++)
                        vd[c] = *reinterpret_cast<const float4 *>(L.D + ((unsigned)(t >> 2) * (unsigned)L.ldd + n0 + c * TS_TN + (t & 3) * 4));
                    return;
                }
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int idx = t + i * NT, k = idx >> 4, q = idx & 15;
                    va[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (k < kc && m0 + q * 4 < L.M) va[i] = *reinterpret_cast<const float4 *>(L.A + (size_t)(k0 + k) * L.lda + m0 + q * 4);
                }
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    vd[c] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if ((t >> 2) < kc && c < ncol) vd[c] = *reinterpret_cast<const float4 *>(L.D + (size_t)(k0 + (t >> 2)) * L.ldd + n0 + c * TS_TN + (t & 3) * 4);
                }
            };
            load_ops(0, kc0, (m0 + TS_TM <= L.M) && TS_K >= TS_KC && ncol == 2 && !wide);
            TS_STAMP(1);
            float4 w_old = make_float4(0.f, 0.f, 0.f, 0.f), v_old = make_float4(0.f, 0.f, 0.f, 0.f);
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < TS_K; k0 += TS_KC) {
                const int kc = (TS_K - k0 < TS_KC) ? TS_K - k0 : TS_KC;
                if (k0) { __syncthreads(); load_ops(k0, kc, false); }
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int idx = t + i * NT, k = idx >> 4, q = idx & 15;
                    *reinterpret_cast<float4 *>(&sA[k * LDA + q * 4]) = va[i];
                }
#pragma unroll
                for (int c = 0; c < 2; c++) *reinterpret_cast<float4 *>(&sD[c * SDI + (t >> 2) * LDD + (t & 3) * 4]) = vd[c];
                __syncthreads();
                if (k0 == 0) {
                    TS_STAMP(2);
                    if (e_ok) { w_old = *reinterpret_cast<const float4 *>(L.W + e_off); v_old = *reinterpret_cast<const float4 *>(L.V + e_off); }
                }
                if (half < ncol) grad_loop(&sD[half * SDI + fq * LDD + fr], LDD, &sA[fq * LDA + (wave & 3) * 16 + fr], LDA, kc, acc0, acc1); // (wave-uniform)
            }
            update(acc0 + acc1, w_old, v_old, e_off, e_ok);
            TS_STAMP(3);
            return;
        }

        // -- a group of layer 0's partial last tile row, h = 16 or 32 weight rows: 64 / h adjacent column tiles.  The two images
        //    swap roles: the h-wide A chunk goes where sD is (one [128][16] image per m tile), the delta chunk of all the group's
        //    columns where sA is.  Wave w of 0..3 runs the gradient loop for column tile w / (h / 16), m tile w % (h / 16); in
        //    the forward half every wave keeps its 16 rows of the next batch, h inputs wide, and forms one slab piece per column
        //    tile from sW, which holds the group's new weights.
        // (one body per height, MTS = h / 16 m tiles: every count below is a constant of its instance)
        auto group = [&](auto mts_c) __attribute__((always_inline)) {
            constexpr int MTS = decltype(mts_c)::value, H = 16 * MTS, NCOL = TS_TM / H; // m tiles; rows; column tiles of a full group
            constexpr int ASH = MTS == 2 ? 3 : 2, DSH = MTS == 2 ? 3 : 4;               // float4s per row of the A chunk / of the delta chunk, as shifts
            const int ncol = ts_merged_columns(0, H, tn, tiles_n);                      // column tiles owned
            const int gc = MTS == 2 ? wave >> 1 : wave, gm = MTS == 2 ? wave & 1 : 0;   // (waves 0..3)
            const int er = gm * 16 + fr;
            const bool e_ok = wave < 4 && gc < ncol;
            const size_t e_off = (size_t)(m0 + er) * L.ldd + n0 + gc * TS_TN + fq * 4;
            float4 va[MTS], vd[NCOL];
            auto load_ops = [&](const int k0, const int kc, const bool plain) __attribute__((always_inline)) {
                if (plain) { // (block-uniform) a whole chunk, rows in place, every column of a full group: no bounds tests
#pragma unroll
                    for (int i = 0; i < MTS; i++) {
                        const int idx = t + i * NT, k = idx >> ASH, q = idx & ((1 << ASH) - 1);
                        va[i] = *reinterpret_cast<const float4 *>(L.A + ((unsigned)k * (unsigned)L.lda + m0 + q * 4));
                    }
#pragma unroll
                    for (int i = 0; i < NCOL; i++) {
                        const int idx = t + i * NT, k = idx >> DSH, q = idx & ((1 << DSH) - 1);
                        vd[i] = *reinterpret_cast<const float4 *>(L.D + ((unsigned)k * (unsigned)L.ldd + n0 + q * 4));
                    }
                    return;
                }
#pragma unroll
                for (int i = 0; i < MTS; i++) {
                    const int idx = t + i * NT, k = idx >> ASH, q = idx & ((1 << ASH) - 1);
                    va[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (k < kc) {
                        size_t a_row = (size_t)(k0 + k);
                        bool live = true;
                        if (TS_REL(p.row_idx)) { live = k0 + k < TS_K_TRUE; a_row = live ? (size_t)TS_REL(p.row_idx)[k0 + k] : 0; }
                        if (live) va[i] = *reinterpret_cast<const float4 *>(L.A + a_row * L.lda + m0 + q * 4);
                    }
                }
#pragma unroll
                for (int i = 0; i < NCOL; i++) {
                    const int idx = t + i * NT, k = idx >> DSH, q = idx & ((1 << DSH) - 1);
                    vd[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (k < kc && q * 4 < ncol * TS_TN) vd[i] = *reinterpret_cast<const float4 *>(L.D + (size_t)(k0 + k) * L.ldd + n0 + q * 4);
                }
            };
            load_ops(0, kc0, TS_K >= TS_KC && !TS_HAS_ROW_IDX && ncol == NCOL && !wide);
            TS_STAMP(1);
            // the next batch's rows of this wave, H inputs wide, in fragment form (as vn below)
            f32x4 vn[MTS];
            int next_row0 = wave * 16 + fr;
            if (TS_REL(p.next_idx) && next_row0 < TS_NEXT_ROWS) next_row0 = TS_REL(p.next_idx)[next_row0];
            auto load_next = [&](const int b0) __attribute__((always_inline)) {
                const int b = b0 + wave * 16 + fr;
                const bool live = b < TS_NEXT_ROWS;
                const size_t row = live ? (b0 == 0 ? (size_t)next_row0 : TS_REL(p.next_idx) ? (size_t)TS_REL(p.next_idx)[b] : (size_t)b) : 0;
                const float *src = TS_REL(p.An) + row * p.ldan + m0 + 4 * fq;
#pragma unroll
                for (int c = 0; c < MTS; c++) {
                    vn[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    if (live) vn[c] = *reinterpret_cast<const f32x4 *>(src + c * 16);
                }
            };
            float4 w_old = make_float4(0.f, 0.f, 0.f, 0.f), v_old = make_float4(0.f, 0.f, 0.f, 0.f);
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < TS_K; k0 += TS_KC) {
                const int kc = (TS_K - k0 < TS_KC) ? TS_K - k0 : TS_KC;
                if (k0) { __syncthreads(); load_ops(k0, kc, false); }
#pragma unroll
                for (int i = 0; i < MTS; i++) {
                    const int idx = t + i * NT, k = idx >> ASH, q = idx & ((1 << ASH) - 1);
                    *reinterpret_cast<float4 *>(&sD[(q >> 2) * SDI + k * LDD + (q & 3) * 4]) = va[i];
                }
#pragma unroll
                for (int i = 0; i < NCOL; i++) {
                    const int idx = t + i * NT, k = idx >> DSH, q = idx & ((1 << DSH) - 1);
                    *reinterpret_cast<float4 *>(&sA[k * LDA + q * 4]) = vd[i];
                }
                __syncthreads();
                if (k0 == 0) {
                    TS_STAMP(2);
                    if (e_ok) { w_old = *reinterpret_cast<const float4 *>(L.W + e_off); v_old = *reinterpret_cast<const float4 *>(L.V + e_off); }
                    load_next(0);
                }
                if (e_ok) grad_loop(&sA[fq * LDA + gc * TS_TN + fr], LDA, &sD[gm * SDI + fq * LDD + fr], LDD, kc, acc0, acc1); // (wave-uniform)
            }
            const float4 w_new = update(acc0 + acc1, w_old, v_old, e_off, e_ok);
            TS_STAMP(3);
            // sW: [column tile][H rows][LDW]; the rows of a column tile the group does not own (a short last group) are zeros
            if (wave < 4) *reinterpret_cast<float4 *>(&sW[((gc * MTS + gm) * 16 + fr) * LDW + fq * 4]) = e_ok ? w_new : make_float4(0.f, 0.f, 0.f, 0.f);
            __syncthreads();
            float *slab = TS_REL(p.slabs) + (size_t)tm * p.slab_rows * p.ldz;
            float wv[NCOL][MTS][4]; // [column tile][16-input chunk][j]: W[m = 16 c + 4 fq + j][n = fr] of column tile cc
#pragma unroll
            for (int cc = 0; cc < NCOL; cc++)
#pragma unroll
                for (int c = 0; c < MTS; c++)
#pragma unroll
                    for (int j = 0; j < 4; j++) wv[cc][c][j] = sW[(cc * H + c * 16 + 4 * fq + j) * LDW + fr];
            for (int b0 = 0; b0 < TS_NEXT_K; b0 += TS_KC) {
                if (b0) load_next(b0);
                const int wr = wave * 16;
                if (b0 + wr < TS_NEXT_K) { // wave-uniform
#pragma unroll
                    for (int cc = 0; cc < NCOL; cc++) {
                        f32x4 z0 = {0.f, 0.f, 0.f, 0.f}, z1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int j = 0; j < 4; j++) z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[cc][0][j], vn[0][j], z0, 0, 0, 0);
                        if (MTS == 2) {
#pragma unroll
                            for (int j = 0; j < 4; j++) z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[cc][MTS - 1][j], vn[MTS - 1][j], z1, 0, 0, 0);
                        }
                        const f32x4 z = z0 + z1;
                        if (cc < ncol) ts_store16(slab + (size_t)(b0 + wr + fr) * p.ldz + n0 + cc * TS_TN + 4 * fq, z); // (block-uniform)
                    }
                }
            }
            TS_STAMP(3);
        };
        if (L.M - m0 == 16) group(ts_int<1>{});
        else group(ts_int<2>{});
        return;
    }
#endif

    // this thread's 16 B of the weight tile (waves 0..3): row er = 16*wave + fr, columns 4*fq .. 4*fq+3 -- the
    // accumulator layout of the transposed gradient product below, so G never leaves its registers
    const int er = (t >> 6) * 16 + fr, eq = fq;
    const bool e_ok = t < 256 && (m0 + er < L.M);
    const size_t e_off = (size_t)(m0 + er) * L.ldd + n0 + eq * 4;

    // ---- everything this block reads first, all loads in flight together ------------------------
    // gradient operands of the first K chunk
    float4 va[4 * RPW], vd[RPW];
    const int kc0 = (TS_K < TS_KC) ? TS_K : TS_KC;
    // A tile wholly inside its layer, a whole first chunk, rows in place: no bounds tests, no exec-mask branches -- every wave
    // runs this prologue before the first barrier, and a guarded 16-B load is ~13 instructions (see gemm_f32_kernel)
    const bool interior = (m0 + TS_TM <= L.M) && (TS_K >= TS_KC) && !(li == 0 && TS_HAS_ROW_IDX) &&
                          (unsigned long long)TS_KC * (unsigned)(L.lda > L.ldd ? L.lda : L.ldd) < 0xffffffffull; // 32-bit offsets
    if (GSRC == 1 && interior) {
#pragma unroll
        for (int i = 0; i < 4 * RPW; i++) {
            const int idx = t + i * NT, k = idx >> 4, q = idx & 15;
            va[i] = *reinterpret_cast<const float4 *>(L.A + ((unsigned)k * (unsigned)L.lda + m0 + q * 4));
        }
#pragma unroll
        for (int i = 0; i < RPW; i++) {
            const int idx = t + i * NT;
            vd[i] = *reinterpret_cast<const float4 *>(L.D + ((unsigned)(idx >> 2) * (unsigned)L.ldd + n0 + (idx & 3) * 4));
        }
    } else if (GSRC == 1) {
#pragma unroll
        for (int i = 0; i < 4 * RPW; i++) {
            const int idx = t + i * NT, k = idx >> 4, q = idx & 15;
            va[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < kc0 && m0 + q * 4 < L.M) {
                size_t a_row = (size_t)k;
                bool live = true;
                if (li == 0 && TS_REL(p.row_idx)) { live = k < TS_K_TRUE; a_row = live ? (size_t)TS_REL(p.row_idx)[k] : 0; }
                if (live) va[i] = *reinterpret_cast<const float4 *>(L.A + a_row * L.lda + m0 + q * 4);
            }
        }
#pragma unroll
        for (int i = 0; i < RPW; i++) {
            const int idx = t + i * NT, k = idx >> 2, q = idx & 3;
            vd[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < kc0) vd[i] = *reinterpret_cast<const float4 *>(L.D + (size_t)k * L.ldd + n0 + q * 4);
        }
    }
    TS_STAMP(1);
    // the tile's W and V.  With a gradient product to wait for (GSRC == 1, TS_DEFER_WV) they are requested BEHIND the first
    // barrier: they are first needed at the update, after the gradient MFMAs, and in front of the barrier their 8 KB share
    // the CU's load path with the 40 KB of gradient operands the barrier waits for.
    constexpr bool defer_wv = TS_DEFER_WV && GSRC == 1;
    float4 w_old = make_float4(0.f, 0.f, 0.f, 0.f), v_old = w_old, g_in = w_old;
    if (!defer_wv && e_ok) {
        if (GDST == 2 || FWD) w_old = *reinterpret_cast<const float4 *>(L.W + e_off);
        if (GDST == 2) v_old = *reinterpret_cast<const float4 *>(L.V + e_off);
    }
    if (GSRC >= 2) g_in = ts_gradient_in<GSRC>(p, L, e_off, e_ok);
    const bool next_plain = interior && fwd && !TS_REL(p.next_idx) && TS_NEXT_ROWS >= TS_KC && (unsigned long long)TS_KC * (unsigned)p.ldan < 0xffffffffull; // the first chunk of the next batch: all rows live, in place
    const bool next_gather = (m0 + TS_TM <= L.M) && fwd && TS_REL(p.next_idx) && TS_NEXT_ROWS >= TS_KC;
    const int stage_cols = (TS_STAGE_N / TS_TN) < 8 ? (TS_STAGE_N / TS_TN) : 8; // tile columns that share the staging copy's 16-row groups (read with fwd only: layer 0)
    // the next batch's rows, already in MFMA fragment form: wave -> 16 batch rows of a 128-row chunk, lane
    // (fr, fq) -> row fr, inputs 16c + 4fq .. +3 of the tile (c = 0..3).  Straight to registers: A_0' is
    // k-contiguous, no wave shares another's rows, and the product below needs no LDS image of it.
    f32x4 vn[RPW][4];
    // a sampled next batch: this lane's row index of the first chunk is fetched NOW, so that the row loads, requested
    // ~3 000 cycles from here, do not start with a dependent round trip
    int next_row0[RPW];
#pragma unroll
    for (int g = 0; g < RPW; g++) {
        next_row0[g] = (wave + g * NW) * 16 + fr;
        if (fwd && TS_REL(p.next_idx) && next_row0[g] < TS_NEXT_ROWS) next_row0[g] = TS_REL(p.next_idx)[next_row0[g]];
    }
    auto load_next = [&](int b0) {
#pragma unroll
        for (int g = 0; g < RPW; g++) {
            const int b = b0 + (wave + g * NW) * 16 + fr;
            if (b0 == 0 && next_plain) { // (block-uniform)
                const float *src = TS_REL(p.An) + ((unsigned)b * (unsigned)p.ldan + m0 + 4 * fq);
#pragma unroll
                for (int c = 0; c < 4; c++) vn[g][c] = *reinterpret_cast<const f32x4 *>(src + c * 16);
                continue;
            }
            if (b0 == 0 && next_gather) { // (block-uniform) a sampled batch, every row live, the tile inside the layer: the same
                                          // four loads from the row the index names (fetched at the top), no bounds tests
                const float *src = TS_REL(p.An) + ((size_t)next_row0[g] * p.ldan + m0 + 4 * fq);
#pragma unroll
                for (int c = 0; c < 4; c++) vn[g][c] = *reinterpret_cast<const f32x4 *>(src + c * 16);
                continue;
            }
            const bool live = b < TS_NEXT_ROWS;
            const size_t row = live ? (b0 == 0 ? (size_t)next_row0[g] : TS_REL(p.next_idx) ? (size_t)TS_REL(p.next_idx)[b] : (size_t)b) : 0;
            const float *src = TS_REL(p.An) + row * p.ldan + m0 + 4 * fq;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                vn[g][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (live && m0 + c * 16 + 4 * fq < L.M) vn[g][c] = *reinterpret_cast<const f32x4 *>(src + c * 16);
            }
        }
    };
    // (requested behind the gradient operands, below: it is needed ~2 500 cycles later, and in front of them it
    //  delayed the first barrier by the time its 32 KB take to cross the CU's load path)
    if (fwd && GSRC != 1) load_next(0);

    // ---- gradient tile, transposed: G^T[n][m] = sum_k D[k][n] A[k][m] -----------------------------
    // Waves 0..3 take one 16-wide m tile each over the whole K chunk; lane (fr, fq) ends with G[m = 16 wave + fr]
    // [n = 4 fq .. 4 fq + 3]: the 16 B of W and V it loaded at the top.  No partial tiles, no second barrier.
    // (Waves 4..7 sit on the same four SIMDs: splitting K over them bought no MFMA time and cost an LDS round trip.)
    float4 g = g_in;
    if (GSRC == 1) {
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < TS_K; k0 += TS_KC) {
            const int kc = (TS_K - k0 < TS_KC) ? TS_K - k0 : TS_KC; // a multiple of 16
            if (k0) {
                __syncthreads();
#pragma unroll
                for (int i = 0; i < 4 * RPW; i++) {
                    const int idx = t + i * NT, k = idx >> 4, q = idx & 15;
                    va[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (k < kc && m0 + q * 4 < L.M) {
                        size_t a_row = (size_t)(k0 + k);
                        bool live = true;
                        if (li == 0 && TS_REL(p.row_idx)) { live = k0 + k < TS_K_TRUE; a_row = live ? (size_t)TS_REL(p.row_idx)[k0 + k] : 0; }
                        if (live) va[i] = *reinterpret_cast<const float4 *>(L.A + a_row * L.lda + m0 + q * 4);
                    }
                }
#pragma unroll
                for (int i = 0; i < RPW; i++) {
                    const int idx = t + i * NT, k = idx >> 2, q = idx & 3;
                    vd[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (k < kc) vd[i] = *reinterpret_cast<const float4 *>(L.D + (size_t)(k0 + k) * L.ldd + n0 + q * 4);
                }
            }
#pragma unroll
            for (int i = 0; i < 4 * RPW; i++) {
                const int idx = t + i * NT, k = idx >> 4, q = idx & 15;
                *reinterpret_cast<float4 *>(&sA[k * LDA + q * 4]) = va[i];
            }
#pragma unroll
            for (int i = 0; i < RPW; i++) {
                const int idx = t + i * NT;
                *reinterpret_cast<float4 *>(&sD[(idx >> 2) * LDD + (idx & 3) * 4]) = vd[i];
            }
            __syncthreads();
            if (k0 == 0) {
                TS_STAMP(2);
                if (defer_wv && e_ok) { // (the batch has at least one row, so this trip runs) needed at the update: in front of the rows below, which are needed later still
                    if (GDST == 2 || FWD) w_old = *reinterpret_cast<const float4 *>(L.W + e_off);
                    if (GDST == 2) v_old = *reinterpret_cast<const float4 *>(L.V + e_off);
                }
                if (fwd) load_next(0); // lands under the gradient MFMAs and the update
            }
            if (wave < 4) {
                const float *ap = &sA[fq * LDA + wave * 16 + fr];
                const float *dp = &sD[fq * LDD + fr];
                int kk = 0;
                if (kc == TS_KC) {
                    // a whole chunk (every step at B = 128): the operands of trip t + 1 are requested before the MFMAs of trip t --
                    // trip by trip, the first MFMA of every trip waited out an LDS round trip that nothing covered (one wave per
                    // SIMD here).  The same MFMAs on the same accumulators in the same order as the loop below.  (All 64 reads up
                    // front took 148 registers: two workgroups no longer fit a CU, and 28 CUs hold two.)
                    float a[2][8], d[2][8];
#pragma unroll
                    for (int j = 0; j < 8; j++) { a[0][j] = ap[(4 * j) * LDA]; d[0][j] = dp[(4 * j) * LDD]; }
#pragma unroll
                    for (int trip = 0; trip < TS_KC / 32; trip++) {
                        const int cur = trip & 1;
                        if (trip + 1 < TS_KC / 32) {
#pragma unroll
                            for (int j = 0; j < 8; j++) { a[cur ^ 1][j] = ap[(32 * (trip + 1) + 4 * j) * LDA]; d[cur ^ 1][j] = dp[(32 * (trip + 1) + 4 * j) * LDD]; }
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int j = 0; j < 8; j += 2) {
                            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(d[cur][j], a[cur][j], acc0, 0, 0, 0);
                            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(d[cur][j + 1], a[cur][j + 1], acc1, 0, 0, 0);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    kk = TS_KC;
                }
                for (; kk + 32 <= kc; kk += 32) { // 8 MFMAs per trip, the trip's 16 LDS reads issued first
                    float a[8], d[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) { a[j] = ap[(kk + 4 * j) * LDA]; d[j] = dp[(kk + 4 * j) * LDD]; }
#pragma unroll
                    for (int j = 0; j < 8; j += 2) {
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(d[j], a[j], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(d[j + 1], a[j + 1], acc1, 0, 0, 0);
                    }
                }
                for (; kk < kc; kk += 4)
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(dp[kk * LDD], ap[kk * LDA], acc0, 0, 0, 0);
            }
        }
        const f32x4 acc = acc0 + acc1; // rows n = 4 fq + r, column m = 16 wave + fr
        g = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }

    // ---- store G, or the momentum update (SCE:333-339) -------------------------------------------
    float4 w_new = w_old;
    if (GDST == 1) {
        if (e_ok) *reinterpret_cast<float4 *>(L.G + e_off) = g;
    } else if (GDST == 2) {
        float4 adj; // ((step*G)/B) + (momentum*prev)
        adj.x = sgd_adj(TS_STEP_OVER_B, g.x, TS_MOMENTUM, v_old.x);
        adj.y = sgd_adj(TS_STEP_OVER_B, g.y, TS_MOMENTUM, v_old.y);
        adj.z = sgd_adj(TS_STEP_OVER_B, g.z, TS_MOMENTUM, v_old.z);
        adj.w = sgd_adj(TS_STEP_OVER_B, g.w, TS_MOMENTUM, v_old.w);
        w_new = make_float4(w_old.x - adj.x, w_old.y - adj.y, w_old.z - adj.z, w_old.w - adj.w);
        if (e_ok) {
            ts_store16(L.W + e_off, (f32x4){w_new.x, w_new.y, w_new.z, w_new.w});
            ts_store16(L.V + e_off, (f32x4){adj.x, adj.y, adj.z, adj.w});
        }
    }
    TS_STAMP(3);
    if (!fwd) return;

    // ---- the next batch's first-layer sums over this tile's 64 input neurons ---------------------
    // Computed TRANSPOSED, Zp^T[n][b] = sum_m W[m][n] A'[b][m]: the accumulator then holds four
    // consecutive n of one batch row per lane -- a 16-B store each, no trip through LDS.
    // MFMA j of chunk c: slot q holds k = 16c + 4q + j on both operands.
    if (t < 256) *reinterpret_cast<float4 *>(&sW[er * LDW + eq * 4]) = e_ok ? w_new : make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    float *slab = TS_REL(p.slabs) + (size_t)tm * p.slab_rows * p.ldz;
    const float *wcol = &sW[(4 * fq) * LDW + fr];
    float wv[4][4];
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
        for (int j = 0; j < 4; j++) wv[c][j] = wcol[(c * 16 + j) * LDW];
    for (int b0 = 0; b0 < TS_NEXT_K; b0 += TS_KC) {
        if (b0) load_next(b0);
#pragma unroll
        for (int g = 0; g < RPW; g++) {
            const int wr = (wave + g * NW) * 16; // this wave's row group of the chunk
            // the contiguous copy of a sampled next batch: every tile of this tile row holds the same rows; column tn copies
            // the 16-row groups g16 with g16 % n_tn == tn (all of them in one column made its 13 workgroups the kernel's last)
            if (TS_REL(p.stage_out) && b0 + wr < TS_NEXT_K && (((b0 + wr) >> 4) % stage_cols) == tn % stage_cols && tn < stage_cols) { // (wave-uniform; rows past the batch and columns past M are zeros in vn)
                float *dst = TS_REL(p.stage_out) + (size_t)(b0 + wr + fr) * p.ldan + m0 + 4 * fq;
#pragma unroll
                for (int c = 0; c < 4; c++)
                    if (m0 + c * 16 + 4 * fq < L.M) *reinterpret_cast<f32x4 *>(dst + c * 16) = vn[g][c];
            }
            if (b0 + wr < TS_NEXT_K) { // wave-uniform
                f32x4 z0 = {0.f, 0.f, 0.f, 0.f}, z1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < 4; c++) {
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        if (c & 1) z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[c][j], vn[g][c][j], z1, 0, 0, 0);
                        else z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[c][j], vn[g][c][j], z0, 0, 0, 0);
                    }
                }
                const f32x4 z = z0 + z1; // rows n = 4*fq + r, column b = fr
                ts_store16(slab + (size_t)(b0 + wr + fr) * p.ldz + n0 + 4 * fq, z);
            }
        }
    }
    TS_STAMP(3);
