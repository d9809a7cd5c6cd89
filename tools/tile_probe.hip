// tile_probe.hip -- development harness (not shipped): tile_step_kernel on the 784-300-100-10 / B = 128
// shapes with random data: HIP-event time per call of every mode, workgroup -> tile maps and sampled next batches, and the
// prologue variants (head arguments / W and V behind the first barrier) against the form they replace, in one process.
// Also the upper bounds (the launch with a class of workgroups taken out of the map) and the merged map and kinds (make_merged_tile_map) against the one-tile launch.
// Build as the library is built (-mllvm -amdgpu-kernarg-preload-count=16).  -DTILE_PROBE_STAMPS: the stamped build -- thread 0
// of every workgroup records the cycle counter at the kernel's top, behind its first vector loads, behind the first barrier and
// at its end; the times of THAT build are not the kernel's (use the plain build's lines), its stamps say where a workgroup's time goes.
#ifdef TILE_PROBE_STAMPS
#include <hip/hip_runtime.h>
__device__ unsigned long long g_stamp[4 * 1024];
// the first and the last of them also on the 100 MHz real-time counter, which every CU reads alike (the cycle counters of two CUs are not
// comparable), and where the workgroup ran: HW_ID (CU, shader array and engine in bits 8..15) and the XCC id
__device__ unsigned long long g_real[4 * 1024];
__device__ unsigned g_where[2 * 1024];
#define TS_STAMP(slot) do { if (threadIdx.x == 0) { g_stamp[(slot) * 1024 + blockIdx.x] = __builtin_readcyclecounter(); \
    if ((slot) == 0 || (slot) == 3) g_real[(slot) * 1024 + blockIdx.x] = __builtin_amdgcn_s_memrealtime(); \
    if ((slot) == 3) { g_where[blockIdx.x] = (unsigned)__builtin_amdgcn_s_getreg(0xF804); g_where[1024 + blockIdx.x] = (unsigned)__builtin_amdgcn_s_getreg(0xF814) & 15u; } } } while (0)
#endif
#include "../graph-neural-net_amd/csrc/tile_step_kernel.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace gnn;
// (the head arguments: tile_step_kernel.h, GNN_TS_HEAD_PARAMS -- in this order)
#define TSHEAD(p, hd) (p).layer[0].A, (p).layer[0].D, (p).layer[0].W, (p).layer[0].V, (p).layer[0].lda, (p).layer[0].ldd, (p).layer[0].M, ((p).K | ((p).row_idx ? 1 : 0)), (hd).geo, (hd).kx
#define LAUNCH(kern, grid, p, hd) hipLaunchKernelGGL(kern, dim3(grid), dim3(TS_THREADS), 0, s, TSHEAD(p, hd), p)
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1);} } while (0)

int main(int argc, char **argv) {
    const int L = 4, dims[4] = {784, 300, 100, 10};
    const int B = argc > 1 ? atoi(argv[1]) : 128;
    int ld[4]; for (int i = 0; i < L; i++) ld[i] = pad_up(dims[i]);
    const int Bp = pad_up(B);
    size_t woff[3], np = 0; for (int l = 0; l < 3; l++) { woff[l] = np; np += (size_t)ld[l] * ld[l + 1]; }
    float *W, *V, *G, *act[4], *delta[4], *slabs, *An;
    CK(hipMalloc(&W, np * 4)); CK(hipMalloc(&V, np * 4)); CK(hipMalloc(&G, np * 4));
    std::vector<float> hw(np, 0.f);
    for (int l = 0; l < 3; l++) for (int i = 0; i < dims[l]; i++) for (int j = 0; j < dims[l + 1]; j++)
        hw[woff[l] + (size_t)i * ld[l + 1] + j] = (rand() / (float)RAND_MAX - 0.5f) * 0.2f;
    CK(hipMemcpy(W, hw.data(), np * 4, hipMemcpyHostToDevice)); CK(hipMemset(V, 0, np * 4)); CK(hipMemset(G, 0, np * 4));
    for (int l = 0; l < L; l++) {
        std::vector<float> h((size_t)Bp * ld[l], 0.f);
        for (int b = 0; b < B; b++) for (int i = 0; i < dims[l]; i++) h[(size_t)b * ld[l] + i] = rand() / (float)RAND_MAX - 0.3f;
        CK(hipMalloc(&act[l], h.size() * 4)); CK(hipMemcpy(act[l], h.data(), h.size() * 4, hipMemcpyHostToDevice));
        for (auto &x : h) x *= 1e-3f;
        CK(hipMalloc(&delta[l], h.size() * 4)); CK(hipMemcpy(delta[l], h.data(), h.size() * 4, hipMemcpyHostToDevice));
    }
    CK(hipMalloc(&An, (size_t)Bp * ld[0] * 4)); CK(hipMemcpy(An, act[0], (size_t)Bp * ld[0] * 4, hipMemcpyDeviceToDevice));
    const int ns = (ld[0] + TS_TM - 1) / TS_TM;
    CK(hipMalloc(&slabs, (size_t)ns * Bp * ld[1] * 4));
    TileStepParams t{}; t.n_layers = 3; int tiles = 0, tiles0 = 0;
    for (int l = 0; l < 3; l++) { GradLayer &gl = t.layer[l]; gl.A = act[l]; gl.lda = ld[l]; gl.D = delta[l + 1]; gl.ldd = ld[l + 1];
        gl.W = W + woff[l]; gl.V = V + woff[l]; gl.G = G + woff[l]; gl.M = ld[l]; gl.N = ld[l + 1];
        gl.tiling = make_xcd_tiling((gl.M + TS_TM - 1) / TS_TM, gl.N / TS_TN); gl.block_begin = tiles; tiles += gl.tiling.blocks(); if (!l) tiles0 = tiles; }
    t.K = Bp; t.k_true = B; t.step_over_b = 1e-4f; t.momentum = 0.9f;
    t.An = An; t.ldan = ld[0]; t.next_rows = B; t.next_K = Bp; t.slabs = slabs; t.slab_rows = Bp; t.ldz = ld[1];
    // workgroup -> tile: the per-layer XCD rectangles of rounds 2-3 (idle blocks included), and the host-built map
    auto old_map = [&](int n_layers_used, int n_blocks) {
        std::vector<uint32_t> m((size_t)n_blocks, ~0u);
        for (int id = 0; id < n_blocks; id++) {
            int li = 0;
            for (int i = 1; i < n_layers_used; i++) if (id >= t.layer[i].block_begin) li = i;
            const XcdTiling &x = t.layer[li].tiling;
            const int loc = id - t.layer[li].block_begin, xx = loc & 7, j = loc >> 3, q = j / x.rn;
            const int tm = (xx >> x.xs) * x.rm + q, tn = (xx & (x.xn - 1)) * x.rn + (j - q * x.rn);
            if (tm < x.tiles_m && tn < x.tiles_n && q < x.rm) m[id] = (uint32_t)li | (uint32_t)tm << 4 | (uint32_t)tn << 18;
        }
        return m;
    };
    auto to_dev = [&](const std::vector<uint32_t> &m) { uint32_t *d; hipMalloc(&d, m.size() * 4); hipMemcpy(d, m.data(), m.size() * 4, hipMemcpyHostToDevice); return d; };
    const int tiles_old = tiles, tiles0_old = tiles0;
    const uint32_t *map_old = to_dev(old_map(3, tiles_old)), *map0_old = to_dev(old_map(1, tiles0_old));
    TileMapLayer ml[3]; for (int l = 0; l < 3; l++) ml[l] = TileMapLayer{ld[l], ld[l + 1]};
    const std::vector<uint32_t> hm = make_tile_map(ml, 3, 32, true), hm0 = make_tile_map(ml, 1, 32, true);
    const uint32_t *map_new = to_dev(hm), *map0_new = to_dev(hm0);
    tiles = (int)hm.size(); tiles0 = (int)hm0.size();
    t.tile_map = map_new;
    t.map_in_args = pack_tile_map(hm, t.map_words) ? 1 : 0;
    // the regular slots' decode words of the two host-built maps; none for the rectangle grids and for the lines that time a lookup
    const TileHead hd_all = make_tile_head(ml, hm), hd_first = make_tile_head(ml, hm0), hd_none{0, 0};
    printf("head words: all layers %08x %08x, layer 0 alone %08x %08x\n", hd_all.geo, hd_all.kx, hd_first.geo, hd_first.kx);
    printf("tiles: %d (layer 0: %d) with the host-built map, %d (%d) with the rectangles of every layer; %d slabs\n", tiles, tiles0, tiles_old, tiles0_old, ns);
    hipStream_t s; CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    auto time_it = [&](const char *name, int n, auto fn) {
        for (int i = 0; i < 20; i++) fn();
        CK(hipEventRecord(e0, s));
        for (int i = 0; i < n; i++) fn();
        CK(hipEventRecord(e1, s)); CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        printf("%-44s %8.2f us per call\n", name, ms * 1000.f / n);
    };
    {
        TileStepParams o = t; o.tile_map = map_old; o.map_in_args = 0;
        TileStepParams tg = t; tg.map_in_args = 0; // the host-built map read from memory
        time_it("tile_step<grad, update, fwd>, rectangles of every layer", 500, [&]() { LAUNCH((tile_step_kernel<1, 2, true>), tiles_old, o, hd_none); });
        time_it("tile_step<grad, update, fwd>, host-built map in the kernel arguments", 500, [&]() { LAUNCH((tile_step_kernel<1, 2, true>), tiles, t, hd_all); });
        time_it("tile_step<grad, update, fwd>, host-built map read from memory", 500, [&]() { LAUNCH((tile_step_kernel<1, 2, true>), tiles, tg, hd_none); });
        time_it("tile_step<grad, update, fwd>, rectangles of every layer", 500, [&]() { LAUNCH((tile_step_kernel<1, 2, true>), tiles_old, o, hd_none); });
        time_it("tile_step<grad, update, fwd>, host-built map in the kernel arguments", 500, [&]() { LAUNCH((tile_step_kernel<1, 2, true>), tiles, t, hd_all); });
        time_it("tile_step<grad, update, fwd>, host-built map read from memory", 500, [&]() { LAUNCH((tile_step_kernel<1, 2, true>), tiles, tg, hd_none); });
        TileStepParams o0 = t; o0.n_layers = 1; o0.tile_map = map0_old; o0.map_in_args = 0;
        TileStepParams n0 = t; n0.n_layers = 1; n0.tile_map = map0_new; n0.map_in_args = pack_tile_map(hm0, n0.map_words) ? 1 : 0;
        time_it("tile_step<fwd only>, rectangles", 500, [&]() { LAUNCH((tile_step_kernel<0, 0, true>), tiles0_old, o0, hd_none); });
        time_it("tile_step<fwd only>, host-built map", 500, [&]() { LAUNCH((tile_step_kernel<0, 0, true>), tiles0, n0, hd_first); });
    }
    {   // the prologue variants of <grad, update, fwd> on the host-built map, three rounds in turn: the form before (arguments from the
        // struct, every tile by lookup, W and V at the top), A (head arguments, regular slots decoded), B (W and V behind the first
        // barrier), A + B, and A + B + C (the slots that keep the lookup ask for all they need in one batch of scalar loads: the library's kernel).  A round's spread from the next is the probe's own noise.
        for (int rep = 0; rep < 3; rep++) {
            time_it("prologue: struct + lookup, W/V at the top (before)", 1000, [&]() { LAUNCH((tile_step_kernel<1, 2, true, false, false, false>), tiles, t, hd_all); });
            time_it("prologue: A  head arguments + decoded tile", 1000, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, false, false>), tiles, t, hd_all); });
            time_it("prologue: B  W/V behind the first barrier", 1000, [&]() { LAUNCH((tile_step_kernel<1, 2, true, false, true, false>), tiles, t, hd_all); });
            time_it("prologue: A + B", 1000, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, false>), tiles, t, hd_all); });
            time_it("prologue: A + B + C  lookup slots in one scalar batch", 1000, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, true>), tiles, t, hd_all); });
        }
        // Upper bounds, before anything is built: the same launch with one class of workgroups TAKEN OUT of the map (idle entries:
        // the workgroup returns at its top, its tile is not computed).  What a class can give back at most by becoming lighter
        // is what the kernel gains when it is not there at all.
        //   no partial row: layer 0's partial last tile row (19 tiles of 16 weights rows on 784-300-100-10)
        //   no partner of a whole tile: the later-layer tiles in the slots that share a CU with a WHOLE layer-0 tile (slot j and
        //   slot j + 8 * 32 share one)
        auto is_whole = [&](uint32_t e) { return e != ~0u && (e & 15u) == 0 && (int)((e >> 4) & 0x3fffu) * TS_TM + TS_TM <= ld[0]; };
        std::vector<uint32_t> hm_nopart = hm, hm_nopartner = hm;
        int n_part = 0, n_partner = 0;
        for (size_t id = 0; id < hm.size(); id++) {
            if (hm[id] != ~0u && (hm[id] & 15u) == 0 && !is_whole(hm[id])) { hm_nopart[id] = ~0u; n_part++; }
            if (id >= 256 && hm[id] != ~0u && (hm[id] & 15u) != 0 && is_whole(hm[id - 256])) { hm_nopartner[id] = ~0u; n_partner++; }
        }
        TileStepParams t_nopart = t, t_nopartner = t;
        t_nopart.tile_map = to_dev(hm_nopart); t_nopart.map_in_args = pack_tile_map(hm_nopart, t_nopart.map_words) ? 1 : 0;
        t_nopartner.tile_map = to_dev(hm_nopartner); t_nopartner.map_in_args = pack_tile_map(hm_nopartner, t_nopartner.map_words) ? 1 : 0;
        printf("bounds: %d partial-row tiles, %d later-layer tiles that share a CU with a whole layer-0 tile\n", n_part, n_partner);
        //   one per CU: the partial row AND, of every two live slots that share a CU (j and j + 32 of one XCD), the later-layer
        //   tile -- no CU runs two workgroups, no XCD more than 32.  Twice: the entries idled in place (the grid and the head words
        //   of "every tile"), and the live entries of every XCD moved up to the front (a grid of at most 256, head words of its own:
        //   the launch a merged map would make, with the merged workgroups' work left out)
        std::vector<uint32_t> hm_one = hm_nopart;
        int n_one_later = 0, n_one_shared = 0;
        for (size_t id = 256; id < hm_one.size(); id++) {
            if (hm_one[id] == ~0u || hm_one[id - 256] == ~0u) continue;
            if ((hm_one[id] & 15u) != 0) { hm_one[id] = ~0u; n_one_later++; }
            else if ((hm_one[id - 256] & 15u) != 0) { hm_one[id - 256] = ~0u; n_one_later++; }
            else n_one_shared++;
        }
        std::vector<uint32_t> hm_one_c(hm.size(), ~0u); // (as long as hm for the tables below; launched with its live slots only)
        int tiles_one = 0, n_one = 0, max_xcd = 0;
        for (int x = 0; x < 8; x++) {
            int n = 0;
            for (size_t id = x; id < hm_one.size(); id += 8) if (hm_one[id] != ~0u) hm_one_c[(size_t)(n++) * 8 + x] = hm_one[id];
            n_one += n; max_xcd = n > max_xcd ? n : max_xcd;
        }
        tiles_one = max_xcd * 8;
        TileStepParams t_one = t, t_one_c = t;
        t_one.tile_map = to_dev(hm_one); t_one.map_in_args = pack_tile_map(hm_one, t_one.map_words) ? 1 : 0;
        t_one_c.tile_map = to_dev(hm_one_c); t_one_c.map_in_args = pack_tile_map(hm_one_c, t_one_c.map_words) ? 1 : 0;
        const TileHead hd_one_c = make_tile_head(ml, std::vector<uint32_t>(hm_one_c.begin(), hm_one_c.begin() + tiles_one));
        printf("bounds: one per CU takes out %d partial-row and %d later-layer tiles, %d live of %d (most in one XCD: %d, CUs still shared: %d); moved up: a grid of %d, head words %08x %08x\n",
               n_part, n_one_later, n_one, tiles, max_xcd, n_one_shared, tiles_one, hd_one_c.geo, hd_one_c.kx);
        for (int rep = 0; rep < 3; rep++) {
            time_it("bound: every tile (A + B + C)", 1000, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, true>), tiles, t, hd_all); });
            time_it("bound: one per CU, idled in place (A + B + C)", 1000, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, true>), tiles, t_one, hd_all); });
            time_it("bound: one per CU, moved up (A + B + C)", 1000, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, true>), tiles_one, t_one_c, hd_one_c); });
        }
        // what was built on that bound: the merged map (make_merged_tile_map: the partial row in groups, the later layers in
        // pairs, 255 workgroups) and the instance that knows its kinds, against the library's one-tile launch
        bool mm_usable = false;
        std::vector<uint32_t> hmm = make_merged_tile_map(ml, 3, 32, mm_usable);
        const int tiles_m = (int)hmm.size();
        const TileHead hd_m = make_tile_head(ml, hmm);
        TileStepParams t_m = t;
        t_m.tile_map = to_dev(hmm); t_m.map_in_args = pack_tile_map(hmm, t_m.map_words) ? 1 : 0;
        if (hmm.size() < hm.size()) hmm.resize(hm.size(), ~0u); // (as long as hm for the tables below)
        printf("merged: a grid of %d, usable %d, packed %d, head words %08x %08x\n", tiles_m, (int)mm_usable, t_m.map_in_args, hd_m.geo, hd_m.kx);
        for (int rep = 0; rep < 3; rep++) {
            time_it("merged: one tile per workgroup (the parent's launch)", 1000, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, true>), tiles, t, hd_all); });
            time_it("merged: the merged map and kinds", 1000, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, true, true>), tiles_m, t_m, hd_m); });
        }
        for (int rep = 0; rep < 3; rep++) {
            time_it("bound: every tile (A + B)", 1000, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, false>), tiles, t, hd_all); });
            time_it("bound: no partial row", 1000, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, false>), tiles, t_nopart, hd_all); });
            time_it("bound: no partner of a whole tile", 1000, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, false>), tiles, t_nopartner, hd_all); });
            time_it("bound: every tile (A + B + C)", 1000, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, true>), tiles, t, hd_all); });
            time_it("bound: no partial row (A + B + C)", 1000, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, true>), tiles, t_nopart, hd_all); });
            time_it("bound: no partner of a whole tile (A + B + C)", 1000, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, true>), tiles, t_nopartner, hd_all); });
        }
#ifdef TILE_PROBE_STAMPS
        // stamps of the whole layer-0 tiles' workgroups (the heavy ones), cycles from the workgroup's own first stamp, mean and maximum
        auto stamps = [&](const char *name, auto fn) {
            fn(); CK(hipStreamSynchronize(s)); fn(); CK(hipStreamSynchronize(s));
            std::vector<unsigned long long> st(4 * 1024);
            CK(hipMemcpyFromSymbol(st.data(), HIP_SYMBOL(g_stamp), st.size() * 8));
            double sum[4] = {0, 0, 0, 0}, mx[4] = {0, 0, 0, 0}; int n = 0;
            auto whole = [&](int id) { return hm[id] != ~0u && (hm[id] & 15u) == 0 && (int)((hm[id] >> 4) & 0x3fffu) * TS_TM + TS_TM <= ld[0]; };
            // (cycles from the workgroup's OWN first stamp: the counters of two CUs are not comparable)
            for (int id = 0; id < tiles; id++) {
                if (!whole(id)) continue;
                n++;
                for (int k = 1; k < 4; k++) { const double d = (double)(st[k * 1024 + id] - st[id]); sum[k] += d; mx[k] = d > mx[k] ? d : mx[k]; }
            }
            printf("stamps %-44s %d workgroups: first loads issued %6.0f (max %6.0f)  first barrier %6.0f (max %6.0f)  end %6.0f (max %6.0f) cycles\n",
                   name, n, sum[1] / n, mx[1], sum[2] / n, mx[2], sum[3] / n, mx[3]);
        };
        // The same workgroups by CLASS -- a whole layer-0 tile (regular), a tile of layer 0's partial last tile row, a tile of a
        // later layer; each alone on its CU or sharing it with another workgroup of this launch -- on the clock that is
        // comparable across CUs: start and end in us from the launch's first start (10-ns ticks), and which class holds the
        // kernel's last end.  The three cycle stamps are from the workgroup's own first stamp, as above.
        auto classes = [&](const char *name, const std::vector<uint32_t> &hm, auto fn) {
            fn(); CK(hipStreamSynchronize(s)); fn(); CK(hipStreamSynchronize(s));
            std::vector<unsigned long long> st(4 * 1024), rt(4 * 1024); std::vector<unsigned> wh(2 * 1024);
            CK(hipMemcpyFromSymbol(st.data(), HIP_SYMBOL(g_stamp), st.size() * 8));
            CK(hipMemcpyFromSymbol(rt.data(), HIP_SYMBOL(g_real), rt.size() * 8));
            CK(hipMemcpyFromSymbol(wh.data(), HIP_SYMBOL(g_where), wh.size() * 4));
            auto cu_of = [&](int id) { return wh[1024 + id] << 8 | ((wh[id] >> 8) & 0xffu); };
            std::vector<int> on_cu(16 * 256, 0);
            unsigned long long first = ~0ull;
            for (int id = 0; id < tiles; id++) if (hm[id] != ~0u) { on_cu[cu_of(id)]++; first = rt[id] < first ? rt[id] : first; }
            static const char *cname[3] = {"whole layer-0 tile (regular)", "partial last row of layer 0", "tile of a later layer"};
            struct C { int n = 0; double start = 0, end = 0, last = 0, cyc[4] = {0, 0, 0, 0}; int last_id = -1; } c[3][2];
            double kernel_end = 0; int end_cls = 0, end_sh = 0, end_id = -1;
            for (int id = 0; id < tiles; id++) {
                if (hm[id] == ~0u) continue;
                const int li = (int)(hm[id] & 15u), tm = (int)((hm[id] >> 4) & 0x3fffu);
                const int cls = li != 0 ? 2 : (tm * TS_TM + TS_TM <= ld[0] ? 0 : 1), sh = on_cu[cu_of(id)] > 1 ? 1 : 0;
                C &k = c[cls][sh];
                const double b = (double)(rt[id] - first) * 0.01, e = (double)(rt[3 * 1024 + id] - first) * 0.01;
                k.n++; k.start += b; k.end += e;
                if (e > k.last) { k.last = e; k.last_id = id; }
                for (int q = 1; q < 4; q++) k.cyc[q] += (double)(st[q * 1024 + id] - st[id]);
                if (e > kernel_end) { kernel_end = e; end_cls = cls; end_sh = sh; end_id = id; }
            }
            printf("classes %s\n", name);
            for (int cls = 0; cls < 3; cls++) for (int sh = 0; sh < 2; sh++) {
                const C &k = c[cls][sh];
                if (!k.n) continue;
                printf("  %-30s %-8s %3d workgroups: start +%.2f  end mean +%.2f  latest +%.2f (wg%d) us | first loads issued %6.0f  first barrier %6.0f  end %6.0f cycles\n",
                       cname[cls], sh ? "sharing" : "alone", k.n, k.start / k.n, k.end / k.n, k.last, k.last_id, k.cyc[1] / k.n, k.cyc[2] / k.n, k.cyc[3] / k.n);
            }
            printf("  the kernel's last end: +%.2f us, wg%d, %s, %s\n", kernel_end, end_id, cname[end_cls], end_sh ? "sharing its CU" : "alone on its CU");
            return std::vector<unsigned long long>(rt);
        };
        auto pairs = [&](const char *name, const std::vector<uint32_t> &hm, auto fn) { // every CU with two workgroups: [start, end] of each, us from the first start
            const std::vector<unsigned long long> rt = classes(name, hm, fn);
            std::vector<unsigned> wh(2 * 1024);
            CK(hipMemcpyFromSymbol(wh.data(), HIP_SYMBOL(g_where), wh.size() * 4));
            unsigned long long first = ~0ull;
            for (int id = 0; id < tiles; id++) if (hm[id] != ~0u) first = rt[id] < first ? rt[id] : first;
            for (int a = 0; a < tiles; a++) for (int b = a + 1; b < tiles; b++) {
                if (hm[a] == ~0u || hm[b] == ~0u || wh[1024 + a] != wh[1024 + b] || ((wh[a] ^ wh[b]) & 0xff00u)) continue;
                auto show = [&](int id) { printf("  wg%-3d layer %u row %2u [+%.2f, +%.2f]", id, hm[id] & 15u, (hm[id] >> 4) & 0x3fffu, (double)(rt[id] - first) * 0.01, (double)(rt[3 * 1024 + id] - first) * 0.01); };
                printf("  xcc %u cu %02x:", wh[1024 + a], (wh[a] >> 8) & 0xffu); show(a); show(b); printf("\n");
            }
        };
        for (int rep = 0; rep < 3; rep++) {
            classes("A + B", hm, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, false>), tiles, t, hd_all); });
            classes("A + B + C (the library's kernel)", hm, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, true>), tiles, t, hd_all); });
        }
        pairs("A + B, with the CUs that hold two workgroups", hm, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, false>), tiles, t, hd_all); });
        pairs("A + B + C (the library's kernel), with the CUs that hold two workgroups", hm, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, true>), tiles, t, hd_all); });
        classes("bound: no partial row", hm_nopart, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, false>), tiles, t_nopart, hd_all); });
        classes("bound: no partner of a whole tile", hm_nopartner, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, false>), tiles, t_nopartner, hd_all); });
        for (int rep = 0; rep < 2; rep++) {
            classes("bound: one per CU, idled in place (A + B + C)", hm_one, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, true>), tiles, t_one, hd_all); });
            classes("bound: one per CU, moved up (A + B + C)", hm_one_c, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, true>), tiles_one, t_one_c, hd_one_c); });
        }
        for (int rep = 0; rep < 3; rep++)
            classes("merged: the merged map and kinds", hmm, [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, true, true>), tiles_m, t_m, hd_m); });
        for (int rep = 0; rep < 2; rep++) {
            stamps("struct + lookup, W/V at the top (before)", [&]() { LAUNCH((tile_step_kernel<1, 2, true, false, false, false>), tiles, t, hd_all); });
            stamps("A  head arguments + decoded tile", [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, false, false>), tiles, t, hd_all); });
            stamps("B  W/V behind the first barrier", [&]() { LAUNCH((tile_step_kernel<1, 2, true, false, true, false>), tiles, t, hd_all); });
            stamps("A + B", [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, false>), tiles, t, hd_all); });
            stamps("A + B + C", [&]() { LAUNCH((tile_step_kernel<1, 2, true, true, true, true>), tiles, t, hd_all); });
        }
#endif
    }
    {   // a pair as in a real step: the tile kernel followed by a dependent small kernel (what the next launch waits for)
        time_it("pair: tile_step + dependent fwd-only launch", 300, [&]() { LAUNCH((tile_step_kernel<1, 2, true>), tiles, t, hd_all); TileStepParams u = t; u.n_layers = 1; u.tile_map = map0_new; u.map_in_args = pack_tile_map(hm0, u.map_words) ? 1 : 0; LAUNCH((tile_step_kernel<0, 0, true>), tiles0, u, hd_first); });
    }
    {   // a SAMPLED next batch: rows gathered through an index vector from a 6 000-row data set, with and without the contiguous copy
        const int NR = 6000;
        float *big; CK(hipMalloc(&big, (size_t)NR * ld[0] * 4)); CK(hipMemset(big, 0, (size_t)NR * ld[0] * 4));
        std::vector<int32_t> hidx(Bp); for (int i = 0; i < Bp; i++) hidx[i] = rand() % NR;
        int32_t *didx; CK(hipMalloc(&didx, Bp * 4)); CK(hipMemcpy(didx, hidx.data(), Bp * 4, hipMemcpyHostToDevice));
        float *copy; CK(hipMalloc(&copy, (size_t)Bp * ld[0] * 4));
        TileStepParams g = t; g.An = big; g.next_idx = didx;
        TileStepParams gc = g; gc.stage_out = copy;
        TileStepParams seq = t; seq.An = big; // the same data set, rows in place
        for (int rep = 0; rep < 2; rep++) {
            time_it("next batch in place (6 000-row set)", 500, [&]() { LAUNCH((tile_step_kernel<1, 2, true>), tiles, seq, hd_all); });
            time_it("next batch gathered by index", 500, [&]() { LAUNCH((tile_step_kernel<1, 2, true>), tiles, g, hd_all); });
            time_it("next batch gathered + contiguous copy written", 500, [&]() { LAUNCH((tile_step_kernel<1, 2, true>), tiles, gc, hd_all); });
        }
    }
    time_it("tile_step<grad, update>", 500, [&]() { LAUNCH((tile_step_kernel<1, 2, false>), tiles, t, hd_all); });
    time_it("tile_step<grad, store G>", 500, [&]() { LAUNCH((tile_step_kernel<1, 1, false>), tiles, t, hd_all); });
    time_it("tile_step<G, update, fwd>", 500, [&]() { LAUNCH((tile_step_kernel<2, 2, true>), tiles, t, hd_all); });
    time_it("tile_step<fwd only> (layer 0 tiles)", 500, [&]() { TileStepParams u = t; u.n_layers = 1; u.tile_map = map0_new; u.map_in_args = pack_tile_map(hm0, u.map_words) ? 1 : 0; LAUNCH((tile_step_kernel<0, 0, true>), tiles0, u, hd_first); });
    return 0;
}
