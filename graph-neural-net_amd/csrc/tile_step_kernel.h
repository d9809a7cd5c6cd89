// tile_step_kernel.h -- the "tile owner" kernel of the small-net path: TWO launches per gradientStep.
//
// A gradientStep (SCE:297-346) has two all-to-all exchanges: the first layer is tiled over the
// columns of W_0 while the chain A_1 -> delta_1 is per batch row, and the weight gradient
// G_l = A_l^T . delta_{l+1} (SCE:253-258, 279-283 summed over the batch by SCE:305-322) is tiled over
// the weight matrix again.  The hop from one step's update to the next step's first layer is NOT
// an exchange: the workgroup that has just updated a tile of W_0 (SCE:333-339) holds exactly the
// weights the next batch's product A_0 . W_0 (SCE:187-192) needs from that tile.  So this kernel,
// for one 64 x 16 tile of one layer's weight matrix:
//
//   GSRC = 1  G = A_l^T . delta_{l+1} over the batch rows            (MFMA, K = batch)
//   GSRC = 2  G = the tile of the all-reduced gradient buffer        (data parallel)
//   GSRC = 3  G = the rank-ordered SUM of the tile in every replica's gradient buffer (data parallel inside the library,
//             GNN_REDUCE_DIRECT: peer pointers -- the reduction, the update and the next step's first layer in ONE launch)
//   GSRC = 4  G = the tile of the REDUCED gradient, each 16-float piece read from the replica that owns its slice
//             (GNN_REDUCE_DIRECT_RS: a reduce-scatter kernel ran before; this launch is the all-gather + update + first layer)
//   GDST = 1  stores G                                               (data parallel: the all-reduce follows)
//   GDST = 2  adj = (step*G)/B + momentum*prev ; W -= adj ; prev = adj
//   FWD       layer 0 only: Zp[b][n] = sum over the tile's 64 input neurons of A_0'[b][m] . W_0[m][n]
//             for the NEXT batch A_0' with the tile's NEW weights -- one K slab of the next step's
//             first-layer sums.  middle4_kernel adds the ceil(d_0/64) slabs in slab order (fixed:
//             results do not depend on dispatch order) and applies f.
//   GSRC = 0, GDST = 0, FWD: the slabs of a batch from the weights as they are (start of a chain).
//
// One step is then { middle4_kernel ; tile_step_kernel } instead of { fwd_first ; middle4 ;
// grad_update }: one dependent launch (~2.5 us fixed on this chip) and the cold re-read of W_0 less.
// The slab arithmetic is the same whether a slab was made by the previous step's tile kernel or by a
// forward-only launch, so a sequence of steps gives bitwise the same weights however it is cut into
// calls.
//
// All contractions on v_mfma_f32_16x16x4_f32 (exact f32).  8 waves:
//   gradient: waves 0..3 -> one m tile of 16 each, product taken transposed (G^T = delta^T . A) so that a lane's
//             accumulator is four consecutive n of one row of the tile: the 16 B of W / V it updates
//   forward : wave -> 16 batch rows of every 128-row chunk; K = the tile's 64 input neurons; A_0' rows go
//             straight to registers in fragment form and the product is taken transposed, so that the
//             slab is stored 16 B per lane from the accumulators (no LDS image, one barrier in all)
#pragma once
#include "fused_kernels.h"
#include "gemm_bf16.h"
#ifndef __HIPCC_RTC__
#include <algorithm>
#include <vector>
#endif

namespace gnn {

constexpr int TS_TM = 64, TS_TN = 16, TS_THREADS = 512, TS_KC = 128;
constexpr int TS_MAX_SLABS = 16; // middle4_kernel keeps one float4 per slab in registers
constexpr int TS_MAX_PEERS = 16; // replicas of one data-parallel handle (dp_handle.h: DP_MAX_REPLICAS)
constexpr int TS_MAP_ARGS = 640; // workgroup -> tile entries that travel in the kernel arguments

struct TileStepParams {
    GradLayer layer[MAX_LAYERS]; // tiling in 64 x 16 tiles; block_begin per layer
    int n_layers;
    int K, k_true;               // padded / live batch rows of the CURRENT batch (gradient)
    float step_over_b, momentum;
    const int32_t *row_idx;      // optional, layer 0: batch row k of A_0 is dataset row row_idx[k]
    // next batch (FWD), layer 0 only
    const float *An; int ldan;   // A_0' rows
    const int32_t *next_idx;     // optional row indices of the next batch
    int next_rows, next_K;       // live / padded rows of the next batch
    float *slabs;                // [n slabs][slab_rows][ldz]
    int slab_rows, ldz;
    // GNN_DTYPE_BF16 (tile_step_bf16_kernel): the bf16 roundings of the operands, same shapes and leading dimensions
    const __bf16 *Ab[MAX_LAYERS]; const __bf16 *Db[MAX_LAYERS]; __bf16 *Wb[MAX_LAYERS];
    const __bf16 *Anb;
    // A sampled next batch (next_idx != null): the workgroups of tile column 0 also write the rows they fetched to a
    // contiguous copy [next_K][ldan] (f32 or bf16 by kernel), which the NEXT step's gradient product then reads in place of
    // the index-gathered rows -- no dependent index load at the start of that kernel.  Null = no copy.
    float *stage_out; __bf16 *stage_out_b;
    // GSRC = 3 / 4: every replica's gradient buffer (3: partial gradients, 4: reduced slices), rank order; Gself = the base
    // of THIS replica's bound gradient buffer (layer[l].G - Gself is the layer's offset in every peer's buffer); slice =
    // floats per owner (a multiple of 16), GSRC = 4 only
    const float *Gpeer[TS_MAX_PEERS]; int n_peer; const float *Gself; unsigned slice;
    // workgroup -> tile: layer | tile row << 4 | tile column << 18, ~0 = idle (make_tile_map below)
    const uint32_t *tile_map;
    // the same map inside the kernel arguments, 16 bits per workgroup (layer | row << 3 | column << 9, 0xffff = idle), when
    // the grid has at most TS_MAP_ARGS entries: the entry then arrives with the first batch of scalar loads instead of
    // one more round trip to memory in front of everything a workgroup does (~700 cycles in tools/tile_probe's stamps)
    int map_in_args;
    uint32_t map_words[TS_MAP_ARGS / 2];
};

// Which workgroup takes which tile.  The dispatcher deals workgroup i to XCD i % 8 and, inside an XCD, the j-th of them to
// the CU that also gets the (j + 32)-th (tools/tile_probe: HW_ID of every workgroup): with 284 live tiles for 256 CUs, 28 CUs
// run two workgroups, and a pair of full layer-0 tiles took 5.2 us where a workgroup alone takes 4.0 -- the pair, not
// the tile, set the kernel's duration.  The per-layer rectangles of XcdTiling also left two XCDs almost empty (a 13th tile
// row of 16 weights) while the others ran 36-40 tiles on 32 CUs, idle blocks in the grid taking CU slots of live ones.
// So the map is built on the host, tile by tile:
//   * full layer-0 tiles ("heavy": gradient + update + the next batch's slab) go to the XCD of their rectangle
//     (panels shared through that XCD's L2); every other tile (a partial last row, the small layers) to the XCD with the
//     fewest tiles so far;
//   * inside an XCD the lightest tiles take the slots that share a CU -- the first k and the last k when it has
//     cus_per_xcd + k tiles -- and idle entries, if any, come last.
// Placement changes which tile a workgroup computes and nothing else: results do not depend on it.
struct TileMapLayer { int M, N; }; // padded rows / columns of W_l
inline std::vector<uint32_t> make_tile_map(const TileMapLayer *layers, int n_layers, int cus_per_xcd, bool next_batch_slabs) {
    struct T { uint32_t e; int w; };
    std::vector<T> per_xcd[8];
    long load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<T> light;
    for (int l = 0; l < n_layers; l++) {
        const int tiles_m = (layers[l].M + TS_TM - 1) / TS_TM, tiles_n = layers[l].N / TS_TN;
        int full_m = 0; // tile rows that count as heavy: layer 0, more than half a tile of weights
        if (l == 0) for (int tm = 0; tm < tiles_m; tm++) if (layers[l].M - tm * TS_TM > TS_TM / 2) full_m = tm + 1;
        const XcdTiling rect = full_m > 0 ? make_xcd_tiling(full_m, tiles_n) : XcdTiling{};
        for (int tm = 0; tm < tiles_m; tm++)
            for (int tn = 0; tn < tiles_n; tn++) {
                const int rows = layers[l].M - tm * TS_TM < TS_TM ? layers[l].M - tm * TS_TM : TS_TM;
                // cost, measured (tools/tile_probe): a layer-0 tile takes ~4.0 us whatever its height (the next batch's slab is
                // formed over all 128 rows either way), a tile of a later layer ~2.5 us
                const T t{(uint32_t)l | (uint32_t)tm << 4 | (uint32_t)tn << 18, (l == 0 && next_batch_slabs) ? 100 + rows / 4 : rows};
                if (l == 0 && tm < full_m) {
                    const int x = (tm / rect.rm) * rect.xn + tn / rect.rn;
                    per_xcd[x].push_back(t);
                    load[x] += t.w;
                } else light.push_back(t);
            }
    }
    std::stable_sort(light.begin(), light.end(), [](const T &a, const T &b) { return a.w > b.w; });
    for (const T &t : light) { // heaviest first, each to the XCD with the fewest tiles (ties: the least work, then the lowest id)
        int best = 0;
        for (int x = 1; x < 8; x++)
            if (per_xcd[x].size() < per_xcd[best].size() || (per_xcd[x].size() == per_xcd[best].size() && load[x] < load[best])) best = x;
        per_xcd[best].push_back(t);
        load[best] += t.w;
    }
    size_t slots = 0;
    for (int x = 0; x < 8; x++) slots = per_xcd[x].size() > slots ? per_xcd[x].size() : slots;
    std::vector<uint32_t> map(slots * 8, ~0u);
    for (int x = 0; x < 8; x++) {
        std::vector<T> &v = per_xcd[x];
        const int n = (int)v.size(), k = n > cus_per_xcd ? (n - cus_per_xcd < n / 2 ? n - cus_per_xcd : n / 2) : 0;
        std::vector<int> order(n);
        for (int i = 0; i < n; i++) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return v[a].w < v[b].w; }); // lightest first
        std::vector<char> is_light(n, 0);
        std::vector<uint32_t> seq;
        for (int i = k; i < 2 * k; i++) { seq.push_back(v[order[i]].e); is_light[order[i]] = 1; } // slots 0 .. k-1
        for (int i = 0; i < k; i++) is_light[order[i]] = 1;
        for (int i = 0; i < n; i++) if (!is_light[i]) seq.push_back(v[i].e);                       // the rest, in rectangle order
        for (int i = 0; i < k; i++) seq.push_back(v[order[i]].e);                                  // the last k: the lightest of all
        for (int j = 0; j < n; j++) map[(size_t)j * 8 + x] = seq[j];
    }
    return map;
}
// the 16-bit form for the kernel arguments; false when the grid or a field does not fit
inline bool pack_tile_map(const std::vector<uint32_t> &map, uint32_t (&words)[TS_MAP_ARGS / 2]) {
    if (map.size() > (size_t)TS_MAP_ARGS) return false;
    for (uint32_t &w : words) w = 0xffffffffu;
    for (size_t i = 0; i < map.size(); i++) {
        uint32_t e16 = 0xffffu;
        if (map[i] != ~0u) {
            const uint32_t li = map[i] & 15u, tm = (map[i] >> 4) & 0x3fffu, tn = map[i] >> 18;
            if (li > 7 || tm > 63 || tn > 126) return false;
            e16 = li | tm << 3 | tn << 9;
        }
        words[i >> 1] = (i & 1) ? ((words[i >> 1] & 0x0000ffffu) | e16 << 16) : ((words[i >> 1] & 0xffff0000u) | e16);
    }
    return true;
}

// ---- the regular slots: workgroup -> tile WITHOUT a lookup ------------------------------------------------------------
// make_tile_map puts the full layer-0 tiles of XCD x in the order of x's rectangle (row-major inside it), behind the
// slots at the front that share a CU (an XCD with fewer light tiles than such slots gives them the FIRST tiles of its
// rectangle -- the order goes on from there; k_x is the slot of the rectangle's first tile).  For those slots the tile is arithmetic in the workgroup's id and two dwords that
// travel as leading kernel arguments (GNN_TS_HEAD_PARAMS below: preloaded into SGPRs), so a full layer-0 workgroup -- the
// heavy ones, 228 of 284 on 784-300-100-10 -- forms the addresses of its first vector loads with no scalar load at all:
//   geo = rm | rn << 6 | xs << 14 | full_m << 16 | tiles_n << 23   (the rectangles of make_xcd_tiling(full_m, tiles_n))
//   kx  = k_x, four bits per XCD
// Every other slot (the pair slots, the small layers, a partial last tile row, idle entries) keeps the lookup -- on the kernels
// with the head prologue as ONE batch of scalar loads (tile_step_body.inc, TS_LOOKUP1: the flag, the map word, layer 1's
// descriptor; layer 0's descriptor from the head arguments), not one dependent round trip after the other.  The MAP
// stays the truth: make_tile_head evaluates the decode for every slot and hands out {0, 0} -- no regular slot -- unless
// each slot the decode claims names exactly its map entry.
struct TileHead { uint32_t geo, kx; };
// id -> (tm, tn) of a regular slot; false: not regular, use the lookup.  No integer division: j / w through the
// reciprocal.  (j + 0.5) / w is at least 0.5 / w >= 2^-9 away from an integer and below rm <= 63, so a relative error of
// a few 2^-24 (the device's v_rcp_f32 is good to 1 ulp, the host divides) moves it by less than 2^-16: the same
// integer on both sides.
__host__ __device__ __forceinline__ bool ts_head_tile(uint32_t geo, uint32_t kx, int id, int &tm, int &tn) {
    const int rm = (int)(geo & 63u), rn = (int)((geo >> 6) & 255u), xs = (int)((geo >> 14) & 3u);
    const int full_m = (int)((geo >> 16) & 127u), tiles_n = (int)(geo >> 23);
    const int x = id & 7, j = (id >> 3) - (int)((kx >> (4 * x)) & 15u);
    const int r0 = (x >> xs) * rm, c0 = (x & ((1 << xs) - 1)) * rn;
    const int h = full_m - r0 < rm ? full_m - r0 : rm, w = tiles_n - c0 < rn ? tiles_n - c0 : rn; // (clipped at the matrix edge)
    if (j < 0 || h <= 0 || w <= 0 || j >= h * w) return false;
#if defined(__HIP_DEVICE_COMPILE__)
    const int q = (int)(((float)j + 0.5f) * __builtin_amdgcn_rcpf((float)w));
#else
    const int q = (int)(((float)j + 0.5f) * (1.0f / (float)w));
#endif
    tm = r0 + q; tn = c0 + (j - q * w);
    return true;
}
// the two words of a map made by make_tile_map(layers, ...); {0, 0} when a field does not fit, a k_x is
// above 15, or one slot the decode calls regular is not the map's entry (force_mismatch: tests only)
inline TileHead make_tile_head(const TileMapLayer *layers, const std::vector<uint32_t> &map, bool force_mismatch = false) {
    const int tiles_m = (layers[0].M + TS_TM - 1) / TS_TM, tiles_n = layers[0].N / TS_TN;
    int full_m = 0;
    for (int tm = 0; tm < tiles_m; tm++) if (layers[0].M - tm * TS_TM > TS_TM / 2) full_m = tm + 1;
    if (full_m == 0 || map.empty() || map.size() % 8 != 0) return TileHead{0, 0};
    const XcdTiling rect = make_xcd_tiling(full_m, tiles_n);
    if (rect.rm > 63 || rect.rn > 255 || rect.xs > 3 || full_m > 127 || tiles_n > 511) return TileHead{0, 0};
    TileHead hd{(uint32_t)rect.rm | (uint32_t)rect.rn << 6 | (uint32_t)rect.xs << 14 | (uint32_t)full_m << 16 | (uint32_t)tiles_n << 23, 0};
    for (int x = 0; x < 8; x++) { // k_x: the slot of the rectangle's first tile
        const int r0 = (x >> rect.xs) * rect.rm, c0 = (x & (rect.xn - 1)) * rect.rn;
        if (r0 >= full_m || c0 >= tiles_n) continue; // (a rectangle past the matrix edge: no tile, no regular slot)
        size_t k = 0;
        while (k * 8 < map.size() && map[k * 8 + x] != ((uint32_t)r0 << 4 | (uint32_t)c0 << 18)) k++;
        if (k > 15) return TileHead{0, 0};
        hd.kx |= (uint32_t)k << (4 * x);
    }
    if (force_mismatch) hd.kx ^= 1u;
    for (size_t id = 0; id < map.size(); id++) {
        int tm = 0, tn = 0;
        if (ts_head_tile(hd.geo, hd.kx, (int)id, tm, tn) && map[id] != ((uint32_t)tm << 4 | (uint32_t)tn << 18)) return TileHead{0, 0};
    }
    return hd;
}

// ---- the merged map: light tiles share a workgroup, so that no CU runs two -----------------------------------------
// make_tile_map gives 784-300-100-10 284 live workgroups for 256 CUs, and the second workgroup of a shared CU decides when
// the kernel ends.  The light tiles do not fill a workgroup: a tile of layer 0's partial last tile row (16 or 32 weight rows)
// uses one or two of the four gradient waves, a tile of a later layer has no forward half.  Here
//   * a whole layer-0 tile (more than 32 rows) keeps its workgroup and the XCD of its rectangle, in rectangle order;
//   * the partial last tile row of layer 0, h = 16 or 32 rows high: one workgroup owns 64 / h adjacent column tiles (the last
//     group of the row may be short); the entry names the first of them;
//   * a later layer: one workgroup owns columns tn and tn + 1 of one tile row, tn even (the last column of an odd count
//     stays single);
// and every unit that is not a whole layer-0 tile goes to the XCD with the fewest entries, behind that XCD's whole tiles.
// The entry formats are make_tile_map's; which kind a slot is follows from (layer, tile row) and how many columns it owns
// from the layer's width (ts_merged_columns).  usable: no XCD holds more than cus_per_xcd entries, so that a grid of the
// map's size puts one workgroup on a CU; a map that is not usable is still complete, and not launched (plan.hip).
// 784-300-100-10: 228 + 5 + 20 + 2 = 255 entries in a grid of 256.
template <int V> struct ts_int { static constexpr int value = V; }; // (a count as a type: tile_step_body.inc, one body per height of a group)
__host__ __device__ __forceinline__ int ts_merged_columns(int li, int rows, int tn, int tiles_n) { // columns the unit at (li, tn) owns; rows: the tile row's height
    const int want = li != 0 ? 2 : rows <= TS_TM / 4 ? 4 : rows <= TS_TM / 2 ? 2 : 1;
    return tiles_n - tn < want ? tiles_n - tn : want;
}
inline std::vector<uint32_t> make_merged_tile_map(const TileMapLayer *layers, int n_layers, int cus_per_xcd, bool &usable) {
    struct T { uint32_t e; int w; };
    std::vector<uint32_t> per_xcd[8];
    long load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<T> light;
    for (int l = 0; l < n_layers; l++) {
        const int tiles_m = (layers[l].M + TS_TM - 1) / TS_TM, tiles_n = layers[l].N / TS_TN;
        int full_m = 0; // (as in make_tile_map)
        if (l == 0) for (int tm = 0; tm < tiles_m; tm++) if (layers[l].M - tm * TS_TM > TS_TM / 2) full_m = tm + 1;
        const XcdTiling rect = full_m > 0 ? make_xcd_tiling(full_m, tiles_n) : XcdTiling{};
        for (int tm = 0; tm < tiles_m; tm++) {
            const int rows = layers[l].M - tm * TS_TM < TS_TM ? layers[l].M - tm * TS_TM : TS_TM;
            const bool whole = l == 0 && tm < full_m;
            for (int tn = 0; tn < tiles_n; tn += whole ? 1 : ts_merged_columns(l, rows, tn, tiles_n)) {
                const uint32_t e = (uint32_t)l | (uint32_t)tm << 4 | (uint32_t)tn << 18;
                if (whole) {
                    const int x = (tm / rect.rm) * rect.xn + tn / rect.rn;
                    per_xcd[x].push_back(e);
                    load[x] += 100 + rows / 4;
                } else light.push_back(T{e, (l == 0 ? 100 : 0) + rows * ts_merged_columns(l, rows, tn, tiles_n) / 4});
            }
        }
    }
    std::stable_sort(light.begin(), light.end(), [](const T &a, const T &b) { return a.w > b.w; });
    for (const T &t : light) { // heaviest first, each to the XCD with the fewest entries (ties: the least work, then the lowest id)
        int best = 0;
        for (int x = 1; x < 8; x++)
            if (per_xcd[x].size() < per_xcd[best].size() || (per_xcd[x].size() == per_xcd[best].size() && load[x] < load[best])) best = x;
        per_xcd[best].push_back(t.e);
        load[best] += t.w;
    }
    size_t slots = 0;
    for (int x = 0; x < 8; x++) slots = per_xcd[x].size() > slots ? per_xcd[x].size() : slots;
    usable = slots <= (size_t)cus_per_xcd;
    std::vector<uint32_t> map(slots * 8, ~0u);
    for (int x = 0; x < 8; x++)
        for (size_t j = 0; j < per_xcd[x].size(); j++) map[j * 8 + x] = per_xcd[x][j];
    return map;
}

// 16-B store that is written THROUGH the XCD's L2 (sc1): the line does not stay dirty, so the end of the kernel has nothing
// to write back for it (a kernel boundary costs ~B / 6 TB/s for B dirty bytes, MI355X_MICROARCH.md, row `boundary`), and the
// bytes leave while the kernel still runs.  Inline asm (the compiler has no spelling for it on a 16-B vector); the s_nop
// covers the store-data hazard the compiler cannot see.
// (The value must come out of an ordinary vector instruction.  Stored straight from an MFMA's destination registers the
//  asm statement read them before the matrix pipe had written them -- the wait states between an MFMA and a memory
//  instruction that reads its result are the compiler's to insert, and it cannot see into inline asm: the bf16 kernel's
//  slabs came out as garbage that changed from run to run.  ts_mfma_result() supplies them.)
__device__ __forceinline__ void ts_mfma_result(f32x4 &v) { asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" : "+v"(v)); }
__device__ __forceinline__ void ts_store16(float *dst, f32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(dst), "v"(v) : "memory");
}

// the gradient tile's 16 B of this lane when it does not come from this launch's own product
template <int GSRC> __device__ __forceinline__ float4 ts_gradient_in(const TileStepParams &p, const GradLayer &L, size_t e_off, bool e_ok) {
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!e_ok) return g;
    if (GSRC == 2) {
        g = *reinterpret_cast<const float4 *>(L.G + e_off);
    } else if (GSRC == 3) {
        const size_t off = (size_t)(L.G - p.Gself) + e_off;
        g = *reinterpret_cast<const float4 *>(p.Gpeer[0] + off);
#pragma unroll
        for (int r = 1; r < TS_MAX_PEERS; r++) {
            if (r < p.n_peer) { // (block-uniform; rank order: the same bits on every replica)
                const float4 o = *reinterpret_cast<const float4 *>(p.Gpeer[r] + off);
                g.x += o.x; g.y += o.y; g.z += o.z; g.w += o.w;
            }
        }
    } else if (GSRC == 4) {
        const size_t off = (size_t)(L.G - p.Gself) + e_off;
        const unsigned owner = (unsigned)off / p.slice; // (a 16-float row piece never straddles two owners)
        const float *src = p.Gpeer[0];
#pragma unroll
        for (int r = 1; r < TS_MAX_PEERS; r++) src = (owner == (unsigned)r) ? p.Gpeer[r] : src;
        g = *reinterpret_cast<const float4 *>(src + off);
    }
    return g;
}

// The slabs and the updated masters are stored write-through (ts_store16).

// The arguments a layer-0 workgroup's FIRST instructions need travel ahead of the struct (the library is built
// with -mllvm -amdgpu-kernarg-preload-count=16, as for GNN_RB_HEAD_PARAMS in rowblock_kernel.h): layer 0's A, D, W, V (the
// bf16 kernel: its bf16 A and D in the first two slots), lda, ldd, M, hd_Kr = the padded batch rows (a multiple of 16) | 1
// when a row index is in use, and the two words of ts_head_tile.  FOURTEEN dwords, and no more: of the 16 user SGPRs the
// kernel-argument pointer takes two, and a fifteenth argument came back as a scalar load in front of the decode.  As fields of the by-value struct they came through the scalar cache from a
// kernel-argument line nothing had touched, in front of the first vector load.  Everything else -- what the forward half
// needs behind the barrier included -- stays in the struct; so does the descriptor of every slot that is not regular.
// HEAD = false (GNN_MLP_TILE_HEAD=0): the prologue as it was, every argument from the struct and every tile from the
// lookup -- the reference point of the bitwise test.  DEFER_WV, LOOKUP1 (off only in tools/tile_probe's comparisons): tile_step_body.inc.
// A launch passes the head, then p.
#define GNN_TS_HEAD_PARAMS const float *hd_A, const float *hd_D, float *hd_W, float *hd_V, int hd_lda, int hd_ldd, int hd_M, int hd_Kr, uint32_t hd_geo, uint32_t hd_kx
#define TS_HEAD_PROLOGUE 1
#define TS_HEAD HEAD
#define TS_DEFER_WV DEFER_WV
#define TS_LOOKUP1 LOOKUP1
// MERGE: the workgroup kinds of make_merged_tile_map (tile_step_body.inc, TS_MERGE_KINDS) -- on in ONE instance, the f32
// training form <1, 2, true> of a single net (launch_small.hip); every other instance compiles to the code it had
#define TS_MERGE_KINDS 1
#define TS_MERGE MERGE
#ifndef TS_STAMP
#define TS_STAMP(slot) // (tools/tile_probe.hip defines it in its stamped build; nothing is stamped in the library)
#endif
#define TS_BID blockIdx.x
#define TS_REL(q) (q)
#define TS_REL_LAYER(L)
#define TS_STEP_OVER_B p.step_over_b
#define TS_MOMENTUM p.momentum
#define TS_K (HEAD ? (hd_Kr & ~1) : p.K)
#define TS_K_TRUE p.k_true
#define TS_HAS_ROW_IDX (HEAD ? (hd_Kr & 1) != 0 : p.row_idx != nullptr)
#define TS_STAGE_N p.layer[0].N // (layer 0's N where it is used, behind the barrier: as a field of L its scalar load was waited for at the top)
#define TS_NEXT_ROWS p.next_rows
#define TS_NEXT_K p.next_K
template <int GSRC, int GDST, bool FWD, bool HEAD = true, bool DEFER_WV = true, bool LOOKUP1 = HEAD, bool MERGE = false>
__global__ __launch_bounds__(TS_THREADS) void tile_step_kernel(GNN_TS_HEAD_PARAMS, TileStepParams p) {
#include "tile_step_body.inc"
}

// ------------------------------------------------------------------------------------------------
// tile_step_bf16_kernel: the same tile owner with bf16 GEMM operands (GNN_DTYPE_BF16): activations, deltas,
// next-batch rows and the weight tile enter the two products as bf16 (written once by their producers), both
// products run on v_mfma_f32_16x16x32_bf16 with f32 accumulation, the update is on the f32 masters and the
// tile's new weights go back to the bf16 shadow.  128 f32 MFMAs per tile become 16 (gradient) + 16 (forward);
// the operand images are half the bytes.  Both gradient operands are k-major ([batch row][neuron]): staged as
// they are and read with ds_read_b64_tr_b16; the weight tile [m][n] is k-major for the forward product too.
// ------------------------------------------------------------------------------------------------

template <int GSRC, int GDST, bool FWD, bool HEAD = true>
__global__ __launch_bounds__(TS_THREADS) void tile_step_bf16_kernel(GNN_TS_HEAD_PARAMS, TileStepParams p) {
#include "tile_step_bf16_body.inc"
}
#undef TS_HEAD_PROLOGUE
#undef TS_HEAD
#undef TS_DEFER_WV
#undef TS_LOOKUP1
#undef TS_MERGE_KINDS
#undef TS_MERGE
#undef TS_HAS_ROW_IDX
#undef TS_STAGE_N
#undef TS_BID
#undef TS_REL
#undef TS_REL_LAYER
#undef TS_STEP_OVER_B
#undef TS_MOMENTUM
#undef TS_K
#undef TS_K_TRUE
#undef TS_NEXT_ROWS
#undef TS_NEXT_K

} // namespace gnn
