// Host-only check of make_merged_tile_map (csrc/tile_step_kernel.h): every tile of every layer is owned by exactly one
// workgroup of the merged map, a unit's columns stay inside one tile row of one layer, a later layer's pairs start at even
// columns, the per-XCD entry counts, and make_tile_head on the merged map slot by slot.  Prints one line of name / value
// pairs.  Compiled and run by tests/test_tile_merge_cpu.py (no GPU).
#include "../../graph-neural-net_amd/csrc/tile_step_kernel.h"
#include <cstdio>
#include <cstdlib>
#include <map>
using namespace gnn;
int main(int argc, char **argv) {
    // usage: tile_merge_check cus_per_xcd d0 d1 .. dL-1   (padded sizes are derived as the library does: multiples of 16)
    if (argc < 4) return 2;
    const int cus = atoi(argv[1]);
    std::vector<int> ld;
    for (int i = 2; i < argc; i++) ld.push_back((atoi(argv[i]) + 15) / 16 * 16);
    std::vector<TileMapLayer> layers;
    for (size_t l = 0; l + 1 < ld.size(); l++) layers.push_back(TileMapLayer{ld[l], ld[l + 1]});
    bool usable = false;
    const std::vector<uint32_t> map = make_merged_tile_map(layers.data(), (int)layers.size(), cus, usable);
    std::map<uint32_t, int> owners; // tile (layer | row << 4 | column << 18) -> workgroups that own it
    size_t expected = 0;
    for (const TileMapLayer &t : layers) expected += (size_t)((t.M + TS_TM - 1) / TS_TM) * (size_t)(t.N / TS_TN);
    int live = 0, out_of_layer = 0, odd_pairs = 0, whole = 0, groups = 0, pairs = 0, singles = 0, max_xcd = 0, whole_not_first = 0;
    int per_xcd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool light_seen[8] = {false, false, false, false, false, false, false, false};
    for (size_t id = 0; id < map.size(); id++) {
        if (map[id] == ~0u) continue;
        live++;
        per_xcd[id & 7]++;
        const int li = (int)(map[id] & 15u), tm = (int)((map[id] >> 4) & 0x3fffu), tn = (int)(map[id] >> 18);
        if (li >= (int)layers.size()) { out_of_layer++; continue; }
        const int tiles_m = (layers[li].M + TS_TM - 1) / TS_TM, tiles_n = layers[li].N / TS_TN;
        const int rows = layers[li].M - tm * TS_TM < TS_TM ? layers[li].M - tm * TS_TM : TS_TM;
        if (tm >= tiles_m || tn >= tiles_n) { out_of_layer++; continue; }
        const bool is_whole = li == 0 && rows > TS_TM / 2;
        const int n = is_whole ? 1 : ts_merged_columns(li, rows, tn, tiles_n); // (what the kernel derives from the entry)
        if (tn + n > tiles_n) out_of_layer++;                                   // a unit never leaves its tile row
        if (li != 0 && (tn & 1)) odd_pairs++;
        if (is_whole) { whole++; whole_not_first += light_seen[id & 7]; }
        else { light_seen[id & 7] = true; if (li == 0) groups++; else if (n == 2) pairs++; else singles++; }
        for (int c = 0; c < n && tn + c < tiles_n; c++) owners[(uint32_t)li | (uint32_t)tm << 4 | (uint32_t)(tn + c) << 18]++;
    }
    int multiply_owned = 0;
    for (const auto &o : owners) multiply_owned += o.second != 1;
    for (int x = 0; x < 8; x++) max_xcd = per_xcd[x] > max_xcd ? per_xcd[x] : max_xcd;
    // make_tile_head on the merged map: every slot the decode claims names its entry
    const TileHead hd = make_tile_head(layers.data(), map);
    int regular = 0, mismatches = 0;
    for (size_t id = 0; id < map.size(); id++) {
        int tm = -1, tn = -1;
        if (!ts_head_tile(hd.geo, hd.kx, (int)id, tm, tn)) continue;
        regular++;
        mismatches += map[id] != ((uint32_t)tm << 4 | (uint32_t)tn << 18);
    }
    uint32_t words[TS_MAP_ARGS / 2];
    const bool packed = pack_tile_map(map, words);
    printf("usable %d grid %zu live %d expected %zu owned %zu multiply_owned %d out_of_layer %d odd_pairs %d max_xcd %d whole %d groups %d pairs %d singles %d "
           "whole_not_first %d plan_regular %d regular %d mismatches %d packed %d\n",
           (int)usable, map.size(), live, expected, owners.size(), multiply_owned, out_of_layer, odd_pairs, max_xcd, whole, groups, pairs, singles,
           whole_not_first, (int)(hd.geo != 0), regular, mismatches, (int)packed);
    return 0;
}
