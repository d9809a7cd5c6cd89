// Host-only check of the tile kernel's lookup-free slots (csrc/tile_step_kernel.h: make_tile_head, ts_head_tile) against the
// map that stays the truth (make_tile_map).  For the map of all layers ("full") and the forward-only map of layer 0 alone
// ("first") it prints how many slots the plan calls regular, how many of them decode to something else than their map entry,
// how many of the other slots the lookup (the packed words when the grid fits them, the table otherwise) does not resolve to
// their entry, and how many layer-0 tiles of whole 64-row height there are / are regular.  Compiled and run by
// tests/test_tile_head_cpu.py (no GPU).
#include "../../graph-neural-net_amd/csrc/tile_step_kernel.h"
#include <cstdio>
#include <cstdlib>
using namespace gnn;
int main(int argc, char **argv) {
    // usage: tile_head_check cus_per_xcd force_mismatch d0 d1 .. dL-1   (padded sizes as the library derives them: multiples of 16)
    if (argc < 5) return 2;
    const int cus = atoi(argv[1]);
    const bool force = atoi(argv[2]) != 0;
    std::vector<int> ld;
    for (int i = 3; i < argc; i++) ld.push_back((atoi(argv[i]) + 15) / 16 * 16);
    std::vector<TileMapLayer> layers;
    for (size_t l = 0; l + 1 < ld.size(); l++) layers.push_back(TileMapLayer{ld[l], ld[l + 1]});
    for (int which = 0; which < 2; which++) {
        const int n_layers = which ? 1 : (int)layers.size();
        const std::vector<uint32_t> map = make_tile_map(layers.data(), n_layers, cus, true);
        const TileHead hd = make_tile_head(layers.data(), map, force);
        uint32_t words[TS_MAP_ARGS / 2];
        const bool packed = pack_tile_map(map, words);
        int regular = 0, mismatches = 0, unresolved = 0, whole = 0, whole_regular = 0;
        for (size_t id = 0; id < map.size(); id++) {
            int tm = -1, tn = -1;
            const bool reg = ts_head_tile(hd.geo, hd.kx, (int)id, tm, tn);
            const bool is_whole = map[id] != ~0u && (map[id] & 15u) == 0 && (int)((map[id] >> 4) & 0x3fffu) * TS_TM + TS_TM <= layers[0].M;
            whole += is_whole;
            if (reg) {
                regular++;
                whole_regular += is_whole;
                mismatches += map[id] != ((uint32_t)tm << 4 | (uint32_t)tn << 18);
            } else { // the kernel's lookup, as tile_step_body.inc reads it
                uint32_t got;
                if (packed) {
                    const uint32_t w = words[id >> 1], e = (id & 1) ? w >> 16 : w & 0xffffu;
                    got = e == 0xffffu ? ~0u : ((e & 7u) | ((e >> 3) & 63u) << 4 | (e >> 9) << 18);
                } else got = map[id];
                unresolved += got != map[id];
            }
        }
        printf("%s grid %zu plan_regular %d regular %d mismatches %d unresolved %d whole %d whole_regular %d\n", which ? "first" : "full",
               map.size(), (int)(hd.geo != 0), regular, mismatches, unresolved, whole, whole_regular);
    }
    return 0;
}
