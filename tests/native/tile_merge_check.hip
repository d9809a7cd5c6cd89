// Host-only check of make_merged_tile_map (csrc/tile_step_kernel.h): every tile of every layer is owned by exactly one
// workgroup of the merged map, a unit's columns stay inside one tile row of one layer, a later layer's pairs start at even
// columns, the per-XCD entry counts, and make_tile_head on the merged map slot by slot.  Three forms:
//   tile_merge_check cus_per_xcd d0 d1 .. dL-1           one line of name / value pairs
//   tile_merge_check entries cus_per_xcd d0 d1 .. dL-1   one line per live entry ("e" id layer tile-row tile-column kind height
//                                                        columns-owned live-rows; kind 0 whole, 1 group, 2 pair, 3 single), then the
//                                                        name / value line with make_rb_plan's verdict ("rb_ok") in front
//   tile_merge_check sweep                               every padded first width 16..1024 x second width 16..384 x three tails x
//                                                        4, 8 and 32 CUs per XCD: "maps" and the count of "violations" of the invariants
// Compiled and run by tests/test_tile_merge_cpu.py and tests/test_tile_merge_cases_cpu.py (no GPU).
#include "../../graph-neural-net_amd/csrc/tile_step_kernel.h"
#include "../../graph-neural-net_amd/csrc/rowblock_kernel.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
using namespace gnn;

struct Report {
    int usable = 0, live = 0, out_of_layer = 0, odd_pairs = 0, whole = 0, groups = 0, pairs = 0, singles = 0, max_xcd = 0, whole_not_first = 0;
    int multiply_owned = 0, plan_regular = 0, regular = 0, mismatches = 0, packed = 0;
    size_t grid = 0, expected = 0, owned = 0;
    // what the tests call a violation: a tile without exactly one owner, a unit outside its tile row or layer, a pair at an odd
    // column, usable that is not (max_xcd <= cus), a regular slot of make_tile_head that is not the map's entry
    int violations(int cus) const {
        return (owned != expected) + multiply_owned + out_of_layer + odd_pairs + (usable != (max_xcd <= cus)) + mismatches;
    }
};

// d: the true widths (padded as the library does: multiples of 16); entries: print one line per live entry
static Report check(const std::vector<int> &d, int cus, bool entries) {
    Report r;
    std::vector<TileMapLayer> layers;
    for (size_t l = 0; l + 1 < d.size(); l++) layers.push_back(TileMapLayer{(d[l] + 15) / 16 * 16, (d[l + 1] + 15) / 16 * 16});
    bool usable = false;
    const std::vector<uint32_t> map = make_merged_tile_map(layers.data(), (int)layers.size(), cus, usable);
    r.usable = usable;
    r.grid = map.size();
    std::map<uint32_t, int> owners; // tile (layer | row << 4 | column << 18) -> workgroups that own it
    for (const TileMapLayer &t : layers) r.expected += (size_t)((t.M + TS_TM - 1) / TS_TM) * (size_t)(t.N / TS_TN);
    int per_xcd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool light_seen[8] = {false, false, false, false, false, false, false, false};
    for (size_t id = 0; id < map.size(); id++) {
        if (map[id] == ~0u) continue;
        r.live++;
        per_xcd[id & 7]++;
        const int li = (int)(map[id] & 15u), tm = (int)((map[id] >> 4) & 0x3fffu), tn = (int)(map[id] >> 18);
        if (li >= (int)layers.size()) { r.out_of_layer++; continue; }
        const int tiles_m = (layers[li].M + TS_TM - 1) / TS_TM, tiles_n = layers[li].N / TS_TN;
        const int rows = layers[li].M - tm * TS_TM < TS_TM ? layers[li].M - tm * TS_TM : TS_TM;
        if (tm >= tiles_m || tn >= tiles_n) { r.out_of_layer++; continue; }
        const bool is_whole = li == 0 && rows > TS_TM / 2;
        const int n = is_whole ? 1 : ts_merged_columns(li, rows, tn, tiles_n); // (what the kernel derives from the entry)
        if (tn + n > tiles_n) r.out_of_layer++;                                 // a unit never leaves its tile row
        if (li != 0 && (tn & 1)) r.odd_pairs++;
        int kind = 0;
        if (is_whole) { r.whole++; r.whole_not_first += light_seen[id & 7]; }
        else {
            light_seen[id & 7] = true;
            if (li == 0) { r.groups++; kind = 1; } else if (n == 2) { r.pairs++; kind = 2; } else { r.singles++; kind = 3; }
        }
        for (int c = 0; c < n && tn + c < tiles_n; c++) owners[(uint32_t)li | (uint32_t)tm << 4 | (uint32_t)(tn + c) << 18]++;
        if (entries) {
            const int live_rows = d[li] - tm * TS_TM < rows ? d[li] - tm * TS_TM : rows; // weight rows that are not padding
            printf("e %zu %d %d %d %d %d %d %d\n", id, li, tm, tn, kind, rows, n, live_rows);
        }
    }
    r.owned = owners.size();
    for (const auto &o : owners) r.multiply_owned += o.second != 1;
    for (int x = 0; x < 8; x++) r.max_xcd = per_xcd[x] > r.max_xcd ? per_xcd[x] : r.max_xcd;
    // make_tile_head on the merged map: every slot the decode claims names its entry
    const TileHead hd = make_tile_head(layers.data(), map);
    r.plan_regular = hd.geo != 0;
    for (size_t id = 0; id < map.size(); id++) {
        int tm = -1, tn = -1;
        if (!ts_head_tile(hd.geo, hd.kx, (int)id, tm, tn)) continue;
        r.regular++;
        r.mismatches += map[id] != ((uint32_t)tm << 4 | (uint32_t)tn << 18);
    }
    uint32_t words[TS_MAP_ARGS / 2];
    r.packed = pack_tile_map(map, words);
    return r;
}

static void print(const Report &r) {
    printf("usable %d grid %zu live %d expected %zu owned %zu multiply_owned %d out_of_layer %d odd_pairs %d max_xcd %d whole %d groups %d pairs %d singles %d "
           "whole_not_first %d plan_regular %d regular %d mismatches %d packed %d\n",
           r.usable, r.grid, r.live, r.expected, r.owned, r.multiply_owned, r.out_of_layer, r.odd_pairs, r.max_xcd, r.whole, r.groups, r.pairs, r.singles,
           r.whole_not_first, r.plan_regular, r.regular, r.mismatches, r.packed);
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "sweep")) {
        const std::vector<std::vector<int>> tails = {{16}, {48, 16}, {128, 80, 16}};
        long maps = 0, violations = 0;
        for (int cus : {4, 8, 32})
            for (int m0 = 16; m0 <= 1024; m0 += 16)
                for (int n1 = 16; n1 <= 384; n1 += 16)
                    for (const std::vector<int> &tail : tails) {
                        std::vector<int> d = {m0, n1};
                        d.insert(d.end(), tail.begin(), tail.end());
                        violations += check(d, cus, false).violations(cus);
                        maps++;
                    }
        printf("maps %ld violations %ld\n", maps, violations);
        return 0;
    }
    const bool entries = argc > 1 && !strcmp(argv[1], "entries");
    const int first = entries ? 2 : 1;
    if (argc < first + 3) return 2;
    const int cus = atoi(argv[first]);
    std::vector<int> d;
    for (int i = first + 1; i < argc; i++) d.push_back(atoi(argv[i]));
    const Report r = check(d, cus, entries);
    if (entries) printf("rb_ok %d ", (int)make_rb_plan(d.data(), (int)d.size()).ok);
    print(r);
    return 0;
}
