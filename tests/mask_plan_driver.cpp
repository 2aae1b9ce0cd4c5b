// Drives swp::plan_mask (smith-waterman_amd/csrc/sw_plan.cpp) for tests/test_mask_plan.py: one case per input line of name=value
// pairs, one JSON object per output line.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../smith-waterman_amd/csrc/sw_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        swp::MaskJob j;
        std::istringstream in(line);
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq), val = kv.substr(eq + 1);
            if (k == "letters") j.letters = std::stoll(val);
            else if (k == "ntargets") j.ntargets = std::stoll(val);
            else if (k == "window") j.window = std::stoi(val);
            else if (k == "count") j.count = std::stoi(val) != 0;
            else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 2; }
        }
        const swp::MaskPlan p = swp::plan_mask(j);
        printf("{\"tile\": %lld, \"starts_per_lane\": %d, \"halo\": %d, \"tiles\": %lld, \"words\": %lld, \"low1_off\": %lld, \"low2_off\": %lld, "
               "\"mask_off\": %lld, \"summary_off\": %lld, \"carry_off\": %lld, \"workspace_bytes\": %lld, \"window_grid\": %lld, \"carry_grid\": %lld, "
               "\"apply_grid\": %lld, \"count_grid\": %lld, \"launches\": %d, \"grid_max\": %lld, \"tile_words\": %lld, \"count_targets\": %d, "
               "\"carry_threads\": %d, \"g_window\": %d}\n",
               (long long)p.tile, p.starts_per_lane, p.halo, (long long)p.tiles, (long long)p.words, (long long)p.low1_off, (long long)p.low2_off,
               (long long)p.mask_off, (long long)p.summary_off, (long long)p.carry_off, (long long)p.workspace_bytes, (long long)p.window_grid,
               (long long)p.carry_grid, (long long)p.apply_grid, (long long)p.count_grid, p.launches, (long long)swp::kPssmHitsGridMax,
               (long long)swp::kMaskTileWords, swp::kMaskCountTargets, swp::kMaskCarryThreads, swp::kMaskG[j.window >= 0 && j.window <= 64 ? j.window : 0]);
    }
    return 0;
}
