// Drives swp::plan_pssm_weights (smith-waterman_amd/csrc/sw_plan.cpp) for tests/test_pssm_weights_plan.py: one case per input line of
// name=value pairs (qlens: a comma-separated list), one JSON object per output line; "hits_*": what swp::plan_pssm_hits gives the same
// queries, letters and device.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../smith-waterman_amd/csrc/sw_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        swp::PssmWeightsJob j;
        std::vector<int64_t> qlens;
        std::istringstream in(line);
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq), val = kv.substr(eq + 1);
            if (k == "qlens") {
                std::istringstream list(val);
                std::string item;
                while (std::getline(list, item, ',')) qlens.push_back(std::stoll(item));
            } else if (k == "nletters") j.queries.nletters = std::stoi(val);
            else if (k == "num_cus") j.queries.num_cus = std::stoi(val);
            else if (k == "top") j.top = std::stoll(val);
            else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 2; }
        }
        j.queries.qlens = qlens.data(); j.queries.nqueries = (int64_t)qlens.size();
        const swp::PssmWeightsPlan p = swp::plan_pssm_weights(j);
        const swp::PssmHitsPlan h = swp::plan_pssm_hits(j.queries);
        printf("{\"stride\": %d, \"tile_cols\": %d, \"max_cols\": %lld, \"tiles_per_query\": %lld, \"grid\": %lld, \"lds_bytes\": %u, \"tile_launches\": %d, "
               "\"finish_grid\": %lld, \"acc_entries\": %lld, \"acc_bytes\": %lld, \"launches\": %d, "
               "\"hits_stride\": %d, \"hits_tile_cols\": %d, \"hits_tiles_per_query\": %lld, \"hits_grid\": %lld, \"hits_lds_bytes\": %u, "
               "\"lds_budget\": %lld, \"code_bytes\": %lld, \"grid_max\": %lld, \"acc_entry_bytes\": %lld}\n",
               p.tiles.stride, p.tiles.tile_cols, (long long)p.tiles.max_cols, (long long)p.tiles.tiles_per_query, (long long)p.tiles.grid, p.tiles.lds_bytes,
               p.tiles.launches, (long long)p.finish_grid, (long long)p.acc_entries, (long long)p.acc_bytes, p.launches, h.stride, h.tile_cols,
               (long long)h.tiles_per_query, (long long)h.grid, h.lds_bytes, (long long)swp::kPssmHitsLdsBytes, (long long)swp::kPssmHitsCodeBytes,
               (long long)swp::kPssmHitsGridMax, (long long)swp::kPssmWeightsAccBytes);
    }
    return 0;
}
