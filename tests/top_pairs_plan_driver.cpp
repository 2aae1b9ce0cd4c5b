// Drives swp::plan_top_pairs (smith-waterman_amd/csrc/sw_plan.cpp) for tests/test_top_pairs_plan.py: one case per input line of
// name=value pairs, one JSON object per output line.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../smith-waterman_amd/csrc/sw_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        swp::TopPairsJob j;
        int64_t budget = 1ll << 30;
        std::istringstream in(line);
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq), val = kv.substr(eq + 1);
            if (k == "npairs") j.npairs = std::stoll(val);
            else if (k == "nqueries") j.nqueries = std::stoll(val);
            else if (k == "ntargets") j.ntargets = std::stoll(val);
            else if (k == "top") j.top = std::stoll(val);
            else if (k == "num_cus") j.num_cus = std::stoi(val);
            else if (k == "budget_bytes") budget = std::stoll(val);
            else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 2; }
        }
        const swp::TopPairsPlan p = swp::plan_top_pairs(j);
        printf("{\"refused\": %s%s%s, \"tbits\": %d, \"lds\": %d, \"grid\": %lld, \"slice\": %lld, \"kernel\": %d, \"T\": %lld, \"items\": %lld, "
               "\"sort_kernel\": %d, \"sort_grid\": %lld, \"launches\": %d, \"keys_need\": %zu, \"pos_need\": %zu, \"seg_need\": %zu, "
               "\"segment_bytes\": %lld, \"top_max\": %lld, \"lds_queries\": %lld, \"min_slice\": %lld, \"sort_grid_max\": %lld, "
               "\"entry_bytes\": %lld, \"prefiltered_cap\": %lld}\n",
               p.refused ? "\"" : "", p.refused ? p.refused : "null", p.refused ? "\"" : "", p.tbits, p.lds ? 1 : 0, (long long)p.grid, (long long)p.slice,
               p.kernel, (long long)p.T, (long long)p.items, p.sort_kernel, (long long)p.sort_grid, p.launches, p.keys_need, p.pos_need, p.seg_need,
               (long long)p.segment_bytes, (long long)swp::kTopMax, (long long)swp::kTopPairsLdsQueries, (long long)swp::kTopPairsMinSlice,
               (long long)swp::kTopPairsSortGrid, (long long)swp::kTopPrefilteredEntryBytes, (long long)swp::top_prefiltered_cap(budget));
    }
    return 0;
}
