// Drives swp::plan_msa_filter (smith-waterman_amd/csrc/sw_plan.cpp) for tests/test_msa_filter_plan.py: one case per input line of
// name=value pairs, one JSON object per output line; with tiles=1 the (row block, compared block) of every tile of a query.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../smith-waterman_amd/csrc/sw_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        swp::MsaFilterJob j;
        bool tiles = false;
        std::istringstream in(line);
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq), val = kv.substr(eq + 1);
            if (k == "nqueries") j.nqueries = std::stoll(val);
            else if (k == "top") j.top = std::stoll(val);
            else if (k == "budget_bytes") j.budget_bytes = std::stoll(val);
            else if (k == "tiles") tiles = std::stoi(val) != 0;
            else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 2; }
        }
        const swp::MsaFilterPlan p = swp::plan_msa_filter(j);
        printf("{\"blocks\": %lld, \"tiles_per_query\": %lld, \"chunk_cols\": %d, \"query_words\": %lld, \"query_bytes\": %lld, \"queries_per_chunk\": %lld, "
               "\"chunks\": %lld, \"workspace_bytes\": %lld, \"pair_grid\": %lld, \"greedy_grid\": %lld, \"last_queries\": %lld, \"last_pair_grid\": %lld, "
               "\"last_greedy_grid\": %lld, \"launches\": %d, \"grid_max\": %lld, \"tile\": %lld, \"min_mib\": %lld, \"tiles\": [",
               (long long)p.blocks, (long long)p.tiles_per_query, p.chunk_cols, (long long)p.query_words, (long long)p.query_bytes,
               (long long)p.queries_per_chunk, (long long)p.chunks, (long long)p.workspace_bytes, (long long)p.pair_grid, (long long)p.greedy_grid,
               (long long)p.last_queries, (long long)p.last_pair_grid, (long long)p.last_greedy_grid, p.launches, (long long)swp::kPssmHitsGridMax,
               (long long)swp::kMsaFilterTile, (long long)swp::kMsaFilterMinMib);
        for (int64_t t = 0; tiles && t < p.tiles_per_query; ++t) {
            int rb, cb;
            swp::msa_filter_tile(t, rb, cb);
            printf("%s[%d, %d]", t ? ", " : "", rb, cb);
        }
        printf("]}\n");
    }
    return 0;
}
