// Drives swp::plan_msa_hits (smith-waterman_amd/csrc/sw_plan.cpp) for tests/test_msa_hits_plan.py: one case per input line of
// name=value pairs, one JSON object per output line.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../smith-waterman_amd/csrc/sw_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        swp::MsaHitsJob j;
        std::istringstream in(line);
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq), val = kv.substr(eq + 1);
            if (k == "nqueries") j.nqueries = std::stoll(val);
            else if (k == "top") j.top = std::stoll(val);
            else if (k == "num_cus") j.num_cus = std::stoi(val);
            else if (k == "rows") j.rows = std::stoi(val) != 0;
            else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 2; }
        }
        const swp::MsaHitsPlan p = swp::plan_msa_hits(j);
        printf("{\"entries\": %lld, \"slice_entries\": %lld, \"slices_per_query\": %lld, \"cols_grid\": %lld, \"scan_chunks\": %lld, \"scan_grid\": %lld, "
               "\"top_rounds\": %lld, \"scan_levels\": %d, \"rows_grid\": %lld, \"sums_bytes\": %lld, \"launches\": %d, \"grid_max\": %lld, \"chunk\": %lld}\n",
               (long long)p.entries, (long long)p.slice_entries, (long long)p.slices_per_query, (long long)p.cols_grid, (long long)p.scan_chunks,
               (long long)p.scan_grid, (long long)p.top_rounds, p.scan_levels, (long long)p.rows_grid, (long long)p.sums_bytes, p.launches,
               (long long)swp::kPssmHitsGridMax, (long long)swp::kMsaScanChunk);
    }
    return 0;
}
