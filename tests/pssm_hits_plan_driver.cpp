// Drives swp::plan_pssm_hits (smith-waterman_amd/csrc/sw_plan.cpp) for tests/test_pssm_hits_plan.py: one case per input line of
// name=value pairs (qlens: a comma-separated list), one JSON object per output line.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../smith-waterman_amd/csrc/sw_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        swp::PssmHitsJob j;
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
            } else if (k == "nletters") j.nletters = std::stoi(val);
            else if (k == "num_cus") j.num_cus = std::stoi(val);
            else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 2; }
        }
        j.qlens = qlens.data(); j.nqueries = (int64_t)qlens.size();
        const swp::PssmHitsPlan p = swp::plan_pssm_hits(j);
        printf("{\"stride\": %d, \"tile_cols\": %d, \"max_cols\": %lld, \"tiles_per_query\": %lld, \"grid\": %lld, \"lds_bytes\": %u, \"launches\": %d, "
               "\"lds_budget\": %lld, \"code_bytes\": %lld, \"grid_max\": %lld}\n",
               p.stride, p.tile_cols, (long long)p.max_cols, (long long)p.tiles_per_query, (long long)p.grid, p.lds_bytes, p.launches,
               (long long)swp::kPssmHitsLdsBytes, (long long)swp::kPssmHitsCodeBytes, (long long)swp::kPssmHitsGridMax);
    }
    return 0;
}
