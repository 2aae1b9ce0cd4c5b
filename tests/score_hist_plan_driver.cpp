// Drives swp::plan_score_hist and swp::plan_hits_threshold (smith-waterman_amd/csrc/sw_plan.cpp) for tests/test_score_hist_plan.py: one
// case per input line of name=value pairs, one JSON object per output line.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../smith-waterman_amd/csrc/sw_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        swp::ScoreHistJob j;
        std::istringstream in(line);
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq), val = kv.substr(eq + 1);
            if (k == "nqueries") j.nqueries = std::stoll(val);
            else if (k == "ntargets") j.ntargets = std::stoll(val);
            else if (k == "num_cus") j.num_cus = std::stoi(val);
            else if (k == "copies") j.copies = std::stoi(val);
            else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 2; }
        }
        const swp::ScoreHistPlan p = swp::plan_score_hist(j);
        const swp::HitsThresholdPlan t = swp::plan_hits_threshold(j.nqueries);
        printf("{\"slices_per_query\": %lld, \"slice\": %lld, \"items\": %lld, \"grid\": %lld, \"copies\": %d, \"lds_bytes\": %lld, \"launches\": %d, "
               "\"grid_max\": %lld, \"cells\": %lld, \"lds_max\": %lld, \"min_slice\": %lld, \"max_slices\": %lld, \"wgs_per_cu\": %d, "
               "\"threshold_grid\": %lld, \"threshold_launches\": %d}\n",
               (long long)p.slices_per_query, (long long)p.slice, (long long)p.items, (long long)p.grid, p.copies, (long long)p.lds_bytes, p.launches,
               (long long)swp::kPssmHitsGridMax, (long long)swp::kScoreHistCells, (long long)swp::kScoreHistLdsMax, (long long)swp::kScoreHistMinSlice,
               (long long)swp::kScoreHistMaxSlices, swp::kScoreHistWgsPerCu, (long long)t.grid, t.launches);
    }
    return 0;
}
