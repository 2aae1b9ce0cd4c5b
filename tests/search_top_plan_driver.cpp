// Drives swp::plan_search_top (smith-waterman_amd/csrc/sw_plan.cpp) for tests/test_search_top_plan.py: one case per input line of
// name=value pairs, one JSON object per output line.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../smith-waterman_amd/csrc/sw_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        swp::SearchTopJob j;
        std::istringstream in(line);
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq), val = kv.substr(eq + 1);
            if (k == "nqueries") j.nqueries = std::stoll(val);
            else if (k == "ntargets") j.ntargets = std::stoll(val);
            else if (k == "top") j.top = std::stoll(val);
            else if (k == "budget_bytes") j.budget_bytes = std::stoll(val);
            else if (k == "num_cus") j.num_cus = std::stoi(val);
            else if (k == "per_cu") j.per_cu = std::stoi(val);
            else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 2; }
        }
        const swp::SearchTopPlan p = swp::plan_search_top(j);
        printf("{\"kernel\": %d, \"chunk_queries\": %lld, \"tbits\": %d, \"nbits\": %d, \"wgs_row\": %lld, \"slice\": %lld, \"results_need\": %zu, "
               "\"hist_need\": %zu, \"state_need\": %zu, \"top_max\": %lld, \"digit_bits\": %d, \"chunks\": [",
               p.kernel, (long long)p.chunk_queries, p.tbits, p.nbits, (long long)p.wgs_row, (long long)p.slice, p.results_need, p.hist_need, p.state_need,
               (long long)swp::kTopMax, swp::kTopDigitBits);
        for (size_t c = 0; c < p.chunk.size(); ++c) printf("%s[%lld, %lld]", c ? ", " : "", (long long)p.chunk[c].q0, (long long)p.chunk[c].nq);
        printf("], \"passes\": [");
        for (int s = 0; s < p.npasses; ++s) printf("%s[%d, %d]", s ? ", " : "", p.pass[s].shift, p.pass[s].bits);
        printf("]}\n");
    }
    return 0;
}
