// Drives plan_search_affine (smith-waterman_amd/csrc/sw_plan.cpp) for tests/test_search_affine_host.py: one case per input line of
// name=value pairs (the fields of SearchAffineJob; per_cu takes one value for all kernels or a comma-separated list), one JSON object
// per output line.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../smith-waterman_amd/csrc/sw_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        swp::SearchAffineJob j;
        std::istringstream in(line);
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq), val = kv.substr(eq + 1);
            if (k == "per_cu") {
                std::vector<int> v;
                std::istringstream li(val);
                std::string x;
                while (std::getline(li, x, ',')) v.push_back(std::stoi(x));
                for (int i = 0; i < swp::kSearchAffineKernels; ++i) j.per_cu[i] = v[v.size() == 1 ? 0 : (size_t)i];
            }
            else if (k == "qlen") j.qlen = std::stoll(val);
            else if (k == "maxlen") j.maxlen = std::stoll(val);
            else if (k == "ntargets") j.ntargets = std::stoll(val);
            else if (k == "num_cus") j.num_cus = std::stoi(val);
            else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 1; }
        }
        const swp::SearchAffinePlan p = swp::plan_search_affine(j);
        printf("{\"C\": %d, \"kernel\": %d, \"nstrips\": %lld, \"qpad\": %lld, \"bnd_row_ints\": %d, \"bnd_per\": %lld, \"grid\": %lld, "
               "\"prof_blocks\": %d, \"prof_need\": %zu, \"bnd_need\": %zu}\n",
               p.C, p.kernel, (long long)p.nstrips, (long long)p.qpad, p.bnd_row_ints, (long long)p.bnd_per, (long long)p.grid, p.prof_blocks,
               p.prof_need, p.bnd_need);
    }
    return 0;
}
