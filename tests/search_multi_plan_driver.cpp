// Drives swp::plan_search_multi (smith-waterman_amd/csrc/sw_plan.cpp) for tests/test_search_multi_plan.py: one case per input line of
// name=value pairs, one JSON object per output line.  qlens and per_cu take comma-separated lists; cover=1 adds, per (query, target
// rank) pair, how many work items of the plan's launches map to it (by the kernel's rule: item w of a launch is the target rank
// rank0 + w / nq and the table entry q0 + w % nq) -- only for plans small enough to enumerate.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../smith-waterman_amd/csrc/sw_plan.h"

static std::vector<int64_t> list_of(const std::string& s) {
    std::vector<int64_t> v;
    std::istringstream in(s);
    std::string x;
    while (std::getline(in, x, ',')) v.push_back(std::stoll(x));
    return v;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        swp::SearchMultiJob j;
        std::vector<int64_t> qlens;
        bool cover = false;
        for (int k = 0; k < swp::kSearchMultiKernels; ++k) j.per_cu[k] = 3;
        std::istringstream in(line);
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq), val = kv.substr(eq + 1);
            if (k == "qlens") qlens = list_of(val);
            else if (k == "per_cu") { const std::vector<int64_t> v = list_of(val); for (int i = 0; i < swp::kSearchMultiKernels; ++i) j.per_cu[i] = (int)v[v.size() == 1 ? 0 : i]; }
            else if (k == "longest") j.longest = std::stoll(val);
            else if (k == "nonempty") j.nonempty = std::stoll(val);
            else if (k == "num_cus") j.num_cus = std::stoi(val);
            else if (k == "budget_bytes") j.budget_bytes = std::stoll(val);
            else if (k == "max_items") j.max_items = std::stoll(val);
            else if (k == "repeat") { const std::vector<int64_t> one = qlens; for (int64_t r = 1; r < std::stoll(val); ++r) qlens.insert(qlens.end(), one.begin(), one.end()); }
            else if (k == "cover") cover = val == "1";
            else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 2; }
        }
        j.qlens = qlens.data(); j.nqueries = (int64_t)qlens.size();
        const swp::SearchMultiPlan p = swp::plan_search_multi(j);
        printf("{\"prof_need\": %zu, \"bnd_need\": %zu, \"table\": [", p.prof_need, p.bnd_need);
        for (size_t t = 0; t < p.table.size(); ++t)
            printf("%s[%lld, %lld, %d, %d, %d]", t ? ", " : "", (long long)p.table[t].prof_off, (long long)p.table[t].row, p.table[t].qlen, p.table[t].qpad, p.table[t].nstrips);
        printf("], \"groups\": [");
        for (size_t g = 0; g < p.group.size(); ++g) printf("%s[%lld, %lld, %lld]", g ? ", " : "", (long long)p.group[g].q0, (long long)p.group[g].nq, (long long)p.group[g].prof_bytes);
        printf("], \"launches\": [");
        for (size_t l = 0; l < p.launch.size(); ++l) {
            const swp::MultiLaunch& x = p.launch[l];
            printf("%s{\"group\": %d, \"C\": %d, \"kernel\": %d, \"q0\": %lld, \"nq\": %lld, \"rank0\": %lld, \"nranks\": %lld, \"items\": %lld, \"bnd_per\": %lld, \"grid\": %lld}",
                   l ? ", " : "", x.group, x.C, x.kernel, (long long)x.q0, (long long)x.nq, (long long)x.rank0, (long long)x.nranks, (long long)x.items,
                   (long long)x.bnd_per, (long long)x.grid);
        }
        printf("]");
        if (cover) {
            std::vector<int> seen((size_t)(j.nqueries * j.nonempty), 0);
            bool inside = true;
            for (const swp::MultiLaunch& x : p.launch)
                for (int64_t w = 0; w < x.items; ++w) {
                    const int64_t rank = x.rank0 + w / x.nq, row = p.table[(size_t)(x.q0 + w % x.nq)].row;
                    if (rank < 0 || rank >= j.nonempty || row < 0 || row >= j.nqueries) { inside = false; continue; }
                    ++seen[(size_t)(row * j.nonempty + rank)];
                }
            int lo = 1 << 30, hi = 0;
            for (int v : seen) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
            printf(", \"cover\": [%d, %d, %d]", inside ? 1 : 0, seen.empty() ? 1 : lo, seen.empty() ? 1 : hi);
        }
        printf("}\n");
    }
    return 0;
}
