// Drives swp::plan_prefilter (smith-waterman_amd/csrc/sw_plan.cpp) for tests/test_prefilter_plan.py: one case per input line of
// name=value pairs, one JSON object per output line.  qlens and per_cu take comma-separated lists (per_cu: one value for all six
// kernels, or six in the order of swp::prefilter_kernel_index).  Beside the plan the line carries the table and the groups
// swp::plan_search_multi gives for the same queries and budget ("multi_table", "multi_groups").
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

static void print_table(const char* name, const std::vector<swk::MultiQuery>& t) {
    printf("\"%s\": [", name);
    for (size_t i = 0; i < t.size(); ++i)
        printf("%s[%lld, %lld, %lld, %d, %d, %d]", i ? ", " : "", (long long)t[i].prof_off, (long long)t[i].qstart, (long long)t[i].row, t[i].qlen, t[i].qpad, t[i].nstrips);
    printf("]");
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        swp::PrefilterJob j;
        std::vector<int64_t> qlens;
        for (int k = 0; k < swp::kPrefilterKernels; ++k) j.per_cu[k] = 3;
        std::istringstream in(line);
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq), val = kv.substr(eq + 1);
            if (k == "qlens") qlens = list_of(val);
            else if (k == "per_cu") { const std::vector<int64_t> v = list_of(val); for (int i = 0; i < swp::kPrefilterKernels; ++i) j.per_cu[i] = (int)v[v.size() == 1 ? 0 : i]; }
            else if (k == "longest") j.longest = std::stoll(val);
            else if (k == "nonempty") j.nonempty = std::stoll(val);
            else if (k == "num_cus") j.num_cus = std::stoi(val);
            else if (k == "budget_bytes") j.budget_bytes = std::stoll(val);
            else if (k == "max_items") j.max_items = std::stoll(val);
            else if (k == "max_entry") j.max_entry = std::stoi(val);
            else if (k == "lanes") j.lanes = std::stoi(val);
            else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 2; }
        }
        j.qlens = qlens.data(); j.nqueries = (int64_t)qlens.size();
        const swp::PrefilterPlan p = swp::plan_prefilter(j);
        swp::SearchMultiJob mj;
        mj.qlens = j.qlens; mj.nqueries = j.nqueries; mj.longest = j.longest; mj.nonempty = j.nonempty; mj.num_cus = j.num_cus; mj.budget_bytes = j.budget_bytes;
        for (int k = 0; k < swp::kSearchMultiKernels; ++k) mj.per_cu[k] = std::min(j.per_cu[2 * k], j.per_cu[2 * k + 1]);
        const swp::SearchMultiPlan m = swp::plan_search_multi(mj);
        printf("{\"prof_need\": %zu, \"bnd_need\": %zu, \"packed_launches\": %lld, \"multi_prof_need\": %zu, ", p.prof_need, p.bnd_need, (long long)p.packed_launches,
               m.prof_need);
        print_table("table", p.table);
        printf(", ");
        print_table("multi_table", m.table);
        printf(", \"groups\": [");
        for (size_t g = 0; g < p.group.size(); ++g) printf("%s[%lld, %lld, %lld]", g ? ", " : "", (long long)p.group[g].q0, (long long)p.group[g].nq, (long long)p.group[g].prof_bytes);
        printf("], \"multi_groups\": [");
        for (size_t g = 0; g < m.group.size(); ++g) printf("%s[%lld, %lld, %lld]", g ? ", " : "", (long long)m.group[g].q0, (long long)m.group[g].nq, (long long)m.group[g].prof_bytes);
        printf("], \"launches\": [");
        for (size_t l = 0; l < p.launch.size(); ++l) {
            const swp::PrefilterLaunch& x = p.launch[l];
            printf("%s{\"group\": %d, \"C\": %d, \"kernel\": %d, \"packed\": %d, \"q0\": %lld, \"nq\": %lld, \"rank0\": %lld, \"nranks\": %lld, \"items\": %lld, "
                   "\"bnd_per\": %lld, \"grid\": %lld}", l ? ", " : "", x.group, x.C, x.kernel, x.packed ? 1 : 0, (long long)x.q0, (long long)x.nq, (long long)x.rank0,
                   (long long)x.nranks, (long long)x.items, (long long)x.bnd_per, (long long)x.grid);
        }
        printf("]}\n");
    }
    return 0;
}
