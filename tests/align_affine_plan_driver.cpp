// Drives plan_align_affine and align_schedule (smith-waterman_amd/csrc/sw_plan.cpp) for tests/test_align_affine_host.py: one case per
// input line of name=value pairs (the fields of AlignAffineJob; per_cu takes one value for all kernels or a comma-separated list;
// budget_mib sets budget_bytes; lens=a,b,.. are hit lengths whose order align_schedule reports), one JSON object per output line.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../smith-waterman_amd/csrc/sw_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        swp::AlignAffineJob j;
        std::vector<int64_t> lens;
        std::istringstream in(line);
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq), val = kv.substr(eq + 1);
            if (k == "per_cu" || k == "lens") {
                std::vector<int64_t> v;
                std::istringstream li(val);
                std::string x;
                while (std::getline(li, x, ',')) v.push_back(std::stoll(x));
                if (k == "lens") lens = v;
                else for (int i = 0; i < swp::kAlignAffineKernels; ++i) j.per_cu[i] = (int)v[v.size() == 1 ? 0 : (size_t)i];
            }
            else if (k == "qlen") j.qlen = std::stoll(val);
            else if (k == "maxhit") j.maxhit = std::stoll(val);
            else if (k == "nhits") j.nhits = std::stoll(val);
            else if (k == "num_cus") j.num_cus = std::stoi(val);
            else if (k == "budget_mib") j.budget_bytes = std::stoll(val) << 20;
            else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 1; }
        }
        const swp::AlignAffinePlan p = swp::plan_align_affine(j);
        printf("{\"fits\": %d, \"C\": %d, \"kernel\": %d, \"nstrips\": %lld, \"qpad\": %lld, \"bnd_per\": %lld, \"slot_bytes\": %lld, \"slots\": %lld, "
               "\"grid\": %lld, \"prof_need\": %zu, \"bnd_need\": %zu, \"dir_need\": %zu, \"order\": [",
               p.fits ? 1 : 0, p.C, p.kernel, (long long)p.nstrips, (long long)p.qpad, (long long)p.bnd_per, (long long)p.slot_bytes, (long long)p.slots,
               (long long)p.grid, p.prof_need, p.bnd_need, p.dir_need);
        // hit h is target h of a database with these lengths
        std::vector<int64_t> offs(lens.size() + 1, 0), hits(lens.size());
        for (size_t i = 0; i < lens.size(); ++i) { offs[i + 1] = offs[i] + lens[i]; hits[i] = (int64_t)i; }
        std::vector<swk::SearchItem> items(lens.size());
        swp::align_schedule(offs.data(), hits.data(), (int64_t)lens.size(), items.data());
        for (size_t i = 0; i < items.size(); ++i) printf("%s%lld", i ? ", " : "", (long long)items[i].idx);
        printf("]}\n");
    }
    return 0;
}
