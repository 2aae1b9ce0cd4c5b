// Drives swp::plan_align_hits (smith-waterman_amd/csrc/sw_plan.cpp) for tests/test_align_hits_plan.py: one case per input line of
// name=value pairs (qlens a comma list, repeated `rep` times), one JSON object per output line.  detail=0 leaves the lists out.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../smith-waterman_amd/csrc/sw_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        swp::AlignHitsJob j;
        std::vector<int64_t> base, qlens;
        int64_t rep = 1, detail = 1;
        std::istringstream in(line);
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq), val = kv.substr(eq + 1);
            if (k == "qlens") { std::istringstream l(val); std::string x; while (std::getline(l, x, ',')) base.push_back(std::stoll(x)); }
            else if (k == "rep") rep = std::stoll(val);
            else if (k == "detail") detail = std::stoll(val);
            else if (k == "top") j.top = std::stoll(val);
            else if (k == "longest") j.longest = std::stoll(val);
            else if (k == "budget_bytes") j.budget_bytes = std::stoll(val);
            else if (k == "profile_budget_bytes") j.profile_budget_bytes = std::stoll(val);
            else if (k == "max_items") j.max_items = std::stoll(val);
            else if (k == "num_cus") j.num_cus = std::stoi(val);
            else if (k == "per_cu") { std::istringstream l(val); std::string x; for (int i = 0; i < 3 && std::getline(l, x, ','); ++i) j.per_cu[i] = std::stoi(x); }
            else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 2; }
        }
        for (int64_t r = 0; r < rep; ++r) qlens.insert(qlens.end(), base.begin(), base.end());
        j.qlens = qlens.data(); j.nqueries = (int64_t)qlens.size();
        const swp::AlignHitsPlan p = swp::plan_align_hits(j);
        int64_t entries = 0, covered = 0;
        bool in_order = true;
        for (const swp::AlignHitsGroup& g : p.group) {
            in_order = in_order && g.q0 == covered;
            covered += g.nq;
            for (const swp::AlignHitsClass& c : g.cls) entries += c.entries;
        }
        printf("{\"fits\": %d, \"worst_qpad\": %lld, \"worst_bytes\": %lld, \"tiers\": %lld, \"slots\": %lld, \"prof_need\": %zu, \"bnd_need\": %zu, "
               "\"dir_need\": %zu, \"items_need\": %zu, \"ngroups\": %zu, \"nlaunches\": %zu, \"entries\": %lld, \"covered\": %lld, \"in_order\": %d, "
               "\"tier_ratio\": %lld, \"tier_floor\": %lld, \"max_tiers\": %d, \"groups\": [",
               p.fits ? 1 : 0, (long long)p.worst_qpad, (long long)p.worst_bytes, (long long)p.tiers, (long long)p.slots, p.prof_need, p.bnd_need, p.dir_need,
               p.items_need, p.group.size(), p.launch.size(), (long long)entries, (long long)covered, in_order ? 1 : 0, (long long)swp::kAlignHitsTierRatio,
               (long long)swp::kAlignHitsTierFloor, swp::kAlignHitsTiers);
        for (size_t g = 0; detail && g < p.group.size(); ++g) {
            const swp::AlignHitsGroup& grp = p.group[g];
            printf("%s{\"q0\": %lld, \"nq\": %lld, \"prof_bytes\": %lld, \"cls\": [", g ? ", " : "", (long long)grp.q0, (long long)grp.nq, (long long)grp.prof_bytes);
            for (int k = 0; k < swp::kAlignHitsKernels; ++k) {
                const swp::AlignHitsClass& c = grp.cls[k];
                printf("%s{\"q0\": %lld, \"nq\": %lld, \"item0\": %lld, \"entries\": %lld, \"qpad\": %lld, \"nstrips\": %lld, \"bound\": [", k ? ", " : "", (long long)c.q0,
                       (long long)c.nq, (long long)c.item0, (long long)c.entries, (long long)c.qpad, (long long)c.nstrips);
                for (int t = 0; t < c.ntiers; ++t) printf("%s%lld", t ? ", " : "", (long long)c.bound[t]);
                printf("]}");
            }
            printf("]}");
        }
        printf("], \"launch\": [");
        for (size_t l = 0; detail && l < p.launch.size(); ++l) {
            const swp::AlignHitsLaunch& x = p.launch[l];
            printf("%s{\"group\": %d, \"C\": %d, \"kernel\": %d, \"tier\": %d, \"slot_bytes\": %lld, \"slots\": %lld, \"bnd_per\": %lld, \"grid\": %lld}", l ? ", " : "",
                   x.group, x.C, x.kernel, x.tier, (long long)x.slot_bytes, (long long)x.slots, (long long)x.bnd_per, (long long)x.grid);
        }
        printf("], \"table\": [");
        for (size_t t = 0; detail && t < p.table.size(); ++t)
            printf("%s[%lld, %lld, %d, %d, %d]", t ? ", " : "", (long long)p.table[t].prof_off, (long long)p.table[t].row, p.table[t].qlen, p.table[t].qpad, p.table[t].nstrips);
        printf("]}\n");
    }
    return 0;
}
