// Drives swp::plan_align_ckpt, swp::plan_align_hits_ckpt and the mode rule (smith-waterman_amd/csrc/sw_plan.cpp) for
// tests/test_align_ckpt_plan.py: one case per input line of name=value pairs, one JSON object per output line.
//   what=one   len qpad_of (a query length) budget_bytes forced nhits per_cu num_cus      -> the plan of sw_align_affine_device
//   what=hits  qlens (comma list) longest budget_bytes forced top per_cu num_cus mode     -> the plan of sw_db_align_affine_hits
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../smith-waterman_amd/csrc/sw_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::string what = "one";
        swp::AlignCkptJob one;
        swp::AlignHitsCkptJob hits;
        std::vector<int64_t> qlens;
        int64_t mode = 1;
        std::istringstream in(line);
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq), val = kv.substr(eq + 1);
            if (k == "what") what = val;
            else if (k == "len") one.maxhit = std::stoll(val);
            else if (k == "qlen") one.qlen = std::stoll(val);
            else if (k == "nhits") one.nhits = std::stoll(val);
            else if (k == "qlens") { std::istringstream l(val); std::string x; while (std::getline(l, x, ',')) qlens.push_back(std::stoll(x)); }
            else if (k == "longest") hits.longest = std::stoll(val);
            else if (k == "top") hits.top = std::stoll(val);
            else if (k == "mode") mode = std::stoll(val);
            else if (k == "budget_bytes") one.budget_bytes = hits.budget_bytes = std::stoll(val);
            else if (k == "forced") one.band_rows = hits.band_rows = std::stoll(val);
            else if (k == "num_cus") one.num_cus = hits.num_cus = std::stoi(val);
            else if (k == "per_cu") {
                std::istringstream l(val); std::string x;
                for (int i = 0; i < 3 && std::getline(l, x, ','); ++i) one.per_cu[i] = hits.per_cu[i] = std::stoi(x);
            }
            else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 2; }
        }
        if (what == "one") {
            const swp::AlignCkptPlan p = swp::plan_align_ckpt(one);
            printf("{\"fits\": %d, \"C\": %d, \"kernel\": %d, \"nstrips\": %lld, \"qpad\": %lld, \"band_rows\": %lld, \"log_band\": %d, \"slot_bytes\": %lld, "
                   "\"formula\": %lld, \"slots\": %lld, \"grid\": %lld, \"bnd_per\": %lld, \"bnd_need\": %zu, \"dir_need\": %zu, \"floor\": %lld, \"min_rows\": %lld, "
                   "\"max_rows\": %lld, \"slot_limit\": %lld}\n",
                   p.fits ? 1 : 0, p.C, p.kernel, (long long)p.nstrips, (long long)p.qpad, (long long)p.band_rows, p.log_band, (long long)p.slot_bytes,
                   (long long)swp::align_ckpt_slot_bytes(one.maxhit, p.qpad, p.band_rows), (long long)p.slots, (long long)p.grid, (long long)p.bnd_per, p.bnd_need,
                   p.dir_need, (long long)swp::kAlignCkptFloorRows, (long long)swp::kAlignCkptMinRows, (long long)swp::kAlignCkptMaxRows,
                   (long long)swp::kAlignSlotLimit);
            continue;
        }
        hits.qlens = qlens.data(); hits.nqueries = (int64_t)qlens.size();
        const swp::AlignHitsPlan whole = swp::plan_align_hits(hits);
        const bool ckpt = swp::align_use_ckpt(mode, whole.fits);
        const swp::AlignHitsPlan p = ckpt ? swp::plan_align_hits_ckpt(hits) : whole;
        printf("{\"whole_fits\": %d, \"ckpt\": %d, \"fits\": %d, \"worst_qpad\": %lld, \"worst_bytes\": %lld, \"dir_need\": %zu, \"bnd_need\": %zu, \"tier_ratio\": %lld, "
               "\"tier_floor\": %lld, \"max_tiers\": %d, \"groups\": [",
               whole.fits ? 1 : 0, ckpt ? 1 : 0, p.fits ? 1 : 0, (long long)p.worst_qpad, (long long)p.worst_bytes, p.dir_need, p.bnd_need,
               (long long)swp::kAlignHitsTierRatio, (long long)swp::kAlignHitsTierFloor, swp::kAlignHitsTiers);
        for (size_t g = 0; g < p.group.size(); ++g) {
            printf("%s{\"cls\": [", g ? ", " : "");
            for (int k = 0; k < swp::kAlignHitsKernels; ++k) {
                const swp::AlignHitsClass& c = p.group[g].cls[k];
                printf("%s{\"nq\": %lld, \"entries\": %lld, \"qpad\": %lld, \"nstrips\": %lld, \"log_band\": %d, \"bound\": [", k ? ", " : "", (long long)c.nq,
                       (long long)c.entries, (long long)c.qpad, (long long)c.nstrips, c.log_band);
                for (int t = 0; t < c.ntiers; ++t) printf("%s%lld", t ? ", " : "", (long long)c.bound[t]);
                printf("]}");
            }
            printf("]}");
        }
        printf("], \"launch\": [");
        for (size_t l = 0; l < p.launch.size(); ++l) {
            const swp::AlignHitsLaunch& x = p.launch[l];
            printf("%s{\"group\": %d, \"C\": %d, \"kernel\": %d, \"tier\": %d, \"log_band\": %d, \"slot_bytes\": %lld, \"slots\": %lld, \"bnd_per\": %lld, \"grid\": %lld}",
                   l ? ", " : "", x.group, x.C, x.kernel, x.tier, x.log_band, (long long)x.slot_bytes, (long long)x.slots, (long long)x.bnd_per, (long long)x.grid);
        }
        printf("]}\n");
    }
    return 0;
}
