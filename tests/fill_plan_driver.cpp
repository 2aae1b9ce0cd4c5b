// Drives the fill planner (smith-waterman_amd/csrc/sw_plan.cpp) for tests/test_fill_plan.py: one case per input line of
// name=value pairs (fields of PlanJob, DeviceFacts and PlanOptions), one JSON object per output line.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../smith-waterman_amd/csrc/sw_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        swp::PlanJob j;
        swp::DeviceFacts d;
        swp::PlanOptions o;
        std::istringstream in(line);
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq);
            const double v = std::stod(kv.substr(eq + 1));
            bool known = false;
#define F(s, f) if (k == #f) { s.f = (decltype(s.f))v; known = true; }
            F(j, cols) F(j, rows) F(j, npairs) F(j, full_stride) F(j, h_elem_bytes) F(j, p_elem_bytes) F(j, has_H) F(j, has_P) F(j, has_top)
            F(j, has_left) F(j, has_right) F(j, has_top_gran) F(j, has_bot_gran) F(j, has_result) F(j, total_rows) F(j, reserve_cus)
            F(j, h_aligned) F(j, p_aligned) F(j, match) F(j, mismatch) F(j, gap) F(j, pair_ratio)
            F(d, num_cus) F(d, xcd_round_robin) F(d, s2_per_cu)
            F(o, engine) F(o, strips_per_group) F(o, consumers) F(o, importers) F(o, max_blocks) F(o, waves_per_block) F(o, store_policy)
            F(o, s2w) F(o, xcd_chain) F(o, split_blk) F(o, split_from) F(o, filler_hop_ps) F(o, filler_tau_ps) F(o, filler_bw_gbs)
            F(o, probe_foreign_pairs) F(o, debug_flags)
#undef F
            if (!known) { fprintf(stderr, "unknown field %s\n", k.c_str()); return 1; }
        }
        const swp::FillPlan p = swp::plan_fill(j, d, o);
        printf("{\"engine\": %d, \"S\": %lld, \"store_nt\": %d, \"NS\": %d, \"NC\": %d, \"importers\": %d, \"threads\": %d, \"grid\": %d, "
               "\"fast\": %d, \"perm\": %d, \"e4stride\": %lld, \"two_cols\": %d, \"W2\": %d, \"ntile\": %lld, \"tstrips\": %lld, "
               "\"edge_need\": %zu, \"cb_need\": %zu, \"edge4_need\": %zu, \"priv_need\": %zu, \"h_bytes\": %zu, \"p_bytes\": %zu, "
               "\"probe_pair_class\": %d, \"tiles\": [",
               p.engine, (long long)p.S, p.store_nt, p.NS, p.NC, p.importers, p.threads, p.grid, p.fast, p.perm, (long long)p.e4stride,
               p.two_cols, p.W2, (long long)p.ntile, (long long)p.tstrips, p.edge_need, p.cb_need, p.edge4_need, p.priv_need, p.h_bytes,
               p.p_bytes, p.probe_pair_class);
        for (int64_t t = 0; p.two_cols && t < p.ntile; ++t) {
            const swp::TilePlan& x = p.tile[t];
            printf("%s{\"c0\": %lld, \"cols\": %lld, \"strips\": %lld, \"grid\": %d, \"nscout\": %d, \"scout_double\": %d, \"xcd_mode\": %d, "
                   "\"split_blk\": %d, \"split_from\": %d, \"split_extra\": %d, \"filler_end_steps\": %d, \"filler_full_steps\": %d, "
                   "\"filler_hop_ps\": %d, \"store_nt\": %d, \"consumers\": %d}",
                   t ? ", " : "", (long long)x.c0, (long long)x.cols, (long long)x.strips, x.grid, x.nscout, x.scout_double, x.xcd_mode,
                   x.split_blk, x.split_from, x.split_extra, x.filler_end_steps, x.filler_full_steps, x.filler_hop_ps, x.store_nt, x.consumers);
        }
        printf("]}\n");
    }
    return 0;
}
