// Drives the planners (smith-waterman_amd/csrc/sw_plan.cpp) for tests/test_fill_plan.py and tests/test_batch_plan.py: one case per
// input line of name=value pairs, one JSON object per output line.  kind=fill (the default), batch or search picks the planner; the
// other fields are those of its job, DeviceFacts and PlanOptions.  Batch cases may add nletters, n and pb (the kernel of a chunk);
// search_per_cu and offsets take comma-separated lists (offsets: the schedule of those targets).
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../smith-waterman_amd/csrc/sw_plan.h"

static std::vector<double> list_of(const std::string& s) {
    std::vector<double> v;
    std::istringstream in(s);
    std::string x;
    while (std::getline(in, x, ',')) v.push_back(std::stod(x));
    return v;
}

static void print_batch(const swp::BatchPlan& p, int kernel) {
    printf("{\"wave\": %d, \"C\": %d, \"nstrips\": %lld, \"front\": %d, \"per\": %lld, \"bnd_per\": %lld, \"chunk\": %lld, \"grid\": %lld, "
           "\"scan_blocks\": %d, \"codes_blocks\": %d, \"fits16\": %d, \"k12\": %d, \"packed16\": %d, \"bcodes_need\": %zu, \"bnd_need\": %zu, "
           "\"single_chunk\": %lld, \"kernel\": %d}\n",
           p.wave, p.C, (long long)p.nstrips, p.front, (long long)p.per, (long long)p.bnd_per, (long long)p.chunk, (long long)p.grid,
           p.scan_blocks, p.codes_blocks, p.fits16, p.k12, p.packed16, p.bcodes_need, p.bnd_need, (long long)p.single_chunk, kernel);
}

static void print_search(const swp::SearchPlan& p, const std::vector<swk::SearchItem>& items) {
    printf("{\"C\": %d, \"wide\": %d, \"kernel\": %d, \"nstrips\": %lld, \"qpad\": %lld, \"bnd_per\": %lld, \"grid\": %lld, "
           "\"prof_blocks\": %d, \"prof_need\": %zu, \"bnd_need\": %zu, \"items\": [",
           p.C, p.wide, p.kernel, (long long)p.nstrips, (long long)p.qpad, (long long)p.bnd_per, (long long)p.grid, p.prof_blocks,
           p.prof_need, p.bnd_need);
    for (size_t i = 0; i < items.size(); ++i)
        printf("%s[%lld, %lld, %lld]", i ? ", " : "", (long long)items[i].start, (long long)items[i].idx, (long long)items[i].len);
    printf("]}\n");
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        swp::PlanJob j;
        swp::BatchJob bj;
        swp::SearchJob sj;
        swp::DeviceFacts d;
        swp::PlanOptions o;
        std::string kind = "fill";
        std::vector<double> offsets;
        unsigned nletters = 4;
        int64_t n = 2;
        int pb = 0;
        std::istringstream in(line);
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq), val = kv.substr(eq + 1);
            if (k == "kind") { kind = val; continue; }
            if (k == "offsets") { offsets = list_of(val); continue; }
            if (k == "search_per_cu") {
                const std::vector<double> v = list_of(val);
                for (int i = 0; i < swp::kSearchKernels; ++i) d.search_per_cu[i] = (int)v[v.size() == 1 ? 0 : i];
                continue;
            }
            const double v = std::stod(val);
            bool known = false;
#define F(s, f) if (k == #f) { s.f = (decltype(s.f))v; known = true; }
            if (kind == "batch") {
                F(bj, cols) F(bj, rows) F(bj, npairs) F(bj, has_H) F(bj, has_P) F(bj, p_elem_bytes) F(bj, match) F(bj, mismatch) F(bj, gap)
                if (k == "nletters") { nletters = (unsigned)v; known = true; }
                if (k == "n") { n = (int64_t)v; known = true; }
                if (k == "pb") { pb = (int)v; known = true; }
            } else if (kind == "search") {
                F(sj, qlen) F(sj, maxlen) F(sj, ntargets) F(sj, match) F(sj, mismatch) F(sj, gap)
            } else {
                F(j, cols) F(j, rows) F(j, npairs) F(j, full_stride) F(j, h_elem_bytes) F(j, p_elem_bytes) F(j, has_H) F(j, has_P) F(j, has_top)
                F(j, has_left) F(j, has_right) F(j, has_top_gran) F(j, has_bot_gran) F(j, has_result) F(j, total_rows) F(j, reserve_cus)
                F(j, h_aligned) F(j, p_aligned) F(j, match) F(j, mismatch) F(j, gap) F(j, pair_ratio)
            }
            F(d, num_cus) F(d, xcd_round_robin) F(d, s2_per_cu)
            F(o, engine) F(o, strips_per_group) F(o, consumers) F(o, importers) F(o, max_blocks) F(o, waves_per_block) F(o, store_policy)
            F(o, s2w) F(o, xcd_chain) F(o, split_blk) F(o, split_from) F(o, filler_hop_ps) F(o, filler_tau_ps) F(o, filler_bw_gbs)
            F(o, probe_foreign_pairs) F(o, debug_flags)
#undef F
            if (!known) { fprintf(stderr, "unknown field %s\n", k.c_str()); return 1; }
        }
        if (kind == "batch") {
            const swp::BatchPlan p = swp::plan_batch(bj, o);
            print_batch(p, swp::batch_kernel(p, nletters, n, pb));
            continue;
        }
        if (kind == "search") {
            std::vector<int64_t> off(offsets.begin(), offsets.end());
            std::vector<swk::SearchItem> items;
            if (!off.empty()) {
                int64_t nonempty = 0;
                for (size_t k = 0; k + 1 < off.size(); ++k) nonempty += off[k + 1] > off[k];
                items.resize((size_t)nonempty);
                swp::search_schedule(off.data(), (int64_t)off.size() - 1, items.data());
            }
            print_search(swp::plan_search(sj, d), items);
            continue;
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
