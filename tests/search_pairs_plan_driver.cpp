// Drives swp::plan_search_pairs (smith-waterman_amd/csrc/sw_plan.cpp) for tests/test_search_pairs_plan.py: one case per input line of
// name=value pairs, one JSON object per output line.  qlens and per_cu take comma-separated lists.  Beside the plan the line carries
// the table and the groups swp::plan_search_multi gives for the same queries, occupancies and budget ("multi_table", "multi_groups"),
// the first pair and the size of the chunks named by chunks=i,j,... ("chunk_at", by arithmetic: nothing is enumerated), the grid of
// every score launch for a full chunk and for the last one, and the weight bucket of every len:qpad of buckets=len:qpad,...
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../smith-waterman_amd/csrc/sw_plan.h"

static std::vector<int64_t> list_of(const std::string& s, char sep = ',') {
    std::vector<int64_t> v;
    std::istringstream in(s);
    std::string x;
    while (std::getline(in, x, sep)) v.push_back(std::stoll(x));
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
        swp::SearchPairsJob j;
        std::vector<int64_t> qlens, chunks;
        std::vector<std::string> buckets;
        for (int k = 0; k < swp::kSearchPairsKernels; ++k) j.per_cu[k] = 3;
        std::istringstream in(line);
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq), val = kv.substr(eq + 1);
            if (k == "qlens") qlens = list_of(val);
            else if (k == "per_cu") { const std::vector<int64_t> v = list_of(val); for (int i = 0; i < swp::kSearchPairsKernels; ++i) j.per_cu[i] = (int)v[v.size() == 1 ? 0 : i]; }
            else if (k == "longest") j.longest = std::stoll(val);
            else if (k == "npairs") j.npairs = std::stoll(val);
            else if (k == "num_cus") j.num_cus = std::stoi(val);
            else if (k == "budget_bytes") j.budget_bytes = std::stoll(val);
            else if (k == "chunk") j.chunk = std::stoll(val);
            else if (k == "chunks") chunks = list_of(val);
            else if (k == "buckets") { std::istringstream b(val); std::string x; while (std::getline(b, x, ',')) buckets.push_back(x); }
            else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 2; }
        }
        j.qlens = qlens.data(); j.nqueries = (int64_t)qlens.size();
        const swp::SearchPairsPlan p = swp::plan_search_pairs(j);
        swp::SearchMultiJob mj;
        mj.qlens = j.qlens; mj.nqueries = j.nqueries; mj.longest = j.longest; mj.nonempty = 1; mj.num_cus = j.num_cus; mj.budget_bytes = j.budget_bytes;
        for (int k = 0; k < swp::kSearchMultiKernels; ++k) mj.per_cu[k] = j.per_cu[k];
        const swp::SearchMultiPlan m = swp::plan_search_multi(mj);
        printf("{\"prof_need\": %zu, \"bnd_need\": %zu, \"items_need\": %zu, \"chunk\": %lld, \"nchunks\": %lld, \"launches_total\": %lld, \"multi_prof_need\": %zu, ",
               p.prof_need, p.bnd_need, p.items_need, (long long)p.chunk, (long long)p.nchunks, (long long)p.launches, m.prof_need);
        print_table("table", p.table);
        printf(", ");
        print_table("multi_table", m.table);
        printf(", \"entry_of\": [");
        for (size_t q = 0; q < p.entry_of.size(); ++q) printf("%s%d", q ? ", " : "", p.entry_of[q]);
        printf("], \"groups\": [");
        for (size_t g = 0; g < p.group.size(); ++g) {
            const swp::PairsGroup& x = p.group[g];
            printf("%s{\"q0\": %lld, \"nq\": %lld, \"prof_bytes\": %lld, \"cls_q0\": [%lld, %lld, %lld, %lld]}", g ? ", " : "", (long long)x.q0, (long long)x.nq,
                   (long long)x.prof_bytes, (long long)x.cls_q0[0], (long long)x.cls_q0[1], (long long)x.cls_q0[2], (long long)x.cls_q0[3]);
        }
        printf("], \"multi_groups\": [");
        for (size_t g = 0; g < m.group.size(); ++g) printf("%s[%lld, %lld, %lld]", g ? ", " : "", (long long)m.group[g].q0, (long long)m.group[g].nq, (long long)m.group[g].prof_bytes);
        const int64_t last = p.nchunks ? p.chunk_pairs(p.nchunks - 1, j.npairs) : 0;
        printf("], \"last_chunk_pairs\": %lld, \"launches\": [", (long long)last);
        for (size_t l = 0; l < p.launch.size(); ++l) {
            const swp::PairsLaunch& x = p.launch[l];
            printf("%s{\"group\": %d, \"C\": %d, \"kernel\": %d, \"q0\": %lld, \"nq\": %lld, \"bnd_per\": %lld, \"max_grid\": %lld, \"grid_full\": %lld, \"grid_last\": %lld}",
                   l ? ", " : "", x.group, x.C, x.kernel, (long long)x.q0, (long long)x.nq, (long long)x.bnd_per, (long long)x.max_grid,
                   (long long)swp::search_pairs_grid(x, p.nchunks ? p.chunk_pairs(0, j.npairs) : 0), (long long)swp::search_pairs_grid(x, last));
        }
        printf("], \"chunk_at\": [");
        for (size_t i = 0; i < chunks.size(); ++i)
            printf("%s[%lld, %lld]", i ? ", " : "", (long long)p.chunk_p0(chunks[i]), (long long)p.chunk_pairs(chunks[i], j.npairs));
        printf("], \"buckets\": [");
        for (size_t i = 0; i < buckets.size(); ++i) {
            const std::vector<int64_t> lq = list_of(buckets[i], ':');
            printf("%s%d", i ? ", " : "", swp::search_pairs_bucket(lq[0], lq[1]));
        }
        printf("]}\n");
    }
    return 0;
}
