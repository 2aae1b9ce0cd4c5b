// Drives swp::plan_search_pairs_lanes (smith-waterman_amd/csrc/sw_plan.cpp) for tests/test_search_pairs_lanes_plan.py: one case per
// input line of name=value pairs, one JSON object per output line.  qlens, per_cu and packed_per_cu take comma-separated lists (one
// value for all three kernels, or three).  Every plan is printed in one format -- "lanes" is swp::plan_search_pairs_lanes's, "pairs"
// is swp::plan_search_pairs's for the same job, with the fields the 32-bit plan does not have at what they are without a packed query --
// so that the test compares them field for field.  bound=np:cells,... prints the planner's bounds for a (chunk, group) of np pairs with
// `cells` cells ("bounds": [[two-pair items, item bytes], ...]); cell=cell0:npk:t0:t:b,... the linear index of a cell ("cell_index").
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

static void print_table(const std::vector<swk::MultiQuery>& t) {
    printf("\"table\": [");
    for (size_t i = 0; i < t.size(); ++i)
        printf("%s[%lld, %lld, %lld, %d, %d, %d]", i ? ", " : "", (long long)t[i].prof_off, (long long)t[i].qstart, (long long)t[i].row, t[i].qlen, t[i].qpad, t[i].nstrips);
    printf("]");
}

static void print_head(const char* name, size_t prof, size_t bnd, size_t items, size_t cells, int64_t chunk, int64_t nchunks, int64_t launches, int64_t packed,
                       const std::vector<swk::MultiQuery>& table, const std::vector<int32_t>& entry_of) {
    printf("\"%s\": {\"prof_need\": %zu, \"bnd_need\": %zu, \"items_need\": %zu, \"cells_need\": %zu, \"chunk\": %lld, \"nchunks\": %lld, \"launches_total\": %lld, "
           "\"packed_launches\": %lld, ", name, prof, bnd, items, cells, (long long)chunk, (long long)nchunks, (long long)launches, (long long)packed);
    print_table(table);
    printf(", \"entry_of\": [");
    for (size_t q = 0; q < entry_of.size(); ++q) printf("%s%d", q ? ", " : "", entry_of[q]);
    printf("], ");
}

static void print_group(bool first, const swp::PairsGroup& x, const int64_t* pk_q1, int64_t cells) {
    printf("%s{\"q0\": %lld, \"nq\": %lld, \"prof_bytes\": %lld, \"cls_q0\": [%lld, %lld, %lld, %lld], \"pk_q1\": [%lld, %lld, %lld], \"cells\": %lld}", first ? "" : ", ",
           (long long)x.q0, (long long)x.nq, (long long)x.prof_bytes, (long long)x.cls_q0[0], (long long)x.cls_q0[1], (long long)x.cls_q0[2], (long long)x.cls_q0[3],
           (long long)pk_q1[0], (long long)pk_q1[1], (long long)pk_q1[2], (long long)cells);
}

static void print_launch(bool first, const swp::PairsLaunch& x, int packed, int64_t grid_full, int64_t grid_last) {
    printf("%s{\"group\": %d, \"C\": %d, \"kernel\": %d, \"packed\": %d, \"q0\": %lld, \"nq\": %lld, \"bnd_per\": %lld, \"max_grid\": %lld, \"grid_full\": %lld, "
           "\"grid_last\": %lld}", first ? "" : ", ", x.group, x.C, x.kernel, packed, (long long)x.q0, (long long)x.nq, (long long)x.bnd_per, (long long)x.max_grid,
           (long long)grid_full, (long long)grid_last);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        swp::SearchPairsLanesJob j;
        std::vector<int64_t> qlens;
        std::vector<std::string> bounds, cells;
        for (int k = 0; k < swp::kSearchPairsKernels; ++k) j.per_cu[k] = j.packed_per_cu[k] = 3;
        std::istringstream in(line);
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq), val = kv.substr(eq + 1);
            if (k == "qlens") qlens = list_of(val);
            else if (k == "per_cu") { const std::vector<int64_t> v = list_of(val); for (int i = 0; i < swp::kSearchPairsKernels; ++i) j.per_cu[i] = (int)v[v.size() == 1 ? 0 : i]; }
            else if (k == "packed_per_cu") { const std::vector<int64_t> v = list_of(val); for (int i = 0; i < swp::kSearchPairsKernels; ++i) j.packed_per_cu[i] = (int)v[v.size() == 1 ? 0 : i]; }
            else if (k == "longest") j.longest = std::stoll(val);
            else if (k == "npairs") j.npairs = std::stoll(val);
            else if (k == "num_cus") j.num_cus = std::stoi(val);
            else if (k == "budget_bytes") j.budget_bytes = std::stoll(val);
            else if (k == "chunk") j.chunk = std::stoll(val);
            else if (k == "max_entry") j.max_entry = std::stoi(val);
            else if (k == "gap_open") j.gap_open = std::stoi(val);
            else if (k == "gap_extend") j.gap_extend = std::stoi(val);
            else if (k == "lanes") j.lanes = std::stoi(val);
            else if (k == "bound") { std::istringstream b(val); std::string x; while (std::getline(b, x, ',')) bounds.push_back(x); }
            else if (k == "cell") { std::istringstream b(val); std::string x; while (std::getline(b, x, ',')) cells.push_back(x); }
            else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 2; }
        }
        j.qlens = qlens.data(); j.nqueries = (int64_t)qlens.size();
        const swp::SearchPairsLanesPlan p = swp::plan_search_pairs_lanes(j);
        const swp::SearchPairsPlan s = swp::plan_search_pairs(j);
        const int64_t full = p.nchunks ? p.chunk_pairs(0, j.npairs) : 0, last = p.nchunks ? p.chunk_pairs(p.nchunks - 1, j.npairs) : 0;
        printf("{\"last_chunk_pairs\": %lld, ", (long long)last);
        print_head("lanes", p.prof_need, p.bnd_need, p.items_need, p.cells_need, p.chunk, p.nchunks, p.launches, p.packed_launches, p.table, p.entry_of);
        printf("\"groups\": [");
        for (size_t g = 0; g < p.group.size(); ++g) print_group(g == 0, p.group[g], p.group[g].pk_q1, p.group[g].cells);
        printf("], \"launches\": [");
        for (size_t l = 0; l < p.launch.size(); ++l) {
            const int64_t c = p.group[(size_t)p.launch[l].group].cells;
            print_launch(l == 0, p.launch[l], p.launch[l].packed ? 1 : 0, swp::search_pairs_lanes_grid(p.launch[l], full, c), swp::search_pairs_lanes_grid(p.launch[l], last, c));
        }
        printf("]}, ");
        print_head("pairs", s.prof_need, s.bnd_need, s.items_need, 0, s.chunk, s.nchunks, s.launches, 0, s.table, s.entry_of);
        printf("\"groups\": [");
        for (size_t g = 0; g < s.group.size(); ++g) print_group(g == 0, s.group[g], s.group[g].cls_q0, 0);   // no packed entry: the packed part of a class ends where the class starts
        printf("], \"launches\": [");
        for (size_t l = 0; l < s.launch.size(); ++l) print_launch(l == 0, s.launch[l], 0, swp::search_pairs_grid(s.launch[l], full), swp::search_pairs_grid(s.launch[l], last));
        printf("]}, \"bounds\": [");
        for (size_t i = 0; i < bounds.size(); ++i) {
            const std::vector<int64_t> nc = list_of(bounds[i], ':');
            printf("%s[%lld, %lld]", i ? ", " : "", (long long)swp::search_pairs_packed_items_max(nc[0], nc[1]), (long long)swp::search_pairs_lanes_item_bytes(nc[0], nc[1]));
        }
        printf("], \"cell_index\": [");
        for (size_t i = 0; i < cells.size(); ++i) {
            const std::vector<int64_t> c = list_of(cells[i], ':');
            printf("%s%lld", i ? ", " : "", (long long)swp::search_pairs_cell(c[0], c[1], c[2], c[3], (int)c[4]));
        }
        printf("]}\n");
    }
    return 0;
}
