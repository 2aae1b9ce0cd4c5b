// Drives swp::plan_search_multi_lanes (smith-waterman_amd/csrc/sw_plan.cpp) for tests/test_search_multi_lanes_plan.py: one case per
// input line of name=value pairs, one JSON object per output line.  qlens, per_cu and packed_per_cu take comma-separated lists (one
// value for all three kernels, or three).  Beside the plan the line carries the table, the groups and the launches swp::plan_search_multi
// gives for the same job ("multi_table", "multi_groups", "multi_launches").  cover=1 walks the work items of every launch the way the
// kernels do -- a 32-bit item w is (rank0 + w / nq, q0 + w % nq), a packed item w the ranks rank0 + 2 (w / nq) and, inside the launch,
// the next one against q0 + w % nq -- and reports [fewest, most] visits of a (table entry, rank) pair and whether the entries' rows
// are all the queries ("cover": [min, max, rows_ok]).
#include <algorithm>
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

static void print_launch(bool first, const swp::MultiLaunch& x, int packed) {
    printf("%s{\"group\": %d, \"C\": %d, \"kernel\": %d, \"packed\": %d, \"q0\": %lld, \"nq\": %lld, \"rank0\": %lld, \"nranks\": %lld, \"items\": %lld, "
           "\"bnd_per\": %lld, \"grid\": %lld}", first ? "" : ", ", x.group, x.C, x.kernel, packed, (long long)x.q0, (long long)x.nq, (long long)x.rank0,
           (long long)x.nranks, (long long)x.items, (long long)x.bnd_per, (long long)x.grid);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        swp::SearchMultiLanesJob j;
        std::vector<int64_t> qlens;
        bool cover = false;
        for (int k = 0; k < swp::kSearchMultiKernels; ++k) j.per_cu[k] = j.packed_per_cu[k] = 3;
        std::istringstream in(line);
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq), val = kv.substr(eq + 1);
            if (k == "qlens") qlens = list_of(val);
            else if (k == "per_cu") { const std::vector<int64_t> v = list_of(val); for (int i = 0; i < swp::kSearchMultiKernels; ++i) j.per_cu[i] = (int)v[v.size() == 1 ? 0 : i]; }
            else if (k == "packed_per_cu") { const std::vector<int64_t> v = list_of(val); for (int i = 0; i < swp::kSearchMultiKernels; ++i) j.packed_per_cu[i] = (int)v[v.size() == 1 ? 0 : i]; }
            else if (k == "longest") j.longest = std::stoll(val);
            else if (k == "nonempty") j.nonempty = std::stoll(val);
            else if (k == "num_cus") j.num_cus = std::stoi(val);
            else if (k == "budget_bytes") j.budget_bytes = std::stoll(val);
            else if (k == "max_items") j.max_items = std::stoll(val);
            else if (k == "max_entry") j.max_entry = std::stoi(val);
            else if (k == "gap_open") j.gap_open = std::stoi(val);
            else if (k == "gap_extend") j.gap_extend = std::stoi(val);
            else if (k == "lanes") j.lanes = std::stoi(val);
            else if (k == "cover") cover = std::stoi(val) != 0;
            else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 2; }
        }
        j.qlens = qlens.data(); j.nqueries = (int64_t)qlens.size();
        const swp::SearchMultiLanesPlan p = swp::plan_search_multi_lanes(j);
        const swp::SearchMultiPlan m = swp::plan_search_multi(j);
        printf("{\"prof_need\": %zu, \"bnd_need\": %zu, \"packed_launches\": %lld, \"multi_prof_need\": %zu, \"multi_bnd_need\": %zu, ", p.prof_need, p.bnd_need,
               (long long)p.packed_launches, m.prof_need, m.bnd_need);
        print_table("table", p.table);
        printf(", ");
        print_table("multi_table", m.table);
        printf(", \"groups\": [");
        for (size_t g = 0; g < p.group.size(); ++g) printf("%s[%lld, %lld, %lld]", g ? ", " : "", (long long)p.group[g].q0, (long long)p.group[g].nq, (long long)p.group[g].prof_bytes);
        printf("], \"multi_groups\": [");
        for (size_t g = 0; g < m.group.size(); ++g) printf("%s[%lld, %lld, %lld]", g ? ", " : "", (long long)m.group[g].q0, (long long)m.group[g].nq, (long long)m.group[g].prof_bytes);
        printf("], \"launches\": [");
        for (size_t l = 0; l < p.launch.size(); ++l) print_launch(l == 0, p.launch[l], p.launch[l].packed ? 1 : 0);
        printf("], \"multi_launches\": [");
        for (size_t l = 0; l < m.launch.size(); ++l) print_launch(l == 0, m.launch[l], 0);
        printf("]");
        if (cover) {
            const int64_t n = j.nqueries, r = j.nonempty;
            std::vector<int> seen((size_t)(n * r), 0);
            bool in_range = true;
            for (const swp::MultiLanesLaunch& l : p.launch)
                for (int64_t w = 0; w < l.items; ++w) {
                    const int64_t t = l.q0 + w % l.nq, step = w / l.nq;
                    const int64_t ra = l.rank0 + (l.packed ? 2 * step : step);
                    const int64_t last = l.packed && 2 * step + 1 < l.nranks ? ra + 1 : ra;    // the partner, where it lies inside the launch
                    for (int64_t k = ra; k <= last; ++k) {
                        if (t < 0 || t >= n || k < 0 || k >= r || k >= l.rank0 + l.nranks) { in_range = false; continue; }
                        ++seen[(size_t)(t * r + k)];
                    }
                }
            std::vector<int64_t> rows;
            for (const swk::MultiQuery& d : p.table) rows.push_back(d.row);
            std::sort(rows.begin(), rows.end());
            bool rows_ok = true;
            for (int64_t q = 0; q < n; ++q) rows_ok = rows_ok && rows[(size_t)q] == q;
            const int lo = seen.empty() ? 1 : *std::min_element(seen.begin(), seen.end()), hi = seen.empty() ? 1 : *std::max_element(seen.begin(), seen.end());
            printf(", \"cover\": [%d, %d, %d]", in_range ? lo : -1, hi, rows_ok ? 1 : 0);
        }
        printf("}\n");
    }
    return 0;
}
