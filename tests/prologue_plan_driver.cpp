// Prints what the fill planner (smith-waterman_amd/csrc/sw_plan.cpp) decides about the prologue's alphabet scan, for
// tests/test_prologue_plan.py: one case per input line "cols rows s2w debug_flags", one output line with the limit, the number of
// tiles and every tile's scan_all.  (tests/fill_plan_driver.cpp prints the rest of a plan; its output has no field for this.)
#include <cstdio>
#include "../smith-waterman_amd/csrc/sw_plan.h"

int main() {
    long long cols, rows, s2w, flags;
    while (scanf("%lld %lld %lld %lld", &cols, &rows, &s2w, &flags) == 4) {
        swp::PlanJob j;
        swp::DeviceFacts d;
        swp::PlanOptions o;
        j.cols = cols; j.rows = rows;
        d.num_cus = 256; d.xcd_round_robin = true; d.s2_per_cu = 1;
        o.s2w = s2w; o.debug_flags = flags;
        const swp::FillPlan p = swp::plan_fill(j, d, o);
        printf("%lld %d %lld", (long long)swp::kScanAllLetters, p.two_cols ? 1 : 0, (long long)p.ntile);
        for (int64_t t = 0; p.two_cols && t < p.ntile; ++t) printf(" %d", p.tile[t].scan_all);
        printf("\n");
    }
    return 0;
}
