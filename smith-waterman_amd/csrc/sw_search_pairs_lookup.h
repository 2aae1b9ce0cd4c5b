// sw_search_pairs_lookup.h -- the look-up the binning launches of a pair list share (sw_search_pairs.hip, sw_search_pairs16.hip; gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"

namespace swk {

// Pair i of the chunk -> its item and its (class, bucket), or "no item of this group".
__device__ __forceinline__ bool sp_lookup(const SearchPairsBinParams& p, int64_t i, SearchPairItem& it, int& k, int& bucket) {
    const sw_pair pr = p.pairs[p.p0 + i];
    if ((u64)pr.query >= (u64)p.nqueries) return false;    // unsigned: a negative index is a huge one; nothing was loaded through it yet
    const int64_t t = p.entry_of[pr.query];
    if (t < p.cls_q0[0] || t >= p.cls_q0[SW_SP_CLASSES]) return false;   // a query of another group: that group's pass takes the pair
    if ((u64)pr.target >= (u64)p.ntargets) return false;
    const int64_t start = p.offsets[pr.target], len = p.offsets[pr.target + 1] - start;
    if (len <= 0) return false;                            // an empty target: the zeros stay
    it.start = start; it.out = p.p0 + i; it.len = (int)len; it.entry = (int)t;
    k = t < p.cls_q0[1] ? 0 : (t < p.cls_q0[2] ? 1 : 2);
    bucket = swp::search_pairs_bucket(len, p.queries[t].qpad);
    return true;
}

}  // namespace swk
