// sw_top_key.h -- the sort key the two selections share (sw_search_top.hip, sw_top_pairs.hip): score << tbits | (2^tbits - 1 - target)
// with tbits = ceil(log2 ntargets).  Plain integer order of the keys is the rank order: score descending, then target ascending.
// Scores are taken modulo 2^24 (the bound every search call enforces) so that no input can carry a key out of its fields.
#pragma once
#include <hip/hip_runtime.h>

namespace swk {

__device__ __forceinline__ unsigned long long top_key(long long score, long long target, int tbits) {
    return ((unsigned long long)(score & 0xFFFFFF) << tbits) | (((1ull << tbits) - 1) - (unsigned long long)target);
}

}  // namespace swk
