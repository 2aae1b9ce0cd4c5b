// sw_search_pairs.hip -- the scores of a device list of (query, target) pairs against a prepared database (sw_db_search_affine_pairs,
// gfx950): the rescoring stage behind a pre-filter, score and arg-max only.
//
// The host of this call knows the queries and the handle's longest target, but neither which pairs the list names nor how long their
// targets are.  So the device turns a chunk of the list into work lists first, as sw_align_hits.hip does for a hit table:
//   * sw_search_pairs_bin<false> looks at every pair of the chunk: query inside [0, nqueries), target inside [0, ntargets) -- both
//     compared UNSIGNED before anything is loaded through them (ah_lookup's rule) --, the query one of this group's, the target not
//     empty.  A pair that passes is counted into count[class of its query][bucket], bucket = floor(log2(len x qpad)).  A pair that can
//     never become an item keeps the {0, 0, 0} the call's memset wrote before the first launch; this kernel writes no result.
//   * sw_search_pairs_bin<true>, a launch later, does the same look-up and writes the item {start, out = p, len, entry}.  The lists of
//     the classes lie back to back in the item buffer, and inside a class's list the buckets, HEAVIEST FIRST: an item goes to (items of
//     the classes before) + (items of the heavier buckets) + (an atomic cursor).  The cursor decides the ORDER in which independent
//     items are taken, nothing an item computes or where it writes: the outputs of two runs are the same bytes.
//   * sw_search_affine_pairs_wave<C>, ONE launch per class: its waves take the items of the class's list from a work counter, the
//     longest pairs first.  Nothing is sized by the item, so the buckets need no launches of their own.  The list's length is read from
//     device memory (the grid was planned on the host for the most it could be); the waves of an empty list leave after that one load.
//
// The sweep of an item -- the cell recurrence, the state per lane, the software-pipelined loads, the boundary column between strips and
// the arg-max -- is the text of sw_gotoh_sweep.inc, which sw_search_affine_wave<C> and sw_search_affine_multi_wave<C> include too;
// the header of sw_search_affine.hip argues it (cells outside the matrix, ties, overflow).  Per item the wave rebuilds, from the item and
// the query's entry of the call's table, the profile descriptor (exactly 257 x qpad bytes), the target descriptor (exactly len bytes),
// qlen and the strips; they are loaded with vector loads and made scalars with readfirstlane.  The result goes to results[out], the pair's place in the caller's list.  All global writes are vector
// stores or plain C++.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"
#include "sw_wave.h"
#include "sw_search_pairs_lookup.h"

namespace swk {

// One thread per pair of the chunk.  SCATTER = false counts the items of every (class, bucket); SCATTER = true, launched behind it,
// writes the items.  Plain global atomics (vector instructions).
template <bool SCATTER>
__global__ void __launch_bounds__(256) sw_search_pairs_bin(SearchPairsBinParams p) {
    __shared__ unsigned int base[SW_SP_CLASSES * SW_SP_BUCKETS];
    if constexpr (SCATTER) {
        // the counts are final since the launch before.  Every workgroup works out where each (class, bucket) starts: class after
        // class, inside a class the heaviest bucket first; workgroup 0 also leaves every class's {length, first item} for its launch.
        for (int s = (int)threadIdx.x; s < SW_SP_CLASSES * SW_SP_BUCKETS; s += (int)blockDim.x) base[s] = p.ctl->count[s / SW_SP_BUCKETS][s % SW_SP_BUCKETS];
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned int at = 0;
            for (int k = 0; k < SW_SP_CLASSES; ++k) {
                const unsigned int first = at;
                for (int b = SW_SP_BUCKETS - 1; b >= 0; --b) {
                    const unsigned int n = base[k * SW_SP_BUCKETS + b];
                    base[k * SW_SP_BUCKETS + b] = at;
                    at += n;
                }
                if (blockIdx.x == 0) p.ctl->list[k] = SearchPairsList{at - first, first};
            }
        }
        __syncthreads();
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.np; i += (int64_t)gridDim.x * blockDim.x) {
        SearchPairItem it;
        int k = 0, bucket = 0;
        if (!sp_lookup(p, i, it, k, bucket)) continue;
        if constexpr (!SCATTER) atomicAdd(&p.ctl->count[k][bucket], 1u);
        else p.items[base[k * SW_SP_BUCKETS + bucket] + atomicAdd(&p.ctl->cursor[k][bucket], 1u)] = it;
    }
}
template __global__ void sw_search_pairs_bin<false>(SearchPairsBinParams);
template __global__ void sw_search_pairs_bin<true>(SearchPairsBinParams);

// C: query columns per lane (4, 8, 16)
template <int C>
__global__ void __launch_bounds__(256) sw_search_affine_pairs_wave(SearchPairsParams p) {
    static_assert(C % 4 == 0 && C <= 16, "C is a multiple of 4");
    constexpr int NQ = C / 4;
    // this launch's list: as long as the binning counted, behind the lists of the classes before
    const SearchPairsList list = *p.list;
    const u32 nitems = list.n;
    if (nitems == 0) return;
    const SearchPairItem* const items = p.items + list.first;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t slot = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;     // resident wave: its own boundary column
    const int ge = p.ge, goe = p.goe;
    // (a launch without a boundary workspace holds one-strip queries only: nothing goes through the empty descriptor)
    const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc((void*)(p.bnd ? p.bnd + slot * p.bnd_per : nullptr), 0,
                                                                        p.bnd ? (int)(p.bnd_per * 4) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc((void*)p.counter, 0, 4, 0x00020000);
    const u32 voffL0 = lane == 0 ? 0u : SW_OOB;    // lane 0 alone touches the counter and the result

    for (;;) {
        // the next item: a vector buffer atomic of lane 0 (the other lanes' offsets lie beyond the descriptor: dropped), read
        // back from lane 0 into a scalar; no lane-divergent branch anywhere in this loop (sw_search_wave says why)
        const u32 w = (u32)__builtin_amdgcn_readlane(__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(1, rC, (int)voffL0, 0, 0), 0);
        if (w >= nitems) break;
        // the item and its query: loads of wave-uniform addresses inside a loop that stores, which the compiler issues as vector loads
        // (global_load_dwordx2 / x3 / x4 in the gfx950 ISA of all three instantiations); readfirstlane tells it that these are scalars
        const SearchPairItem it = items[w];
        const MultiQuery d = p.queries[sw_uniform(it.entry)];
        const int len = sw_uniform(it.len);
        const int64_t start = sw_uniform64(it.start), out = sw_uniform64(it.out);
        const int qlen = sw_uniform(d.qlen), nstrips = sw_uniform(d.nstrips);
        const int64_t M = qlen + 1;
        const u32 qpad = (u32)sw_uniform(d.qpad);
        const bool multi = nstrips > 1;
        // the query's profile and the target's bytes through descriptors of exactly their extents: rows outside the target read 0 and
        // are mapped to PAD by the sweep
        const __amdgpu_buffer_rsrc_t rQ = __builtin_amdgcn_make_buffer_rsrc((void*)(p.prof + sw_uniform64(d.prof_off)), 0, (int)(SW_SEARCH_ROWS * qpad), 0x00020000);
        const __amdgpu_buffer_rsrc_t rT = __builtin_amdgcn_make_buffer_rsrc((void*)(p.db + start), 0, len, 0x00020000);
#include "sw_gotoh_sweep.inc"
        {
            const __amdgpu_buffer_rsrc_t rR = __builtin_amdgcn_make_buffer_rsrc((void*)(p.results + out), 0, (int)sizeof(sw_result), 0x00020000);
            const u64 score = kbest >> 40, pos = kbest ? SW_KEY_IDX_MASK - (kbest & SW_KEY_IDX_MASK) : 0;
            const sw_v4i v = {(int)(u32)pos, (int)(u32)(pos >> 32), (int)(u32)score, 0};
            __builtin_amdgcn_raw_buffer_store_b128(v, rR, (int)voffL0, 0, 0);                 // max_pos, max_score
            __builtin_amdgcn_raw_buffer_store_b64(sw_v2i{0, 0}, rR, (int)voffL0, 16, 0);      // path_len
        }
    }
}

template __global__ void sw_search_affine_pairs_wave<4>(SearchPairsParams);
template __global__ void sw_search_affine_pairs_wave<8>(SearchPairsParams);
template __global__ void sw_search_affine_pairs_wave<16>(SearchPairsParams);

}  // namespace swk
