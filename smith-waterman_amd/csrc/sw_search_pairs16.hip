// sw_search_pairs16.hip -- the scores of a device pair list on packed 16-bit lanes ("search_pairs_lanes" = 16, gfx950):
// sw_search_pairs_pk_wave<C> is sw_search_affine_pairs_wave<C> (sw_search_pairs.hip) with TWO listed pairs of one query per wave, in the
// manner of sw_search_multi_pk_wave<C>: one pair in the low halves (A), its partner in the high halves (B).  The sweep is
// sw_gotoh_sweep16.inc, unchanged; what the call writes is, byte for byte, what the 32-bit kernel writes for the same list.
//
// Two pairs may share a wave only if they name the same query: one profile, one qlen, one strip count.  The many-query search finds its
// partners in the handle's sorted schedule; a list has no order, so the device pairs the pairs itself.  The unit of the binning is the
// CELL (packed query, bucket), bucket = floor(log2(len x qpad)) as in sw_search_pairs.hip: inside a cell the lengths differ by less
// than a factor of two, so a full item keeps at least 3/4 of its half-lanes on rows inside a target.  Per (chunk, group) that holds
// packed queries (swp::plan_search_pairs_lanes), three launches:
//   * sw_search_pairs_pk_bin<false> looks every pair up as sw_search_pairs_bin does (the same function: indices compared unsigned before
//     anything is loaded through them) and counts it -- a pair of a packed query into its cell, any other into count[class][bucket] of
//     the 32-bit lists.
//   * sw_search_pairs_pk_scan, ONE workgroup, gives every cell its base in units of two-pair items: the cells lie class after class,
//     inside a class the heaviest bucket first (swp::search_pairs_cell), so an exclusive prefix sum of ceil(n / 2) over them is the
//     order the score launches want.  It DEFINES the empty half of every odd cell's last item (length 0: whatever the item buffer held
//     before is gone), leaves every class's two-pair list {length, first item}, places the 32-bit lists behind the two-pair items
//     (a two-pair item is two SearchPairItem long) and adds the (chunk, group)'s two-pair items to the call's total.
//   * sw_search_pairs_pk_bin<true> looks every pair up again and writes its item: a packed one takes r from its cell's cursor and is
//     half r & 1 of item base + r / 2; the ranks 0 .. n - 1 of a cell are all handed out, so the half the scan defined (half 1 of the
//     last item of an odd cell) is exactly the one no pair gets, and half 0 of every item is a pair.
// The cursor decides which pair meets which partner and in which half.  That changes no byte of the output: no instruction of the sweep
// moves a value between the halves, and what the halves share -- the steps, the visits of the arg-max branch -- changes nothing that
// counts (the header of sw_search_multi16.hip proves both).  The same bytes come out on every run.
//
// The sweep takes its steps from lenA, so the wave puts the longer half in A itself, wave-uniformly, after loading the item.  An item
// with an empty half runs with a partner of length 0 -- every row PAD, nothing loaded through its descriptor -- whose result is not
// stored, as the odd last rank does in sw_search_multi_pk_wave.  Either result goes to results[out] of its own half; two halves that
// name the same target (a duplicate in the list) are partners like any other.
//
// Nothing wraps: the planner sends a query here under swp::search_multi_packed against the handle's longest target, which bounds every
// target a list can name.  The boundary workspace per resident wave is that of the 32-bit launch of the class.
// All global writes are vector stores or plain C++, all atomics vector atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"
#include "sw_wave.h"
#include "sw_gotoh_cell16.h"
#include "sw_search_pairs_lookup.h"

namespace swk {

namespace {

// the three arrays behind the control words: counts, cursors, bases
__device__ __forceinline__ unsigned int* spk_cells(const SearchPairsPackedBinParams& p, int which) {
    return (unsigned int*)((char*)p.pk + swp::kSearchPairsCellsHead) + which * p.cells;
}

// the cell of a packed entry t of class k and a bucket, or -1: t is not one of the class's packed entries
__device__ __forceinline__ int64_t spk_cell(const SearchPairsPackedBinParams& p, int k, int64_t t, int bucket) {
    if (t >= p.pk_q1[k]) return -1;
    int64_t cell0 = 0;
    for (int c = 0; c < k; ++c) cell0 += SW_SP_BUCKETS * (p.pk_q1[c] - p.bin.cls_q0[c]);
    return swp::search_pairs_cell(cell0, p.pk_q1[k] - p.bin.cls_q0[k], p.bin.cls_q0[k], t, bucket);
}

}  // namespace

// One thread per pair of the chunk.  SCATTER = false counts, SCATTER = true, two launches later, writes the items.
template <bool SCATTER>
__global__ void __launch_bounds__(256) sw_search_pairs_pk_bin(SearchPairsPackedBinParams p) {
    unsigned int* const count = spk_cells(p, 0);
    unsigned int* const cursor = spk_cells(p, 1);
    const unsigned int* const base = spk_cells(p, 2);
    SearchPairItem2* const items2 = (SearchPairItem2*)p.bin.items;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.bin.np; i += (int64_t)gridDim.x * blockDim.x) {
        SearchPairItem it;
        int k = 0, bucket = 0;
        if (!sp_lookup(p.bin, i, it, k, bucket)) continue;
        const int64_t cell = spk_cell(p, k, it.entry, bucket);
        if (cell >= 0) {
            if constexpr (!SCATTER) atomicAdd(&count[cell], 1u);
            else {
                const unsigned int r = atomicAdd(&cursor[cell], 1u);
                items2[base[cell] + (r >> 1)].half[r & 1] = it;
            }
        } else {
            if constexpr (!SCATTER) atomicAdd(&p.bin.ctl->count[k][bucket], 1u);
            else p.bin.items[p.pk->base32[k][bucket] + atomicAdd(&p.bin.ctl->cursor[k][bucket], 1u)] = it;
        }
    }
}
template __global__ void sw_search_pairs_pk_bin<false>(SearchPairsPackedBinParams);
template __global__ void sw_search_pairs_pk_bin<true>(SearchPairsPackedBinParams);

// One workgroup, between the two.  Thread t scans the cells [t per, (t + 1) per) of the linear order.
__global__ void __launch_bounds__(256) sw_search_pairs_pk_scan(SearchPairsPackedBinParams p) {
    __shared__ unsigned int part[256], first[SW_SP_CLASSES + 1], total;
    const unsigned int* const count = spk_cells(p, 0);
    unsigned int* const base = spk_cells(p, 2);
    SearchPairItem2* const items2 = (SearchPairItem2*)p.bin.items;
    const int64_t per = (p.cells + 255) / 256, lo0 = (int64_t)threadIdx.x * per, lo = lo0 < p.cells ? lo0 : p.cells, hi = lo + per < p.cells ? lo + per : p.cells;
    unsigned int sum = 0;
    for (int64_t c = lo; c < hi; ++c) sum += (count[c] + 1) >> 1;
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int at = 0;
        for (int t = 0; t < 256; ++t) { const unsigned int n = part[t]; part[t] = at; at += n; }
        total = at;
        for (int k = 0; k <= SW_SP_CLASSES; ++k) first[k] = at;    // (a class behind the last cell starts at the end)
    }
    __syncthreads();
    // where the classes' cells start in the linear order
    int64_t cls_cell[SW_SP_CLASSES];
    for (int k = 0, c0 = 0; k < SW_SP_CLASSES; ++k) { cls_cell[k] = c0; c0 += SW_SP_BUCKETS * (int)(p.pk_q1[k] - p.bin.cls_q0[k]); }
    unsigned int at = part[threadIdx.x];
    for (int64_t c = lo; c < hi; ++c) {
        const unsigned int n = count[c];
        for (int k = 0; k < SW_SP_CLASSES; ++k)
            if (c == cls_cell[k]) first[k] = at;
        base[c] = at;
        if (n & 1) items2[at + (n >> 1)].half[1] = SearchPairItem{0, 0, 0, 0};   // the half no pair of this call gets
        at += (n + 1) >> 1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 0; k < SW_SP_CLASSES; ++k) p.pk->list[k] = SearchPairsList{first[k + 1] - first[k], first[k]};
        // the 32-bit lists behind the two-pair items, as sw_search_pairs_bin<true> lays them out: class after class, heaviest bucket first
        unsigned int at32 = 2 * total;
        for (int k = 0; k < SW_SP_CLASSES; ++k) {
            const unsigned int first32 = at32;
            for (int b = SW_SP_BUCKETS - 1; b >= 0; --b) {
                p.pk->base32[k][b] = at32;
                at32 += p.bin.ctl->count[k][b];
            }
            p.bin.ctl->list[k] = SearchPairsList{at32 - first32, first32};
        }
        atomicAdd(p.total, (unsigned long long)total);
    }
}

// C: query columns per lane (4, 8, 16)
template <int C>
__global__ void __launch_bounds__(256) sw_search_pairs_pk_wave(SearchPairsPackedParams p) {
    static_assert(C % 4 == 0 && C <= 16, "C is a multiple of 4");
    constexpr int NQ = C / 4;
    // this launch's list: as long as the scan counted, behind the lists of the classes before
    const SearchPairsList list = *p.list;
    const u32 nitems = list.n;
    if (nitems == 0) return;
    const SearchPairItem2* const items = p.items + list.first;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t slot = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;     // resident wave: its own boundary column
    const u32 ge2 = ((u32)p.ge & 0xFFFFu) * 0x10001u, goe2 = ((u32)p.goe & 0xFFFFu) * 0x10001u;
    // (a launch without a boundary workspace holds one-strip queries only: nothing goes through the empty descriptor)
    const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc((void*)(p.bnd ? p.bnd + slot * p.bnd_per : nullptr), 0,
                                                                        p.bnd ? (int)(p.bnd_per * 4) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc((void*)p.counter, 0, 4, 0x00020000);
    const u32 voffL0 = lane == 0 ? 0u : SW_OOB;    // lane 0 alone touches the counter and the results

    for (;;) {
        // the next item: a vector buffer atomic of lane 0, read back into a scalar; no lane-divergent branch anywhere in this loop
        const u32 w = (u32)__builtin_amdgcn_readlane(__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(1, rC, (int)voffL0, 0, 0), 0);
        if (w >= nitems) break;
        const SearchPairItem h0 = items[w].half[0], h1 = items[w].half[1];
        const MultiQuery d = p.queries[sw_uniform(h0.entry)];          // (half 0 is never empty; both halves name this query)
        // the longer half is A: the steps of the sweep come from lenA.  Wave-uniform: every lane loaded the same item
        const int len0 = sw_uniform(h0.len), len1 = sw_uniform(h1.len);
        const bool swap = len1 > len0;
        const int lenA = swap ? len1 : len0, lenB = swap ? len0 : len1;
        const int64_t startA = sw_uniform64(swap ? h1.start : h0.start), startB = sw_uniform64(swap ? h0.start : h1.start);
        const int64_t outA = sw_uniform64(swap ? h1.out : h0.out), outB = sw_uniform64(swap ? h0.out : h1.out);
        const bool partner = lenB > 0;             // an empty half: every row of B is PAD, its result is not stored
        const int qlen = sw_uniform(d.qlen), nstrips = sw_uniform(d.nstrips);
        const int64_t M = qlen + 1;
        const u32 qpad = (u32)sw_uniform(d.qpad);
        const bool multi = nstrips > 1;
        const __amdgpu_buffer_rsrc_t rQ = __builtin_amdgcn_make_buffer_rsrc((void*)(p.prof + sw_uniform64(d.prof_off)), 0, (int)(SW_SEARCH_ROWS * qpad), 0x00020000);
        // the targets' bytes through descriptors of exactly their extents: rows outside read 0 and are mapped to PAD by the sweep
        const __amdgpu_buffer_rsrc_t rTA = __builtin_amdgcn_make_buffer_rsrc((void*)(p.db + startA), 0, lenA, 0x00020000);
        const __amdgpu_buffer_rsrc_t rTB = __builtin_amdgcn_make_buffer_rsrc((void*)(p.db + startB), 0, lenB, 0x00020000);
#include "sw_gotoh_sweep16.inc"
        gs16_store(p.results + outA, kbestA, voffL0);
        if (partner) gs16_store(p.results + outB, kbestB, voffL0);
    }
}

template __global__ void sw_search_pairs_pk_wave<4>(SearchPairsPackedParams);
template __global__ void sw_search_pairs_pk_wave<8>(SearchPairsPackedParams);
template __global__ void sw_search_pairs_pk_wave<16>(SearchPairsPackedParams);

}  // namespace swk
