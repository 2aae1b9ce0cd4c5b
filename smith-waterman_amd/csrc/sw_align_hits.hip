// sw_align_hits.hip -- the alignments of the hits of many queries, straight from a device hit table (sw_db_align_affine_hits, gfx950).
//
// The host of this call knows the queries and the handle's longest target, but not which targets the table names: it cannot size a slot
// by the longest hit as sw_align_affine_device does, and a slot for the handle's longest target would leave a few dozen waves at work.
// So the device sorts the work by size first, with no spinning and no allocator:
//   * sw_align_hits_bin<false> looks at every entry (q, r) of a group's rows: used (r < clamp(nhits[q], 0, top)), target inside
//     [0, ntargets) -- compared UNSIGNED before anything is loaded through it --, target not empty.  Every other entry gets its all-zero
//     sw_alignment here and becomes no item.  A used entry's direction matrix takes len x qpad bytes (qpad: its query's padded
//     length, the row stride); the kernel counts it into the smallest tier of the query's class that holds it (swp::plan_align_hits).
//   * sw_align_hits_bin<true>, a launch later, does the same look-up and writes the item into its list: the lists of a class lie back
//     to back in the class's part of the item buffer, tier after tier, each as long as the first launch counted.  The position inside a
//     list comes from an atomic and so differs from run to run -- it decides the ORDER in which independent items are taken, nothing an
//     item computes or where it writes: the outputs of two runs are the same bytes.
//   * sw_align_hits_wave<C>, one launch per (class, tier), largest tier first: every wave owns a slot of the tier's size and takes items
//     from the list's work counter.  The length of the list is read from device memory (the grid was planned on the host for the most
//     it could be); the waves of an empty list leave after that one load.
//
// The fill and the walk are the texts sw_align_affine_wave<C> runs: sw_align_dirfill.inc and sw_align_walk.inc.  What is per launch
// there is rebuilt per item here, from the item and the query's entry of the call's table: the profile descriptor (exactly 257 x qpad
// bytes at the query's offset), qlen, qpad -- the row stride of the direction matrix inside the slot -- and the strips, and the output
// index q * top + r.  They are loaded with vector loads and made scalars with readfirstlane.  All global writes are vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"
#include "sw_wave.h"

namespace swk {

namespace {

// The look-up both binning launches share: entry e of the group's rows -> its item and its (class, tier), or "zero alignment".
__device__ __forceinline__ bool ah_lookup(const AlignHitsBinParams& p, int64_t e, AlignHitItem& it, int& k, int& tier) {
    const int64_t t = e / p.top, r = e - t * p.top;
    const MultiQuery d = p.queries[t];
    it.out = d.row * p.top + r;
    it.entry = (int)t;
    it.start = 0; it.len = 0;
    int64_t used = p.top;
    if (p.nhits) { const int64_t n = p.nhits[d.row]; used = n < 0 ? 0 : (n < p.top ? n : p.top); }
    if (r >= used) return false;
    const u64 target = (u64)p.hits[it.out].target;
    if (target >= (u64)p.ntargets) return false;           // unsigned: a negative index is a huge one; nothing was loaded through it yet
    const int64_t start = p.offsets[target], len = p.offsets[target + 1] - start;
    if (len <= 0) return false;                            // an empty target: the zero alignment
    it.start = start; it.len = (int)len;
    k = t < p.cls_q0[1] ? 0 : (t < p.cls_q0[2] ? 1 : 2);
    const int64_t bytes = p.log_band[k] ? swp::align_ckpt_slot_bytes(len, d.qpad, 1ll << p.log_band[k]) : len * (int64_t)d.qpad;
    tier = 0;
    while (tier + 1 < p.ntiers[k] && bytes > p.bound[k][tier]) ++tier;   // (the top tier holds the worst case: the host has checked that)
    return true;
}

}  // namespace

// One thread per entry of the group's rows.  SCATTER = false counts the items of every list and writes the zero alignments;
// SCATTER = true, launched behind it, writes the items.  Plain global atomics (vector instructions).
template <bool SCATTER>
__global__ void __launch_bounds__(256) sw_align_hits_bin(AlignHitsBinParams p) {
    const int64_t total = p.nq * p.top;
    if constexpr (SCATTER) {   // the counts are final since the launch before: one thread reports how many lists of the group hold items
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            unsigned int n = 0;
            for (int k = 0; k < SW_AH_CLASSES; ++k)
                for (int t = 0; t < SW_AH_TIERS; ++t) n += p.ctl->count[k][t] != 0;
            atomicAdd(p.filled, n);
        }
    }
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        AlignHitItem it;
        int k = 0, tier = 0;
        const bool item = ah_lookup(p, e, it, k, tier);
        if constexpr (!SCATTER) {
            if (item) atomicAdd(&p.ctl->count[k][tier], 1u);
            else p.aln[it.out] = sw_alignment{0, 0, 0, 0, 0, 0, 0};
        } else if (item) {
            int64_t base = p.cls_q0[k] * p.top;            // the class's part of the list, then the lower tiers' items
            for (int t = 0; t < tier; ++t) base += p.ctl->count[k][t];
            p.items[base + atomicAdd(&p.ctl->cursor[k][tier], 1u)] = it;
        }
    }
}
template __global__ void sw_align_hits_bin<false>(AlignHitsBinParams);
template __global__ void sw_align_hits_bin<true>(AlignHitsBinParams);

// C: query columns per lane (4, 8, 16)
template <int C>
__global__ void __launch_bounds__(256) sw_align_hits_wave(AlignHitsParams p) {
    static_assert(C % 4 == 0 && C <= 16, "C is a multiple of 4");
    constexpr int NQ = C / 4;
    using walk_round_t = int;
    __shared__ sw_v4i win_all[4][SW_WIN * SW_WIN / 16];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t slot = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;     // resident wave: its own boundary column and direction matrix
    if (slot >= p.nslots) return;
    // this launch's list: behind the lists of the class's lower tiers, as long as the binning counted
    u32 first = 0;
    for (int t = 0; t < p.tier; ++t) first += p.counts[t];
    const u32 nitems = p.counts[p.tier];
    if (nitems == 0) return;
    const AlignHitItem* const items = p.items + first;
    const int ge = p.ge, goe = p.goe;
    // (a launch without a boundary workspace holds one-strip queries only: nothing goes through the empty descriptor)
    const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc((void*)(p.bnd ? p.bnd + slot * p.bnd_per : nullptr), 0,
                                                                        p.bnd ? (int)(p.bnd_per * 4) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rD = __builtin_amdgcn_make_buffer_rsrc((void*)(p.dir + slot * p.slot_bytes), 0, (int)p.slot_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc((void*)p.counter, 0, 4, 0x00020000);
    const u32 voffL0 = lane == 0 ? 0u : SW_OOB;    // lane 0 alone touches the counter and the result
    sw_v4i* const win = win_all[wave];
    const unsigned char* const winb = (const unsigned char*)win;
    const bool has_ops = p.ops != nullptr;
    const int64_t ops_cap = p.ops_cap;
    const int ops_size = (int)(has_ops ? (ops_cap < 0x7FFFFF00ll ? ops_cap : 0x7FFFFF00ll) : 0);

    for (;;) {
        // the next item: a vector buffer atomic of lane 0, read back into a scalar (sw_search_wave says why)
        const u32 w = (u32)__builtin_amdgcn_readlane(__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(1, rC, (int)voffL0, 0, 0), 0);
        if (w >= nitems) break;
        // the item and its query: vector loads of wave-uniform addresses; readfirstlane tells the compiler that these are scalars
        const AlignHitItem it = items[w];
        const MultiQuery d = p.queries[sw_uniform(it.entry)];
        const int len = sw_uniform(it.len);
        const int64_t start = sw_uniform64(it.start), out = sw_uniform64(it.out);
        const int qlen = sw_uniform(d.qlen), nstrips = sw_uniform(d.nstrips);
        const int64_t M = qlen + 1;
        const u32 qpad = (u32)sw_uniform(d.qpad);          // the profile's row length and the row stride of the direction matrix
        const bool multi = nstrips > 1;
        const __amdgpu_buffer_rsrc_t rQ = __builtin_amdgcn_make_buffer_rsrc((void*)(p.prof + sw_uniform64(d.prof_off)), 0, (int)(SW_SEARCH_ROWS * qpad), 0x00020000);
        const __amdgpu_buffer_rsrc_t rT = __builtin_amdgcn_make_buffer_rsrc((void*)(p.db + start), 0, len, 0x00020000);
#include "sw_align_dirfill.inc"

        // ---- the walk: every store of this hit has left the wave; the matrix is read past the L1 (sc1), a window at a time
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const __amdgpu_buffer_rsrc_t rO = __builtin_amdgcn_make_buffer_rsrc((void*)(has_ops ? p.ops + out * ops_cap : nullptr), 0, ops_size, 0x00020000);
#define SW_WALK_BAND const int bf = 1, bl = len;   // the slot holds the whole matrix
#define SW_WALK_ALN __builtin_amdgcn_make_buffer_rsrc((void*)(p.aln + out), 0, (int)sizeof(sw_alignment), 0x00020000)
#include "sw_align_walk.inc"
#undef SW_WALK_BAND
#undef SW_WALK_ALN
    }
}

template __global__ void sw_align_hits_wave<4>(AlignHitsParams);
template __global__ void sw_align_hits_wave<8>(AlignHitsParams);
template __global__ void sw_align_hits_wave<16>(AlignHitsParams);

}  // namespace swk
