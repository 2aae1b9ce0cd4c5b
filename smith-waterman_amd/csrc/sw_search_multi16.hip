// sw_search_multi16.hip -- the many-query affine search on packed 16-bit lanes ("search_lanes" = 16, gfx950): sw_search_multi_pk_wave<C>
// is sw_search_affine_multi_wave<C> (sw_search_multi.hip) with TWO targets of one query per wave, in the manner of sw_prefilter_wave16<C>:
// schedule rank rank0 + 2 r in the low halves (target A), rank0 + 2 r + 1 in the high halves (target B).  Persistent waves, the work
// counter taken with lane 0's vector buffer atomic, a wave-uniform MultiQuery per item, the profiles of sw_search_profile_submat_multi /
// sw_search_profile_pssm_multi unchanged.  The sweep is sw_gotoh_sweep16.inc.  What it writes is, byte for byte, what the 32-bit kernel
// writes for the same (query, target) pairs.
//
// Item w of a launch runs the ranks rank0 + 2 (w / nq) and the next one against entry w % nq of the launch's queries (sw_plan.h,
// plan_search_multi_lanes).  The schedule is sorted by decreasing length, so A is the longer target: the steps of the item come from
// lenA, and B's rows beyond lenB read the PAD profile row like any row outside a target.  An odd last rank runs with a partner of
// length 0 -- every row PAD -- whose result is not stored.
//
// The cell, both halves at once:  t = diag + s (two SDWA adds, one per half: VOP3P has no SDWA; s is a signed profile byte of A's row
// in the low half, of B's row in the high half);  hn = max(t, e, f, 0) (three v_pk_max_i16);  x = hn + goe (v_pk_add_i16);
// e = max(e + ge, x), f = max(f + ge, x) (an add and a max each): 10 VALU per column of both targets, where the 32-bit sweep spends 8
// per cell.  Two columns make one asm statement (GS16_CELL2) so that no SDWA result is read by the instruction behind its write: on
// gfx950 a write with a destination select needs one instruction between it and a reader, and the compiler does not look into asm
// text.  The four adds come first -- A's half of column k, of column k + 1, then B's halves, which PRESERVE the first two --, and the
// first reader of a sum stands two instructions behind its last write.  The statement ends with plain v_pk_max_i16.
//
// No instruction clamps.  Nothing wraps, because the planner (swp::search_multi_packed) sends a query here only where
//     max(max_entry, 0) x min(qlen, longest target) <= 32767     and     gap_open + 2 gap_extend >= -32768:
//   * Above.  H of a cell is the score of a local alignment that ends there: at most min(i, j) aligned pairs of at most max_entry each,
//     so 0 <= H <= 32767.  t = diag + s only exceeds 0 as such a score.  E, F <= H of their own cell + goe <= H.  Cells outside the
//     matrix (PAD rows, columns beyond the query: profile -1) derive from cells inside by steps <= 0 (the header of sw_search_affine.hip).
//   * Below.  H >= 0, so x = hn + goe >= goe, and every stored e and f is max(.., x) >= goe; they start at goe and enter a strip as goe
//     or as a stored f.  The most negative intermediate is therefore e + ge or f + ge >= goe + ge = gap_open + 2 gap_extend >= -32768.
//     t = diag + s >= 0 - 128.  The bound is exact for the adds as written: at gap_open + 2 gap_extend = -32769 the sum goe + ge, which
//     every row above a target computes, leaves int16.
// A wrong bound would show as a wrong score: a clamp would hide it.
//
// The partner.  No instruction moves a value between the halves: SDWA writes one half and preserves the other, v_pk_* work per half,
// DPP and the boundary pair move whole registers between lanes.  The halves share only control: the steps (from lenA), and the branch
// that looks for the arg-max cells, taken at a step where SOME half of some lane reaches its target's best so far.  Inside the branch
// either target keeps its own best (sbestA / sbestB, wave-uniform), and per lane its own best row maximum and the step and column
// where it was first seen (the step is a 32-bit value: rows up to 2^20 - 1 need no 16-bit field).  Extra visits of the branch, called
// for by the partner, change nothing that counts (sw_gotoh_sweep16.inc).  The tie rule is the 32-bit one per target: highest score,
// lowest i (qlen + 1) + j among equals.
//
// The boundary column between strips holds per row the pair (H of the last column, F past it) of both targets in the same two ints the
// 32-bit kernels use: a launch's boundary workspace is that of the 32-bit launch of the same queries.
// All global writes are vector stores or plain C++, all atomics vector atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"
#include "sw_wave.h"
#include "sw_gotoh_cell16.h"

namespace swk {

// C: query columns per lane (4, 8, 16)
template <int C>
__global__ void __launch_bounds__(256) sw_search_multi_pk_wave(SearchMultiPackedParams p) {
    static_assert(C % 4 == 0 && C <= 16, "C is a multiple of 4");
    constexpr int NQ = C / 4;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t slot = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;     // resident wave: its own boundary column
    const u32 ge2 = ((u32)p.ge & 0xFFFFu) * 0x10001u, goe2 = ((u32)p.goe & 0xFFFFu) * 0x10001u;
    // (a launch without a boundary workspace holds one-strip queries only: nothing goes through the empty descriptor)
    const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc((void*)(p.bnd ? p.bnd + slot * p.bnd_per : nullptr), 0,
                                                                        p.bnd ? (int)(p.bnd_per * 4) : 0, 0x00020000);
    const u32 nq = p.nq;
    const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc((void*)p.counter, 0, 4, 0x00020000);
    const u32 voffL0 = lane == 0 ? 0u : SW_OOB;    // lane 0 alone touches the counter and the results

    for (;;) {
        // the next item: a vector buffer atomic of lane 0, read back into a scalar; no lane-divergent branch anywhere in this loop
        const u32 w = (u32)__builtin_amdgcn_readlane(__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(1, rC, (int)voffL0, 0, 0), 0);
        if ((int64_t)w >= p.nitems) break;
        const u32 pr = w / nq;                     // the pair of ranks 2 pr, 2 pr + 1 of the launch
        const int64_t ra = 2 * (int64_t)pr;
        const bool partner = ra + 1 < p.nranks;    // an odd last rank: no partner (its own item is loaded again, its length taken as 0)
        const int64_t rb = partner ? ra + 1 : ra;
        const SearchItem ia = p.items[p.rank0 + ra], ib = p.items[p.rank0 + rb];
        const MultiQuery d = p.queries[w - pr * nq];
        const int lenA = sw_uniform((int)ia.len), lenB = partner ? sw_uniform((int)ib.len) : 0;   // lenA >= lenB: the schedule is sorted
        const int qlen = sw_uniform(d.qlen), nstrips = sw_uniform(d.nstrips);
        const int64_t M = qlen + 1;
        const u32 qpad = (u32)sw_uniform(d.qpad);
        const bool multi = nstrips > 1;
        const __amdgpu_buffer_rsrc_t rQ = __builtin_amdgcn_make_buffer_rsrc((void*)(p.prof + sw_uniform64(d.prof_off)), 0, (int)(SW_SEARCH_ROWS * qpad), 0x00020000);
        // the targets' bytes through descriptors of exactly their extents: rows outside read 0 and are mapped to PAD by the sweep
        const __amdgpu_buffer_rsrc_t rTA = __builtin_amdgcn_make_buffer_rsrc((void*)(p.db + sw_uniform64(ia.start)), 0, lenA, 0x00020000);
        const __amdgpu_buffer_rsrc_t rTB = __builtin_amdgcn_make_buffer_rsrc((void*)(p.db + sw_uniform64(ib.start)), 0, lenB, 0x00020000);
#include "sw_gotoh_sweep16.inc"
        sw_result* const row = p.results + sw_uniform64(d.row) * p.ntargets;
        gs16_store(row + sw_uniform64(ia.idx), kbestA, voffL0);
        if (partner) gs16_store(row + sw_uniform64(ib.idx), kbestB, voffL0);
    }
}

template __global__ void sw_search_multi_pk_wave<4>(SearchMultiPackedParams);
template __global__ void sw_search_multi_pk_wave<8>(SearchMultiPackedParams);
template __global__ void sw_search_multi_pk_wave<16>(SearchMultiPackedParams);

}  // namespace swk
