// sw_search_multi.hip -- many queries against a prepared database (sw_db_search_affine): the affine search of sw_search_affine.hip with
// a loop around it that takes (target, query) pairs, score and arg-max only (gfx950).
//
// The sweep of a pair -- the cell recurrence, the state per lane, the software-pipelined loads, the boundary column between strips and the
// arg-max -- is the text of sw_gotoh_sweep.inc, which sw_search_affine_wave<C> includes too; the header of sw_search_affine.hip
// argues it (cells outside the matrix, ties, overflow).  This file holds what a wave does between two sweeps:
//   * work item w, taken with the vector buffer atomic of lane 0, is the pair (target rank rank0 + w / nq, query w % nq of the launch):
//     every query of the launch against the longest target first (sw_plan.h, plan_search_multi);
//   * the query comes as a wave-uniform MultiQuery from the call's device table: the profile descriptor (257 x qpad bytes at prof_off
//     of the group's workspace), qlen, the strips and the result row are rebuilt per item -- scalar loads and scalar
//     arithmetic, a few dozen cycles against the thousands of a sweep;
//   * the result goes to results[row * ntargets + idx]: query-major, the caller's order on both axes.
// A launch holds the queries of ONE class (columns per lane), so C stays a template parameter and the sweep keeps its registers.
// sw_search_profile_submat_multi fills the profiles of a whole group in one launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"
#include "sw_wave.h"

namespace swk {

// The profiles of the table entries tab[0 .. nq): for entry t, prof[prof_off + x * qpad + c] = sub[q[qstart + c]][x] for x < 256, c < qlen;
// row 256 (PAD) and columns >= qlen: -1 (the layout of sw_search_profile_submat).  qpad is a multiple of 256, so a workgroup writes
// 256 adjacent columns of one row per step; every query is cut into `parts` interleaved shares, dealt to the workgroups in turn.
__global__ void __launch_bounds__(256) sw_search_profile_submat_multi(const unsigned char* __restrict__ q, const MultiQuery* __restrict__ tab, int64_t nq, int parts,
                                                                      signed char* __restrict__ prof, const signed char* __restrict__ sub) {
    for (int64_t job = blockIdx.x; job < nq * parts; job += gridDim.x) {
        const MultiQuery d = tab[job / parts];
        const int part = (int)(job % parts), per_row = d.qpad >> 8, nchunks = SW_SEARCH_ROWS * per_row;
        const unsigned char* qq = q + d.qstart;
        signed char* out = prof + d.prof_off;
        for (int ch = part; ch < nchunks; ch += parts) {
            const int x = ch / per_row, c = ((ch - x * per_row) << 8) + (int)threadIdx.x;
            out[(int64_t)x * d.qpad + c] = (x < 256 && c < d.qlen) ? sub[(int)qq[c] * 256 + x] : (signed char)-1;
        }
    }
}

// C: query columns per lane (4, 8, 16)
template <int C>
__global__ void __launch_bounds__(256) sw_search_affine_multi_wave(SearchMultiParams p) {
    static_assert(C % 4 == 0 && C <= 16, "C is a multiple of 4");
    constexpr int NQ = C / 4;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t slot = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;     // resident wave: its own boundary column
    const int ge = p.ge, goe = p.goe;
    // (a launch without a boundary workspace holds one-strip queries only: nothing goes through the empty descriptor)
    const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc((void*)(p.bnd ? p.bnd + slot * p.bnd_per : nullptr), 0,
                                                                        p.bnd ? (int)(p.bnd_per * 4) : 0, 0x00020000);
    const u32 nq = p.nq;
    const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc((void*)p.counter, 0, 4, 0x00020000);
    const u32 voffL0 = lane == 0 ? 0u : SW_OOB;    // lane 0 alone touches the counter and the result

    for (;;) {
        // the next pair: a vector buffer atomic of lane 0 (the other lanes' offsets lie beyond the descriptor: dropped), read
        // back from lane 0 into a scalar; no lane-divergent branch anywhere in this loop (sw_search_wave says why)
        const u32 w = (u32)__builtin_amdgcn_readlane(__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(1, rC, (int)voffL0, 0, 0), 0);
        if ((int64_t)w >= p.nitems) break;
        const u32 rank = w / nq;
        const SearchItem it = p.items[p.rank0 + rank];
        const MultiQuery d = p.queries[w - rank * nq];
        const int len = (int)it.len;
        // the query of this item: its profile through a descriptor of exactly its extent, its own row stride, strips and matrix width
        // (the table is read with vector loads: readfirstlane tells the compiler that these are scalars)
        const int qlen = __builtin_amdgcn_readfirstlane(d.qlen), nstrips = __builtin_amdgcn_readfirstlane(d.nstrips);
        const int64_t M = qlen + 1;
        const u32 qpad = (u32)__builtin_amdgcn_readfirstlane(d.qpad);
        const bool multi = nstrips > 1;
        const __amdgpu_buffer_rsrc_t rQ = __builtin_amdgcn_make_buffer_rsrc((void*)(p.prof + d.prof_off), 0, (int)(SW_SEARCH_ROWS * qpad), 0x00020000);
        // the target's bytes through a descriptor of exactly its extent: rows outside it read 0 and are mapped to PAD by the sweep
        const __amdgpu_buffer_rsrc_t rT = __builtin_amdgcn_make_buffer_rsrc((void*)(p.db + it.start), 0, len, 0x00020000);
#include "sw_gotoh_sweep.inc"
        {
            const __amdgpu_buffer_rsrc_t rR = __builtin_amdgcn_make_buffer_rsrc((void*)(p.results + d.row * p.ntargets + it.idx), 0, (int)sizeof(sw_result), 0x00020000);
            const u64 score = kbest >> 40, pos = kbest ? SW_KEY_IDX_MASK - (kbest & SW_KEY_IDX_MASK) : 0;
            const sw_v4i v = {(int)(u32)pos, (int)(u32)(pos >> 32), (int)(u32)score, 0};
            __builtin_amdgcn_raw_buffer_store_b128(v, rR, (int)voffL0, 0, 0);                 // max_pos, max_score
            __builtin_amdgcn_raw_buffer_store_b64(sw_v2i{0, 0}, rR, (int)voffL0, 16, 0);      // path_len
        }
    }
}

template __global__ void sw_search_affine_multi_wave<4>(SearchMultiParams);
template __global__ void sw_search_affine_multi_wave<8>(SearchMultiParams);
template __global__ void sw_search_affine_multi_wave<16>(SearchMultiParams);

}  // namespace swk
