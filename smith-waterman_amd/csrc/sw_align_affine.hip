// sw_align_affine.hip -- the alignment of chosen hits under affine scoring (gfx950): Gotoh's recurrence re-filled with one direction
// byte per cell, and the walk of the canonical alignment (include/swhip.h) through its three states, both by the same wave.
//
// The fill is the text of sw_align_dirfill.inc (the direction byte and its open bits are defined there), the walk and the store of the
// result that of sw_align_walk.inc (the sc1 rule, the windows, the runs, the two passes).  What this kernel owns: a launch serves one
// query, so the profile, qlen, qpad and the strips are the launch's; a resident wave owns a slot of len_max x qpad direction bytes and
// a boundary column, and takes hits from the host-built list through the work counter.  It keeps the timing stamps between the two
// texts.  All global writes are vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"
#include "sw_wave.h"

namespace swk {

// C: query columns per lane (4, 8, 16)
template <int C>
__global__ void __launch_bounds__(256) sw_align_affine_wave(AlignAffineParams p) {
    static_assert(C % 4 == 0 && C <= 16, "C is a multiple of 4");
    constexpr int NQ = C / 4;
    using walk_round_t = int;
    __shared__ sw_v4i win_all[4][SW_WIN * SW_WIN / 16];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t slot = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;     // resident wave: its own boundary column and direction matrix
    if (slot >= p.nslots) return;
    const int qlen = (int)p.qlen;
    const int64_t M = qlen + 1;
    const int ge = p.ge, goe = p.goe;
    const int nstrips = (qlen + 64 * C - 1) / (64 * C);
    const bool multi = nstrips > 1;
    const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc((void*)(multi ? p.bnd + slot * p.bnd_per : nullptr), 0,
                                                                        multi ? (int)(p.bnd_per * 4) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rQ = __builtin_amdgcn_make_buffer_rsrc((void*)p.prof, 0, (int)(SW_SEARCH_ROWS * p.qpad), 0x00020000);
    const __amdgpu_buffer_rsrc_t rD = __builtin_amdgcn_make_buffer_rsrc((void*)(p.dir + slot * p.slot_bytes), 0, (int)p.slot_bytes, 0x00020000);
    const u32 qpad = (u32)p.qpad;
    const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc((void*)p.counter, 0, 4, 0x00020000);
    const u32 voffL0 = lane == 0 ? 0u : SW_OOB;    // lane 0 alone touches the counter and the result
    sw_v4i* const win = win_all[wave];
    const unsigned char* const winb = (const unsigned char*)win;
    const bool has_ops = p.ops != nullptr;
    const int64_t ops_cap = p.ops_cap;
    const int ops_size = (int)(has_ops ? (ops_cap < 0x7FFFFF00ll ? ops_cap : 0x7FFFFF00ll) : 0);

    for (;;) {
        // the next hit: a vector buffer atomic of lane 0, read back into a scalar (sw_search_wave says why)
        const u32 w = (u32)__builtin_amdgcn_readlane(__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(1, rC, (int)voffL0, 0, 0), 0);
        if ((int64_t)w >= p.nitems) break;
        const SearchItem it = p.items[w];
        const int len = (int)it.len;
        const __amdgpu_buffer_rsrc_t rT = __builtin_amdgcn_make_buffer_rsrc((void*)(p.db + it.start), 0, len, 0x00020000);
        const u64 tick0 = p.stamps ? wall_clock64() : 0;
#include "sw_align_dirfill.inc"

        // ---- the walk: every store of this hit has left the wave; the matrix is read past the L1 (sc1), a window at a time
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const u64 tick1 = p.stamps ? wall_clock64() : 0;
        const __amdgpu_buffer_rsrc_t rO = __builtin_amdgcn_make_buffer_rsrc((void*)(has_ops ? p.ops + it.idx * ops_cap : nullptr), 0, ops_size, 0x00020000);
#define SW_WALK_BAND const int bf = 1, bl = len;   // the slot holds the whole matrix
#define SW_WALK_ALN __builtin_amdgcn_make_buffer_rsrc((void*)(p.aln + it.idx), 0, (int)sizeof(sw_alignment), 0x00020000)
#include "sw_align_walk.inc"
#undef SW_WALK_BAND
#undef SW_WALK_ALN
        if (p.stamps) {   // timing aid ("debug_buf"): ticks of the 100 MHz clock spent in fills and in walks, summed over the waves
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const u64 tick2 = wall_clock64();
            if (lane == 0) { atomicAdd(p.stamps, tick1 - tick0); atomicAdd(p.stamps + 1, tick2 - tick1); }
        }
    }
}

template __global__ void sw_align_affine_wave<4>(AlignAffineParams);
template __global__ void sw_align_affine_wave<8>(AlignAffineParams);
template __global__ void sw_align_affine_wave<16>(AlignAffineParams);

}  // namespace swk
