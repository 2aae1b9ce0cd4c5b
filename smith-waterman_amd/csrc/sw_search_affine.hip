// sw_search_affine.hip -- database search with a substitution matrix and affine gaps (Gotoh), score and arg-max only (gfx950).
//
// Per target (rows, i) against the query (columns, j), with go = gap_open <= 0, ge = gap_extend <= 0 (a gap of k letters: go + k ge):
//   E[i][j] = max(E[i-1][j], H[i-1][j] + go) + ge        F[i][j] = max(F[i][j-1], H[i][j-1] + go) + ge
//   H[i][j] = max(0, H[i-1][j-1] + S[q[j-1]][t[i-1]], E[i][j], F[i][j])          H = 0, E = F = -inf on row 0 / column 0
// and the arg-max by the rule of sw_search_wave: highest H, lowest linear index i (qlen + 1) + j among equals, 0 if nothing is positive.
//
// Mapping: that of sw_search_wave (sw_search.hip).  One wave owns one target, lane l keeps C adjacent query columns and works on row
// u - l at step u; strips of 64 C columns follow each other through a boundary column in a per-wave workspace; the targets come from
// a counter taken with the vector buffer atomic of one lane; scores from the 257 x qpad signed-byte profile (sw_search_profile_submat
// fills it from the caller's table).  The sweep of one target is the text of sw_gotoh_sweep.inc, which the many-query and
// the pair-list kernels (sw_search_multi.hip, sw_search_pairs.hip) include too; what follows is about that text.
// State.  Per lane and column k: h[k] = H[r-1][k] (after the step: H[r][k]) and e[k] = E[r][k], ALREADY advanced to the row the lane
// works on next.  Along the lane's columns runs f = F[r][k], already advanced to the column it is used in.  With goe = go + ge a cell is
//   hn = max(0, diag + s, e[k], f);  x = hn + goe;  e[k] = max(e[k] + ge, x)  (= E[r+1][k]);  f = max(f + ge, x)  (= F[r][k+1])
// -- 8 VALU for the recurrence alone (the linear kernel's is 4); the whole row loop, with the row maximum, the hand-over, the loads'
// addressing and the arg-max search, counts 12.5 - 17.9 per cell (where the measured rate is set beside both).  Two values cross a lane per step by DPP: h[C-1] (the next lane's diagonal / left H) and f past the last column (the next
// lane's F in its first column); the same pair per row crosses a strip boundary (two ints per row).
// Cells outside the matrix.  -inf never appears: row 0 has H = 0 and E[1][j] = max(E[0][j], go) + ge = goe whatever E[0][j] <= go is, so
// e starts at goe; likewise F[i][1] = goe, the value that enters lane 0 of strip 0.  Every value is then >= goe (H >= 0), and the
// host bounds goe >= -2^24: nothing overflows.  Rows above the matrix (lane l before step l + 1) read the PAD profile row (-1): there
// h stays 0, e and f stay goe (max(goe + ge, 0 + goe) = goe) -- exactly the row-0 state.  Rows below the target (PAD, -1) and columns
// beyond the query (-1) hold derived values: by induction over the recurrence, H, E and F of such a cell are each at most the H of some
// cell INSIDE the matrix in a row and a column not behind it (inside, E <= H and F <= H of the same cell; every move outside adds
// -1, ge or goe, all <= 0; a boundary row no strip wrote enters as (0, goe)).  So no outside cell exceeds the true maximum V, and if
// one equals V an inside cell with V and a lower linear index exists.  The lane that holds the true arg-max cell Z therefore meets Z
// -- rows ascending, columns ascending within a row, strict improvement only -- before any outside cell of value V: outside cells
// below lie in later rows, and one to the right in an earlier row would imply an inside cell of value V with a lower index than Z.
// Other lanes may end on an outside cell; the range check r <= len, c <= qlen on the key drops those, and they held less than V or a
// higher index anyway.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"
#include "sw_wave.h"

namespace swk {

// prof[x * qpad + c] = sub[q[c]][x] for x < 256, c < qlen; row 256 (PAD) and columns >= qlen: -1.  sub: 256 x 256, row = query byte.
__global__ void __launch_bounds__(256) sw_search_profile_submat(const unsigned char* __restrict__ q, int64_t qlen, int64_t qpad, signed char* __restrict__ prof,
                                                                const signed char* __restrict__ sub) {
    const int64_t n = (int64_t)SW_SEARCH_ROWS * qpad;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t x = i / qpad, c = i - x * qpad;
        prof[i] = (x < 256 && c < qlen) ? sub[(int64_t)q[c] * 256 + x] : (signed char)-1;
    }
}

// C: query columns per lane (4, 8, 16)
template <int C>
__global__ void __launch_bounds__(256) sw_search_affine_wave(SearchAffineParams p) {
    static_assert(C % 4 == 0 && C <= 16, "C is a multiple of 4");
    constexpr int NQ = C / 4;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t slot = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;     // resident wave: its own boundary column
    const int qlen = (int)p.qlen;
    const int64_t M = qlen + 1;
    const int ge = p.ge, goe = p.goe;
    const int nstrips = (qlen + 64 * C - 1) / (64 * C);
    const bool multi = nstrips > 1;
    const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc((void*)(multi ? p.bnd + slot * p.bnd_per : nullptr), 0,
                                                                        multi ? (int)(p.bnd_per * 4) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rQ = __builtin_amdgcn_make_buffer_rsrc((void*)p.prof, 0, (int)(SW_SEARCH_ROWS * p.qpad), 0x00020000);
    const u32 qpad = (u32)p.qpad;
    const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc((void*)p.counter, 0, 4, 0x00020000);
    const u32 voffL0 = lane == 0 ? 0u : SW_OOB;    // lane 0 alone touches the counter and the result

    for (;;) {
        // the next target: a vector buffer atomic of lane 0 (the other lanes' offsets lie beyond the descriptor: dropped), read
        // back from lane 0 into a scalar; no lane-divergent branch anywhere in this loop (sw_search_wave says why)
        const u32 w = (u32)__builtin_amdgcn_readlane(__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(1, rC, (int)voffL0, 0, 0), 0);
        if ((int64_t)w >= p.nitems) break;
        const SearchItem it = p.items[w];
        const int len = (int)it.len;
        // the target's bytes through a descriptor of exactly its extent: rows outside it read 0 and are mapped to PAD by the sweep
        const __amdgpu_buffer_rsrc_t rT = __builtin_amdgcn_make_buffer_rsrc((void*)(p.db + it.start), 0, len, 0x00020000);
#include "sw_gotoh_sweep.inc"
        {
            const __amdgpu_buffer_rsrc_t rR = __builtin_amdgcn_make_buffer_rsrc((void*)(p.results + it.idx), 0, (int)sizeof(sw_result), 0x00020000);
            const u64 score = kbest >> 40, pos = kbest ? SW_KEY_IDX_MASK - (kbest & SW_KEY_IDX_MASK) : 0;
            const sw_v4i v = {(int)(u32)pos, (int)(u32)(pos >> 32), (int)(u32)score, 0};
            __builtin_amdgcn_raw_buffer_store_b128(v, rR, (int)voffL0, 0, 0);                 // max_pos, max_score
            __builtin_amdgcn_raw_buffer_store_b64(sw_v2i{0, 0}, rR, (int)voffL0, 16, 0);      // path_len
        }
    }
}

template __global__ void sw_search_affine_wave<4>(SearchAffineParams);
template __global__ void sw_search_affine_wave<8>(SearchAffineParams);
template __global__ void sw_search_affine_wave<16>(SearchAffineParams);

}  // namespace swk
