// sw_search.hip -- database search: ONE query against many targets of any length and any byte alphabet (gfx950).
//
// Per target k the reference fill (serial_smithW.c:141-145, 187-256) of a = query (columns), b = target k (rows), score and
// arg-max only; the recurrence, the tie rule and the 24-bit score / 40-bit index key are those of sw_batch_wave (sw_batch.hip).
//
// Mapping.  One 64-lane wave owns one target at a time; lane l keeps the C adjacent query columns c0 .. c0 + C - 1 of its current
// row in registers and works, at step u, on row u - l (the anti-diagonal sweep of sw_batch_wave, ONE DPP move per step).  A target
// of len rows takes len + 64 steps per strip of 64 C columns; queries wider than one strip are swept strip after strip through a
// boundary column in a per-wave workspace.
// Scores.  The score of a cell depends only on the query column and the target letter, so a profile  prof[x][c]  (one signed byte per
// cell: the score of query column c against byte value x) is built once per call, and a lane reads, per row, the C bytes of ITS
// columns in the profile row of the target's letter: one 4-, 8- or 16-byte load per lane and row, and per cell one v_add_u32_sdwa
// (the diagonal term plus the sign-extended score byte), 4.25 VALU per cell in all as in sw_batch_wave.  The rows are indexed by the
// byte value itself (256 letters) plus one row PAD = 256 that scores -1 everywhere -- the letter of every row outside the target;
// columns beyond the query score -1 too.  So, as in sw_batch_wave, cells outside the matrix stay at 0 above it and derive from the
// matrix by non-positive moves below / right of it: they can never win the arg-max.  Only the rows of letters that occur in the
// database are ever read, so the cache footprint is that of a profile over the database's alphabet (25 x 1 KB per strip for proteins).
// Scores beyond a signed byte (WIDE) keep the same profile layout with a selector byte (1 match, 0 mismatch, -1 outside) and pick
// the score with two selects per cell.
// Schedule.  The host sorts the targets by decreasing length (stable) and hands the waves a list of {start, index, length}; resident
// waves take the next target from a counter with a VECTOR buffer atomic of one lane, so the long targets start first and the short
// ones fill the tail.  Results are written at the original index.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"
#include "sw_wave.h"

namespace swk {

// prof[x * qpad + c], x = 0..256, c = 0..qpad-1: the score of query column c + 1 against byte value x (row 256 and columns >= qlen: -1).
// WIDE: 1 (match) / 0 (mismatch) / -1 instead of the scores.
__global__ void __launch_bounds__(256) sw_search_profile(const unsigned char* __restrict__ q, int64_t qlen, int64_t qpad, signed char* __restrict__ prof,
                                                         int match, int mismatch, int wide) {
    const int64_t n = (int64_t)SW_SEARCH_ROWS * qpad;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t x = i / qpad, c = i - x * qpad;
        int v = -1;
        if (x < 256 && c < qlen) {
            const bool eq = q[c] == (unsigned char)x;
            v = wide ? (eq ? 1 : 0) : (eq ? match : mismatch);
        }
        prof[i] = (signed char)v;
    }
}

// C: query columns per lane (4, 8, 16); WIDE: scores beyond a signed byte (selector profile)
template <int C, bool WIDE>
__global__ void __launch_bounds__(256) sw_search_wave(SearchParams p) {
    static_assert(C % 4 == 0 && C <= 16, "C is a multiple of 4");
    constexpr int NQ = C / 4;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t slot = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;     // resident wave: its own boundary column
    const int qlen = (int)p.qlen;
    const int64_t M = qlen + 1;
    const int ngap = p.ngap;
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
        // back from lane 0 into a scalar.  (No lane-divergent branch anywhere in this loop: with `if (lane == 0)` around the atomic
        // and the result stores, the compiler turned the loop exit into a per-lane exec mask.)
        const u32 w = (u32)__builtin_amdgcn_readlane(__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(1, rC, (int)voffL0, 0, 0), 0);
        if ((int64_t)w >= p.nitems) break;
        const SearchItem it = p.items[w];
        const int len = (int)it.len;
        // the target's bytes through a descriptor of exactly its extent: rows outside it read 0 and are mapped to PAD below
        const __amdgpu_buffer_rsrc_t rT = __builtin_amdgcn_make_buffer_rsrc((void*)(p.db + it.start), 0, len, 0x00020000);
        const int G = (len + 64 + 3) / 4;      // steps 0 .. len + 63 (lane 63's last row)
        u64 kbest = 0;                         // per lane: best (score << 40 | MASK - index) over the strips done
        int sbest = 1;                         // wave-uniform: highest valid H seen so far (at least 1: zeros never count)

        for (int st = 0; st < nstrips; ++st) {
            const int c0 = st * 64 * C + lane * C + 1;
            const u32 colb = (u32)(c0 - 1);
            int h[C];
#pragma unroll
            for (int k = 0; k < C; ++k) h[k] = 0;
            int diag0 = 0, lbest = 0, lk = 0, lstep = 0;
            // boundary column: lane 63 writes its last column (row u - 63) for the next strip, lane 0 reads row u of the previous one
            const bool bw = multi && st + 1 < nstrips, br = multi && st > 0;
            sw_v4i bq = {0, 0, 0, 0};
            const u32 voffB = lane == 0 ? 64u * 4u : SW_OOB;
            if (br) {   // (sc1 loads: served from L2, which this wave's own earlier stores have reached once vmcnt has drained)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                bq = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 0, 16);
            }
            // row r = 4 g + j - lane of this lane reads target byte r - 1; outside 1..len it takes the PAD row
            auto raw_of = [&](int g, int j) -> u32 {
                const u32 pos = (u32)(4 * g + j - lane - 1);
                return (u32)__builtin_amdgcn_raw_buffer_load_b8(rT, (int)(pos < (u32)len ? pos : SW_OOB), 0, 0);
            };
            auto row_off = [&](int g, int j, u32 raw) -> u32 {
                const u32 pos = (u32)(4 * g + j - lane - 1);
                return (pos < (u32)len ? raw : 256u) * qpad + colb;
            };
            // software pipeline: the bytes of group g + 2 and the profile rows of group g + 1 are in flight while group g computes
            u32 raw[4], S[4][NQ], Sn[4][NQ];
#pragma unroll
            for (int j = 0; j < 4; ++j) raw[j] = raw_of(0, j);
#pragma unroll
            for (int j = 0; j < 4; ++j) sw_load_row<C>(rQ, row_off(0, j, raw[j]), S[j]);
#pragma unroll
            for (int j = 0; j < 4; ++j) raw[j] = raw_of(1, j);

            for (int g = 0; g < G; ++g) {
#pragma unroll
                for (int j = 0; j < 4; ++j) sw_load_row<C>(rQ, row_off(g + 1, j, raw[j]), Sn[j]);
#pragma unroll
                for (int j = 0; j < 4; ++j) raw[j] = raw_of(g + 2, j);
                const sw_v4i bcur = bq;
                if (br) bq = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 16 * (g + 1), 16);

                sw_for<0, 4>([&](auto J) {
                    constexpr int j = decltype(J)::value;
                    const int u = 4 * g + j;
                    // lane 0: H of the previous strip's last column in row u (0 beyond the target: rows no strip of this target wrote)
                    const int left = sw_dpp_shr1((br && u <= len) ? bcur[j] : 0, h[C - 1]);
                    int dprev = diag0, prev = left;
                    diag0 = left;
                    sw_for<0, C>([&](auto K) {
                        constexpr int k = decltype(K)::value;
                        const int old = h[k];
                        int s = sw_sbyte(S[j][k >> 2], k & 3);
                        if constexpr (WIDE) {
                            const int sel = s;
                            s = sel > 0 ? p.match : p.mismatch;
                            s = sel < 0 ? -1 : s;
                        }
                        const int t = dprev + s;
                        const int u2 = max(old, prev);
                        const int hn = max(max(t, u2 - ngap), 0);
                        h[k] = hn;
                        dprev = old;
                        prev = hn;
                    });
                    if (bw) __builtin_amdgcn_raw_buffer_store_b32(h[C - 1], rB, lane == 63 ? 4 : (int)SW_OOB, 4 * u, 0);   // row u - 63 at index row + 64
                    // ---- arg-max: the row maximum against the wave's best so far; only a step that reaches it looks for the cell
                    int m = h[0];
#pragma unroll
                    for (int k = 1; k + 1 < C; k += 2) m = max(max(m, h[k]), h[k + 1]);
                    m = max(m, h[C - 1]);
                    if (__builtin_amdgcn_ballot_w64(m >= sbest) != 0) {
                        sbest = max(sbest, sw_wave_max(m));
                        int kk = 0;                                   // first column of my row that holds its maximum
#pragma unroll
                        for (int k = C - 1; k >= 0; --k) kk = (h[k] == m) ? k : kk;
                        const bool imp = m > lbest;                   // strictly: an earlier row of this lane wins a tie
                        lk = imp ? kk : lk;
                        lstep = imp ? u : lstep;
                        lbest = max(lbest, m);
                    }
                });
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int q = 0; q < NQ; ++q) S[j][q] = Sn[j][q];
            }
            {
                const int r = lstep - lane, c = c0 + lk;
                if (lbest > 0 && r >= 1 && r <= len && c <= qlen) {
                    const u64 key = ((u64)(u32)lbest << 40) | (SW_KEY_IDX_MASK - ((u64)r * (u64)M + (u64)c));
                    kbest = key > kbest ? key : kbest;
                }
            }
        }
        // the target's arg-max: highest score, lowest linear index among equals (serial_smithW.c:240-242)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const u32 olo = (u32)__shfl_xor((int)(u32)kbest, off), ohi = (u32)__shfl_xor((int)(u32)(kbest >> 32), off);
            const u64 o = ((u64)ohi << 32) | olo;
            kbest = o > kbest ? o : kbest;
        }
        {
            const __amdgpu_buffer_rsrc_t rR = __builtin_amdgcn_make_buffer_rsrc((void*)(p.results + it.idx), 0, (int)sizeof(sw_result), 0x00020000);
            const u64 score = kbest >> 40, pos = kbest ? SW_KEY_IDX_MASK - (kbest & SW_KEY_IDX_MASK) : 0;
            const sw_v4i v = {(int)(u32)pos, (int)(u32)(pos >> 32), (int)(u32)score, 0};
            __builtin_amdgcn_raw_buffer_store_b128(v, rR, (int)voffL0, 0, 0);                 // max_pos, max_score
            __builtin_amdgcn_raw_buffer_store_b64(sw_v2i{0, 0}, rR, (int)voffL0, 16, 0);      // path_len
        }
    }
}

#define SS_INST(C, W) template __global__ void sw_search_wave<C, W>(SearchParams);
SS_INST(4, false) SS_INST(8, false) SS_INST(16, false) SS_INST(4, true) SS_INST(8, true) SS_INST(16, true)
#undef SS_INST

}  // namespace swk
