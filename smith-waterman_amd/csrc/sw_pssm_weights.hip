// sw_pssm_weights.hip -- position-based sequence weights of aligned hits (sw_db_pssm_hit_weights, gfx950): the table that
// sw_db_pssm_from_hits takes as d_weights, written on the device between sw_db_align_pssm_hits and that call.  include/swhip.h states
// the rule (Henikoff & Henikoff 1994 in integers: n[j][k], k_j, the terms floor(F / (k_j n)), A_r, the rounded share of per_hit x U);
// sw_pssm_hit_weights_host (sw_hits_host.cpp) is the same rule in plain C++.  Used entries and the walk are those of sw_pssm_hits.hip,
// through sw_pssm_walk.h.
//
// sw_pssm_weights_tile: one workgroup (4 waves) per (query, tile of columns), the tiles and the LDS layout of swp::plan_pssm_hits: the
// 256-byte table from a target byte to its place in a column, then `stride` dwords per column, stride odd and > nletters.
//   * COUNT.  The COUNT of sw_pssm_from_hits with every weight 1: n[j][k] in LDS (ds_add_u32).
//   * TERMS.  After a barrier one thread per column counts its nonzero entries into the column's spare dword (k_j).  After another,
//     one thread per (column, letter) replaces the count in place by its term floor(F / (k_j n)): one 32-bit division per LDS entry
//     (k_j n <= 2^20), none per op -- a column's term is shared by every entry that pairs the column with that letter, up to 4096 of them.
//   * SUM.  After a barrier the waves walk the same entries again.  Each 'M' lane reads its term from LDS and adds term + 2^40 to a
//     64-bit register: the terms in the low 40 bits (T_r < 2^40), the pairs above them (m_r < 2^20).  At the end of the entry the wave
//     sums the 64 registers and one lane adds the sum to the entry's accumulator in global memory: one 64-bit atomic add per (entry, tile
//     that the entry has a counted pair in).  Integer adds commute: the same bytes on every run.
// sw_pssm_weights_finish: one workgroup per query.  Thread t takes the entries t, t + 256, ...: A_r = floor(T_r / m_r) into LDS, the
// sums of A_r and of (A_r > 0) over the wave (shuffles) and the four waves (LDS), then every w(q, r): one 64-bit division each.
// An entry that is not used, or lies at or beyond the query's count, was never added to: its accumulator is the zero the call's memset
// left, so A_r = 0 and w = 0 -- every entry of d_weights is written.
// LDS banks: as in sw_pssm_hits.hip -- the lanes of a run of 'M' touch adjacent columns, which the odd stride puts into different banks;
// the reads of SUM are plain ds_read_b32, equal addresses are a broadcast.  In TERMS adjacent threads take adjacent letters of a column.
// Bounds: hits, nhits, aln at q * top + r with r < top; ops at (q * top + r) * ops_cap + [0, nops), nops <= ops_cap; the database at
// offsets[t] + i with t < ntargets, i < len; LDS at (j - c0) * stride + k with c0 <= j < c0 + cols, k <= nletters < stride; acc and
// weights at q * top + r with q < nqueries, r < top.  No floats.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"
#include "sw_wave.h"
#include "sw_pssm_walk.h"

namespace swk {

namespace {
constexpr int kTermShift = 20;                                       // F = 2^20
constexpr int kPairShift = 40;                                       // the pairs of an accumulator stand above its terms

__device__ __forceinline__ u64 sw_wave_sum64(u64 v) {                // over the 64 lanes, in every lane
    for (int s = 32; s > 0; s >>= 1) {
        const u32 lo = (u32)__shfl_xor((int)(u32)v, s), hi = (u32)__shfl_xor((int)(u32)(v >> 32), s);
        v += ((u64)hi << 32) | lo;
    }
    return v;
}
}  // namespace

__global__ void __launch_bounds__(256) sw_pssm_weights_tile(PssmWeightsParams p) {
    extern __shared__ unsigned int lds_dw[];
    unsigned char* code = (unsigned char*)lds_dw;                    // 256 bytes: target byte -> place in a column, 255 (with < 256 letters): none
    int* cnt = (int*)(lds_dw + 64);                                  // tile_cols x stride: counts, then terms; k_j in the spare dword
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nl = p.nletters, stride = p.stride;
    for (int64_t job = blockIdx.x; job < p.t.nqueries * p.tiles_per_query; job += gridDim.x) {
        const int64_t q = job / p.tiles_per_query, c0 = (job % p.tiles_per_query) * p.tile_cols;
        const int64_t qlen = p.t.qoffs[q + 1] - p.t.qoffs[q];
        if (c0 >= qlen) continue;                                    // (uniform in the workgroup: a shorter query has fewer tiles)
        const int cols = (int)min((int64_t)p.tile_cols, qlen - c0);
        const int64_t c1 = c0 + cols;
        __syncthreads();                                             // the last tile's terms have been read
        code[tid] = p.code[tid];
        for (int e = tid; e < cols * stride; e += 256) cnt[e] = 0;
        __syncthreads();
        const int64_t nh = sw_pssm_query_hits(p.t, q);

        // ---- COUNT
        for (int64_t r = wave; r < nh; r += 4) {
            const int64_t e = q * p.t.top + r;
            sw_alignment a;
            int64_t toff, len;
            if (!sw_pssm_entry_used(p.t, e, qlen, a, toff, len)) continue;
            if (!sw_pssm_reaches_tile(a, c0, c1)) continue;
            const unsigned char* tb = p.t.db + toff;
            sw_pssm_walk(sw_pssm_entry_ops(p.t, e), a, len, c0, c1, lane, [&](int64_t j, int64_t i) {
                const int k = code[tb[i]];
                if (k < nl) atomicAdd(&cnt[(int)(j - c0) * stride + k], 1);
            });
        }
        __syncthreads();

        // ---- TERMS
        for (int c = tid; c < cols; c += 256) {
            int kj = 0;
            for (int k = 0; k < nl; ++k) kj += cnt[c * stride + k] > 0;
            cnt[c * stride + nl] = kj;
        }
        __syncthreads();
        for (int e = tid, c = tid / nl, k = tid - (tid / nl) * nl; e < cols * nl; e += 256) {
            int* row = cnt + c * stride;
            const unsigned n = (unsigned)row[k];
            if (n) row[k] = (int)((1u << kTermShift) / ((unsigned)row[nl] * n));    // (k_j n <= 256 x 4096: the term is >= 1)
            k += 256 % nl; c += 256 / nl;
            if (k >= nl) { k -= nl; ++c; }
        }
        __syncthreads();

        // ---- SUM
        for (int64_t r = wave; r < nh; r += 4) {
            const int64_t e = q * p.t.top + r;
            sw_alignment a;
            int64_t toff, len;
            if (!sw_pssm_entry_used(p.t, e, qlen, a, toff, len)) continue;
            if (!sw_pssm_reaches_tile(a, c0, c1)) continue;
            const unsigned char* tb = p.t.db + toff;
            u64 mine = 0;
            sw_pssm_walk(sw_pssm_entry_ops(p.t, e), a, len, c0, c1, lane, [&](int64_t j, int64_t i) {
                const int k = code[tb[i]];
                if (k < nl) mine += (u64)(u32)cnt[(int)(j - c0) * stride + k] + (1ull << kPairShift);
            });
            const u64 sum = sw_wave_sum64(mine);
            if (lane == 0 && sum) atomicAdd(&p.acc[e], sum);
        }
    }
}

__global__ void __launch_bounds__(256) sw_pssm_weights_finish(PssmWeightsParams p) {
    __shared__ int A[SW_TOP_MAX];
    __shared__ u64 part_sum[4];
    __shared__ int part_used[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t top = p.t.top;
    for (int64_t q = blockIdx.x; q < p.t.nqueries; q += gridDim.x) {
        __syncthreads();                                             // the last query's sums have been read
        u64 s = 0, u = 0;
        for (int64_t r = tid; r < top; r += 256) {
            const u64 v = p.acc[q * top + r];
            const u64 T = v & ((1ull << kPairShift) - 1), m = v >> kPairShift;
            const int a = m ? (int)(T / m) : 0;
            A[r] = a;
            s += (u64)a; u += a > 0;
        }
        s = sw_wave_sum64(s); u = sw_wave_sum64(u);
        if (lane == 0) { part_sum[wave] = s; part_used[wave] = (int)u; }
        __syncthreads();
        const u64 S = part_sum[0] + part_sum[1] + part_sum[2] + part_sum[3];
        const u64 U = (u64)(part_used[0] + part_used[1] + part_used[2] + part_used[3]);
        const u64 scale = 2 * (u64)p.per_hit * U;                    // (< 2^30; times A_r <= 2^20, plus S <= 2^32: below 2^51)
        for (int64_t r = tid; r < top; r += 256) {
            int w = 0;
            if (S > 0) w = (int)min((scale * (u64)A[r] + S) / (2 * S), (u64)65535);
            p.weights[q * top + r] = w;
        }
    }
}

}  // namespace swk
