// sw_pssm_hits.hip -- the next iteration's PSSM from aligned hits (sw_db_pssm_from_hits, gfx950): the step that closes the loop
// sw_db_search_pssm_top -> sw_db_align_pssm_hits -> here -> sw_db_search_pssm_top.  include/swhip.h states the rule (used entries, the
// walk, weights, counts, the rounded weighted mean); sw_pssm_from_hits_host (sw_hits_host.cpp) is the same rule in plain C++.
//
// One workgroup (4 waves) per (query, tile of `tile_cols` columns); the plan (swp::plan_pssm_hits) fixes the tile so that its counts --
// `stride` int32 per column, stride odd and > nletters -- and the 256-byte table from a target byte to its place in a column fit the LDS.
//   * COUNT.  The waves take the query's entries round robin; the used-entry guards, the skip of an entry whose columns cannot reach
//     the tile and the walk of its ops, 64 at a time, are those of sw_pssm_walk.h.  The entry's weight is loaded at a wave-uniform
//     address.  An 'M' lane whose column lies in the tile (and inside qlen / the target) loads its target byte, maps it through the
//     table and adds the entry's weight to its count in LDS (ds_add_u32; integer adds commute, so the bytes that come out do not
//     depend on the order).
//   * WRITE.  After a barrier one thread per column sums its counts into the column's spare dword (N[j]).  After another, thread e of
//     the tile's cols x nletters entries stores count e if the counts were asked for, then computes entry e: the prior's byte, the
//     column's counts from LDS (the same address across the lanes of a column: a broadcast) against S[b][k] from global memory (adjacent
//     k in adjacent lanes; nletters x nletters bytes, cache resident), floor division, clamp, one byte store.
//     Entry e of the prior is read by the thread that writes entry e of the output and by no other, and tiles are disjoint: that is
//     what makes d_pssm_out == d_prior safe.  No global atomics, no floats.
// LDS banks: lanes of a wave add to (column, letter) pairs that follow the alignment -- adjacent columns for a run of 'M'; with the odd
// stride adjacent columns at the same letter fall into different banks, and equal addresses (duplicate targets) serialise in the
// atomic unit, which is the cost top = 4096 over a handful of targets pays.
// Bounds: prior / out / counts are touched inside [qoffs[q] + c0, qoffs[q] + c0 + cols) x nletters of the query's own columns only; hits,
// nhits, aln, weights at q * top + r with r < top; ops at (q * top + r) * ops_cap + [0, nops), nops <= ops_cap; the database at
// offsets[t] + i with t < ntargets, i < len; LDS at (j - c0) * stride + k with c0 <= j < c0 + cols, k <= nletters < stride.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"
#include "sw_wave.h"
#include "sw_pssm_walk.h"

namespace swk {

namespace {
// floor(a / b) for b > 0 (C++ '/' truncates toward zero)
__device__ __forceinline__ int64_t sw_floor_div(int64_t a, int64_t b) {
    int64_t q = a / b;
    if (a % b != 0 && a < 0) --q;
    return q;
}
}  // namespace

__global__ void __launch_bounds__(256) sw_pssm_from_hits(PssmHitsParams p) {
    extern __shared__ unsigned int lds_dw[];
    unsigned char* code = (unsigned char*)lds_dw;                    // 256 bytes: target byte -> place in a column, 255 (with < 256 letters): none
    int* cnt = (int*)(lds_dw + 64);                                  // tile_cols x stride
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nl = p.nletters, stride = p.stride;
    for (int64_t job = blockIdx.x; job < p.t.nqueries * p.tiles_per_query; job += gridDim.x) {
        const int64_t q = job / p.tiles_per_query, c0 = (job % p.tiles_per_query) * p.tile_cols;
        const int64_t g0 = p.t.qoffs[q], qlen = p.t.qoffs[q + 1] - g0;
        if (c0 >= qlen) continue;                                    // (uniform in the workgroup: a shorter query has fewer tiles)
        const int cols = (int)min((int64_t)p.tile_cols, qlen - c0);
        const int64_t c1 = c0 + cols;
        __syncthreads();                                             // the last tile's counts have been read
        code[tid] = p.code[tid];
        for (int e = tid; e < cols * stride; e += 256) cnt[e] = 0;
        __syncthreads();

        // ---- COUNT
        const int64_t nh = sw_pssm_query_hits(p.t, q);
        for (int64_t r = wave; r < nh; r += 4) {
            const int64_t e = q * p.t.top + r;
            sw_alignment a;
            int64_t toff, len;
            if (!sw_pssm_entry_used(p.t, e, qlen, a, toff, len)) continue;
            int w = 1;
            if (p.weights) w = min(max(p.weights[e], 0), 65535);
            if (w == 0) continue;
            if (!sw_pssm_reaches_tile(a, c0, c1)) continue;
            const unsigned char* tb = p.t.db + toff;
            sw_pssm_walk(sw_pssm_entry_ops(p.t, e), a, len, c0, c1, lane, [&](int64_t j, int64_t i) {
                const int k = code[tb[i]];
                if (k < nl) atomicAdd(&cnt[(int)(j - c0) * stride + k], w);
            });
        }
        __syncthreads();

        // ---- WRITE
        for (int c = tid; c < cols; c += 256) {
            int n = 0;
            for (int k = 0; k < nl; ++k) n += cnt[c * stride + k];
            cnt[c * stride + nl] = n;
        }
        __syncthreads();
        const int64_t base = (g0 + c0) * nl;                         // of the tile in prior / out
        const int64_t cbase = (g0 + c0 - p.col0) * nl;               // ... and in counts
        for (int e = tid, c = tid / nl, k = tid - (tid / nl) * nl; e < cols * nl; e += 256) {
            const int* row = cnt + c * stride;
            if (p.counts) p.counts[cbase + e] = row[k];
            if (p.out) {
                const int P = min((int)p.prior[base + e], p.smax);
                const int64_t den = (int64_t)p.prior_weight + row[nl];
                int v = P;
                if (row[nl] > 0) {                                   // (den == prior_weight gives P back exactly)
                    int64_t num = (int64_t)p.prior_weight * P;
                    for (int b = 0; b < nl; ++b) {
                        const int cb = row[b];
                        if (cb) num += (int64_t)cb * p.S[b * nl + k];
                    }
                    v = (int)min(max(sw_floor_div(2 * num + den, 2 * den), (int64_t)-128), (int64_t)127);
                }
                p.out[base + e] = (signed char)v;
            }
            k += 256 % nl; c += 256 / nl;
            if (k >= nl) { k -= nl; ++c; }
        }
    }
}

}  // namespace swk
