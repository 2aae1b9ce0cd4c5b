// sw_top_pairs.hip -- the best `top` entries of every query of a scored pair list (sw_top_hits_pairs_device): what turns the output of
// sw_db_search_affine_pairs, which lies in the order of the pre-filter's atomic cursor, into the nqueries x top hit table that
// sw_db_align_affine_hits takes.
//
// An entry qualifies when its query and its target lie inside their bounds -- each compared UNSIGNED before anything is indexed with
// it, so the pre-filter's {-1, -1} tail drops out by itself -- and its score reaches min_score.  Its sort item is the key of
// sw_top_key.h beside its list position; the rank order is key descending, then position ascending, and no two items are equal in it.
//
//   sw_top_pairs_count     qualifying entries per query.  Up to swp::kTopPairsLdsQueries queries a workgroup counts its slice of the
//                          list in an LDS histogram and adds every non-empty bin to the query's global count with one vector atomic.
//   sw_top_pairs_scan      one workgroup: the exclusive prefix sums of the counts, for any number of queries -- the start of every
//                          query's segment, kept twice: `offs` stays, `cnt` becomes the segment's cursor.
//   sw_top_pairs_scatter   every qualifying entry's item into its query's segment.  The LDS form counts the slice again, reserves one
//                          range per (workgroup, query) with one vector atomic on the cursor and hands the slots out from LDS.  Which
//                          slot of its segment an item gets differs between runs; the sort below removes that.
//   sw_top_pairs_sort      one workgroup per query: the segment into LDS, a bitonic sort by the rank order, the row of hits with max_pos
//                          and max_score fetched through the list position, the {-1, 0, 0} tail and nhits.  A segment longer than the
//                          LDS array is streamed (STREAM): the best T items so far stay in front, the next ITEMS - T are loaded behind
//                          them, all are sorted and the first T kept.
// A real key can be 0 (score 0, target 2^tbits - 1), so real items carry bit 63 (a key has at most 24 + 31 bits) and the padding of a
// sort, key 0 and position 2^32 - 1, lies behind every one of them.
#include "sw_kernels.h"
#include "sw_top_key.h"

namespace swk {

constexpr int kTopPairsLds = (int)swp::kTopPairsLdsQueries;
constexpr unsigned long long kTopPairsReal = 1ull << 63;
constexpr int kTopPairsSortThreads = 1024;

// Entry i: does it qualify, and with which query and key.
__device__ __forceinline__ bool top_pairs_item(const TopPairsParams& p, int64_t i, int64_t& query, unsigned long long& key) {
    const sw_pair pr = p.pairs[i];
    if ((unsigned long long)pr.query >= (unsigned long long)p.nqueries || (unsigned long long)pr.target >= (unsigned long long)p.ntargets) return false;
    const long long s = p.results[i].max_score;
    if (s < p.min_score) return false;
    query = pr.query;
    key = top_key(s, pr.target, p.tbits);
    return true;
}

template <bool LDS>
__global__ void __launch_bounds__(256) sw_top_pairs_count(TopPairsParams p) {
    __shared__ unsigned int h[LDS ? kTopPairsLds : 1];
    const int nq = (int)p.nqueries;
    if (LDS) {
        for (int b = threadIdx.x; b < nq; b += 256) h[b] = 0;
        __syncthreads();
    }
    const int64_t lo = (int64_t)blockIdx.x * p.slice, hi = min(p.npairs, lo + p.slice);
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        int64_t q;
        unsigned long long k;
        if (!top_pairs_item(p, i, q, k)) continue;
        if (LDS) atomicAdd(&h[q], 1u);
        else atomicAdd(&p.cnt[q], 1u);
    }
    if (LDS) {
        __syncthreads();
        for (int b = threadIdx.x; b < nq; b += 256) {
            const unsigned c = h[b];
            if (c) atomicAdd(&p.cnt[b], c);
        }
    }
}

// One workgroup, tiles of 256 x 16 counts: every thread sums its 16, the 256 sums are scanned in LDS, the carry runs from tile to tile.
__global__ void __launch_bounds__(256) sw_top_pairs_scan(TopPairsParams p) {
    constexpr int kPer = 16;
    __shared__ unsigned int part[256];
    const unsigned t = threadIdx.x;
    unsigned carry = 0;
    for (int64_t base = 0; base < p.nqueries; base += 256 * kPer) {
        const int64_t i0 = base + (int64_t)t * kPer;
        unsigned v[kPer], sum = 0;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            v[k] = i0 + k < p.nqueries ? p.cnt[i0 + k] : 0u;
            sum += v[k];
        }
        part[t] = sum;
        __syncthreads();
        for (unsigned off = 1; off < 256; off <<= 1) {
            const unsigned x = t >= off ? part[t - off] : 0u;
            __syncthreads();
            part[t] += x;
            __syncthreads();
        }
        unsigned at = carry + part[t] - sum;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            if (i0 + k < p.nqueries) { p.offs[i0 + k] = at; p.cnt[i0 + k] = at; }
            at += v[k];
        }
        carry += part[255];
        __syncthreads();
    }
    if (t == 0) p.offs[p.nqueries] = carry;
}

template <bool LDS>
__global__ void __launch_bounds__(256) sw_top_pairs_scatter(TopPairsParams p) {
    __shared__ unsigned int h[LDS ? kTopPairsLds : 1];
    const int nq = (int)p.nqueries;
    const int64_t lo = (int64_t)blockIdx.x * p.slice, hi = min(p.npairs, lo + p.slice);
    if (LDS) {
        for (int b = threadIdx.x; b < nq; b += 256) h[b] = 0;
        __syncthreads();
        for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
            int64_t q;
            unsigned long long k;
            if (top_pairs_item(p, i, q, k)) atomicAdd(&h[q], 1u);
        }
        __syncthreads();
        for (int b = threadIdx.x; b < nq; b += 256) {   // the workgroup's range of every segment it has items for
            const unsigned c = h[b];
            if (c) h[b] = atomicAdd(&p.cnt[b], c);
        }
        __syncthreads();
    }
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        int64_t q;
        unsigned long long k;
        if (!top_pairs_item(p, i, q, k)) continue;
        const unsigned slot = LDS ? atomicAdd(&h[q], 1u) : atomicAdd(&p.cnt[q], 1u);
        if ((int64_t)slot < p.npairs) { p.keys[slot] = k; p.pos[slot] = (unsigned)i; }
    }
}

// Sorts key[0 .. N) / pos[0 .. N), N a power of two, into the rank order: key descending, then position ascending.  Every thread of
// the workgroup calls it; it ends behind a barrier.
__device__ __forceinline__ void top_pairs_bitonic(unsigned long long* key, unsigned int* pos, unsigned N, unsigned t) {
    for (unsigned k = 2; k <= N; k <<= 1)
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            for (unsigned m = t; m < N / 2; m += kTopPairsSortThreads) {
                const unsigned i = ((m & ~(j - 1)) << 1) | (m & (j - 1)), x = i | j;
                const unsigned long long a = key[i], b = key[x];
                const unsigned pa = pos[i], pb = pos[x];
                const bool b_first = b > a || (b == a && pb < pa);
                const bool a_first = a > b || (a == b && pa < pb);
                if ((i & k) == 0 ? b_first : a_first) { key[i] = b; key[x] = a; pos[i] = pb; pos[x] = pa; }
            }
            __syncthreads();
        }
}

template <int ITEMS, bool STREAM>
__global__ void __launch_bounds__(kTopPairsSortThreads) sw_top_pairs_sort(TopPairsParams p) {
    __shared__ unsigned long long key[ITEMS];
    __shared__ unsigned int pos[ITEMS];
    const unsigned t = threadIdx.x;
    const unsigned T = min(p.T, (unsigned)ITEMS / 2);
    for (int64_t row = blockIdx.x; row < p.nqueries; row += gridDim.x) {
        unsigned base = 0, len = 0;
        if (p.npairs > 0) { base = p.offs[row]; len = p.offs[row + 1] - base; }
        unsigned have = min(len, (unsigned)ITEMS), consumed = have;
        for (unsigned i = t; i < have; i += kTopPairsSortThreads) { key[i] = p.keys[base + i] | kTopPairsReal; pos[i] = p.pos[base + i]; }
        while (len > 0) {
            unsigned N = 1;
            while (N < have) N <<= 1;
            for (unsigned i = have + t; i < N; i += kTopPairsSortThreads) { key[i] = 0; pos[i] = 0xFFFFFFFFu; }
            __syncthreads();
            top_pairs_bitonic(key, pos, N, t);
            if (!STREAM || consumed >= len) break;
            const unsigned take = min(len - consumed, (unsigned)ITEMS - T);   // (have == ITEMS >= T here: the segment is longer)
            for (unsigned i = t; i < take; i += kTopPairsSortThreads) {
                key[T + i] = p.keys[base + consumed + i] | kTopPairsReal;
                pos[T + i] = p.pos[base + consumed + i];
            }
            consumed += take;
            have = T + take;
        }
        const int64_t n = min((int64_t)len, p.top);
        sw_hit* out = p.hits + row * p.top;
        for (int64_t i = t; i < p.top; i += kTopPairsSortThreads) {
            sw_hit h = {-1, 0, 0};
            if (i < n) {
                const unsigned e = pos[i];
                h.target = p.pairs[e].target; h.max_pos = p.results[e].max_pos; h.max_score = p.results[e].max_score;
            }
            out[i] = h;
        }
        if (t == 0) p.nhits[row] = n;
        __syncthreads();   // the next row overwrites the items
    }
}

template __global__ void sw_top_pairs_count<false>(TopPairsParams);
template __global__ void sw_top_pairs_count<true>(TopPairsParams);
template __global__ void sw_top_pairs_scatter<false>(TopPairsParams);
template __global__ void sw_top_pairs_scatter<true>(TopPairsParams);
template __global__ void sw_top_pairs_sort<(int)swp::kTopMax, false>(TopPairsParams);
template __global__ void sw_top_pairs_sort<(int)swp::kTopMax, true>(TopPairsParams);
template __global__ void sw_top_pairs_sort<2 * (int)swp::kTopMax, true>(TopPairsParams);

}  // namespace swk
