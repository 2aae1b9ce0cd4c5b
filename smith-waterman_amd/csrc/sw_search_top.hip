// sw_search_top.hip -- the best `top` targets of every row of a query-major result table (sw_top_hits_device, sw_db_search_affine_top).
//
// A target's key is  score << tbits | (2^tbits - 1 - target)  with tbits = ceil(log2 ntargets).  Keys are unique per target and their
// integer order is the rank order: score descending, then target ascending.  The `top` largest keys of a row are therefore ONE set, and
// sorting them gives ONE sequence, whatever order the atomics below happen to run in.
//
//   rows of at most swp::kTopMax targets   sw_top_sort alone: one workgroup loads the row's keys into LDS, sorts them (bitonic) and
//                                          writes the hits.
//   longer rows                            a radix select finds the key of rank `top`, highest digit first.  Per digit sw_top_hist counts,
//                                          over the keys that carry the digits found so far, the values of the next one: wgs_row
//                                          workgroups per row, each with an LDS histogram over its slice and one vector atomic add per
//                                          non-empty bin into the row's global histogram; sw_top_scan (one workgroup per row) walks the bins
//                                          from the top, fixes the digit and clears the bins.  sw_top_compact gathers the keys at or above
//                                          the key found -- exactly `top` of them, or every qualifying one where fewer qualify -- into the
//                                          start of the row's own hits with a per-row counter, and sw_top_sort orders them as above.
// The counting passes and the compaction read max_score only, 8 of every 24 bytes; max_pos and max_score of a hit are copied from the
// table once the ranks are known.  Scores are taken modulo 2^24 (the bound every search call enforces) so that no input can carry a key
// out of its fields; a slot is checked against `top` before it is written.
#include "sw_kernels.h"
#include "sw_top_key.h"

namespace swk {

constexpr int kTopBins = 1 << swp::kTopDigitBits;
static_assert(kTopBins % 256 == 0);

__global__ void __launch_bounds__(256) sw_top_hist(TopParams p) {
    __shared__ unsigned int h[kTopBins];
    const unsigned row = blockIdx.x / p.wgs_row, w = blockIdx.x % p.wgs_row;
    unsigned long long prefix = 0;
    if (!p.first) {
        const TopState st = p.state[row];
        if (st.all) return;
        prefix = st.prefix;
    }
    for (int b = threadIdx.x; b < kTopBins; b += 256) h[b] = 0;
    __syncthreads();
    const int64_t lo = (int64_t)w * p.slice, hi = min(p.ntargets, lo + p.slice);
    const sw_result* r = p.results + (int64_t)row * p.ntargets;
    const int up = p.shift + p.bits;
    const unsigned mask = (1u << p.bits) - 1;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        const long long s = r[i].max_score;
        if (s < p.min_score) continue;
        const unsigned long long k = top_key(s, i, p.tbits);
        if ((k >> up) != prefix) continue;   // (the first pass: nothing above its digit, prefix 0)
        atomicAdd(&h[(unsigned)(k >> p.shift) & mask], 1u);
    }
    __syncthreads();
    unsigned int* g = p.hist + ((size_t)row << swp::kTopDigitBits);
    for (int b = threadIdx.x; b < kTopBins; b += 256) {
        const unsigned c = h[b];
        if (c) atomicAdd(&g[b], c);
    }
}

// One workgroup per row: the digit of this pass.  Thread t owns the 8 bins below nb - 8 t, highest first, so that thread 0 of the
// workgroup finds the thread whose bins hold the wanted rank from 256 partial sums, and that thread the bin.
__global__ void __launch_bounds__(256) sw_top_scan(TopParams p) {
    constexpr int kPer = kTopBins / 256;
    __shared__ unsigned int part[256];
    __shared__ int owner;
    __shared__ unsigned int above_owner;
    const unsigned row = blockIdx.x, t = threadIdx.x;
    TopState st;
    if (p.first) { st.prefix = 0; st.want = (unsigned)p.top; st.all = 0; st.count = 0; st.n = (unsigned)p.top; }
    else st = p.state[row];
    if (st.all) return;
    unsigned int* g = p.hist + ((size_t)row << swp::kTopDigitBits);
    const int nb = 1 << p.bits;
    unsigned c[kPer], sum = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int b = nb - 1 - ((int)t * kPer + k);
        c[k] = 0;
        if (b >= 0) { c[k] = g[b]; g[b] = 0; }
        sum += c[k];
    }
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        unsigned above = 0;
        int T = -1;
        for (int x = 0; x < 256; ++x) {
            if (above + part[x] >= st.want) { T = x; break; }
            above += part[x];
        }
        owner = T; above_owner = above;
    }
    __syncthreads();
    const int T = owner;
    unsigned above = above_owner;
    if (T < 0) {   // fewer keys than the rank: every qualifying target is a hit (the first pass finds that out)
        if (t == 0) { st.all = 1; st.n = min(above, (unsigned)p.top); st.count = 0; p.state[row] = st; }
        return;
    }
    if ((int)t == T) {
        int digit = 0;
        bool found = false;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            if (!found) {
                if (above + c[k] >= st.want) { digit = nb - 1 - ((int)t * kPer + k); found = true; }
                else above += c[k];
            }
        }
        st.prefix = (st.prefix << p.bits) | (unsigned long long)digit;
        st.want -= above;
        st.count = 0;
        p.state[row] = st;
    }
}

__global__ void __launch_bounds__(256) sw_top_compact(TopParams p) {
    const unsigned row = blockIdx.x / p.wgs_row, w = blockIdx.x % p.wgs_row;
    const TopState st = p.state[row];
    const unsigned long long thr = st.all ? 0ull : st.prefix;
    const int64_t lo = (int64_t)w * p.slice, hi = min(p.ntargets, lo + p.slice);
    const sw_result* r = p.results + (int64_t)row * p.ntargets;
    unsigned long long* keys = (unsigned long long*)(p.hits + (int64_t)row * p.top);
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        const long long s = r[i].max_score;
        if (s < p.min_score) continue;
        const unsigned long long k = top_key(s, i, p.tbits);
        if (k < thr) continue;
        const unsigned slot = atomicAdd(&p.state[row].count, 1u);
        if ((int64_t)slot < p.top) keys[slot] = k;
    }
}

// One workgroup per row: its keys into LDS (the whole row, or what sw_top_compact left at the start of the row's hits), a bitonic sort
// to descending order over the next power of two (padded with zeros, which sort behind every key that counts), then the hits in rank
// order and the {-1, 0, 0} tail.
__global__ void __launch_bounds__(256) sw_top_sort(TopParams p) {
    __shared__ unsigned long long key[swp::kTopMax];
    __shared__ unsigned int qualifying;
    const unsigned row = blockIdx.x, t = threadIdx.x;
    const sw_result* r = p.results + (int64_t)row * p.ntargets;
    sw_hit* out = p.hits + (int64_t)row * p.top;
    unsigned len, n;
    if (p.selected) {
        n = len = (unsigned)min((int64_t)p.state[row].n, min(p.top, swp::kTopMax));
        const unsigned long long* src = (const unsigned long long*)out;
        for (unsigned i = t; i < len; i += 256) key[i] = src[i];
    } else {
        if (t == 0) qualifying = 0;
        __syncthreads();
        len = (unsigned)min(p.ntargets, swp::kTopMax);
        unsigned mine = 0;
        for (unsigned i = t; i < len; i += 256) {
            const long long s = r[i].max_score;
            const bool ok = s >= p.min_score;
            key[i] = ok ? top_key(s, i, p.tbits) : 0ull;   // (a key of zero that qualifies exists only where every target does)
            mine += ok;
        }
        if (mine) atomicAdd(&qualifying, mine);
        __syncthreads();
        n = (unsigned)min((int64_t)qualifying, p.top);
    }
    unsigned N = 1;
    while (N < len) N <<= 1;
    for (unsigned i = len + t; i < N; i += 256) key[i] = 0;
    __syncthreads();
    for (unsigned k = 2; k <= N; k <<= 1)
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            for (unsigned i = t; i < N; i += 256) {
                const unsigned x = i ^ j;
                if (x > i) {
                    const unsigned long long a = key[i], b = key[x];
                    if ((i & k) == 0 ? a < b : a > b) { key[i] = b; key[x] = a; }
                }
            }
            __syncthreads();
        }
    const unsigned long long tmask = (1ull << p.tbits) - 1;
    for (int64_t i = t; i < p.top; i += 256) {
        sw_hit h = {-1, 0, 0};
        if (i < (int64_t)n) {
            const int64_t target = (int64_t)(tmask - (key[i] & tmask));
            h.target = target; h.max_pos = r[target].max_pos; h.max_score = r[target].max_score;
        }
        out[i] = h;
    }
    if (t == 0) p.nhits[row] = n;
}

}  // namespace swk
