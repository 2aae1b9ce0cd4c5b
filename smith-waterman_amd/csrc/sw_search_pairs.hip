// sw_search_pairs.hip -- the scores of a device list of (query, target) pairs against a prepared database (sw_db_search_affine_pairs,
// gfx950): the rescoring stage behind a pre-filter, score and arg-max only.
//
// The host of this call knows the queries and the handle's longest target, but neither which pairs the list names nor how long their
// targets are.  So the device turns a chunk of the list into work lists first, as sw_align_hits.hip does for a hit table:
//   * sw_search_pairs_bin<false> looks at every pair of the chunk: query inside [0, nqueries), target inside [0, ntargets) -- both
//     compared UNSIGNED before anything is loaded through them (ah_lookup's rule) --, the query one of this group's, the target not
//     empty.  A pair that passes is counted into count[class of its query][bucket], bucket = floor(log2(len x qpad)).  A pair that can
//     never become an item keeps the {0, 0, 0} the call's memset wrote before the first launch; this kernel writes no result.
//   * sw_search_pairs_bin<true>, a launch later, does the same look-up and writes the item {start, out = p, len, entry}.  The lists of
//     the classes lie back to back in the item buffer, and inside a class's list the buckets, HEAVIEST FIRST: an item goes to (items of
//     the classes before) + (items of the heavier buckets) + (an atomic cursor).  The cursor decides the ORDER in which independent
//     items are taken, nothing an item computes or where it writes: the outputs of two runs are the same bytes.
//   * sw_search_affine_pairs_wave<C>, ONE launch per class: its waves take the items of the class's list from a work counter, the
//     longest pairs first.  Nothing is sized by the item, so the buckets need no launches of their own.  The list's length is read from
//     device memory (the grid was planned on the host for the most it could be); the waves of an empty list leave after that one load.
//
// The cell recurrence, the state per lane, the software-pipelined loads, the boundary column between strips and the arg-max are those of
// sw_search_affine_multi_wave<C> (sw_search_affine.hip argues them: cells outside the matrix, ties, overflow); the strip body below is a
// further copy.  Per item the wave rebuilds, from the item and the query's entry of the call's table, the profile descriptor (exactly
// 257 x qpad bytes), the target descriptor (exactly len bytes), M = qlen + 1 and the strips; they are loaded with vector loads and made
// scalars with readfirstlane.  The result goes to results[out], the pair's place in the caller's list.  All global writes are vector
// stores or plain C++.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"

namespace swk {

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

constexpr u32 SP_OOB = 0xFFFFFF00u;     // buffer offset beyond every descriptor: the access is dropped (loads return 0)

__device__ __forceinline__ int sp_dpp_shr1(int old, int src) {   // lane l <- lane l-1; lane 0 keeps `old`
    return __builtin_amdgcn_update_dpp(old, src, 0x138, 0xF, 0xF, false);
}
__device__ __forceinline__ int sp_sbyte(u32 w, int j) { return (int)(signed char)(w >> (8 * j)); }

__device__ __forceinline__ int sp_wave_max(int v) {   // max over the 64 lanes, wave-uniform result (v >= 0)
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true));   // row_shr:1
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true));   // row_shr:2
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true));   // row_shr:4
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true));   // row_shr:8
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, true));   // row_bcast:15
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, true));   // row_bcast:31
    return __builtin_amdgcn_readlane(v, 63);
}

typedef int sp_v4i __attribute__((ext_vector_type(4)));
typedef int sp_v2i __attribute__((ext_vector_type(2)));

// the C profile bytes of one lane and row (C / 4 dwords)
template <int C>
__device__ __forceinline__ void sp_load_row(__amdgpu_buffer_rsrc_t r, u32 off, u32 (&s)[C / 4]) {
    if constexpr (C == 16) {
        const sp_v4i v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0);
        s[0] = (u32)v.x; s[1] = (u32)v.y; s[2] = (u32)v.z; s[3] = (u32)v.w;
    } else if constexpr (C == 8) {
        const sp_v2i v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 0);
        s[0] = (u32)v.x; s[1] = (u32)v.y;
    } else {
        s[0] = __builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0);
    }
}

template <int I, int N, typename F>
__device__ __forceinline__ void sp_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        sp_for<I + 1, N>(f);
    }
}

__device__ __forceinline__ int sp_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t sp_uniform64(int64_t v) {
    return (int64_t)(((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)((u64)v >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)(u32)(u64)v));
}

// The look-up both binning launches share: pair i of the chunk -> its item and its (class, bucket), or "no item of this group".
__device__ __forceinline__ bool sp_lookup(const SearchPairsBinParams& p, int64_t i, SearchPairItem& it, int& k, int& bucket) {
    const sw_pair pr = p.pairs[p.p0 + i];
    if ((u64)pr.query >= (u64)p.nqueries) return false;    // unsigned: a negative index is a huge one; nothing was loaded through it yet
    const int64_t t = p.entry_of[pr.query];
    if (t < p.cls_q0[0] || t >= p.cls_q0[SW_SP_CLASSES]) return false;   // a query of another group: that group's pass takes the pair
    if ((u64)pr.target >= (u64)p.ntargets) return false;
    const int64_t start = p.offsets[pr.target], len = p.offsets[pr.target + 1] - start;
    if (len <= 0) return false;                            // an empty target: the zeros stay
    it.start = start; it.out = p.p0 + i; it.len = (int)len; it.entry = (int)t;
    k = t < p.cls_q0[1] ? 0 : (t < p.cls_q0[2] ? 1 : 2);
    bucket = swp::search_pairs_bucket(len, p.queries[t].qpad);
    return true;
}

}  // namespace

// One thread per pair of the chunk.  SCATTER = false counts the items of every (class, bucket); SCATTER = true, launched behind it,
// writes the items.  Plain global atomics (vector instructions).
template <bool SCATTER>
__global__ void __launch_bounds__(256) sw_search_pairs_bin(SearchPairsBinParams p) {
    __shared__ unsigned int base[SW_SP_CLASSES * SW_SP_BUCKETS];
    if constexpr (SCATTER) {
        // the counts are final since the launch before.  Every workgroup works out where each (class, bucket) starts: class after
        // class, inside a class the heaviest bucket first; workgroup 0 also leaves every class's {length, first item} for its launch.
        for (int s = (int)threadIdx.x; s < SW_SP_CLASSES * SW_SP_BUCKETS; s += (int)blockDim.x) base[s] = p.ctl->count[s / SW_SP_BUCKETS][s % SW_SP_BUCKETS];
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned int at = 0;
            for (int k = 0; k < SW_SP_CLASSES; ++k) {
                const unsigned int first = at;
                for (int b = SW_SP_BUCKETS - 1; b >= 0; --b) {
                    const unsigned int n = base[k * SW_SP_BUCKETS + b];
                    base[k * SW_SP_BUCKETS + b] = at;
                    at += n;
                }
                if (blockIdx.x == 0) p.ctl->list[k] = SearchPairsList{at - first, first};
            }
        }
        __syncthreads();
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.np; i += (int64_t)gridDim.x * blockDim.x) {
        SearchPairItem it;
        int k = 0, bucket = 0;
        if (!sp_lookup(p, i, it, k, bucket)) continue;
        if constexpr (!SCATTER) atomicAdd(&p.ctl->count[k][bucket], 1u);
        else p.items[base[k * SW_SP_BUCKETS + bucket] + atomicAdd(&p.ctl->cursor[k][bucket], 1u)] = it;
    }
}
template __global__ void sw_search_pairs_bin<false>(SearchPairsBinParams);
template __global__ void sw_search_pairs_bin<true>(SearchPairsBinParams);

// C: query columns per lane (4, 8, 16)
template <int C>
__global__ void __launch_bounds__(256) sw_search_affine_pairs_wave(SearchPairsParams p) {
    static_assert(C % 4 == 0 && C <= 16, "C is a multiple of 4");
    constexpr int NQ = C / 4;
    // this launch's list: as long as the binning counted, behind the lists of the classes before
    const SearchPairsList list = *p.list;
    const u32 nitems = list.n;
    if (nitems == 0) return;
    const SearchPairItem* const items = p.items + list.first;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t slot = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;     // resident wave: its own boundary column
    const int ge = p.ge, goe = p.goe;
    // (a launch without a boundary workspace holds one-strip queries only: nothing goes through the empty descriptor)
    const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc((void*)(p.bnd ? p.bnd + slot * p.bnd_per : nullptr), 0,
                                                                        p.bnd ? (int)(p.bnd_per * 4) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc((void*)p.counter, 0, 4, 0x00020000);
    const u32 voffL0 = lane == 0 ? 0u : SP_OOB;    // lane 0 alone touches the counter and the result

    for (;;) {
        // the next item: a vector buffer atomic of lane 0 (the other lanes' offsets lie beyond the descriptor: dropped), read
        // back from lane 0 into a scalar; no lane-divergent branch anywhere in this loop (sw_search_wave says why)
        const u32 w = (u32)__builtin_amdgcn_readlane(__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(1, rC, (int)voffL0, 0, 0), 0);
        if (w >= nitems) break;
        // the item and its query: loads of wave-uniform addresses inside a loop that stores, which the compiler issues as vector loads
        // (global_load_dwordx2 / x3 / x4 in the gfx950 ISA of all three instantiations); readfirstlane tells it that these are scalars
        const SearchPairItem it = items[w];
        const MultiQuery d = p.queries[sp_uniform(it.entry)];
        const int len = sp_uniform(it.len);
        const int64_t start = sp_uniform64(it.start), out = sp_uniform64(it.out);
        const int qlen = sp_uniform(d.qlen), nstrips = sp_uniform(d.nstrips);
        const int64_t M = qlen + 1;
        const u32 qpad = (u32)sp_uniform(d.qpad);
        const bool multi = nstrips > 1;
        // the query's profile and the target's bytes through descriptors of exactly their extents: rows outside the target read 0 and
        // are mapped to PAD below
        const __amdgpu_buffer_rsrc_t rQ = __builtin_amdgcn_make_buffer_rsrc((void*)(p.prof + sp_uniform64(d.prof_off)), 0, (int)(SW_SEARCH_ROWS * qpad), 0x00020000);
        const __amdgpu_buffer_rsrc_t rT = __builtin_amdgcn_make_buffer_rsrc((void*)(p.db + start), 0, len, 0x00020000);
        const int G = (len + 64 + 3) / 4;      // steps 0 .. len + 63 (lane 63's last row)
        u64 kbest = 0;                         // per lane: best (score << 40 | MASK - index) over the strips done
        int sbest = 1;                         // wave-uniform: highest H seen so far (at least 1: zeros never count)

        for (int st = 0; st < nstrips; ++st) {
            const int c0 = st * 64 * C + lane * C + 1;
            const u32 colb = (u32)(c0 - 1);
            int h[C], e[C];
#pragma unroll
            for (int k = 0; k < C; ++k) { h[k] = 0; e[k] = goe; }
            int diag0 = 0, fout = goe, lbest = 0, lk = 0, lstep = 0;
            // boundary column, per row the pair (H of the strip's last column, F of the next strip's first): lane 63 writes row
            // u - 63 at pair index row + 64, lane 0 reads row u of the previous strip
            const bool bw = multi && st + 1 < nstrips, br = multi && st > 0;
            sp_v4i bq0 = {0, 0, 0, 0}, bq1 = {0, 0, 0, 0};
            const u32 voffB = lane == 0 ? 64u * 8u : SP_OOB;
            if (br) {   // (sc1 loads: served from L2, which this wave's own earlier stores have reached once vmcnt has drained)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                bq0 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 0, 16);
                bq1 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 16, 16);
            }
            // row r = 4 g + j - lane of this lane reads target byte r - 1; outside 1..len it takes the PAD row
            auto raw_of = [&](int g, int j) -> u32 {
                const u32 pos = (u32)(4 * g + j - lane - 1);
                return (u32)__builtin_amdgcn_raw_buffer_load_b8(rT, (int)(pos < (u32)len ? pos : SP_OOB), 0, 0);
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
            for (int j = 0; j < 4; ++j) sp_load_row<C>(rQ, row_off(0, j, raw[j]), S[j]);
#pragma unroll
            for (int j = 0; j < 4; ++j) raw[j] = raw_of(1, j);

            for (int g = 0; g < G; ++g) {
#pragma unroll
                for (int j = 0; j < 4; ++j) sp_load_row<C>(rQ, row_off(g + 1, j, raw[j]), Sn[j]);
#pragma unroll
                for (int j = 0; j < 4; ++j) raw[j] = raw_of(g + 2, j);
                const int bh[4] = {bq0.x, bq0.z, bq1.x, bq1.z}, bf[4] = {bq0.y, bq0.w, bq1.y, bq1.w};
                if (br) {
                    bq0 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 32 * (g + 1), 16);
                    bq1 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 32 * (g + 1) + 16, 16);
                }

                sp_for<0, 4>([&](auto J) {
                    constexpr int j = decltype(J)::value;
                    const int u = 4 * g + j;
                    // lane 0: the previous strip's pair of row u ((0, goe) beyond the target: rows no strip of this target wrote,
                    // and in strip 0: H[i][0] = 0, F[i][1] = goe)
                    const bool bin = br && u <= len;
                    const int left = sp_dpp_shr1(bin ? bh[j] : 0, h[C - 1]);
                    int f = sp_dpp_shr1(bin ? bf[j] : goe, fout);
                    int dprev = diag0;
                    diag0 = left;
                    sp_for<0, C>([&](auto K) {
                        constexpr int k = decltype(K)::value;
                        const int old = h[k];
                        const int t = dprev + sp_sbyte(S[j][k >> 2], k & 3);
                        const int hn = max(max(max(t, e[k]), f), 0);
                        const int x = hn + goe;
                        e[k] = max(e[k] + ge, x);
                        f = max(f + ge, x);
                        h[k] = hn;
                        dprev = old;
                    });
                    fout = f;
                    if (bw) __builtin_amdgcn_raw_buffer_store_b64(sp_v2i{h[C - 1], fout}, rB, lane == 63 ? 8 : (int)SP_OOB, 8 * u, 0);   // row u - 63 at pair index row + 64
                    // ---- arg-max: the row maximum against the wave's best so far; only a step that reaches it looks for the cell
                    int m = h[0];
#pragma unroll
                    for (int k = 1; k + 1 < C; k += 2) m = max(max(m, h[k]), h[k + 1]);
                    m = max(m, h[C - 1]);
                    if (__builtin_amdgcn_ballot_w64(m >= sbest) != 0) {
                        sbest = max(sbest, sp_wave_max(m));
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
        // the pair's arg-max: highest score, lowest linear index among equals
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const u32 olo = (u32)__shfl_xor((int)(u32)kbest, off), ohi = (u32)__shfl_xor((int)(u32)(kbest >> 32), off);
            const u64 o = ((u64)ohi << 32) | olo;
            kbest = o > kbest ? o : kbest;
        }
        {
            const __amdgpu_buffer_rsrc_t rR = __builtin_amdgcn_make_buffer_rsrc((void*)(p.results + out), 0, (int)sizeof(sw_result), 0x00020000);
            const u64 score = kbest >> 40, pos = kbest ? SW_KEY_IDX_MASK - (kbest & SW_KEY_IDX_MASK) : 0;
            const sp_v4i v = {(int)(u32)pos, (int)(u32)(pos >> 32), (int)(u32)score, 0};
            __builtin_amdgcn_raw_buffer_store_b128(v, rR, (int)voffL0, 0, 0);                 // max_pos, max_score
            __builtin_amdgcn_raw_buffer_store_b64(sp_v2i{0, 0}, rR, (int)voffL0, 16, 0);      // path_len
        }
    }
}

template __global__ void sw_search_affine_pairs_wave<4>(SearchPairsParams);
template __global__ void sw_search_affine_pairs_wave<8>(SearchPairsParams);
template __global__ void sw_search_affine_pairs_wave<16>(SearchPairsParams);

}  // namespace swk
