// sw_search_multi.hip -- many queries against a prepared database (sw_db_search_affine): the affine search of sw_search_affine.hip with
// a loop around it that takes (target, query) pairs, score and arg-max only (gfx950).
//
// The cell recurrence, the state per lane, the software-pipelined loads, the boundary column between strips and the arg-max are those of
// sw_search_affine_wave<C>, and that file's header argues them (cells outside the matrix, ties, overflow); the strip body below is a
// second copy of it.  What is new is what a wave does between two sweeps:
//   * work item w, taken with the vector buffer atomic of lane 0, is the pair (target rank rank0 + w / nq, query w % nq of the launch):
//     every query of the launch against the longest target first (sw_plan.h, plan_search_multi);
//   * the query comes as a wave-uniform MultiQuery from the call's device table: the profile descriptor (257 x qpad bytes at prof_off
//     of the group's workspace), M = qlen + 1, the strips and the result row are rebuilt per item -- scalar loads and scalar
//     arithmetic, a few dozen cycles against the thousands of a sweep;
//   * the result goes to results[row * ntargets + idx]: query-major, the caller's order on both axes.
// A launch holds the queries of ONE class (columns per lane), so C stays a template parameter and the strip body keeps its registers.
// sw_search_profile_submat_multi fills the profiles of a whole group in one launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"

namespace swk {

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

constexpr u32 SA_OOB = 0xFFFFFF00u;     // buffer offset beyond every descriptor: the access is dropped (loads return 0)

__device__ __forceinline__ int sa_dpp_shr1(int old, int src) {   // lane l <- lane l-1; lane 0 keeps `old`
    return __builtin_amdgcn_update_dpp(old, src, 0x138, 0xF, 0xF, false);
}
__device__ __forceinline__ int sa_sbyte(u32 w, int j) { return (int)(signed char)(w >> (8 * j)); }

__device__ __forceinline__ int sa_wave_max(int v) {   // max over the 64 lanes, wave-uniform result (v >= 0)
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true));   // row_shr:1
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true));   // row_shr:2
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true));   // row_shr:4
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true));   // row_shr:8
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, true));   // row_bcast:15
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, true));   // row_bcast:31
    return __builtin_amdgcn_readlane(v, 63);
}

typedef int sa_v4i __attribute__((ext_vector_type(4)));
typedef int sa_v2i __attribute__((ext_vector_type(2)));

// the C profile bytes of one lane and row (C / 4 dwords)
template <int C>
__device__ __forceinline__ void sa_load_row(__amdgpu_buffer_rsrc_t r, u32 off, u32 (&s)[C / 4]) {
    if constexpr (C == 16) {
        const sa_v4i v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0);
        s[0] = (u32)v.x; s[1] = (u32)v.y; s[2] = (u32)v.z; s[3] = (u32)v.w;
    } else if constexpr (C == 8) {
        const sa_v2i v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 0);
        s[0] = (u32)v.x; s[1] = (u32)v.y;
    } else {
        s[0] = __builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0);
    }
}

template <int I, int N, typename F>
__device__ __forceinline__ void sa_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        sa_for<I + 1, N>(f);
    }
}

}  // namespace

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
    const u32 voffL0 = lane == 0 ? 0u : SA_OOB;    // lane 0 alone touches the counter and the result

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
        // the target's bytes through a descriptor of exactly its extent: rows outside it read 0 and are mapped to PAD below
        const __amdgpu_buffer_rsrc_t rT = __builtin_amdgcn_make_buffer_rsrc((void*)(p.db + it.start), 0, len, 0x00020000);
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
            sa_v4i bq0 = {0, 0, 0, 0}, bq1 = {0, 0, 0, 0};
            const u32 voffB = lane == 0 ? 64u * 8u : SA_OOB;
            if (br) {   // (sc1 loads: served from L2, which this wave's own earlier stores have reached once vmcnt has drained)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                bq0 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 0, 16);
                bq1 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 16, 16);
            }
            // row r = 4 g + j - lane of this lane reads target byte r - 1; outside 1..len it takes the PAD row
            auto raw_of = [&](int g, int j) -> u32 {
                const u32 pos = (u32)(4 * g + j - lane - 1);
                return (u32)__builtin_amdgcn_raw_buffer_load_b8(rT, (int)(pos < (u32)len ? pos : SA_OOB), 0, 0);
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
            for (int j = 0; j < 4; ++j) sa_load_row<C>(rQ, row_off(0, j, raw[j]), S[j]);
#pragma unroll
            for (int j = 0; j < 4; ++j) raw[j] = raw_of(1, j);

            for (int g = 0; g < G; ++g) {
#pragma unroll
                for (int j = 0; j < 4; ++j) sa_load_row<C>(rQ, row_off(g + 1, j, raw[j]), Sn[j]);
#pragma unroll
                for (int j = 0; j < 4; ++j) raw[j] = raw_of(g + 2, j);
                const int bh[4] = {bq0.x, bq0.z, bq1.x, bq1.z}, bf[4] = {bq0.y, bq0.w, bq1.y, bq1.w};
                if (br) {
                    bq0 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 32 * (g + 1), 16);
                    bq1 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 32 * (g + 1) + 16, 16);
                }

                sa_for<0, 4>([&](auto J) {
                    constexpr int j = decltype(J)::value;
                    const int u = 4 * g + j;
                    // lane 0: the previous strip's pair of row u ((0, goe) beyond the target: rows no strip of this target wrote,
                    // and in strip 0: H[i][0] = 0, F[i][1] = goe)
                    const bool bin = br && u <= len;
                    const int left = sa_dpp_shr1(bin ? bh[j] : 0, h[C - 1]);
                    int f = sa_dpp_shr1(bin ? bf[j] : goe, fout);
                    int dprev = diag0;
                    diag0 = left;
                    sa_for<0, C>([&](auto K) {
                        constexpr int k = decltype(K)::value;
                        const int old = h[k];
                        const int t = dprev + sa_sbyte(S[j][k >> 2], k & 3);
                        const int hn = max(max(max(t, e[k]), f), 0);
                        const int x = hn + goe;
                        e[k] = max(e[k] + ge, x);
                        f = max(f + ge, x);
                        h[k] = hn;
                        dprev = old;
                    });
                    fout = f;
                    if (bw) __builtin_amdgcn_raw_buffer_store_b64(sa_v2i{h[C - 1], fout}, rB, lane == 63 ? 8 : (int)SA_OOB, 8 * u, 0);   // row u - 63 at pair index row + 64
                    // ---- arg-max: the row maximum against the wave's best so far; only a step that reaches it looks for the cell
                    int m = h[0];
#pragma unroll
                    for (int k = 1; k + 1 < C; k += 2) m = max(max(m, h[k]), h[k + 1]);
                    m = max(m, h[C - 1]);
                    if (__builtin_amdgcn_ballot_w64(m >= sbest) != 0) {
                        sbest = max(sbest, sa_wave_max(m));
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
            const __amdgpu_buffer_rsrc_t rR = __builtin_amdgcn_make_buffer_rsrc((void*)(p.results + d.row * p.ntargets + it.idx), 0, (int)sizeof(sw_result), 0x00020000);
            const u64 score = kbest >> 40, pos = kbest ? SW_KEY_IDX_MASK - (kbest & SW_KEY_IDX_MASK) : 0;
            const sa_v4i v = {(int)(u32)pos, (int)(u32)(pos >> 32), (int)(u32)score, 0};
            __builtin_amdgcn_raw_buffer_store_b128(v, rR, (int)voffL0, 0, 0);                 // max_pos, max_score
            __builtin_amdgcn_raw_buffer_store_b64(sa_v2i{0, 0}, rR, (int)voffL0, 16, 0);      // path_len
        }
    }
}

template __global__ void sw_search_affine_multi_wave<4>(SearchMultiParams);
template __global__ void sw_search_affine_multi_wave<8>(SearchMultiParams);
template __global__ void sw_search_affine_multi_wave<16>(SearchMultiParams);

}  // namespace swk
