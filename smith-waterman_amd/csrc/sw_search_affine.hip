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
// fills it from the caller's table).
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
    const u32 voffL0 = lane == 0 ? 0u : SA_OOB;    // lane 0 alone touches the counter and the result

    for (;;) {
        // the next target: a vector buffer atomic of lane 0 (the other lanes' offsets lie beyond the descriptor: dropped), read
        // back from lane 0 into a scalar; no lane-divergent branch anywhere in this loop (sw_search_wave says why)
        const u32 w = (u32)__builtin_amdgcn_readlane(__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(1, rC, (int)voffL0, 0, 0), 0);
        if ((int64_t)w >= p.nitems) break;
        const SearchItem it = p.items[w];
        const int len = (int)it.len;
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
        // the target's arg-max: highest score, lowest linear index among equals
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const u32 olo = (u32)__shfl_xor((int)(u32)kbest, off), ohi = (u32)__shfl_xor((int)(u32)(kbest >> 32), off);
            const u64 o = ((u64)ohi << 32) | olo;
            kbest = o > kbest ? o : kbest;
        }
        {
            const __amdgpu_buffer_rsrc_t rR = __builtin_amdgcn_make_buffer_rsrc((void*)(p.results + it.idx), 0, (int)sizeof(sw_result), 0x00020000);
            const u64 score = kbest >> 40, pos = kbest ? SW_KEY_IDX_MASK - (kbest & SW_KEY_IDX_MASK) : 0;
            const sa_v4i v = {(int)(u32)pos, (int)(u32)(pos >> 32), (int)(u32)score, 0};
            __builtin_amdgcn_raw_buffer_store_b128(v, rR, (int)voffL0, 0, 0);                 // max_pos, max_score
            __builtin_amdgcn_raw_buffer_store_b64(sa_v2i{0, 0}, rR, (int)voffL0, 16, 0);      // path_len
        }
    }
}

template __global__ void sw_search_affine_wave<4>(SearchAffineParams);
template __global__ void sw_search_affine_wave<8>(SearchAffineParams);
template __global__ void sw_search_affine_wave<16>(SearchAffineParams);

}  // namespace swk
