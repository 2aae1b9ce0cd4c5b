// sw_align_affine.hip -- the alignment of chosen hits under affine scoring (gfx950): Gotoh's recurrence re-filled with one direction
// byte per cell, and the walk of the canonical alignment (include/swhip.h) through its three states, both by the same wave.
//
// The fill is that of sw_search_affine_wave (sw_search_affine.hip: the mapping, the state per lane, the cells outside the matrix and
// the arg-max are described there and hold here word for word).  What a cell (r, c) adds is its direction byte:
//   bits 0-1  where H[r][c] came from: 0 nothing positive, 1 the diagonal, 2 E[r][c], 3 F[r][c] -- compared in that order, the
//             reference's DIAGONAL > UP > LEFT
//   bit 2     E[r+1][c] = max(E[r][c] + ge, H[r][c] + goe) took the second: the gap BELOW this cell opens here (a tie opens)
//   bit 3     F[r][c+1] likewise: the gap RIGHT of this cell opens here
// The open bits are recorded in the cell that computes them, so nothing crosses a lane or a strip on their account; the walk in state
// E at (i, j) reads bit 2 of (i-1, j), in state F bit 3 of (i, j-1), and row 1 / column 1 are open by definition (E[1][j] = F[i][1] =
// goe).  A lane packs the C bytes of its row into C / 4 dwords and stores them with one 4 / 8 / 16-byte vector store at
// (r - 1) * qpad + c - 1 of its wave's slot: the wave writes whole lines of a row; rows outside 1..len go to an offset beyond the
// descriptor and are dropped.
//
// The walk.  After the last strip the wave drains vmcnt -- its own stores have then reached the L2 -- and reads the matrix with sc1
// loads only, which are served from the L2: the L1 of the CU may still hold lines of the hit that used the slot before.  It stages
// windows of 64 rows x 64 bytes in LDS (16 bytes per lane and load, coalesced) that end at the cell it stands on, and takes a whole
// run per LDS round trip: in state H lane l looks at (i - l, j - l) and the ballot of "came from the diagonal" gives the length of
// the run of M; in state E / F lane l looks at the open bit l cells up / left and the first opener ends the run of D / I.  It walks
// twice: once to count the ops and find the begin corner, once to write the ops in alignment order (skipped where they do not fit).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"
#include "sw_wave.h"

namespace swk {

namespace {

constexpr int AA_SC1 = 16;              // aux bit of the buffer builtins: sc1

constexpr int AA_WIN = 64;              // the walk's window: AA_WIN rows of AA_WIN direction bytes per wave

}  // namespace

// C: query columns per lane (4, 8, 16)
template <int C>
__global__ void __launch_bounds__(256) sw_align_affine_wave(AlignAffineParams p) {
    static_assert(C % 4 == 0 && C <= 16, "C is a multiple of 4");
    constexpr int NQ = C / 4;
    __shared__ sw_v4i win_all[4][AA_WIN * AA_WIN / 16];
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
    const int ops_size = (int)(p.ops ? (p.ops_cap < 0x7FFFFF00ll ? p.ops_cap : 0x7FFFFF00ll) : 0);

    for (;;) {
        // the next hit: a vector buffer atomic of lane 0, read back into a scalar (sw_search_wave says why)
        const u32 w = (u32)__builtin_amdgcn_readlane(__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(1, rC, (int)voffL0, 0, 0), 0);
        if ((int64_t)w >= p.nitems) break;
        const SearchItem it = p.items[w];
        const int len = (int)it.len;
        const __amdgpu_buffer_rsrc_t rT = __builtin_amdgcn_make_buffer_rsrc((void*)(p.db + it.start), 0, len, 0x00020000);
        const int G = (len + 64 + 3) / 4;      // steps 0 .. len + 63 (lane 63's last row)
        const u64 tick0 = p.stamps ? wall_clock64() : 0;
        u64 kbest = 0;                         // per lane: best (score << 40 | MASK - index) over the strips done
        int sbest = 1;                         // wave-uniform: highest H seen so far (at least 1: zeros never count)

        for (int st = 0; st < nstrips; ++st) {
            const int c0 = st * 64 * C + lane * C + 1;
            const u32 colb = (u32)(c0 - 1);
            int h[C], e[C];
#pragma unroll
            for (int k = 0; k < C; ++k) { h[k] = 0; e[k] = goe; }
            int diag0 = 0, fout = goe, lbest = 0, lk = 0, lstep = 0;
            const bool bw = multi && st + 1 < nstrips, br = multi && st > 0;
            sw_v4i bq0 = {0, 0, 0, 0}, bq1 = {0, 0, 0, 0};
            const u32 voffB = lane == 0 ? 64u * 8u : SW_OOB;
            if (br) {   // (sc1 loads: served from L2, which this wave's own earlier stores have reached once vmcnt has drained)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                bq0 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 0, AA_SC1);
                bq1 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 16, AA_SC1);
            }
            auto raw_of = [&](int g, int j) -> u32 {
                const u32 pos = (u32)(4 * g + j - lane - 1);
                return (u32)__builtin_amdgcn_raw_buffer_load_b8(rT, (int)(pos < (u32)len ? pos : SW_OOB), 0, 0);
            };
            auto row_off = [&](int g, int j, u32 raw) -> u32 {
                const u32 pos = (u32)(4 * g + j - lane - 1);
                return (pos < (u32)len ? raw : 256u) * qpad + colb;
            };
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
                const int bh[4] = {bq0.x, bq0.z, bq1.x, bq1.z}, bf[4] = {bq0.y, bq0.w, bq1.y, bq1.w};
                if (br) {
                    bq0 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 32 * (g + 1), AA_SC1);
                    bq1 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 32 * (g + 1) + 16, AA_SC1);
                }

                sw_for<0, 4>([&](auto J) {
                    constexpr int j = decltype(J)::value;
                    const int u = 4 * g + j;
                    const bool bin = br && u <= len;
                    const int left = sw_dpp_shr1(bin ? bh[j] : 0, h[C - 1]);
                    int f = sw_dpp_shr1(bin ? bf[j] : goe, fout);
                    int dprev = diag0;
                    diag0 = left;
                    u32 dw[NQ];
#pragma unroll
                    for (int q = 0; q < NQ; ++q) dw[q] = 0;
                    sw_for<0, C>([&](auto K) {
                        constexpr int k = decltype(K)::value;
                        const int old = h[k];
                        const int t = dprev + sw_sbyte(S[j][k >> 2], k & 3);
                        const int ek = e[k];
                        const int hn = max(max(max(t, ek), f), 0);
                        u32 d = hn == ek ? 2u : 3u;            // the compare order of the canonical alignment: diagonal, E, F
                        d = hn == t ? 1u : d;
                        d = hn == 0 ? 0u : d;
                        const int x = hn + goe, eg = ek + ge, fg = f + ge;
                        d |= x >= eg ? 4u : 0u;                // opening wins a tie against extending
                        d |= x >= fg ? 8u : 0u;
                        e[k] = max(eg, x);
                        f = max(fg, x);
                        h[k] = hn;
                        dprev = old;
                        dw[k >> 2] |= d << (8 * (k & 3));
                    });
                    fout = f;
                    if (bw) __builtin_amdgcn_raw_buffer_store_b64(sw_v2i{h[C - 1], fout}, rB, lane == 63 ? 8 : (int)SW_OOB, 8 * u, 0);   // row u - 63 at pair index row + 64
                    {   // the direction bytes of row u - lane, columns c0 .. c0 + C - 1
                        const u32 r1 = (u32)(u - lane - 1);
                        sw_store_row<C>(rD, r1 < (u32)len ? r1 * qpad + colb : SW_OOB, dw);
                    }
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
        // the hit's arg-max: highest score, lowest linear index among equals
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const u32 olo = (u32)__shfl_xor((int)(u32)kbest, off), ohi = (u32)__shfl_xor((int)(u32)(kbest >> 32), off);
            const u64 o = ((u64)ohi << 32) | olo;
            kbest = o > kbest ? o : kbest;
        }
        kbest = ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(kbest >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)(u32)kbest);
        const u64 score = kbest >> 40, pos = kbest ? SW_KEY_IDX_MASK - (kbest & SW_KEY_IDX_MASK) : 0;
        const int i1 = (int)(pos / (u64)M), j1 = (int)(pos - (u64)i1 * (u64)M);

        // ---- the walk: every store of this hit has left the wave; the matrix is read past the L1 (sc1), a window at a time
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const u64 tick1 = p.stamps ? wall_clock64() : 0;
        const __amdgpu_buffer_rsrc_t rO = __builtin_amdgcn_make_buffer_rsrc((void*)(p.ops ? p.ops + it.idx * p.ops_cap : nullptr), 0, ops_size, 0x00020000);
        int i0 = 0, j0 = 0, nops = 0;
        for (int pass = 0; pass < 2; ++pass) {
            if (pass == 1 && (nops == 0 || p.ops == nullptr || (int64_t)nops > p.ops_cap)) break;
            int i = i1, j = j1, state = 0, n = 0;
            int wr0 = 1 << 30, wcb = 1 << 30;      // first row and first byte column of the window in LDS (none yet)
            bool done = score == 0;
            // `cnt` ops `ch` behind the n already taken: the walk goes backwards, op k from the end lies at nops - 1 - k
            auto emit = [&](int cnt, int ch) {
                if (pass == 1) __builtin_amdgcn_raw_buffer_store_b8((unsigned char)ch, rO, lane < cnt ? nops - 1 - n - lane : (int)SW_OOB, 0, 0);
                n += cnt;
            };
            // (every round takes at least one op or changes the state once per op: the bound is never reached, it only keeps a damaged
            //  matrix from holding the wave)
            for (int round = 0, rounds = 2 * (len + qlen) + 8; !done && round < rounds; ++round) {
                if (i < 1 || j < 1) break;          // H at the edge of the matrix: 0 (E and F leave for H before they get here)
                // the cell the lanes look back from: (i, j) in H, one up in E, one left in F
                const int ai = state == 2 ? i - 1 : i, aj = state == 3 ? j - 1 : j;
                if (ai >= 1 && aj >= 1 && (ai < wr0 || aj - 1 < wcb)) {
                    wr0 = ai - (AA_WIN - 1);
                    wcb = ((aj - 1) & ~15) - (AA_WIN - 16);
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    sw_v4i v[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int row = wr0 + 16 * q + (lane >> 2), cb = wcb + 16 * (lane & 3);
                        const bool in = row >= 1 && row <= len && cb >= 0;
                        v[q] = __builtin_amdgcn_raw_buffer_load_b128(rD, in ? (int)((u32)(row - 1) * qpad + (u32)cb) : (int)SW_OOB, 0, AA_SC1);
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) win[(16 * q + (lane >> 2)) * (AA_WIN / 16) + (lane & 3)] = v[q];
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
                // lane l: the cell l steps back along the state's direction; `known`: outside the matrix (a fixed answer) or in the window
                const int r = state == 3 ? ai : ai - lane, c = state == 2 ? aj : aj - lane;
                const bool inside = r >= 1 && c >= 1, inwin = inside && r >= wr0 && c - 1 >= wcb;
                const bool known = !inside || inwin;
                const int b = inwin ? (int)winb[(r - wr0) * AA_WIN + (c - 1 - wcb)] : 0;
                if (state == 0) {
                    const u64 notdiag = ~__builtin_amdgcn_ballot_w64(known && (b & 3) == 1);
                    const int run = notdiag ? (int)__builtin_ctzll(notdiag) : 64;
                    emit(run, 'M');
                    i -= run; j -= run;
                    if (run < 64 && __builtin_amdgcn_readlane((int)known, run)) {
                        const int src = __builtin_amdgcn_readlane(b, run) & 3;
                        if (src == 0) done = true; else state = src;
                    }
                } else {
                    const bool open = !inside || (b & (state == 2 ? 4 : 8)) != 0;
                    const u64 stop = __builtin_amdgcn_ballot_w64(!known || open);
                    const int first = stop ? (int)__builtin_ctzll(stop) : 64;
                    // lanes 0 .. first - 1 extend; lane `first` opens (one more op, back to H) or lies beyond the window
                    const bool opens = first < 64 && __builtin_amdgcn_readlane((int)known, first);
                    const int cnt = first + (opens ? 1 : 0);
                    emit(cnt, state == 2 ? 'D' : 'I');
                    if (state == 2) i -= cnt; else j -= cnt;
                    if (opens) state = 0;
                }
            }
            if (pass == 0) { nops = n; i0 = i; j0 = j; }
        }
        {
            const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc((void*)(p.aln + it.idx), 0, (int)sizeof(sw_alignment), 0x00020000);
            const bool any = score != 0;
            const sw_v4i v0 = {(int)(u32)pos, (int)(u32)(pos >> 32), (int)(u32)score, 0};
            const sw_v4i v1 = {any ? j0 : 0, 0, any ? i0 : 0, 0};
            const sw_v4i v2 = {any ? j1 : 0, 0, any ? i1 : 0, 0};
            __builtin_amdgcn_raw_buffer_store_b128(v0, rA, (int)voffL0, 0, 0);                    // max_pos, max_score
            __builtin_amdgcn_raw_buffer_store_b128(v1, rA, (int)voffL0, 16, 0);                   // q_begin, t_begin
            __builtin_amdgcn_raw_buffer_store_b128(v2, rA, (int)voffL0, 32, 0);                   // q_end, t_end
            __builtin_amdgcn_raw_buffer_store_b64(sw_v2i{nops, 0}, rA, (int)voffL0, 48, 0);       // nops
        }
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
