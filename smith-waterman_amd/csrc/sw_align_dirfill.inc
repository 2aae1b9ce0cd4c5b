// sw_align_dirfill.inc -- the whole-matrix direction fill of one (target, query) item under affine gaps by one wave (gfx950): the
// statements that sw_align_affine_wave<C> and sw_align_hits_wave<C> run between taking an item and walking its alignment.  Each of them
// includes this file once, inside its loop over the items; there is no other copy of the text.  (Text, not a function, for the reason
// sw_gotoh_sweep.inc gives; included, the kernels' instructions are those of the copies this file replaces -- DESIGN 9f.)  The band
// fill of sw_align_ckpt.hip (bands, resumed state, checkpoint rows) is not a copy of it and stays there.
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
// In scope where it is included (sw_wave.h for the primitives), all wave-uniform but `lane`:
//   C (a constant expression: columns per lane, 4 / 8 / 16) and NQ = C / 4;  int lane;
//   __amdgpu_buffer_rsrc_t rQ  the query's profile, 257 x qpad bytes;  rT  exactly the target's len bytes;
//                          rB  the wave's boundary column (an empty descriptor where nstrips == 1: nothing goes through it);
//                          rD  the wave's slot: len x qpad direction bytes, row stride qpad;
//   int len, qlen, nstrips;  u32 qpad;  int64_t M = qlen + 1;  bool multi = nstrips > 1;  int ge, goe.
// It leaves the direction bytes of rows 1..len in the slot -- stores that may still be in flight: the includer drains vmcnt before it
// reads them -- and, wave-uniform, the item's arg-max (highest score, lowest linear index among equals; all 0 if nothing is positive):
//   u64 score, pos = i1 M + j1;  int i1, j1  the row and the column of the cell.
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
            const bool bw = multi && st + 1 < nstrips, br = multi && st > 0;
            sw_v4i bq0 = {0, 0, 0, 0}, bq1 = {0, 0, 0, 0};
            const u32 voffB = lane == 0 ? 64u * 8u : SW_OOB;
            if (br) {   // (sc1 loads: served from L2, which this wave's own earlier stores have reached once vmcnt has drained)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                bq0 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 0, SW_SC1);
                bq1 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 16, SW_SC1);
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
                    bq0 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 32 * (g + 1), SW_SC1);
                    bq1 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 32 * (g + 1) + 16, SW_SC1);
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
        // the item's arg-max: highest score, lowest linear index among equals
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const u32 olo = (u32)__shfl_xor((int)(u32)kbest, off), ohi = (u32)__shfl_xor((int)(u32)(kbest >> 32), off);
            const u64 o = ((u64)ohi << 32) | olo;
            kbest = o > kbest ? o : kbest;
        }
        kbest = ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(kbest >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)(u32)kbest);
        const u64 score = kbest >> 40, pos = kbest ? SW_KEY_IDX_MASK - (kbest & SW_KEY_IDX_MASK) : 0;
        const int i1 = (int)(pos / (u64)M), j1 = (int)(pos - (u64)i1 * (u64)M);
