// sw_gotoh_sweep.inc -- the score-only sweep of one (target, query) pair under affine gaps by one wave (gfx950): the statements that
// sw_search_affine_wave<C>, sw_search_affine_multi_wave<C> and sw_search_affine_pairs_wave<C> run between taking a work item and storing
// its result.  Each of them includes this file once, inside its loop over the work items; there is no other copy of the text.  The header
// of sw_search_affine.hip defines the recurrence and argues the state per lane, the cells outside the matrix, the tie rule and the
// overflow bound: that argument is about these statements.  (Text, not a function: as a __forceinline__ routine the same statements
// compiled to different code objects, 0.3 - 1.3 % slower per kernel on the MI355X -- DESIGN 9f; included, the kernels' instructions are
// those of the copies this file replaces.)  The direction-byte fills of the alignment kernels keep sweeps of their own.
//
// In scope where it is included (sw_wave.h for the primitives), all wave-uniform but `lane`:
//   C (a constant expression: columns per lane, 4 / 8 / 16) and NQ = C / 4;  int lane;
//   __amdgpu_buffer_rsrc_t rQ  the query's profile, 257 x qpad bytes;  rT  exactly the target's len bytes;
//                          rB  the wave's boundary column (an empty descriptor where nstrips == 1: nothing goes through it);
//   int len, qlen, nstrips;  u32 qpad;  int64_t M = qlen + 1;  bool multi = nstrips > 1;  int ge, goe.
// (M, multi and NQ stay with the kernels, each where it has always declared them: declared here instead, the instructions come out in
// another order.)  It leaves, in every lane,  u64 kbest = score << 40 | SW_KEY_IDX_MASK - (row M + column)  of the pair's arg-max --
// highest score, lowest linear index among equals -- or 0 if nothing is positive.
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
            sw_v4i bq0 = {0, 0, 0, 0}, bq1 = {0, 0, 0, 0};
            const u32 voffB = lane == 0 ? 64u * 8u : SW_OOB;
            if (br) {   // (sc1 loads: served from L2, which this wave's own earlier stores have reached once vmcnt has drained)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                bq0 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 0, 16);
                bq1 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 16, 16);
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
                const int bh[4] = {bq0.x, bq0.z, bq1.x, bq1.z}, bf[4] = {bq0.y, bq0.w, bq1.y, bq1.w};
                if (br) {
                    bq0 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 32 * (g + 1), 16);
                    bq1 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 32 * (g + 1) + 16, 16);
                }

                sw_for<0, 4>([&](auto J) {
                    constexpr int j = decltype(J)::value;
                    const int u = 4 * g + j;
                    // lane 0: the previous strip's pair of row u ((0, goe) beyond the target: rows no strip of this target wrote,
                    // and in strip 0: H[i][0] = 0, F[i][1] = goe)
                    const bool bin = br && u <= len;
                    const int left = sw_dpp_shr1(bin ? bh[j] : 0, h[C - 1]);
                    int f = sw_dpp_shr1(bin ? bf[j] : goe, fout);
                    int dprev = diag0;
                    diag0 = left;
                    sw_for<0, C>([&](auto K) {
                        constexpr int k = decltype(K)::value;
                        const int old = h[k];
                        const int t = dprev + sw_sbyte(S[j][k >> 2], k & 3);
                        const int hn = max(max(max(t, e[k]), f), 0);
                        const int x = hn + goe;
                        e[k] = max(e[k] + ge, x);
                        f = max(f + ge, x);
                        h[k] = hn;
                        dprev = old;
                    });
                    fout = f;
                    if (bw) __builtin_amdgcn_raw_buffer_store_b64(sw_v2i{h[C - 1], fout}, rB, lane == 63 ? 8 : (int)SW_OOB, 8 * u, 0);   // row u - 63 at pair index row + 64
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
        // the pair's arg-max: highest score, lowest linear index among equals
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const u32 olo = (u32)__shfl_xor((int)(u32)kbest, off), ohi = (u32)__shfl_xor((int)(u32)(kbest >> 32), off);
            const u64 o = ((u64)ohi << 32) | olo;
            kbest = o > kbest ? o : kbest;
        }
