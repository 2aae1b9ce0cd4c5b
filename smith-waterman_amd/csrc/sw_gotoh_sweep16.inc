// sw_gotoh_sweep16.inc -- the score-only sweep of TWO targets against one query under affine gaps by one wave, on packed 16-bit lanes
// (gfx950): the statements sw_search_multi_pk_wave<C> runs between taking a work item and storing its two results.  It is the text of
// sw_gotoh_sweep.inc with every score a pair of 16-bit halves: target A (the longer one) in the low halves, target B in the high halves.
// Same rows, same columns, same skew of one row per lane; the letters differ, so a row costs two byte loads and two profile-row loads.
// The header of sw_search_multi16.hip argues the halves' bounds and what the partner may and may not see.
//
// In scope where it is included (sw_wave.h for the primitives; GS16_CELL2 / gs16_cell2, gs16_max, gs16_min of the including file), all
// wave-uniform but `lane`:
//   C (a constant expression: columns per lane, 4 / 8 / 16) and NQ = C / 4;  int lane;
//   __amdgpu_buffer_rsrc_t rQ  the query's profile, 257 x qpad bytes;  rTA, rTB  exactly the targets' lenA, lenB bytes;
//                          rB  the wave's boundary column (an empty descriptor where nstrips == 1: nothing goes through it);
//   int lenA >= lenB >= 0, qlen, nstrips;  u32 qpad;  int64_t M = qlen + 1;  bool multi = nstrips > 1;
//   u32 ge2, goe2: gap_extend and gap_open + gap_extend in both halves.
// It leaves, in every lane,  u64 kbestA, kbestB = score << 40 | SW_KEY_IDX_MASK - (row M + column)  of either pair's arg-max -- highest
// score, lowest linear index among equals -- or 0 if nothing is positive.
        const int G = (lenA + 64 + 3) / 4;     // steps 0 .. lenA + 63 (lane 63's last row of the longer target)
        u64 kbestA = 0, kbestB = 0;            // per lane and target: best (score << 40 | MASK - index) over the strips done
        int sbestA = 1, sbestB = 1;            // wave-uniform, per target: highest H seen so far (at least 1: zeros never count)

        for (int st = 0; st < nstrips; ++st) {
            const int c0 = st * 64 * C + lane * C + 1;
            const u32 colb = (u32)(c0 - 1);
            u32 h[C], e[C];
#pragma unroll
            for (int k = 0; k < C; ++k) { h[k] = 0; e[k] = goe2; }
            u32 diag0 = 0, fout = goe2;
            // per lane and target: the best row maximum and where it was first seen, step << 4 | column of the lane
            int lbestA = 0, lbestB = 0, lposA = 0, lposB = 0;
            // boundary column, per row the pair (H of the strip's last column, F of the next strip's first), both targets in each of the
            // two ints: lane 63 writes row u - 63 at pair index row + 64, lane 0 reads row u of the previous strip
            const bool bw = multi && st + 1 < nstrips, br = multi && st > 0;
            sw_v4i bq0 = {0, 0, 0, 0}, bq1 = {0, 0, 0, 0};
            const u32 voffB = lane == 0 ? 64u * 8u : SW_OOB;
            if (br) {   // (sc1 loads: served from L2, which this wave's own earlier stores have reached once vmcnt has drained)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                bq0 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 0, 16);
                bq1 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 16, 16);
            }
            // row r = 4 g + j - lane of this lane reads byte r - 1 of either target; outside 1..len it takes the PAD row
            auto raw_of = [&](__amdgpu_buffer_rsrc_t rT, int len, int g, int j) -> u32 {
                const u32 pos = (u32)(4 * g + j - lane - 1);
                return (u32)__builtin_amdgcn_raw_buffer_load_b8(rT, (int)(pos < (u32)len ? pos : SW_OOB), 0, 0);
            };
            auto row_off = [&](int len, int g, int j, u32 raw) -> u32 {
                const u32 pos = (u32)(4 * g + j - lane - 1);
                return (pos < (u32)len ? raw : 256u) * qpad + colb;
            };
            // software pipeline: the bytes of group g + 2 and the profile rows of group g + 1 are in flight while group g computes
            u32 rawA[4], rawB[4], SA[4][NQ], SB[4][NQ], SAn[4][NQ], SBn[4][NQ];
#pragma unroll
            for (int j = 0; j < 4; ++j) { rawA[j] = raw_of(rTA, lenA, 0, j); rawB[j] = raw_of(rTB, lenB, 0, j); }
#pragma unroll
            for (int j = 0; j < 4; ++j) { sw_load_row<C>(rQ, row_off(lenA, 0, j, rawA[j]), SA[j]); sw_load_row<C>(rQ, row_off(lenB, 0, j, rawB[j]), SB[j]); }
#pragma unroll
            for (int j = 0; j < 4; ++j) { rawA[j] = raw_of(rTA, lenA, 1, j); rawB[j] = raw_of(rTB, lenB, 1, j); }

            for (int g = 0; g < G; ++g) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { sw_load_row<C>(rQ, row_off(lenA, g + 1, j, rawA[j]), SAn[j]); sw_load_row<C>(rQ, row_off(lenB, g + 1, j, rawB[j]), SBn[j]); }
#pragma unroll
                for (int j = 0; j < 4; ++j) { rawA[j] = raw_of(rTA, lenA, g + 2, j); rawB[j] = raw_of(rTB, lenB, g + 2, j); }
                const u32 bh[4] = {(u32)bq0.x, (u32)bq0.z, (u32)bq1.x, (u32)bq1.z}, bf[4] = {(u32)bq0.y, (u32)bq0.w, (u32)bq1.y, (u32)bq1.w};
                if (br) {
                    bq0 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 32 * (g + 1), 16);
                    bq1 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 32 * (g + 1) + 16, 16);
                }

                sw_for<0, 4>([&](auto J) {
                    constexpr int j = decltype(J)::value;
                    const int u = 4 * g + j;
                    // lane 0: the previous strip's pair of row u.  Rows up to lenA were written by that strip for BOTH targets (its steps
                    // come from lenA too); B's rows beyond lenB hold cells outside its matrix, which nothing inside depends on.  Beyond
                    // lenA, and in strip 0: (0, goe) -- H[i][0] = 0, F[i][1] = goe
                    const bool bin = br && u <= lenA;
                    const u32 left = (u32)sw_dpp_shr1((int)(bin ? bh[j] : 0u), (int)h[C - 1]);
                    u32 f = (u32)sw_dpp_shr1((int)(bin ? bf[j] : goe2), (int)fout);
                    u32 dprev = diag0;
                    diag0 = left;
                    sw_for<0, C / 2>([&](auto K) {
                        constexpr int k = 2 * decltype(K)::value;     // the cells k and k + 1 of both targets
                        u32 hn0, hn1;
                        gs16_cell2<k & 3>(hn0, hn1, dprev, h[k], e[k], e[k + 1], f, SA[j][k >> 2], SB[j][k >> 2], goe2, ge2);
                        dprev = h[k + 1];
                        h[k] = hn0;
                        h[k + 1] = hn1;
                    });
                    fout = f;
                    if (bw) __builtin_amdgcn_raw_buffer_store_b64(sw_v2i{(int)h[C - 1], (int)fout}, rB, lane == 63 ? 8 : (int)SW_OOB, 8 * u, 0);   // row u - 63 at pair index row + 64
                    // ---- arg-max: both row maxima against the wave's best of either target so far; only a step at which some half
                    // reaches its target's best looks for the cells (min(m, sbest - 1) differs from m in a half exactly where m >= sbest)
                    u32 m = h[0];
#pragma unroll
                    for (int k = 1; k < C; ++k) m = gs16_max(m, h[k]);
                    const u32 below = (u32)(sbestA - 1) | ((u32)(sbestB - 1) << 16);
                    if (__builtin_amdgcn_ballot_w64(gs16_min(m, below) != m) != 0) {
                        const int mA = (int)(m & 0xFFFFu), mB = (int)(m >> 16);     // (h >= 0 in both halves)
                        sbestA = max(sbestA, sw_wave_max(mA));
                        sbestB = max(sbestB, sw_wave_max(mB));
                        int kA = 0, kB = 0;                            // first column of my row that holds its maximum, per target
#pragma unroll
                        for (int k = C - 1; k >= 0; --k) {
                            kA = ((int)(h[k] & 0xFFFFu) == mA) ? k : kA;
                            kB = ((int)(h[k] >> 16) == mB) ? k : kB;
                        }
                        // strictly: an earlier row of this lane wins a tie.  (A step that only the partner's half called for changes
                        // nothing that counts: the first row at which a lane holds its target's final maximum is always such a step.)
                        lposA = mA > lbestA ? (u << 4 | kA) : lposA;
                        lposB = mB > lbestB ? (u << 4 | kB) : lposB;
                        lbestA = max(lbestA, mA);
                        lbestB = max(lbestB, mB);
                    }
                });
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int q = 0; q < NQ; ++q) { SA[j][q] = SAn[j][q]; SB[j][q] = SBn[j][q]; }
            }
            {   // each target with its own length: rows beyond it are not its matrix
                const int rA = (lposA >> 4) - lane, cA = c0 + (lposA & 15);
                if (lbestA > 0 && rA >= 1 && rA <= lenA && cA <= qlen) {
                    const u64 key = ((u64)(u32)lbestA << 40) | (SW_KEY_IDX_MASK - ((u64)rA * (u64)M + (u64)cA));
                    kbestA = key > kbestA ? key : kbestA;
                }
                const int rB = (lposB >> 4) - lane, cB = c0 + (lposB & 15);
                if (lbestB > 0 && rB >= 1 && rB <= lenB && cB <= qlen) {
                    const u64 key = ((u64)(u32)lbestB << 40) | (SW_KEY_IDX_MASK - ((u64)rB * (u64)M + (u64)cB));
                    kbestB = key > kbestB ? key : kbestB;
                }
            }
        }
        // either pair's arg-max: highest score, lowest linear index among equals
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const u32 alo = (u32)__shfl_xor((int)(u32)kbestA, off), ahi = (u32)__shfl_xor((int)(u32)(kbestA >> 32), off);
            const u32 blo = (u32)__shfl_xor((int)(u32)kbestB, off), bhi = (u32)__shfl_xor((int)(u32)(kbestB >> 32), off);
            const u64 oa = ((u64)ahi << 32) | alo, ob = ((u64)bhi << 32) | blo;
            kbestA = oa > kbestA ? oa : kbestA;
            kbestB = ob > kbestB ? ob : kbestB;
        }
