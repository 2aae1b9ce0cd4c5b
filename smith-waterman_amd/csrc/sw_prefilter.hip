// sw_prefilter.hip -- the ungapped pre-filter of a many-query search (sw_db_prefilter_ungapped, gfx950): for every (query, target) pair
// the best score U of a gapless local alignment, D[i][j] = max(0, D[i-1][j-1] + s), U = max D (include/swhip.h), and the list of the
// pairs with U >= min_score -- the list sw_db_search_affine_pairs rescores.
//
// The mapping is that of sw_search_affine_multi_wave<C> (sw_search_multi.hip): persistent workgroups of four waves, a wave takes items
// from a work counter with the vector buffer atomic of lane 0; an item is (target rank, query of the launch), the longest targets first;
// the query comes as a MultiQuery of the call's table, its profile is the 257 x qpad byte profile of sw_search_profile_submat_multi,
// unchanged; lane l holds columns st * 64 C + l C + 1 .. + C of strip st.
//
// The sweep is simpler than Gotoh's, because a cell depends on its diagonal neighbour ONLY:
//   * No skew.  Nothing flows along a row, so every lane works on the SAME row at the same step: len steps for len rows (the Gotoh
//     sweep needs len + 63), and the target's letter is wave-uniform per step: the profile row's base is scalar arithmetic and goes
//     into the row load as its scalar offset (pf_load_row).
//   * No move.  A lane updates its columns from the highest down, d[k] = max(0, d[k-1] + s[k]), so d[k-1] still holds row i - 1 when
//     d[k] needs it.  The lowest column takes the left lane's highest one (read through DPP before that lane overwrites it; lane 0
//     takes the boundary value or 0).  Per cell: the add of the profile byte, max with 0, max into the lane's running best.
//   * The boundary column between strips carries ONE value per row: lane 63 stores its highest column of row i - 1 (before the
//     update of step i), lane 0 of the next strip reads it as the diagonal of row i.  A wave's boundary space holds two such columns
//     and the strips alternate between them, so a strip never writes the column it reads.
//   * Cells outside the matrix need no masking: rows beyond the target read the PAD row, columns beyond the query hold the profile's
//     -1, and a cell there derives from a cell of the matrix by strictly negative steps -- it stays below a value the best already holds.
//   * No arg-max: the best is a running maximum per lane and one wave maximum at the end of the item.
//
// sw_prefilter_wave16<C> runs TWO targets of the same query per wave on packed 16-bit lanes, in the manner of sw_batch_wave16: schedule
// rank 2r in the low halves, rank 2r + 1 in the high halves.  Same rows, same columns; the letters differ, so there are two byte loads
// and two profile-row loads per row and two SDWA adds per pair of cells (VOP3P has no SDWA), then one v_pk_max_i16 with 0 and one into the best: 4 VALU
// for two cells.  The shorter target's rows beyond its end read the PAD row; an odd last rank runs with an all-PAD partner whose result
// is dropped.  The planner sends a query here only where max(largest table entry, 0) x min(qlen, longest target) <= 32767; below,
// D >= 0 and an entry >= -128 keep the un-clamped sum inside int16.
//
// At the end of an item lane 0 stores the score (where a score table was asked for) and, where U >= min_score, takes a slot of the list
// with one vector atomic on the launch's 32-bit cursor: the slot is (pairs of the launches before) + cursor, and the pair is stored only
// where the slot lies below pairs_cap.  sw_prefilter_commit, one thread between two launches, folds the cursor into the 64-bit total.
// All global writes are vector stores or plain C++, all atomics vector atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"
#include "sw_wave.h"

namespace swk {

// Between the launches of a call (and before the first): the cursor of the launch that has ended joins the total, the work counter and
// the cursor start the next launch at zero, and the caller's count (where it has one) holds the total so far.
__global__ void sw_prefilter_commit(PrefilterCtl* ctl, int64_t* npairs, int first) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const long long total = first ? 0 : ctl->total + (long long)ctl->cursor;
    ctl->total = total;
    ctl->cursor = 0;
    ctl->work = 0;
    if (npairs) *npairs = total;
}

namespace {

// the end of an item: lane 0 stores the score and, for a passing pair, takes a slot and stores the pair where the slot is inside the list
__device__ __forceinline__ void pf_finish(const PrefilterParams& p, int score, int64_t row, int64_t idx, long long base, __amdgpu_buffer_rsrc_t rCur, u32 voffL0) {
    if (p.scores) {
        const __amdgpu_buffer_rsrc_t rS = __builtin_amdgcn_make_buffer_rsrc((void*)(p.scores + row * p.ntargets + idx), 0, 4, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b32(score, rS, (int)voffL0, 0, 0);
    }
    if (score >= p.min_score) {   // (wave-uniform)
        const u32 at = (u32)__builtin_amdgcn_readlane(__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(1, rCur, (int)voffL0, 0, 0), 0);
        const long long slot = base + (long long)at;
        if (slot < p.pairs_cap) {
            const __amdgpu_buffer_rsrc_t rP = __builtin_amdgcn_make_buffer_rsrc((void*)(p.pairs + slot), 0, (int)sizeof(sw_pair), 0x00020000);
            const sw_v4i v = {(int)(u32)(u64)row, (int)(u32)((u64)row >> 32), (int)(u32)(u64)idx, (int)(u32)((u64)idx >> 32)};
            __builtin_amdgcn_raw_buffer_store_b128(v, rP, (int)voffL0, 0, 0);
        }
    }
}

// the C profile bytes of one lane and row: the row's base is wave-uniform here (every lane works on the same row), so it travels as the
// load's scalar offset and costs no vector arithmetic; `col` is the lane's first column
template <int C>
__device__ __forceinline__ void pf_load_row(__amdgpu_buffer_rsrc_t r, u32 col, u32 rowbase, u32 (&s)[C / 4]) {
    if constexpr (C == 16) {
        const sw_v4i v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)col, (int)rowbase, 0);
        s[0] = (u32)v.x; s[1] = (u32)v.y; s[2] = (u32)v.z; s[3] = (u32)v.w;
    } else if constexpr (C == 8) {
        const sw_v2i v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)col, (int)rowbase, 0);
        s[0] = (u32)v.x; s[1] = (u32)v.y;
    } else {
        s[0] = __builtin_amdgcn_raw_buffer_load_b32(r, (int)col, (int)rowbase, 0);
    }
}

// two cells of both targets, columns k (byte BHI of the row dwords) and k - 1 (byte BLO), as ONE statement: t = d[k-1] + s, d[k] = max(t, 0),
// best = max(best, d[k]) in both halves.  An SDWA result is read one instruction after the one that follows it, as in sw_batch_wave16.
#define PF_CELL2(BHI, BLO)                                                                                                            \
    asm("v_add_u32_sdwa %0, %3, sext(%6) dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:" BHI "\n\t"                     \
        "v_add_u32_sdwa %1, %5, sext(%6) dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:" BLO "\n\t"                     \
        "v_add_u32_sdwa %0, %3, sext(%7) dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1 src1_sel:" BHI "\n\t"                \
        "v_add_u32_sdwa %1, %5, sext(%7) dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1 src1_sel:" BLO "\n\t"                \
        "v_pk_max_i16 %2, %0, 0\n\t"                                                                                                  \
        "v_pk_max_i16 %3, %1, 0\n\t"                                                                                                  \
        "v_pk_max_i16 %4, %4, %2\n\t"                                                                                                 \
        "v_pk_max_i16 %4, %4, %3"                                                                                                     \
        : "=&v"(tA), "=&v"(tB), "=&v"(dhi), "+v"(dlo), "+v"(best) : "v"(dprev), "v"(SA), "v"(SB))
// dhi: d[k] (out), dlo: d[k-1] (in: row i - 1, out: row i), dprev: d[k-2] of row i - 1 (or the diagonal of the lane's first column)
template <int J>
__device__ __forceinline__ void pf_cell2(u32& dhi, u32& dlo, u32 dprev, u32 SA, u32 SB, u32& best) {
    static_assert(J == 1 || J == 3, "the higher byte of a pair");
    u32 tA, tB;
    if constexpr (J == 3) PF_CELL2("BYTE_3", "BYTE_2");
    else PF_CELL2("BYTE_1", "BYTE_0");
}

}  // namespace

// C: query columns per lane (4, 8, 16); 32-bit lanes, one (target, query) item per wave
template <int C>
__global__ void __launch_bounds__(256) sw_prefilter_wave(PrefilterParams p) {
    static_assert(C % 4 == 0 && C <= 16, "C is a multiple of 4");
    constexpr int NQ = C / 4;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t slot = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;     // resident wave: its own boundary columns
    const int64_t half = p.bnd_per / 2;                                      // ints of one boundary column
    const u32 nq = p.nq;
    const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc((void*)&p.ctl->work, 0, 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rCur = __builtin_amdgcn_make_buffer_rsrc((void*)&p.ctl->cursor, 0, 4, 0x00020000);
    const long long base = p.ctl->total;           // (only sw_prefilter_commit writes it, between launches)
    const u32 voffL0 = lane == 0 ? 0u : SW_OOB;    // lane 0 alone touches the counters and the results

    for (;;) {
        // the next item: a vector buffer atomic of lane 0, read back into a scalar; no lane-divergent branch in this loop
        const u32 w = (u32)__builtin_amdgcn_readlane(__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(1, rC, (int)voffL0, 0, 0), 0);
        if ((int64_t)w >= p.nitems) break;
        const u32 rank = w / nq;
        const SearchItem it = p.items[p.rank0 + rank];
        const MultiQuery d = p.queries[w - rank * nq];
        const int len = sw_uniform((int)it.len);
        const int nstrips = sw_uniform(d.nstrips);
        const u32 qpad = (u32)sw_uniform(d.qpad);
        const __amdgpu_buffer_rsrc_t rQ = __builtin_amdgcn_make_buffer_rsrc((void*)(p.prof + sw_uniform64(d.prof_off)), 0, (int)(SW_SEARCH_ROWS * qpad), 0x00020000);
        // the target's bytes through a descriptor of exactly its extent; rows outside it are mapped to PAD below
        const __amdgpu_buffer_rsrc_t rT = __builtin_amdgcn_make_buffer_rsrc((void*)(p.db + sw_uniform64(it.start)), 0, len, 0x00020000);
        const int G = (len + 3) / 4;               // rows 1 .. 4 G in groups of four; those beyond len take the PAD row
        int best = 0;

        for (int st = 0; st < nstrips; ++st) {
            const u32 colb = (u32)(st * 64 * C + lane * C);
            int dd[C];
#pragma unroll
            for (int k = 0; k < C; ++k) dd[k] = 0;
            // boundary columns: strip st writes column st & 1 (lane 63, row i - 1 at int i - 1), strip st + 1 reads it (lane 0)
            const bool bw = st + 1 < nstrips, br = st > 0;
            int* const bcol = p.bnd ? p.bnd + slot * p.bnd_per : nullptr;
            const __amdgpu_buffer_rsrc_t rBw = __builtin_amdgcn_make_buffer_rsrc((void*)(bcol && bw ? bcol + (st & 1) * half : nullptr), 0, bcol && bw ? (int)(half * 4) : 0, 0x00020000);
            const __amdgpu_buffer_rsrc_t rBr = __builtin_amdgcn_make_buffer_rsrc((void*)(bcol && br ? bcol + ((st - 1) & 1) * half : nullptr), 0, bcol && br ? (int)(half * 4) : 0, 0x00020000);
            const u32 voffBr = lane == 0 ? 0u : SW_OOB, voffBw = lane == 63 ? 0u : SW_OOB;
            sw_v4i bq = {0, 0, 0, 0};
            if (br) {   // (sc1 loads: served from L2, which this wave's own earlier stores have reached once vmcnt has drained)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                bq = __builtin_amdgcn_raw_buffer_load_b128(rBr, (int)voffBr, 0, 16);
            }
            // row 4 g + j + 1 reads target byte 4 g + j, the same in every lane; beyond the target it takes the PAD row
            auto raw_of = [&](int g, int j) -> u32 {
                const u32 pos = (u32)(4 * g + j);
                return (u32)__builtin_amdgcn_raw_buffer_load_b8(rT, (int)(pos < (u32)len ? pos : SW_OOB), 0, 0);
            };
            auto row_base = [&](int g, int j, u32 raw) -> u32 {
                const u32 pos = (u32)(4 * g + j);
                return (pos < (u32)len ? (u32)sw_uniform((int)raw) : 256u) * qpad;
            };
            // software pipeline: the bytes of group g + 2 and the profile rows of group g + 1 are in flight while group g computes
            u32 raw[4], S[4][NQ], Sn[4][NQ];
#pragma unroll
            for (int j = 0; j < 4; ++j) raw[j] = raw_of(0, j);
#pragma unroll
            for (int j = 0; j < 4; ++j) pf_load_row<C>(rQ, colb, row_base(0, j, raw[j]), S[j]);
#pragma unroll
            for (int j = 0; j < 4; ++j) raw[j] = raw_of(1, j);

            for (int g = 0; g < G; ++g) {
#pragma unroll
                for (int j = 0; j < 4; ++j) pf_load_row<C>(rQ, colb, row_base(g + 1, j, raw[j]), Sn[j]);
#pragma unroll
                for (int j = 0; j < 4; ++j) raw[j] = raw_of(g + 2, j);
                const int bd[4] = {bq.x, bq.y, bq.z, bq.w};
                if (br) bq = __builtin_amdgcn_raw_buffer_load_b128(rBr, (int)voffBr, 16 * (g + 1), 16);

                sw_for<0, 4>([&](auto J) {
                    constexpr int j = decltype(J)::value;
                    // lane 63's highest column still holds row i - 1: the next strip's diagonal of row i
                    if (bw) __builtin_amdgcn_raw_buffer_store_b32(dd[C - 1], rBw, (int)voffBw, 4 * (4 * g + j), 0);
                    const int diag = sw_dpp_shr1(br ? bd[j] : 0, dd[C - 1]);
                    const int t0 = diag + sw_sbyte(S[j][0], 0);
                    sw_for<1, C>([&](auto K) {
                        constexpr int k = C - decltype(K)::value;     // C - 1 down to 1
                        dd[k] = max(dd[k - 1] + sw_sbyte(S[j][k >> 2], k & 3), 0);
                        best = max(best, dd[k]);
                    });
                    dd[0] = max(t0, 0);
                    best = max(best, dd[0]);
                });
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int q = 0; q < NQ; ++q) S[j][q] = Sn[j][q];
            }
        }
        pf_finish(p, sw_wave_max(best), sw_uniform64(d.row), sw_uniform64(it.idx), base, rCur, voffL0);
    }
}

template __global__ void sw_prefilter_wave<4>(PrefilterParams);
template __global__ void sw_prefilter_wave<8>(PrefilterParams);
template __global__ void sw_prefilter_wave<16>(PrefilterParams);

// C: query columns per lane (4, 8, 16); packed 16-bit lanes, the targets of ranks 2 r (low halves) and 2 r + 1 (high halves) per wave
template <int C>
__global__ void __launch_bounds__(256) sw_prefilter_wave16(PrefilterParams p) {
    static_assert(C % 4 == 0 && C <= 16, "C is a multiple of 4");
    constexpr int NQ = C / 4;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t slot = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    const int64_t half = p.bnd_per / 2;
    const u32 nq = p.nq;
    const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc((void*)&p.ctl->work, 0, 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rCur = __builtin_amdgcn_make_buffer_rsrc((void*)&p.ctl->cursor, 0, 4, 0x00020000);
    const long long base = p.ctl->total;
    const u32 voffL0 = lane == 0 ? 0u : SW_OOB;

    for (;;) {
        const u32 w = (u32)__builtin_amdgcn_readlane(__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(1, rC, (int)voffL0, 0, 0), 0);
        if ((int64_t)w >= p.nitems) break;
        const u32 pr = w / nq;                     // the pair of ranks 2 pr, 2 pr + 1 of the launch
        const int64_t ra = 2 * (int64_t)pr, rb = ra + 1 < p.nranks ? ra + 1 : ra;   // an odd last rank: no partner (its own item is loaded again, its length taken as 0)
        const bool partner = ra + 1 < p.nranks;
        const SearchItem ia = p.items[p.rank0 + ra], ib = p.items[p.rank0 + rb];
        const MultiQuery d = p.queries[w - pr * nq];
        const int lenA = sw_uniform((int)ia.len), lenB = partner ? sw_uniform((int)ib.len) : 0;   // lenA >= lenB: the schedule is sorted
        const int nstrips = sw_uniform(d.nstrips);
        const u32 qpad = (u32)sw_uniform(d.qpad);
        const __amdgpu_buffer_rsrc_t rQ = __builtin_amdgcn_make_buffer_rsrc((void*)(p.prof + sw_uniform64(d.prof_off)), 0, (int)(SW_SEARCH_ROWS * qpad), 0x00020000);
        const __amdgpu_buffer_rsrc_t rTA = __builtin_amdgcn_make_buffer_rsrc((void*)(p.db + sw_uniform64(ia.start)), 0, lenA, 0x00020000);
        const __amdgpu_buffer_rsrc_t rTB = __builtin_amdgcn_make_buffer_rsrc((void*)(p.db + sw_uniform64(ib.start)), 0, lenB, 0x00020000);
        const int G = (lenA + 3) / 4;
        u32 best = 0;                              // both halves

        for (int st = 0; st < nstrips; ++st) {
            const u32 colb = (u32)(st * 64 * C + lane * C);
            u32 dd[C];
#pragma unroll
            for (int k = 0; k < C; ++k) dd[k] = 0;
            const bool bw = st + 1 < nstrips, br = st > 0;
            int* const bcol = p.bnd ? p.bnd + slot * p.bnd_per : nullptr;
            const __amdgpu_buffer_rsrc_t rBw = __builtin_amdgcn_make_buffer_rsrc((void*)(bcol && bw ? bcol + (st & 1) * half : nullptr), 0, bcol && bw ? (int)(half * 4) : 0, 0x00020000);
            const __amdgpu_buffer_rsrc_t rBr = __builtin_amdgcn_make_buffer_rsrc((void*)(bcol && br ? bcol + ((st - 1) & 1) * half : nullptr), 0, bcol && br ? (int)(half * 4) : 0, 0x00020000);
            const u32 voffBr = lane == 0 ? 0u : SW_OOB, voffBw = lane == 63 ? 0u : SW_OOB;
            sw_v4i bq = {0, 0, 0, 0};
            if (br) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                bq = __builtin_amdgcn_raw_buffer_load_b128(rBr, (int)voffBr, 0, 16);
            }
            auto raw_of = [&](__amdgpu_buffer_rsrc_t rT, int len, int g, int j) -> u32 {
                const u32 pos = (u32)(4 * g + j);
                return (u32)__builtin_amdgcn_raw_buffer_load_b8(rT, (int)(pos < (u32)len ? pos : SW_OOB), 0, 0);
            };
            auto row_base = [&](int len, int g, int j, u32 raw) -> u32 {
                const u32 pos = (u32)(4 * g + j);
                return (pos < (u32)len ? (u32)sw_uniform((int)raw) : 256u) * qpad;
            };
            u32 rawA[4], rawB[4], SA[4][NQ], SB[4][NQ], SAn[4][NQ], SBn[4][NQ];
#pragma unroll
            for (int j = 0; j < 4; ++j) { rawA[j] = raw_of(rTA, lenA, 0, j); rawB[j] = raw_of(rTB, lenB, 0, j); }
#pragma unroll
            for (int j = 0; j < 4; ++j) { pf_load_row<C>(rQ, colb, row_base(lenA, 0, j, rawA[j]), SA[j]); pf_load_row<C>(rQ, colb, row_base(lenB, 0, j, rawB[j]), SB[j]); }
#pragma unroll
            for (int j = 0; j < 4; ++j) { rawA[j] = raw_of(rTA, lenA, 1, j); rawB[j] = raw_of(rTB, lenB, 1, j); }

            for (int g = 0; g < G; ++g) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { pf_load_row<C>(rQ, colb, row_base(lenA, g + 1, j, rawA[j]), SAn[j]); pf_load_row<C>(rQ, colb, row_base(lenB, g + 1, j, rawB[j]), SBn[j]); }
#pragma unroll
                for (int j = 0; j < 4; ++j) { rawA[j] = raw_of(rTA, lenA, g + 2, j); rawB[j] = raw_of(rTB, lenB, g + 2, j); }
                const int bd[4] = {bq.x, bq.y, bq.z, bq.w};
                if (br) bq = __builtin_amdgcn_raw_buffer_load_b128(rBr, (int)voffBr, 16 * (g + 1), 16);

                sw_for<0, 4>([&](auto J) {
                    constexpr int j = decltype(J)::value;
                    if (bw) __builtin_amdgcn_raw_buffer_store_b32((int)dd[C - 1], rBw, (int)voffBw, 4 * (4 * g + j), 0);
                    const u32 diag = (u32)sw_dpp_shr1(br ? bd[j] : 0, (int)dd[C - 1]);
                    sw_for<0, C / 2>([&](auto K) {
                        constexpr int k = C - 1 - 2 * decltype(K)::value;     // C - 1, C - 3, ..., 1: the cells k and k - 1
                        u32 dprev = diag;
                        if constexpr (k >= 2) dprev = dd[k - 2];
                        pf_cell2<k & 3>(dd[k], dd[k - 1], dprev, SA[j][k >> 2], SB[j][k >> 2], best);
                    });
                });
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int q = 0; q < NQ; ++q) { SA[j][q] = SAn[j][q]; SB[j][q] = SBn[j][q]; }
            }
        }
        const int scoreA = sw_wave_max((int)(best & 0xFFFFu)), scoreB = sw_wave_max((int)(best >> 16));
        const int64_t row = sw_uniform64(d.row);
        pf_finish(p, scoreA, row, sw_uniform64(ia.idx), base, rCur, voffL0);
        if (partner) pf_finish(p, scoreB, row, sw_uniform64(ib.idx), base, rCur, voffL0);
    }
}

template __global__ void sw_prefilter_wave16<4>(PrefilterParams);
template __global__ void sw_prefilter_wave16<8>(PrefilterParams);
template __global__ void sw_prefilter_wave16<16>(PrefilterParams);

}  // namespace swk
