// sw_align_hits.hip -- the alignments of the hits of many queries, straight from a device hit table (sw_db_align_affine_hits, gfx950).
//
// The host of this call knows the queries and the handle's longest target, but not which targets the table names: it cannot size a slot
// by the longest hit as sw_align_affine_device does, and a slot for the handle's longest target would leave a few dozen waves at work.
// So the device sorts the work by size first, with no spinning and no allocator:
//   * sw_align_hits_bin<false> looks at every entry (q, r) of a group's rows: used (r < clamp(nhits[q], 0, top)), target inside
//     [0, ntargets) -- compared UNSIGNED before anything is loaded through it --, target not empty.  Every other entry gets its all-zero
//     sw_alignment here and becomes no item.  A used entry's direction matrix takes len x qpad bytes (qpad: its query's padded
//     length, the row stride); the kernel counts it into the smallest tier of the query's class that holds it (swp::plan_align_hits).
//   * sw_align_hits_bin<true>, a launch later, does the same look-up and writes the item into its list: the lists of a class lie back
//     to back in the class's part of the item buffer, tier after tier, each as long as the first launch counted.  The position inside a
//     list comes from an atomic and so differs from run to run -- it decides the ORDER in which independent items are taken, nothing an
//     item computes or where it writes: the outputs of two runs are the same bytes.
//   * sw_align_hits_wave<C>, one launch per (class, tier), largest tier first: every wave owns a slot of the tier's size and takes items
//     from the list's work counter.  The length of the list is read from device memory (the grid was planned on the host for the most
//     it could be); the waves of an empty list leave after that one load.
//
// The fill, the direction byte, the sc1 rule and the two-pass windowed walk are those of sw_align_affine_wave<C> (sw_align_affine.hip
// describes them, and the text there holds here word for word); the sweep below is a second copy.  What was per launch there is
// rebuilt per item here, from the item and the query's entry of the call's table: the profile descriptor (exactly 257 x qpad bytes
// at the query's offset), qlen, qpad -- the row stride of the direction matrix inside the slot -- and the strips, and the output index
// q * top + r.  They are loaded with vector loads and made scalars with readfirstlane.  All global writes are vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"
#include "sw_wave.h"

namespace swk {

namespace {

constexpr int AH_SC1 = 16;              // aux bit of the buffer builtins: sc1

constexpr int AH_WIN = 64;              // the walk's window: AH_WIN rows of AH_WIN direction bytes per wave

// The look-up both binning launches share: entry e of the group's rows -> its item and its (class, tier), or "zero alignment".
__device__ __forceinline__ bool ah_lookup(const AlignHitsBinParams& p, int64_t e, AlignHitItem& it, int& k, int& tier) {
    const int64_t t = e / p.top, r = e - t * p.top;
    const MultiQuery d = p.queries[t];
    it.out = d.row * p.top + r;
    it.entry = (int)t;
    it.start = 0; it.len = 0;
    int64_t used = p.top;
    if (p.nhits) { const int64_t n = p.nhits[d.row]; used = n < 0 ? 0 : (n < p.top ? n : p.top); }
    if (r >= used) return false;
    const u64 target = (u64)p.hits[it.out].target;
    if (target >= (u64)p.ntargets) return false;           // unsigned: a negative index is a huge one; nothing was loaded through it yet
    const int64_t start = p.offsets[target], len = p.offsets[target + 1] - start;
    if (len <= 0) return false;                            // an empty target: the zero alignment
    it.start = start; it.len = (int)len;
    k = t < p.cls_q0[1] ? 0 : (t < p.cls_q0[2] ? 1 : 2);
    const int64_t bytes = p.log_band[k] ? swp::align_ckpt_slot_bytes(len, d.qpad, 1ll << p.log_band[k]) : len * (int64_t)d.qpad;
    tier = 0;
    while (tier + 1 < p.ntiers[k] && bytes > p.bound[k][tier]) ++tier;   // (the top tier holds the worst case: the host has checked that)
    return true;
}

}  // namespace

// One thread per entry of the group's rows.  SCATTER = false counts the items of every list and writes the zero alignments;
// SCATTER = true, launched behind it, writes the items.  Plain global atomics (vector instructions).
template <bool SCATTER>
__global__ void __launch_bounds__(256) sw_align_hits_bin(AlignHitsBinParams p) {
    const int64_t total = p.nq * p.top;
    if constexpr (SCATTER) {   // the counts are final since the launch before: one thread reports how many lists of the group hold items
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            unsigned int n = 0;
            for (int k = 0; k < SW_AH_CLASSES; ++k)
                for (int t = 0; t < SW_AH_TIERS; ++t) n += p.ctl->count[k][t] != 0;
            atomicAdd(p.filled, n);
        }
    }
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        AlignHitItem it;
        int k = 0, tier = 0;
        const bool item = ah_lookup(p, e, it, k, tier);
        if constexpr (!SCATTER) {
            if (item) atomicAdd(&p.ctl->count[k][tier], 1u);
            else p.aln[it.out] = sw_alignment{0, 0, 0, 0, 0, 0, 0};
        } else if (item) {
            int64_t base = p.cls_q0[k] * p.top;            // the class's part of the list, then the lower tiers' items
            for (int t = 0; t < tier; ++t) base += p.ctl->count[k][t];
            p.items[base + atomicAdd(&p.ctl->cursor[k][tier], 1u)] = it;
        }
    }
}
template __global__ void sw_align_hits_bin<false>(AlignHitsBinParams);
template __global__ void sw_align_hits_bin<true>(AlignHitsBinParams);

// C: query columns per lane (4, 8, 16)
template <int C>
__global__ void __launch_bounds__(256) sw_align_hits_wave(AlignHitsParams p) {
    static_assert(C % 4 == 0 && C <= 16, "C is a multiple of 4");
    constexpr int NQ = C / 4;
    __shared__ sw_v4i win_all[4][AH_WIN * AH_WIN / 16];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t slot = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;     // resident wave: its own boundary column and direction matrix
    if (slot >= p.nslots) return;
    // this launch's list: behind the lists of the class's lower tiers, as long as the binning counted
    u32 first = 0;
    for (int t = 0; t < p.tier; ++t) first += p.counts[t];
    const u32 nitems = p.counts[p.tier];
    if (nitems == 0) return;
    const AlignHitItem* const items = p.items + first;
    const int ge = p.ge, goe = p.goe;
    // (a launch without a boundary workspace holds one-strip queries only: nothing goes through the empty descriptor)
    const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc((void*)(p.bnd ? p.bnd + slot * p.bnd_per : nullptr), 0,
                                                                        p.bnd ? (int)(p.bnd_per * 4) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rD = __builtin_amdgcn_make_buffer_rsrc((void*)(p.dir + slot * p.slot_bytes), 0, (int)p.slot_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc((void*)p.counter, 0, 4, 0x00020000);
    const u32 voffL0 = lane == 0 ? 0u : SW_OOB;    // lane 0 alone touches the counter and the result
    sw_v4i* const win = win_all[wave];
    const unsigned char* const winb = (const unsigned char*)win;
    const int ops_size = (int)(p.ops ? (p.ops_cap < 0x7FFFFF00ll ? p.ops_cap : 0x7FFFFF00ll) : 0);

    for (;;) {
        // the next item: a vector buffer atomic of lane 0, read back into a scalar (sw_search_wave says why)
        const u32 w = (u32)__builtin_amdgcn_readlane(__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(1, rC, (int)voffL0, 0, 0), 0);
        if (w >= nitems) break;
        // the item and its query: vector loads of wave-uniform addresses; readfirstlane tells the compiler that these are scalars
        const AlignHitItem it = items[w];
        const MultiQuery d = p.queries[sw_uniform(it.entry)];
        const int len = sw_uniform(it.len);
        const int64_t start = sw_uniform64(it.start), out = sw_uniform64(it.out);
        const int qlen = sw_uniform(d.qlen), nstrips = sw_uniform(d.nstrips);
        const int64_t M = qlen + 1;
        const u32 qpad = (u32)sw_uniform(d.qpad);          // the profile's row length and the row stride of the direction matrix
        const bool multi = nstrips > 1;
        const __amdgpu_buffer_rsrc_t rQ = __builtin_amdgcn_make_buffer_rsrc((void*)(p.prof + sw_uniform64(d.prof_off)), 0, (int)(SW_SEARCH_ROWS * qpad), 0x00020000);
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
            const bool bw = multi && st + 1 < nstrips, br = multi && st > 0;
            sw_v4i bq0 = {0, 0, 0, 0}, bq1 = {0, 0, 0, 0};
            const u32 voffB = lane == 0 ? 64u * 8u : SW_OOB;
            if (br) {   // (sc1 loads: served from L2, which this wave's own earlier stores have reached once vmcnt has drained)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                bq0 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 0, AH_SC1);
                bq1 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 16, AH_SC1);
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
                    bq0 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 32 * (g + 1), AH_SC1);
                    bq1 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 32 * (g + 1) + 16, AH_SC1);
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
        const __amdgpu_buffer_rsrc_t rO = __builtin_amdgcn_make_buffer_rsrc((void*)(p.ops ? p.ops + out * p.ops_cap : nullptr), 0, ops_size, 0x00020000);
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
                    wr0 = ai - (AH_WIN - 1);
                    wcb = ((aj - 1) & ~15) - (AH_WIN - 16);
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    sw_v4i v[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int row = wr0 + 16 * q + (lane >> 2), cb = wcb + 16 * (lane & 3);
                        const bool in = row >= 1 && row <= len && cb >= 0;
                        v[q] = __builtin_amdgcn_raw_buffer_load_b128(rD, in ? (int)((u32)(row - 1) * qpad + (u32)cb) : (int)SW_OOB, 0, AH_SC1);
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) win[(16 * q + (lane >> 2)) * (AH_WIN / 16) + (lane & 3)] = v[q];
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
                // lane l: the cell l steps back along the state's direction; `known`: outside the matrix (a fixed answer) or in the window
                const int r = state == 3 ? ai : ai - lane, c = state == 2 ? aj : aj - lane;
                const bool inside = r >= 1 && c >= 1, inwin = inside && r >= wr0 && c - 1 >= wcb;
                const bool known = !inside || inwin;
                const int b = inwin ? (int)winb[(r - wr0) * AH_WIN + (c - 1 - wcb)] : 0;
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
            const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc((void*)(p.aln + out), 0, (int)sizeof(sw_alignment), 0x00020000);
            const bool any = score != 0;
            const sw_v4i v0 = {(int)(u32)pos, (int)(u32)(pos >> 32), (int)(u32)score, 0};
            const sw_v4i v1 = {any ? j0 : 0, 0, any ? i0 : 0, 0};
            const sw_v4i v2 = {any ? j1 : 0, 0, any ? i1 : 0, 0};
            __builtin_amdgcn_raw_buffer_store_b128(v0, rA, (int)voffL0, 0, 0);                    // max_pos, max_score
            __builtin_amdgcn_raw_buffer_store_b128(v1, rA, (int)voffL0, 16, 0);                   // q_begin, t_begin
            __builtin_amdgcn_raw_buffer_store_b128(v2, rA, (int)voffL0, 32, 0);                   // q_end, t_end
            __builtin_amdgcn_raw_buffer_store_b64(sw_v2i{nops, 0}, rA, (int)voffL0, 48, 0);       // nops
        }
    }
}

template __global__ void sw_align_hits_wave<4>(AlignHitsParams);
template __global__ void sw_align_hits_wave<8>(AlignHitsParams);
template __global__ void sw_align_hits_wave<16>(AlignHitsParams);

}  // namespace swk
