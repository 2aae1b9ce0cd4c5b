// sw_align_ckpt.hip -- the alignment of hits in bounded memory, whatever their length (the calls accept 2^20 - 1 letters) (gfx950): sw_align_affine_wave's result, bit for bit, from
// a slot that holds one BAND of B rows of direction bytes and one small checkpoint per band instead of the whole direction matrix
// ("align_checkpoint", include/swhip.h).
//
// A hit of `len` rows is cut into bands of B rows (a power of two): band b covers rows bB + 1 .. min(bB + B, len).  The state of
// Gotoh's recurrence that crosses from row bB to row bB + 1 is, per column, H[bB][c] and E[bB + 1][c] (F starts anew in every row):
// checkpoint b - 1, 8 bytes per column.  A slot is  [ band: min(B, len) x qpad direction bytes | checkpoints: (ceil(len / B) - 1) x
// (qpad ints of H, qpad ints of E) ]  -- swp::align_ckpt_slot_bytes.
//
//   Pass 1, the sweep: band after band, strip after strip, the score-only body of sw_search_affine_wave (its mapping, pipelined loads,
//   boundary column and packed arg-max key hold here word for word).  A lane that has just finished row (b + 1) B of a band that is not
//   the hit's last stores its C values of h and of e (already advanced to the next row) into checkpoint b.  The boundary column between
//   two strips is a band's, not the hit's.
//   Pass 2, the bands the walk enters: the direction fill (sw_align_dirfill.inc defines the byte) into the slot's band, resumed from checkpoint b - 1
//   (h, e of the lane's columns; diag0 = H[bB][c0 - 1], the column left of the lane's first, from the same checkpoint row), for the
//   strips at or left of the walk's column only.
//   A hit of one band (len <= B) has no checkpoint and no sweep: its only band is filled at once, arg-max included, as today.
//
// Resuming.  In the whole-matrix kernels a lane that has not reached its first row reads the profile's PAD row, and (h, e) = (0, goe)
// is a fixed point of that row; a checkpoint state is not.  The first 64 steps of every band therefore run in a peeled loop that holds
// h, e and diag0 of the lanes whose band row is still <= 0 under a select (and keeps them out of the arg-max); the steady loop is the
// whole-matrix kernels' own.
//
// The walk is the text of sw_align_walk.inc, which the whole-matrix kernels run too: it clips a window to the rows the slot holds and
// takes a look-back into a row above them as "not known".  What this file adds is the walk's hook: when the cell the lanes look back
// from leaves the band in the slot, the wave re-fills the band above it and goes on.  The second pass of the walk re-fills the bands it
// needs again -- none when the alignment stayed inside one band.
//
// Visibility: only the wave that wrote a slot reads it; it drains vmcnt before the first read of a checkpoint row or of a band, and
// every such read is an sc1 buffer load (served from the L2: sw_align_walk.inc has the argument).  Offsets: every 32-bit offset lies
// within a band, a checkpoint area or a boundary column of one band; the target is addressed through a descriptor per band whose base
// is a 64-bit pointer.  All global writes are vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"
#include "sw_wave.h"

namespace swk {

namespace {

// C ints of a lane in a checkpoint row: C / 4 vector stores / sc1 loads of 16 bytes (16 / 32 / 64 bytes per lane)
template <int C>
__device__ __forceinline__ void ak_store_ints(__amdgpu_buffer_rsrc_t r, u32 off, const int (&v)[C]) {
#pragma unroll
    for (int q = 0; q < C / 4; ++q)
        __builtin_amdgcn_raw_buffer_store_b128(sw_v4i{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]}, r, (int)off, 16 * q, 0);
}
template <int C>
__device__ __forceinline__ void ak_load_ints(__amdgpu_buffer_rsrc_t r, u32 off, int (&v)[C]) {
#pragma unroll
    for (int q = 0; q < C / 4; ++q) {
        const sw_v4i x = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 16 * q, SW_SC1);
        v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
    }
}

// What a wave keeps over all its hits: its slot (band, checkpoints, boundary column), its LDS window and the scoring.
struct AkWave {
    int lane;
    sw_v4i* win;
    __amdgpu_buffer_rsrc_t rB;           // boundary column of a band
    unsigned char* slot; int64_t slot_bytes;   // per hit: min(B, len) x qpad direction bytes, then its checkpoint rows
    int B, logB;                         // band height
    int ge, goe;
    unsigned long long* stamps;
};
// One hit: the target, the query's profile and where the result goes (all wave-uniform).
struct AkHit {
    const unsigned char* target; int len;
    __amdgpu_buffer_rsrc_t rQ; u32 qpad; int qlen, nstrips;
    __amdgpu_buffer_rsrc_t rO; int64_t ops_cap; bool has_ops;   // the hit's own ops_cap bytes
    __amdgpu_buffer_rsrc_t rA;                                  // the hit's sw_alignment
};

// The wave routine: (target, query profile, slot, B) -> (sw_alignment, ops).
template <int C>
__device__ __forceinline__ void ak_align_hit(const AkWave& w, const AkHit& hit) {
    constexpr int NQ = C / 4;
    const int lane = w.lane, B = w.B, ge = w.ge, goe = w.goe;
    const int len = hit.len, qlen = hit.qlen, nstrips = hit.nstrips;
    const u32 qpad = hit.qpad;
    const int64_t M = qlen + 1;
    const bool multi = nstrips > 1;
    const int64_t band_want = (int64_t)(len < B ? len : B) * (int64_t)qpad;
    const int64_t band_bytes = band_want < w.slot_bytes ? band_want : w.slot_bytes;   // (the planner sized the slot for more: never beyond it)
    const __amdgpu_buffer_rsrc_t rB = w.rB, rQ = hit.rQ;
    // the walk's names for the hit's ops (sw_align_walk.inc).  References: copies made here move the instructions of all six kernels
    const __amdgpu_buffer_rsrc_t& rO = hit.rO;
    const int64_t& ops_cap = hit.ops_cap;
    const bool& has_ops = hit.has_ops;
    using walk_round_t = u64;
    const __amdgpu_buffer_rsrc_t rD = __builtin_amdgcn_make_buffer_rsrc((void*)w.slot, 0, (int)band_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rK = __builtin_amdgcn_make_buffer_rsrc((void*)(w.slot + band_bytes), 0, (int)(w.slot_bytes - band_bytes), 0x00020000);
    const int nbands = len > 0 ? (int)(((int64_t)len + B - 1) >> w.logB) : 1;
    const u32 voffL0 = lane == 0 ? 0u : SW_OOB;
    u64 kbest = 0;                         // per lane: best (score << 40 | MASK - index) over the bands and strips done
    int sbest = 1;                         // wave-uniform: highest H seen so far (at least 1: zeros never count)

    // Strip `st` of band `b`: rows b B + 1 .. b B + rows, resumed from checkpoint b - 1.  DIR: with direction bytes into the slot's band
    // (arg-max only if `amax`); otherwise score-only with the arg-max, and the checkpoint of the band's last row where one is due.
    auto unit = [&](auto DIR_, const int b, const int st, const bool amax) __attribute__((always_inline)) {
        constexpr bool DIR = decltype(DIR_)::value;
        const int64_t row0 = (int64_t)b << w.logB;
        const int rows = (int)((int64_t)len - row0 < (int64_t)B ? (int64_t)len - row0 : (int64_t)B);
        const __amdgpu_buffer_rsrc_t rT = __builtin_amdgcn_make_buffer_rsrc((void*)(hit.target + row0), 0, rows, 0x00020000);
        const int G = (rows + 64 + 3) / 4;     // steps 0 .. rows + 63 (lane 63's last row)
        const int c0 = st * 64 * C + lane * C + 1;
        const u32 colb = (u32)(c0 - 1);
        const bool ck_out = !DIR && row0 + B < (int64_t)len;          // the band's last row is a checkpoint row (rows == B)
        const u32 kout = (u32)b * 8u * qpad + colb * 4u;               // my columns' H in checkpoint b; their E lies 4 qpad bytes on
        int h[C], e[C];
        int diag0 = 0, fout = goe, lbest = 0, lk = 0, lstep = 0;
        const bool bw = multi && st + 1 < nstrips, br = multi && st > 0;
        if (b > 0 || br) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // my own checkpoint / boundary stores have reached the L2
        if (b > 0) {
            const u32 kin = (u32)(b - 1) * 8u * qpad + colb * 4u;
            ak_load_ints<C>(rK, kin, h);
            ak_load_ints<C>(rK, kin + 4u * qpad, e);
            diag0 = __builtin_amdgcn_raw_buffer_load_b32(rK, colb ? (int)(kin - 4u) : (int)SW_OOB, 0, SW_SC1);   // H[b B][c0 - 1]; column 0: 0
        } else {
#pragma unroll
            for (int k = 0; k < C; ++k) { h[k] = 0; e[k] = goe; }
        }
        sw_v4i bq0 = {0, 0, 0, 0}, bq1 = {0, 0, 0, 0};
        const u32 voffB = lane == 0 ? 64u * 8u : SW_OOB;
        if (br) {
            bq0 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 0, SW_SC1);
            bq1 = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)voffB, 16, SW_SC1);
        }
        auto raw_of = [&](int g, int j) -> u32 {
            const u32 pos = (u32)(4 * g + j - lane - 1);
            return (u32)__builtin_amdgcn_raw_buffer_load_b8(rT, (int)(pos < (u32)rows ? pos : SW_OOB), 0, 0);
        };
        auto row_off = [&](int g, int j, u32 raw) -> u32 {
            const u32 pos = (u32)(4 * g + j - lane - 1);
            return (pos < (u32)rows ? raw : 256u) * qpad + colb;
        };
        u32 raw[4], S[4][NQ], Sn[4][NQ];
#pragma unroll
        for (int j = 0; j < 4; ++j) raw[j] = raw_of(0, j);
#pragma unroll
        for (int j = 0; j < 4; ++j) sw_load_row<C>(rQ, row_off(0, j, raw[j]), S[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) raw[j] = raw_of(1, j);

        // four steps; HOLD: the peeled first 64 steps, where a lane whose band row u - lane is still <= 0 keeps its resumed state
        auto steps4 = [&](auto HOLD_, const int g) __attribute__((always_inline)) {
            constexpr bool HOLD = decltype(HOLD_)::value;
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
                const bool held = HOLD && u <= lane;
                const bool bin = br && u <= rows;
                const int left = sw_dpp_shr1(bin ? bh[j] : 0, h[C - 1]);
                int f = sw_dpp_shr1(bin ? bf[j] : goe, fout);
                int dprev = diag0;
                if constexpr (HOLD) diag0 = held ? diag0 : left; else diag0 = left;
                u32 dw[NQ];
#pragma unroll
                for (int q = 0; q < NQ; ++q) dw[q] = 0;
                sw_for<0, C>([&](auto K) {
                    constexpr int k = decltype(K)::value;
                    const int old = h[k];
                    const int t = dprev + sw_sbyte(S[j][k >> 2], k & 3);
                    const int ek = e[k];
                    const int hn = max(max(max(t, ek), f), 0);
                    const int x = hn + goe, eg = ek + ge, fg = f + ge;
                    if constexpr (DIR) {
                        u32 d = hn == ek ? 2u : 3u;            // the compare order of the canonical alignment: diagonal, E, F
                        d = hn == t ? 1u : d;
                        d = hn == 0 ? 0u : d;
                        d |= x >= eg ? 4u : 0u;                // opening wins a tie against extending
                        d |= x >= fg ? 8u : 0u;
                        dw[k >> 2] |= d << (8 * (k & 3));
                    }
                    const int en = max(eg, x);
                    f = max(fg, x);
                    if constexpr (HOLD) { e[k] = held ? ek : en; h[k] = held ? old : hn; }
                    else { e[k] = en; h[k] = hn; }
                    dprev = old;
                });
                fout = f;
                if (bw) __builtin_amdgcn_raw_buffer_store_b64(sw_v2i{h[C - 1], fout}, rB, lane == 63 ? 8 : (int)SW_OOB, 8 * u, 0);   // band row u - 63 at pair index row + 64
                if constexpr (DIR) {   // the direction bytes of band row u - lane, columns c0 .. c0 + C - 1
                    const u32 r1 = (u32)(u - lane - 1);
                    sw_store_row<C>(rD, r1 < (u32)rows ? r1 * qpad + colb : SW_OOB, dw);
                } else if constexpr (!HOLD) {   // (B >= 64: no checkpoint row within the peeled steps)
                    if (ck_out && u >= B) {     // the lane that has just finished row B of the band: h = H[row], e = E[row + 1]
                        const u32 off = u - lane == B ? kout : SW_OOB;
                        ak_store_ints<C>(rK, off, h);
                        ak_store_ints<C>(rK, off == SW_OOB ? SW_OOB : off + 4u * qpad, e);
                    }
                }
                // ---- arg-max: the row maximum against the wave's best so far; only a step that reaches it looks for the cell
                if (!DIR || amax) {
                    int m = h[0];
#pragma unroll
                    for (int k = 1; k + 1 < C; k += 2) m = max(max(m, h[k]), h[k + 1]);
                    m = max(m, h[C - 1]);
                    if constexpr (HOLD) m = held ? 0 : m;             // a resumed state is not a row of this band
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
                }
            });
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int q = 0; q < NQ; ++q) S[j][q] = Sn[j][q];
        };
        for (int g = 0; g < 16; ++g) steps4(std::true_type{}, g);          // steps 0 .. 63 (G >= 16; an empty hit has no step beyond them)
        for (int g = 16; g < G; ++g) steps4(std::false_type{}, g);
        if (!DIR || amax) {
            const int r = lstep - lane, c = c0 + lk;
            if (lbest > 0 && r >= 1 && r <= rows && c <= qlen) {
                const u64 key = ((u64)(u32)lbest << 40) | (SW_KEY_IDX_MASK - ((u64)(row0 + r) * (u64)M + (u64)c));
                kbest = key > kbest ? key : kbest;
            }
        }
    };

    const u64 tick0 = w.stamps ? wall_clock64() : 0;
    if (nbands == 1) {
        for (int st = 0; st < nstrips; ++st) unit(std::true_type{}, 0, st, true);
    } else {
        for (int b = 0; b < nbands; ++b)
            for (int st = 0; st < nstrips; ++st) unit(std::false_type{}, b, st, false);
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

    // ---- the walk: a window at a time from the band in the slot, read past the L1 (sc1) once this wave's stores have left it
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const u64 tick1 = w.stamps ? wall_clock64() : 0;
    u64 refill_ticks = 0;
    sw_v4i* const win = w.win;
    const unsigned char* const winb = (const unsigned char*)win;
    int cur = nbands == 1 ? 0 : -1;            // the band whose direction bytes the slot holds
    // The hook of the walk: when the cell the lanes look back from has left the band in the slot, fill its band, the strips up to its
    // column, and forget the window; then the first and the last row of the band in the slot (cur >= 0 whenever a cell is inside).
#define SW_WALK_BAND \
    if (ai >= 1 && aj >= 1) { \
        const int need = (ai - 1) >> w.logB; \
        if (need != cur) { \
            const u64 t0 = w.stamps ? wall_clock64() : 0; \
            const int last = (aj - 1) / (64 * C); \
            for (int st = 0; st <= last; ++st) unit(std::true_type{}, need, st, false); \
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); \
            cur = need; \
            wr0 = wcb = 1 << 30; \
            if (w.stamps) refill_ticks += wall_clock64() - t0; \
        } \
    } \
    const int bf = (cur << w.logB) + 1; \
    const int bl = (int)((int64_t)bf + B - 1 < (int64_t)len ? (int64_t)bf + B - 1 : (int64_t)len);
#define SW_WALK_ALN hit.rA
#include "sw_align_walk.inc"
#undef SW_WALK_BAND
#undef SW_WALK_ALN
    if (w.stamps) {   // timing aid ("debug_buf", three words here): ticks of the 100 MHz clock in the sweep, the walk and its re-fills
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const u64 tick2 = wall_clock64();
        if (lane == 0) {
            atomicAdd(w.stamps, tick1 - tick0);
            atomicAdd(w.stamps + 1, tick2 - tick1 - refill_ticks);
            atomicAdd(w.stamps + 2, refill_ticks);
        }
    }
}

}  // namespace

// C: query columns per lane (4, 8, 16); the hits of one query, from the host-built list of sw_align_affine_device
template <int C>
__global__ void __launch_bounds__(256) sw_align_ckpt_wave(AlignCkptParams p) {
    static_assert(C % 4 == 0 && C <= 16, "C is a multiple of 4");
    __shared__ sw_v4i win_all[4][SW_WIN * SW_WIN / 16];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t slot = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;     // resident wave: its own boundary column, band and checkpoints
    if (slot >= p.nslots) return;
    const int nstrips = (int)((p.qlen + 64 * C - 1) / (64 * C));
    AkWave w;
    w.lane = lane; w.win = win_all[wave];
    w.rB = __builtin_amdgcn_make_buffer_rsrc((void*)(nstrips > 1 ? p.bnd + slot * p.bnd_per : nullptr), 0, nstrips > 1 ? (int)(p.bnd_per * 4) : 0, 0x00020000);
    w.slot = p.dir + slot * p.slot_bytes; w.slot_bytes = p.slot_bytes;
    w.B = 1 << p.log_band; w.logB = p.log_band;
    w.ge = p.ge; w.goe = p.goe; w.stamps = p.stamps;
    const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc((void*)p.counter, 0, 4, 0x00020000);
    const u32 voffL0 = lane == 0 ? 0u : SW_OOB;    // lane 0 alone touches the counter
    const int ops_size = (int)(p.ops ? (p.ops_cap < 0x7FFFFF00ll ? p.ops_cap : 0x7FFFFF00ll) : 0);
    for (;;) {
        // the next hit: a vector buffer atomic of lane 0, read back into a scalar (sw_search_wave says why)
        const u32 n = (u32)__builtin_amdgcn_readlane(__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(1, rC, (int)voffL0, 0, 0), 0);
        if ((int64_t)n >= p.nitems) break;
        const SearchItem it = p.items[n];
        AkHit hit;
        hit.target = p.db + it.start; hit.len = (int)it.len;
        hit.rQ = __builtin_amdgcn_make_buffer_rsrc((void*)p.prof, 0, (int)(SW_SEARCH_ROWS * p.qpad), 0x00020000);
        hit.qpad = (u32)p.qpad; hit.qlen = (int)p.qlen; hit.nstrips = nstrips;
        hit.rO = __builtin_amdgcn_make_buffer_rsrc((void*)(p.ops ? p.ops + it.idx * p.ops_cap : nullptr), 0, ops_size, 0x00020000);
        hit.ops_cap = p.ops_cap; hit.has_ops = p.ops != nullptr;
        hit.rA = __builtin_amdgcn_make_buffer_rsrc((void*)(p.aln + it.idx), 0, (int)sizeof(sw_alignment), 0x00020000);
        ak_align_hit<C>(w, hit);
    }
}

// The items of a device hit table: the lists, the item format and the per-item look-up of sw_align_hits_wave<C> (sw_align_hits.hip).
template <int C>
__global__ void __launch_bounds__(256) sw_align_hits_ckpt_wave(AlignHitsCkptParams p) {
    static_assert(C % 4 == 0 && C <= 16, "C is a multiple of 4");
    __shared__ sw_v4i win_all[4][SW_WIN * SW_WIN / 16];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t slot = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    if (slot >= p.nslots) return;
    // this launch's list: behind the lists of the class's lower tiers, as long as the binning counted
    u32 first = 0;
    for (int t = 0; t < p.tier; ++t) first += p.counts[t];
    const u32 nitems = p.counts[p.tier];
    if (nitems == 0) return;
    const AlignHitItem* const items = p.items + first;
    AkWave w;
    w.lane = lane; w.win = win_all[wave];
    w.rB = __builtin_amdgcn_make_buffer_rsrc((void*)(p.bnd ? p.bnd + slot * p.bnd_per : nullptr), 0, p.bnd ? (int)(p.bnd_per * 4) : 0, 0x00020000);
    w.slot = p.dir + slot * p.slot_bytes; w.slot_bytes = p.slot_bytes;
    w.B = 1 << p.log_band; w.logB = p.log_band;
    w.ge = p.ge; w.goe = p.goe; w.stamps = nullptr;
    const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc((void*)p.counter, 0, 4, 0x00020000);
    const u32 voffL0 = lane == 0 ? 0u : SW_OOB;    // lane 0 alone touches the counter
    const int ops_size = (int)(p.ops ? (p.ops_cap < 0x7FFFFF00ll ? p.ops_cap : 0x7FFFFF00ll) : 0);
    for (;;) {
        const u32 n = (u32)__builtin_amdgcn_readlane(__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(1, rC, (int)voffL0, 0, 0), 0);
        if (n >= nitems) break;
        // the item and its query: vector loads of wave-uniform addresses; readfirstlane tells the compiler that these are scalars
        const AlignHitItem it = items[n];
        const MultiQuery d = p.queries[sw_uniform(it.entry)];
        const int64_t start = sw_uniform64(it.start), out = sw_uniform64(it.out);
        AkHit hit;
        hit.target = p.db + start; hit.len = sw_uniform(it.len);
        hit.qpad = (u32)sw_uniform(d.qpad); hit.qlen = sw_uniform(d.qlen); hit.nstrips = sw_uniform(d.nstrips);
        hit.rQ = __builtin_amdgcn_make_buffer_rsrc((void*)(p.prof + sw_uniform64(d.prof_off)), 0, (int)(SW_SEARCH_ROWS * hit.qpad), 0x00020000);
        hit.rO = __builtin_amdgcn_make_buffer_rsrc((void*)(p.ops ? p.ops + out * p.ops_cap : nullptr), 0, ops_size, 0x00020000);
        hit.ops_cap = p.ops_cap; hit.has_ops = p.ops != nullptr;
        hit.rA = __builtin_amdgcn_make_buffer_rsrc((void*)(p.aln + out), 0, (int)sizeof(sw_alignment), 0x00020000);
        ak_align_hit<C>(w, hit);
    }
}

template __global__ void sw_align_ckpt_wave<4>(AlignCkptParams);
template __global__ void sw_align_ckpt_wave<8>(AlignCkptParams);
template __global__ void sw_align_ckpt_wave<16>(AlignCkptParams);
template __global__ void sw_align_hits_ckpt_wave<4>(AlignHitsCkptParams);
template __global__ void sw_align_hits_ckpt_wave<8>(AlignHitsCkptParams);
template __global__ void sw_align_hits_ckpt_wave<16>(AlignHitsCkptParams);

}  // namespace swk
