// sw_mask.hip -- the low-complexity mask of a prepared database (sw_db_mask_low_complexity, gfx950).  include/swhip.h states the rule;
// sw_mask_low_complexity_host (sw_mask_host.cpp) is the same rule window by window.  The work is FLAT over the concatenated positions
// 0 .. letters - 1 in the tiles of swp::plan_mask: a run of low windows cannot cross a target's end (the last W - 1 starts of every
// target are invalid), so a position needs no target index.  Integers only; no global atomics; every word and byte has one writer per
// launch.  Bit p % 64 of word p / 64 of a bit array is position p: the neighbour "to the right" of a bit is the next HIGHER bit.
//
// sw_mask_windows: one workgroup per tile.  The tile's bytes and a halo of W - 1 behind them are staged in LDS as letter classes (0..31,
//   32 for a no-letter and for what lies beyond the last letter); bit 6 of a staged byte says "a target ends here", set from the device
//   offsets: one thread's binary search finds the first target that ends in the tile, the threads then take the following targets 256 at a time
//   (LDS ors; empty targets set nothing).  Lane l owns the starts 16 l .. 16 l + 15: it builds the counts of its first window and
//   slides, one letter out and one in, S moving by G[c] - G[c - 1] and G[c + 1] - G[c] from a 64-entry table in LDS; its 32 byte
//   counters lie in LDS at a stride of 9 dwords (odd: the 32 lanes of a half wave on 32 banks).  A start is valid while its window
//   holds no no-letter and no end flag among its first W - 1 bytes.  The lane's 16 low1 and 16 low2 bits are one half-word of each
//   array -- consecutive starts, so no ballot.  Wave 0 then reads the tile's 64 + 64 words back from LDS for the SUMMARY: bit 0 / 1 the
//   first / last position is low2, bit 2 / 3 the run that touches the left / right edge holds a low1 inside the tile, bit 4 the whole
//   tile is one run.
// sw_mask_carries: ONE workgroup of 1024 threads.  Summaries join associatively (sw_mask_join), so thread k joins its contiguous share
//   of the tiles, the shares' joins meet in LDS, where a scan in ten doubling steps gives every thread the join of what lies left and of
//   what lies right of its share (the join is not commutative: the left operand stays left), and two walks over the share
//   give every border the join of ALL tiles left of it and of ALL tiles right of it: the run that crosses the border is triggered iff
//   both sides touch it and either side's touching run holds a low1 -- however many whole-run tiles lie between.  carry bit 0 / 1: the
//   run across the tile's left / right border is triggered.
// sw_mask_apply: one workgroup per tile.  Wave 0, a lane per word, spreads the triggers through the runs (sw_mask_tile_starts): inside
//   a word low2 + low1 + carry ripples a trigger up to the end of its run, the bit-reversed words do the other direction; across the
//   words of the tile the same addition runs on the ballots of "generates a carry" and "passes a carry on", its carry-in the tile's
//   carry bit.  Wave 1 does the same for the tile BEFORE -- cheap, and it spares a launch: the dilation needs the last word of that
//   tile.  Dilation: masked = OR of the triggered starts shifted by 0 .. W - 1, at most one neighbouring word since W <= 64.  The mask
//   words go to the workspace (for the count) and all threads write the bytes: a head of up to 3 bytes up to the output's next dword
//   boundary, then a dword per lane, then a tail of up to 3 bytes -- offsets[0] may be odd; the input is read as dwords too where it
//   is misaligned by as much as the output, as four bytes per lane otherwise.
// sw_mask_count: thread per target, population counts of the mask words between its offsets; a target of more than
//   swp::kMaskCountLaneWords words is taken by its whole wave afterwards.  Every entry is written, 0 for an empty target.
// Bounds: in / out at base + p with p < letters only; the bit arrays at tile x 64 + w, w < 64, tile < tiles; summary and carry at tile;
// the staged bytes at j < kTile + 64, where a lane reads up to 16 l + 15 + W - 1 <= kTile + 62; offs at t + 1 <= ntargets.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"
#include "sw_mask_table.h"
#include "sw_wave.h"

namespace swk {

namespace {
constexpr int kTile = (int)swp::kMaskTile, kStarts = swp::kMaskStartsPerLane, kWords = (int)swp::kMaskTileWords;
constexpr int kStage = kTile + 64;                       // staged bytes: the tile and the longest halo, rounded up
constexpr int kCntStride = 9;                            // dwords between two lanes' counters (32 byte counters + 1 dword)
constexpr unsigned kNone = 32, kEnd = 0x40;              // class of a no-letter; flag "a target ends here"
constexpr int kCarryThreads = swp::kMaskCarryThreads;
constexpr unsigned kLrun = 1, kRrun = 2, kLtrig = 4, kRtrig = 8, kFull = 16, kEmpty = 32;   // a summary; kEmpty: the join of no tile
static_assert(kTile == 256 * kStarts && kStarts == 16 && kWords == 64, "a lane's bits are one half-word, a tile's words one wave");

__constant__ int kMaskG[SW_MASK_WINDOW_MAX + 1] = {SW_MASK_G_LITERALS};

// the summary of two neighbouring stretches of tiles, a left of b
__device__ __forceinline__ unsigned sw_mask_join(unsigned a, unsigned b) {
    if (a & kEmpty) return b;
    if (b & kEmpty) return a;
    const bool crossed = (a & kRrun) && (b & kLrun);
    const bool ltrig = (a & kLtrig) || ((a & kFull) && crossed && (b & kLtrig));
    const bool rtrig = (b & kRtrig) || ((b & kFull) && crossed && (a & kRtrig));
    return (a & kLrun) | (b & kRrun) | (ltrig ? kLtrig : 0) | (rtrig ? kRtrig : 0) | (a & b & kFull);
}

// is the run across a border triggered: x = bits 0 / 1 "touches the border" / "its touching run holds a low1" of everything left of it,
// r the summary of everything right of it
__device__ __forceinline__ unsigned sw_mask_border(unsigned x, unsigned r) {
    return (x & 1) && !(r & kEmpty) && (r & kLrun) && ((x & 2) || (r & kLtrig));
}

// The triggered starts of word `lane` of a tile: the low2 bits whose run holds a low1 anywhere.  Called by a whole wave.
__device__ __forceinline__ u64 sw_mask_tile_starts(const MaskParams& p, int64_t tile, int lane) {
    const u64 m = p.low2[tile * kWords + lane], s = p.low1[tile * kWords + lane];
    const unsigned c = p.carry[tile];
    // upwards: a carry enters at a trigger and ripples to the end of its run
    const u64 up = m + s;
    const u64 gu = __ballot(up < m), pu = __ballot(up == ~0ull);          // word generates a carry / passes one on (then s == 0, m full)
    const u64 cu = (((gu | pu) + gu + (c & 1)) ^ pu) >> lane & 1;         // the carry into this word (gu and pu are disjoint)
    const u64 fu = (((up + cu) ^ m) & m) | s;
    // downwards: the same on the reversed bits, the words in reversed order
    const u64 mr = __brevll(m), sr = __brevll(s), dn = mr + sr;
    const u64 gd = __brevll(__ballot(dn < mr)), pd = __brevll(__ballot(dn == ~0ull));
    const u64 cd = (((gd | pd) + gd + ((c >> 1) & 1)) ^ pd) >> (63 - lane) & 1;
    const u64 fd = __brevll((((dn + cd) ^ mr) & mr) | sr);
    return fu | fd;
}

// the bits of mask word w that lie in the positions [b, e), w between the words of b and e - 1
__device__ __forceinline__ int sw_mask_range_pop(const u64* mask, int64_t w, int64_t b, int64_t e) {
    u64 v = mask[w];
    if (w == (b >> 6)) v &= ~0ull << (b & 63);
    if (w == ((e - 1) >> 6) && (e & 63)) v &= (1ull << (e & 63)) - 1;
    return __popcll(v);
}
}  // namespace

__global__ void __launch_bounds__(256) sw_mask_windows(MaskParams p) {
    __shared__ unsigned sCls[kStage / 4];
    __shared__ unsigned sCnt[256 * kCntStride];
    __shared__ int sDelta[64];
    __shared__ unsigned char sMap[256];
    __shared__ u64 sBits[2][kWords];
    __shared__ int64_t sFirst;
    const int tid = (int)threadIdx.x, lane = tid & 63, W = p.window;
    if (tid < 64) sDelta[tid] = kMaskG[tid + 1] - kMaskG[tid];
    {
        unsigned c = kNone;
        for (int k = 0; k < p.nletters; ++k) c = p.letters_[k] == tid ? (unsigned)k : c;
        sMap[tid] = (unsigned char)c;
    }
    unsigned char* cb = (unsigned char*)sCls;
    unsigned char* cnt = (unsigned char*)(sCnt + tid * kCntStride);
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        __syncthreads();                                             // (the class map stands; the tile before has been read)
        const int64_t t0 = tile * kTile;
        const int stage = kTile + W - 1;
        for (int j = tid; j < kStage; j += 256) {
            const int64_t pos = t0 + j;
            cb[j] = j < stage && pos < p.letters ? sMap[p.in[p.base + pos]] : (unsigned char)kNone;
        }
#pragma unroll
        for (int i = 0; i < kCntStride; ++i) sCnt[tid * kCntStride + i] = 0;
        if (tid == 255) {   // ONE thread (of the wave with the least to stage) finds the first target whose last letter lies at or behind t0
            int64_t lo = 0, hi = p.ntargets;
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (p.offs[mid + 1] > p.base + t0) hi = mid; else lo = mid + 1;
            }
            sFirst = lo;
        }
        __syncthreads();
        {   // the end flags: the targets from that one on while they end in the stage
            for (int64_t t = sFirst + tid; t < p.ntargets; t += 256) {
                const int64_t end = p.offs[t + 1], e = end - 1 - p.base - t0;     // e >= 0 from the search
                if (e >= stage) break;
                if (end > p.offs[t]) atomicOr(&sCls[e >> 2], kEnd << (8 * (e & 3)));
            }
        }
        __syncthreads();
        const int j0 = tid * kStarts;
        int S = 0, bad = 0, ends = 0;
        for (int x = 0; x < W; ++x) {
            const unsigned b = cb[j0 + x], c = b & 63;
            if (x < W - 1) ends += (int)(b >> 6) & 1;
            if (c < kNone) { const unsigned n = cnt[c]; S += sDelta[n]; cnt[c] = (unsigned char)(n + 1); } else ++bad;
        }
        unsigned b1 = 0, b2 = 0;
        for (int r = 0; r < kStarts; ++r) {
            if (r) {                                                 // from start j0 + r - 1 to start j0 + r
                const unsigned o = cb[j0 + r - 1], co = o & 63;
                ends -= (int)(o >> 6) & 1;
                if (co < kNone) { const unsigned n = cnt[co] - 1u; cnt[co] = (unsigned char)n; S -= sDelta[n]; } else --bad;
                ends += (int)(cb[j0 + r + W - 2] >> 6) & 1;
                const unsigned c = cb[j0 + r + W - 1] & 63;
                if (c < kNone) { const unsigned n = cnt[c]; S += sDelta[n]; cnt[c] = (unsigned char)(n + 1); } else ++bad;
            }
            const bool valid = bad == 0 && ends == 0;
            const int D = p.gw - S;
            b1 |= (unsigned)(valid && D <= p.bound1) << r;
            b2 |= (unsigned)(valid && D <= p.bound2) << r;
        }
        ((unsigned short*)p.low1)[(t0 >> 4) + tid] = (unsigned short)b1;
        ((unsigned short*)p.low2)[(t0 >> 4) + tid] = (unsigned short)b2;
        ((unsigned short*)sBits[0])[tid] = (unsigned short)b1;
        ((unsigned short*)sBits[1])[tid] = (unsigned short)b2;
        __syncthreads();
        if (tid < 64) {                                              // wave 0: the summary
            const u64 s = sBits[0][lane], m = sBits[1][lane];
            const u64 open = __ballot(m != ~0ull);                   // the words that are not one run
            const int kl = open ? __builtin_ctzll(open) : 64, kr = open ? 63 - __builtin_clzll(open) : -1;
            const int ones_lo = m == ~0ull ? 64 : __builtin_ctzll(~m), ones_hi = m == ~0ull ? 64 : __builtin_clzll(~m);
            const u64 mask_lo = ones_lo >= 64 ? ~0ull : (1ull << ones_lo) - 1;
            const u64 mask_hi = ones_hi >= 64 ? ~0ull : ones_hi == 0 ? 0 : ~0ull << (64 - ones_hi);
            const bool tl = lane < kl ? s != 0 : lane == kl && (s & mask_lo) != 0;
            const bool tr = lane > kr ? s != 0 : lane == kr && (s & mask_hi) != 0;
            const u64 anyl = __ballot(tl), anyr = __ballot(tr);
            const u64 first = __ballot(m & 1), last = __ballot(m >> 63);
            if (lane == 0)
                p.summary[tile] = ((first & 1) ? kLrun : 0) | ((last >> 63) ? kRrun : 0) | (anyl ? kLtrig : 0) | (anyr ? kRtrig : 0) | (open ? 0 : kFull);
        }
    }
}

__global__ void __launch_bounds__(kCarryThreads) sw_mask_carries(MaskParams p) {
    __shared__ unsigned sPre[kCarryThreads], sSuf[kCarryThreads];
    const int tid = (int)threadIdx.x;
    const int64_t per = (p.tiles + kCarryThreads - 1) / kCarryThreads;
    const int64_t first = std::min<int64_t>(p.tiles, tid * per), last = std::min<int64_t>(p.tiles, first + per);
    unsigned own = kEmpty;
    for (int64_t i = first; i < last; ++i) own = sw_mask_join(own, p.summary[i]);
    sPre[tid] = sSuf[tid] = own;
    __syncthreads();
    for (int d = 1; d < kCarryThreads; d <<= 1) {                    // both scans at once: the shares tid - 2d + 1 .. tid and tid .. tid + 2d - 1
        const unsigned a = tid >= d ? sw_mask_join(sPre[tid - d], sPre[tid]) : sPre[tid];
        const unsigned b = tid + d < kCarryThreads ? sw_mask_join(sSuf[tid], sSuf[tid + d]) : sSuf[tid];
        __syncthreads();
        sPre[tid] = a; sSuf[tid] = b;
        __syncthreads();
    }
    unsigned left = tid ? sPre[tid - 1] : kEmpty, right = tid + 1 < kCarryThreads ? sSuf[tid + 1] : kEmpty;   // everything left / right of the share
    // forwards: what lies left of every tile's left border, kept in the carry word for the walk back
    for (int64_t i = first; i < last; ++i) {
        p.carry[i] = left & kEmpty ? 0 : ((left & kRrun) ? 1 : 0) | ((left & kRtrig) ? 2 : 0);
        left = sw_mask_join(left, p.summary[i]);
    }
    unsigned xnext = left & kEmpty ? 0 : ((left & kRrun) ? 1 : 0) | ((left & kRtrig) ? 2 : 0);   // ... of the border behind the share
    for (int64_t i = last - 1; i >= first; --i) {
        const unsigned tr = sw_mask_border(xnext, right);
        right = sw_mask_join(p.summary[i], right);
        xnext = p.carry[i];
        p.carry[i] = sw_mask_border(xnext, right) | (tr << 1);
    }
}

__global__ void __launch_bounds__(256) sw_mask_apply(MaskParams p) {
    __shared__ u64 sStarts[kWords + 1];                              // [0]: the last word of the tile before
    __shared__ u64 sMask[kWords];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, W = p.window;
    const unsigned mb4 = p.mask_byte * 0x01010101u;
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        __syncthreads();                                             // (the tile before has been written out)
        if (wave == 0) sStarts[1 + lane] = sw_mask_tile_starts(p, tile, lane);
        else if (wave == 1) {
            const u64 v = tile > 0 ? sw_mask_tile_starts(p, tile - 1, lane) : 0;
            if (lane == 63) sStarts[0] = v;
        }
        __syncthreads();
        if (tid < kWords) {
            const u64 cur = sStarts[1 + tid], prev = sStarts[tid];
            u64 m = cur;
            for (int k = 1; k < W; ++k) m |= (cur << k) | (prev >> (64 - k));
            sMask[tid] = m;
            p.mask[tile * kWords + tid] = m;
        }
        __syncthreads();
        const int64_t t0 = tile * kTile;
        const int n = (int)std::min<int64_t>(kTile, p.letters - t0);
        const unsigned char* src = p.in + p.base + t0;
        unsigned char* dst = p.out + p.base + t0;
        // a head of up to 3 bytes brings the STORES to a dword boundary, then whole dwords, then a tail of up to 3 bytes; the loads are
        // dwords too where the input is misaligned by as much as the output, four bytes otherwise (uniform: a tile is a multiple of 4 long)
        const int head = std::min(n, (int)((4 - ((uintptr_t)dst & 3)) & 3)), nd = (n - head) >> 2;
        const bool same = (((uintptr_t)src ^ (uintptr_t)dst) & 3) == 0;
        for (int d = tid; d < nd; d += 256) {
            const int q = head + 4 * d;
            const unsigned v = same ? *(const unsigned*)(src + q)
                                    : (unsigned)src[q] | (unsigned)src[q + 1] << 8 | (unsigned)src[q + 2] << 16 | (unsigned)src[q + 3] << 24;
            u64 w = sMask[q >> 6] >> (q & 63);
            if ((q & 63) > 60) w |= sMask[(q >> 6) + 1] << (64 - (q & 63));          // (q + 3 < n lies in that word: it exists)
            const unsigned bits = (unsigned)w & 15;
            const unsigned bm = ((bits * 0x00204081u) & 0x01010101u) * 0xffu;        // 0xff in byte k where bit k is set
            *(unsigned*)(dst + q) = (v & ~bm) | (mb4 & bm);
        }
        if (tid < n - 4 * nd) {                                                      // head and tail: at most 6 bytes
            const int j = tid < head ? tid : 4 * nd + tid;
            dst[j] = (sMask[j >> 6] >> (j & 63)) & 1 ? (unsigned char)p.mask_byte : src[j];
        }
    }
}

__global__ void __launch_bounds__(256) sw_mask_count(MaskParams p) {
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int64_t groups = (p.ntargets + swp::kMaskCountTargets - 1) / swp::kMaskCountTargets;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t t = g * swp::kMaskCountTargets + tid;
        const bool have = t < p.ntargets;
        const int64_t b = have ? p.offs[t] - p.base : 0, e = have ? p.offs[t + 1] - p.base : 0;
        const bool some = e > b;
        const int64_t wb = b >> 6, we = some ? (e - 1) >> 6 : wb;
        const bool wide = some && we - wb >= swp::kMaskCountLaneWords;
        int n = 0;
        if (some && !wide)
            for (int64_t w = wb; w <= we; ++w) n += sw_mask_range_pop(p.mask, w, b, e);
        for (u64 todo = __ballot(wide); todo; todo &= todo - 1) {    // (uniform: one long target per step, the whole wave on it)
            const int l = __builtin_ctzll(todo);
            const int64_t bb = __shfl(b, l), ee = __shfl(e, l);
            int part = 0;
            for (int64_t w = (bb >> 6) + lane; w <= ((ee - 1) >> 6); w += 64) part += sw_mask_range_pop(p.mask, w, bb, ee);
            for (int o = 32; o; o >>= 1) part += __shfl_xor(part, o);
            if (lane == l) n = part;
        }
        if (have) p.nmasked[t] = n;
    }
}

}  // namespace swk
