// sw_msa_filter.hip -- the filter of a hit alignment (sw_msa_filter_device, gfx950): which rows of a query's top x qlen column rows
// (sw_db_msa_from_hits) are kept -- long enough, not nearly identical to the query, not nearly identical to a kept row of better rank.
// include/swhip.h states the rule; sw_msa_filter_host (sw_hits_host.cpp) is the same rule in plain C++.  The shape is that of
// non-maximum suppression: all pairs in parallel into a bit matrix, then one short sequential pass per query.  Integers only, no
// atomics; every word, every half-word of a plane and every output has one writer per launch.
//
// sw_msa_filter_pairs: one workgroup (4 waves) per (query, tile (rb, cb), cb <= rb) of swp::plan_msa_filter.  The rows 64 rb .. + 63
//   (block A) and 64 cb .. + 63 (block B) are staged in LDS 64 columns at a time: a thread packs four bytes it loads one by one -- rows
//   start at any byte -- into a dword; a column >= qlen or a row >= top gives '-', so the pad counts nowhere.  Lane l of EVERY wave
//   owns row 64 rb + l: its 16 dwords of the chunk in registers (read from LDS at an odd dword stride: no bank conflicts) and per dword
//   the mask of its letters, 0x80 in every byte that is not '-'.  Wave w compares with rows 64 cb + 16 w .. + 15 of block B, read as LDS
//   broadcasts (every lane the same address): per dword x = a ^ b, the exact zero-byte test ~(((x & 0x7f7f7f7f) + 0x7f7f7f7f) | x),
//   an and with the letter mask, and a population count that adds into the pair's counter -- 16 counters per lane, kept over the
//   chunks.  n_r is the population count of the masks.  Then bit i of the wave's 16 bits is 100 same >= max_ident_pct n_r (on the
//   diagonal only for r' < r), stored as one half-word of word r of plane cb.  Wave 0 of a diagonal tile also counts against the
//   query's letters and stores the row's own test (covered, and with letters not redundant to the query) into the last plane.
// sw_msa_filter_greedy: one workgroup per query, the row blocks in rank order.  Lane l of wave w ors (plane c word & kept[c]) over
//   the earlier blocks c = w, w + 4, ...: neighbouring lanes load neighbouring words, nothing depends on a load; the four partial
//   results meet in LDS.  Wave 0 then resolves the 64 x 64 dependency inside the block without memory: the lanes' diagonal words are
//   read lane by lane (readlane) against the mask of the rows kept so far, in 64 uniform steps.  At the end all threads write keep,
//   the filtered hit table (a thread reads an entry before it writes it: in place is allowed) and the count.
// Bounds: cols at (qoffs[q] - col0) x top + r x qlen + j with r < top, j < qlen; queries at qoffs[q] + j, j < qlen; the workspace at
// (q - q0) x query_words + c x 64 blocks + r with c <= blocks, r < 64 blocks; hits, hits_out, keep at q x top + r, r < top; nkept at q.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"
#include "sw_wave.h"

namespace swk {

namespace {
constexpr int kTile = (int)swp::kMsaFilterTile;          // rows of a block
constexpr int kCols = (int)swp::kMsaFilterChunkCols;     // columns staged at a time
constexpr int kDw = kCols / 4;                           // ... in dwords
constexpr int kStrideA = kDw + 1;                        // odd: lane l reads dword k of its own row at bank (17 l + k) % 32
constexpr unsigned kDashes = 0x2d2d2d2du, kLow7 = 0x7f7f7f7fu, kHigh = 0x80808080u;
static_assert(kTile == 64 && kCols == 64, "a lane per row, a thread per staged dword in four rounds");

// the bytes [col, col + 4) of row `row`, '-' where the row or the column does not exist
__device__ __forceinline__ unsigned sw_filter_load4(const unsigned char* rows, int64_t row, int64_t top, int col, int qlen) {
    if (row >= top) return kDashes;
    const unsigned char* p = rows + row * qlen;
    unsigned v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const unsigned c = col + b < qlen ? p[col + b] : (unsigned)'-';
        v |= c << (8 * b);
    }
    return v;
}

// 0x80 in every byte of x that is NOT zero (exact: the low seven bits cannot carry into the next byte)
__device__ __forceinline__ unsigned sw_filter_nonzero(unsigned x) { return (((x & kLow7) + kLow7) | x) & kHigh; }
}  // namespace

__global__ void __launch_bounds__(256, 4) sw_msa_filter_pairs(MsaFilterParams p) {
    __shared__ unsigned sA[kTile * kStrideA];
    __shared__ __attribute__((aligned(16))) unsigned sB[kTile * kDw];
    __shared__ unsigned sQ[kDw];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t plane = p.blocks * kTile;
    for (int64_t job = blockIdx.x; job < p.nq * p.tiles_per_query; job += gridDim.x) {
        const int64_t qi = job / p.tiles_per_query;
        int rb, cb;
        swp::msa_filter_tile(job - qi * p.tiles_per_query, rb, cb);
        const int64_t g0 = sw_uniform64(p.qoffs[p.q0 + qi]);     // (the same for every lane: the loops below are uniform)
        const int qlen = sw_uniform((int)(p.qoffs[p.q0 + qi + 1] - g0));
        const unsigned char* rows = p.cols + (g0 - p.col0) * p.top;
        const bool diag = rb == cb;
        const unsigned char* qs = diag && p.queries ? p.queries + g0 : nullptr;
        int same[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) same[i] = 0;
        int n = 0, sameq = 0;
        for (int c0 = 0; c0 < qlen; c0 += kCols) {
            __syncthreads();                                         // (the chunk before has been read)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int d = tid + 256 * i, row = d / kDw, k = d % kDw;
                sA[row * kStrideA + k] = sw_filter_load4(rows, (int64_t)rb * kTile + row, p.top, c0 + 4 * k, qlen);
                sB[row * kDw + k] = sw_filter_load4(rows, (int64_t)cb * kTile + row, p.top, c0 + 4 * k, qlen);
            }
            if (qs && tid < kDw) sQ[tid] = sw_filter_load4(qs, 0, 1, c0 + 4 * tid, qlen);
            __syncthreads();
            unsigned a[kDw], m[kDw];
#pragma unroll
            for (int k = 0; k < kDw; ++k) {
                a[k] = sA[lane * kStrideA + k];
                m[k] = sw_filter_nonzero(a[k] ^ kDashes);
                n += __popc(m[k]);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const unsigned* b = sB + (16 * wave + i) * kDw;
#pragma unroll
                for (int k = 0; k < kDw; ++k) same[i] += __popc(m[k] & ~sw_filter_nonzero(a[k] ^ b[k]));
                // two rows of block B in flight, not all sixteen (registers for more waves): the empty statement takes the two counters,
                // so their sums are done before it, and may touch memory, so no load crosses it
                if (i & 1) { asm volatile("" : "+v"(same[i - 1]), "+v"(same[i]) :: "memory"); __builtin_amdgcn_sched_barrier(0); }
            }
            if (qs && wave == 0) {
#pragma unroll
                for (int k = 0; k < kDw; ++k) sameq += __popc(m[k] & ~sw_filter_nonzero(a[k] ^ sQ[k]));
            }
        }
        const int64_t r = (int64_t)rb * kTile + lane;
        if (r < p.top) {
            unsigned bits = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int64_t rp = (int64_t)cb * kTile + 16 * wave + i;
                const bool red = rp < p.top && (!diag || rp < r) && 100 * same[i] >= p.max_ident_pct * n;
                bits |= (unsigned)red << i;
            }
            unsigned long long* wq = p.ws + qi * p.query_words;
            ((unsigned short*)(wq + cb * plane + r))[wave] = (unsigned short)bits;
            if (diag && wave == 0) {
                const bool own = n >= 1 && 100 * n >= p.min_cover_pct * qlen && (!p.queries || 100 * sameq < p.max_ident_pct * n);
                wq[p.blocks * plane + r] = own;
            }
        }
    }
}

__global__ void __launch_bounds__(256) sw_msa_filter_greedy(MsaFilterParams p) {
    __shared__ unsigned long long kept[kTile];                       // per row block the rows kept (SW_TOP_MAX / 64 blocks at most)
    __shared__ unsigned sup[4][kTile];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t plane = p.blocks * kTile;
    for (int64_t qi = blockIdx.x; qi < p.nq; qi += gridDim.x) {
        const unsigned long long* wq = p.ws + qi * p.query_words;
        __syncthreads();                                             // (the query before has been written out)
        for (int b = 0; b < (int)p.blocks; ++b) {
            const int64_t r = (int64_t)b * kTile + lane;
            unsigned s = 0;
            for (int c = wave; c < b; c += 4) s |= (wq[c * plane + r] & kept[c]) != 0;
            sup[wave][lane] = s;
            __syncthreads();
            if (wave == 0) {
                const bool alive = r < p.top && wq[p.blocks * plane + r] != 0 && !(sup[0][lane] | sup[1][lane] | sup[2][lane] | sup[3][lane]);
                const unsigned long long d = r < p.top ? wq[b * plane + r] : 0;
                const int dlo = (int)(unsigned)d, dhi = (int)(unsigned)(d >> 32);
                const unsigned long long cand = __ballot(alive);
                unsigned long long k = 0;
                for (int i = 0; i < kTile; ++i) {                    // (uniform: one row per step, the words from the lanes' registers)
                    if (!((cand >> i) & 1)) continue;
                    const unsigned long long di = (unsigned)__builtin_amdgcn_readlane(dlo, i) | ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(dhi, i) << 32);
                    if (!(di & k)) k |= 1ull << i;
                }
                if (lane == 0) kept[b] = k;
            }
            __syncthreads();
        }
        const int64_t e0 = (p.q0 + qi) * p.top;
        for (int64_t r = tid; r < p.top; r += 256) {
            const int k = (int)((kept[r >> 6] >> (r & 63)) & 1);
            if (p.keep) p.keep[e0 + r] = k;
            if (p.hits_out) {
                const sw_hit h = p.hits[e0 + r];
                p.hits_out[e0 + r] = sw_hit{k ? h.target : -1, h.max_pos, h.max_score};
            }
        }
        if (p.nkept && tid == 0) {
            int64_t total = 0;
            for (int b = 0; b < (int)p.blocks; ++b) total += __popcll(kept[b]);
            p.nkept[p.q0 + qi] = total;
        }
    }
}

}  // namespace swk
