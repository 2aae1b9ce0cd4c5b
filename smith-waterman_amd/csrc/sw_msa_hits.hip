// sw_msa_hits.hip -- the query-anchored multiple alignment of aligned hits (sw_db_msa_from_hits, gfx950): the column rows and the A3M
// rows of the entries of a hit table, from the tables sw_db_align_affine_hits / sw_db_align_pssm_hits leave on the device.
// include/swhip.h states the rule (used entries, the walk, valid inserts, the two layouts); sw_msa_from_hits_host (sw_hits_host.cpp) is
// the same rule in plain C++.  Used entries and the walk come from sw_pssm_walk.h: the ops 64 at a time, one op per lane, the lane's
// (j, i) and the inserts before it from three ballots and mbcnt.  No floats, no atomics; every byte has one writer per launch.
//
// sw_msa_cols (launch A): one workgroup (4 waves) per (query, slice of `slice_entries` entries), the waves take the slice's entries
//   round robin -- ALL entries r < top, used or not.  A wave first sets the entry's column row to '-': the bytes up to the first
//   dword boundary by one lane each, whole dwords (0x2d2d2d2d) strided over the lanes, the last bytes by one lane each.  For a used
//   entry it then waits for those stores (s_waitcnt vmcnt(0): a store leaves the counter when the wave's own L2 has it -- the pair stores
//   below go to the same bytes from other lanes, through the same L2; no release fence, nobody else reads the row in this launch) and walks: an 'M' lane that pairs stores t[i] at byte j.  The popcounts of the walk's ballots give nmatch, nident and
//   ninsert; lane 0 stores {0, len, nmatch, nident, ninsert}.
// sw_msa_scan_chunks, sw_msa_scan_top (launch B, two levels): a workgroup scans a chunk of 256 `len`s in LDS (Hillis-Steele: 8 steps),
//   stores every entry's exclusive prefix WITHIN its chunk into `off` and the chunk's sum into the workspace; then ONE workgroup scans
//   the chunks' sums 256 at a time with a running carry, leaves every chunk's offset in their place and the total in *d_a3m_bytes.
//   No atomics, no workgroup waits for another: the levels are separate launches.
// sw_msa_rows (launch C): one wave per entry.  off = the entry's prefix + its chunk's offset, stored by lane 0.  A used entry whose row
//   lies inside the cap: '-' for the columns in front of q_begin; the walk -- a lane whose op consumes a column stores t[i] or '-' at
//   off + j + k, a valid insert stores its byte (A-Z: + 32) at off + j + k, k the inserts before the op --; '-' for the columns from
//   the walk's end on, at off + j + ninsert.  Every byte of the row is written once.
// Bounds: hits, nhits, aln, rows at q * top + r with r < top; ops at (q * top + r) * ops_cap + [0, nops), nops <= ops_cap; the database
// at offsets[t] + i with t < ntargets, i < len; the queries at qoffs[q] + j, j < qlen; cols at (qoffs[q] - col0) * top + r * qlen +
// [0, qlen); a3m at off + [0, len) only where off + len <= a3m_cap, and there j + k < qlen + ninsert = len for every store (k counts
// inserts BEFORE the op; a column store has j < qlen, an insert j <= qlen and k < ninsert); the workspace at e / 256 < chunks.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"
#include "sw_wave.h"
#include "sw_pssm_walk.h"

namespace swk {

namespace {
constexpr int kChunk = (int)swp::kMsaScanChunk;
static_assert(kChunk == 256, "a scan chunk is one entry per thread of a workgroup");

// n bytes '-' from p on, by one wave: whole dwords where p's alignment allows
__device__ __forceinline__ void sw_msa_dashes(unsigned char* p, int n, int lane) {
    const int head = min(n, (int)(-(uintptr_t)p & 3));
    if (lane < head) p[lane] = '-';
    const int ndw = (n - head) >> 2, tail = (n - head) & 3;
    unsigned int* d = (unsigned int*)(p + head);
    for (int k = lane; k < ndw; k += 64) d[k] = 0x2d2d2d2du;
    if (lane < tail) p[head + 4 * ndw + lane] = '-';
}

// The exclusive scan of one value per thread over the 256 threads of the workgroup, in LDS; leaves the sum of all in `total`.
template <typename T>
__device__ __forceinline__ T sw_msa_scan256(T v, T* s, int tid, T& total) {
    s[tid] = v;
    __syncthreads();
    for (int d = 1; d < kChunk; d <<= 1) {
        const T x = tid >= d ? s[tid - d] : (T)0;
        __syncthreads();
        s[tid] += x;
        __syncthreads();
    }
    const T incl = s[tid];
    total = s[kChunk - 1];
    __syncthreads();                                                 // (s may be written again)
    return incl - v;
}
}  // namespace

__global__ void __launch_bounds__(256) sw_msa_cols(MsaHitsParams p) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const HitTables& t = p.t;
    for (int64_t job = blockIdx.x; job < t.nqueries * p.slices_per_query; job += gridDim.x) {
        const int64_t q = job / p.slices_per_query, r0 = (job % p.slices_per_query) * p.slice_entries;
        const int64_t g0 = t.qoffs[q];
        const int qlen = (int)(t.qoffs[q + 1] - g0);
        const int64_t nh = sw_pssm_query_hits(t, q);
        const unsigned char* qs = p.queries ? p.queries + g0 : nullptr;
        const int64_t r1 = min(t.top, r0 + p.slice_entries);
        for (int64_t r = r0 + wave; r < r1; r += 4) {
            const int64_t e = q * t.top + r;
            unsigned char* row = p.cols ? p.cols + (g0 - p.col0) * t.top + r * qlen : nullptr;
            if (row) sw_msa_dashes(row, qlen, lane);
            sw_alignment a;
            int64_t toff = 0, len64 = 0;
            int nmatch = 0, nident = 0, nins = 0;
            const bool used = r < nh && sw_pssm_entry_used(t, e, qlen, a, toff, len64);
            if (used) {
                if (row) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the dashes have reached the L2 before a pair overwrites one
                const unsigned char* tb = t.db + toff;
                int j_end;
                sw_msa_walk(sw_pssm_entry_ops(t, e), a, qlen, (int)len64, lane, j_end, nins, [&](bool pair, bool, bool, int j, int i, int) {
                    bool same = false;
                    if (pair) {
                        const unsigned char c = tb[i];
                        if (row) row[j] = c;
                        same = qs && qs[j] == c;
                    }
                    nmatch += __popcll(__ballot(pair));
                    nident += __popcll(__ballot(same));
                });
            }
            if (p.rows && lane == 0) p.rows[e] = sw_msa_row{0, used ? qlen + nins : 0, nmatch, nident, nins};
        }
    }
}

__global__ void __launch_bounds__(256) sw_msa_scan_chunks(MsaHitsParams p) {
    __shared__ int s[kChunk];
    const int tid = (int)threadIdx.x;
    for (int64_t c = blockIdx.x; c < p.chunks; c += gridDim.x) {
        const int64_t e = c * kChunk + tid;
        const int v = e < p.entries ? p.rows[e].len : 0;             // (256 rows of less than 2^21 bytes: the sum fits 32 bits)
        int total;
        const int before = sw_msa_scan256(v, s, tid, total);
        if (e < p.entries) p.rows[e].off = before;
        if (tid == 0) p.chunk_off[c] = total;
    }
}

__global__ void __launch_bounds__(256) sw_msa_scan_top(MsaHitsParams p) {
    __shared__ int64_t s[kChunk];
    const int tid = (int)threadIdx.x;
    int64_t carry = 0;
    for (int64_t c0 = 0; c0 < p.chunks; c0 += kChunk) {
        const int64_t c = c0 + tid;
        const int64_t v = c < p.chunks ? p.chunk_off[c] : 0;
        int64_t total;
        const int64_t before = sw_msa_scan256(v, s, tid, total);
        if (c < p.chunks) p.chunk_off[c] = carry + before;
        carry += total;
    }
    if (tid == 0 && p.a3m_bytes) *p.a3m_bytes = carry;
}

__global__ void __launch_bounds__(256) sw_msa_rows(MsaHitsParams p) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t e = (int64_t)blockIdx.x * 4 + wave; e < p.entries; e += (int64_t)gridDim.x * 4) {
        const sw_msa_row mine = p.rows[e];
        const int64_t off = mine.off + p.chunk_off[e / kChunk];
        if (lane == 0) p.rows[e].off = off;
        if (!p.a3m || mine.len <= 0 || off + mine.len > p.a3m_cap) continue;
        const HitTables& t = p.t;
        const int64_t q = e / t.top, r = e - q * t.top;
        const int qlen = (int)(t.qoffs[q + 1] - t.qoffs[q]);
        sw_alignment a;
        int64_t toff = 0, len64 = 0;
        if (r >= sw_pssm_query_hits(t, q) || !sw_pssm_entry_used(t, e, qlen, a, toff, len64)) continue;
        if (mine.len != qlen + mine.ninsert) continue;               // (launch A's row of these same tables: never)
        unsigned char* out = p.a3m + off;
        const unsigned char* tb = t.db + toff;
        sw_msa_dashes(out, (int)a.q_begin, lane);
        int j_end, nins;
        sw_msa_walk(sw_pssm_entry_ops(t, e), a, qlen, (int)len64, lane, j_end, nins, [&](bool pair, bool col, bool ins, int j, int i, int k) {
            // (j + k < qlen + the inserts of the whole walk = mine.len: the same tables give the same walk; compared all the same)
            if (j + k >= mine.len) return;
            if (col) out[j + k] = pair ? tb[i] : (unsigned char)'-';
            else if (ins) {
                const unsigned char c = tb[i];
                out[j + k] = c >= 'A' && c <= 'Z' ? (unsigned char)(c + 32) : c;
            }
        });
        sw_msa_dashes(out + j_end + nins, max(0, min(qlen - j_end, mine.len - j_end - nins)), lane);
    }
}

}  // namespace swk
