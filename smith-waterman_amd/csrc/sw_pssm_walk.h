// sw_pssm_walk.h -- what kernels that read a hit table's alignments share (gfx950): the clamped count of a query, the guards that make
// entry (q, r) a USED ENTRY and THE WALK of its ops, as include/swhip.h states them for sw_db_pssm_from_hits.  One wave per entry;
// everything is __forceinline__ inside an unnamed namespace, as in sw_wave.h.  sw_pssm_from_hits (sw_pssm_hits.hip) and both passes of
// sw_pssm_weights.hip go through the guards, the reach test and sw_pssm_walk, the two walking launches of sw_msa_hits.hip through the
// guards and sw_msa_walk, the walk over all columns with the inserts counted.  The loop over a query's entries stays written out in the
// tile kernels: behind one helper sw_pssm_weights_tile measured 1 % slower at top = 4096.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"

namespace swk {

namespace {

// The entries of query q that count: nhits[q] clamped to 0..top, top without the counts.
__device__ __forceinline__ int64_t sw_pssm_query_hits(const HitTables& t, int64_t q) { return t.nhits ? min(max(t.nhits[q], (int64_t)0), t.top) : t.top; }

// The ops of entry e
__device__ __forceinline__ const unsigned char* sw_pssm_entry_ops(const HitTables& t, int64_t e) { return (const unsigned char*)t.ops + e * t.ops_cap; }

// Entry e = q * top + r (r below the query's clamped count) of a query of qlen columns: is it used?  Entry and alignment are loaded at
// wave-uniform addresses, and every index is compared, unsigned, before anything is loaded through it.  A used entry leaves its
// alignment, its target's first byte in the database and its target's length.
__device__ __forceinline__ bool sw_pssm_entry_used(const HitTables& t, int64_t e, int64_t qlen, sw_alignment& a, int64_t& toff, int64_t& len) {
    const uint64_t tg = (uint64_t)t.hits[e].target;
    if (tg >= (uint64_t)t.ntargets) return false;
    a = t.aln[e];
    if (a.max_score < t.include_min || a.nops <= 0 || a.nops > t.ops_cap) return false;
    toff = t.offsets[tg];
    len = t.offsets[tg + 1] - toff;
    return (uint64_t)a.q_begin <= (uint64_t)qlen && (uint64_t)a.t_begin <= (uint64_t)len;
}

// Can the columns [q_begin, q_begin + nops) of a used entry reach the tile [c0, c1)?  (no sum of two table values: none can overflow)
__device__ __forceinline__ bool sw_pssm_reaches_tile(const sw_alignment& a, int64_t c0, int64_t c1) { return a.q_begin < c1 && a.nops > c0 - a.q_begin; }

// The walk of a used entry through the tile of columns [c0, c1), c1 <= qlen, by one wave: the ops 64 at a time, one op per lane: one
// ballot of "consumes a query column", one of "consumes a target byte"; the number of set bits below a lane (mbcnt) gives the lane its
// (j, i), the popcounts advance the wave-uniform bases.  No serial walk, no scan.  at_pair(j, i) runs in every 'M' lane whose column
// lies in the tile and whose target byte inside the target.  The walk ends with the tile: j only grows.
template <typename F>
__device__ __forceinline__ void sw_pssm_walk(const unsigned char* ops, const sw_alignment& a, int64_t len, int64_t c0, int64_t c1, int lane, F&& at_pair) {
    int64_t jb = a.q_begin, ib = a.t_begin;                          // wave-uniform bases of the chunk
    for (int64_t o = 0; o < a.nops && jb < c1 && ib < len; o += 64) {
        const int op = o + lane < a.nops ? (int)ops[o + lane] : 0;
        const bool m = op == 'M';
        const uint64_t bq = __ballot(m || op == 'I'), bt = __ballot(m || op == 'D');
        const int64_t j = jb + (int64_t)__builtin_amdgcn_mbcnt_hi((unsigned)(bq >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bq, 0u));
        const int64_t i = ib + (int64_t)__builtin_amdgcn_mbcnt_hi((unsigned)(bt >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bt, 0u));
        if (m && j >= c0 && j < c1 && i < len) at_pair(j, i);
        jb += __popcll(bq); ib += __popcll(bt);
    }
}

// The same walk over ALL columns of the query, with the running count of VALID INSERTS -- a 'D' op met with i < len and j <= qlen --
// that the rows of sw_db_msa_from_hits need (sw_msa_hits.hip): a third ballot, whose set bits below a lane are the inserts the walk has
// seen before the lane's op.  at_op(pair, col, ins, j, i, k) runs in EVERY lane of every chunk (it may ballot): pair: an 'M' that pairs
// column j with target byte i; col: an 'M' or 'I' that consumes column j < qlen (pair implies col); ins: a valid insert of target
// byte i before column j; k: the valid inserts before this op.  (j, i, k stay below 2^21 + 64: q_begin <= qlen, t_begin <= len, both at
// most 2^20 - 1, and the walk ends with the first chunk that starts behind the query or the target -- no later op pairs, inserts, or
// sees another insert.)  Leaves j_end, the first column the chunks walked did not reach (<= qlen), and the number of valid inserts.
template <typename F>
__device__ __forceinline__ void sw_msa_walk(const unsigned char* ops, const sw_alignment& a, int qlen, int len, int lane, int& j_end, int& inserts, F&& at_op) {
    int jb = (int)a.q_begin, ib = (int)a.t_begin, kb = 0;            // wave-uniform bases of the chunk
    for (int64_t o = 0; o < a.nops && jb <= qlen && ib < len; o += 64) {
        const int op = o + lane < a.nops ? (int)ops[o + lane] : 0;
        const bool m = op == 'M';
        const uint64_t bq = __ballot(m || op == 'I'), bt = __ballot(m || op == 'D');
        const int j = jb + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bq >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bq, 0u));
        const int i = ib + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bt >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bt, 0u));
        const bool ins = op == 'D' && i < len && j <= qlen;
        const uint64_t bd = __ballot(ins);
        const int k = kb + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bd >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bd, 0u));
        const bool col = (m || op == 'I') && j < qlen;
        at_op(m && col && i < len, col, ins, j, i, k);
        jb += __popcll(bq); ib += __popcll(bt); kb += __popcll(bd);
    }
    j_end = min(jb, qlen); inserts = kb;
}

}  // namespace

}  // namespace swk
