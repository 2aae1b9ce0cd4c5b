// sw_hits_host.cpp -- the CPU legs of the calls that read a hit table's alignments (sw_pssm_from_hits_host, sw_pssm_hit_weights_host,
// sw_msa_from_hits_host; include/swhip.h states their rules) and of the filter of the column rows (sw_msa_filter_host), the argument
// checks they share with the device calls, and sw_write_a3m.
// What a USED ENTRY is and how its ops are WALKED stands here once, for all three legs.  Plain C++ that needs nothing of the library but
// the header and the error text: a stand-alone program can compile this file alone (tests/pssm_hits_driver.cpp does, under the address
// and undefined-behaviour sanitizers).
#include <cstdio>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/swhip.h"

namespace swh {   // sw_host.cpp
void set_err(const char* fmt, ...);
// (shared with sw_api_search.hip through sw_ctx.h, not exported by the library)
__attribute__((visibility("hidden"))) int check_pssm_update(const char* who, const sw_pssm_update* upd, int64_t top, const void* hits, const void* aln,
                                                            const void* ops, int64_t ops_cap, const void* out, const void* counts);
__attribute__((visibility("hidden"))) int check_pssm_weighting(const char* who, const sw_pssm_weighting* wt, int64_t top, const void* hits, const void* aln,
                                                               const void* ops, int64_t ops_cap, const void* weights);
__attribute__((visibility("hidden"))) int check_msa(const char* who, const int64_t* qoffsets, int64_t nqueries, int64_t top, const void* hits, const void* aln,
                                                    const void* ops, int64_t ops_cap, const void* cols, const void* rows, const void* a3m, int64_t a3m_cap,
                                                    const void* a3m_bytes);
__attribute__((visibility("hidden"))) int check_msa_filter(const char* who, const int64_t* qoffsets, int64_t nqueries, int64_t top, const void* cols,
                                                           const sw_msa_filter* filter, const void* hits, const void* hits_out, const void* keep);
__attribute__((visibility("hidden"))) void pssm_update_table(const sw_submat* sub, const char* letters, int n, int8_t* S);
}  // namespace swh

namespace {

constexpr int64_t kMaxDim = (1 << 20) - 1;   // swk::SW_MAX_DIM (this file does not see the kernels' header)

// The table arguments of every call that reads a hit table's alignments.
int check_hit_tables(const char* who, int64_t top, const void* hits, const void* aln, const void* ops, int64_t ops_cap) {
    using swh::set_err;
    if (top < 1 || top > SW_TOP_MAX) { set_err("%s: top = %lld is out of range 1..%d", who, (long long)top, SW_TOP_MAX); return SW_EINVAL; }
    if (!hits || !aln || !ops) { set_err("%s: NULL hit table, alignment array or ops buffer", who); return SW_EINVAL; }
    if (ops_cap < 1) { set_err("%s: ops_cap = %lld is below 1", who, (long long)ops_cap); return SW_EINVAL; }
    return SW_OK;
}

// The targets' lengths, from their offsets; leaves the longest.
int check_target_lengths(const char* who, const int64_t* offsets, int64_t ntargets, int64_t* longest) {
    *longest = 0;
    for (int64_t k = 0; k < ntargets; ++k) {
        const int64_t len = offsets[k + 1] - offsets[k];
        if (len < 0 || len > kMaxDim) { swh::set_err("%s: target %lld has length %lld, out of range 0..%lld", who, (long long)k, (long long)len, (long long)kMaxDim); return SW_EINVAL; }
        *longest = std::max(*longest, len);
    }
    return SW_OK;
}

}  // namespace

namespace swh {

// What sw_db_pssm_from_hits and sw_pssm_from_hits_host check beyond the search arguments.
int check_pssm_update(const char* who, const sw_pssm_update* upd, int64_t top, const void* hits, const void* aln, const void* ops, int64_t ops_cap,
                      const void* out, const void* counts) {
    if (!upd || !upd->sub) { set_err("%s: NULL update rule or substitution matrix", who); return SW_EINVAL; }
    if (int rc = check_hit_tables(who, top, hits, aln, ops, ops_cap)) return rc;
    if (upd->prior_weight < 0 || upd->prior_weight > 65535) { set_err("%s: prior_weight = %d is out of range 0..65535", who, upd->prior_weight); return SW_EINVAL; }
    if (!out && !counts) { set_err("%s: both outputs are NULL", who); return SW_EINVAL; }
    return SW_OK;
}

// What sw_db_pssm_hit_weights and sw_pssm_hit_weights_host check beyond the search arguments.
int check_pssm_weighting(const char* who, const sw_pssm_weighting* wt, int64_t top, const void* hits, const void* aln, const void* ops, int64_t ops_cap,
                         const void* weights) {
    if (!wt || !weights) { set_err("%s: NULL weighting rule or weight table", who); return SW_EINVAL; }
    if (int rc = check_hit_tables(who, top, hits, aln, ops, ops_cap)) return rc;
    if (wt->per_hit < 1 || wt->per_hit > 65535) { set_err("%s: per_hit = %d is out of range 1..65535", who, wt->per_hit); return SW_EINVAL; }
    return SW_OK;
}

// What sw_db_msa_from_hits and sw_msa_from_hits_host check beyond their pointers and the targets: the query offsets (the rule of every
// many-query call), the tables and the outputs.
int check_msa(const char* who, const int64_t* qoffsets, int64_t nqueries, int64_t top, const void* hits, const void* aln, const void* ops, int64_t ops_cap,
              const void* cols, const void* rows, const void* a3m, int64_t a3m_cap, const void* a3m_bytes) {
    if (!qoffsets) { set_err("%s: NULL query offsets", who); return SW_EINVAL; }
    if (nqueries < 0) { set_err("%s: negative query count", who); return SW_EINVAL; }
    if (qoffsets[0] < 0) { set_err("%s: qoffsets[0] = %lld is negative", who, (long long)qoffsets[0]); return SW_EINVAL; }
    for (int64_t q = 0; q < nqueries; ++q) {
        const int64_t len = qoffsets[q + 1] - qoffsets[q];
        if (len < 1 || len > kMaxDim) { set_err("%s: query %lld has length %lld, out of range 1..%lld", who, (long long)q, (long long)len, (long long)kMaxDim); return SW_EINVAL; }
    }
    if (int rc = check_hit_tables(who, top, hits, aln, ops, ops_cap)) return rc;
    if (!cols && !rows) { set_err("%s: no output: the column rows and the row table are both NULL", who); return SW_EINVAL; }
    if (!rows && (a3m || a3m_bytes)) { set_err("%s: A3M bytes or their total without the row table", who); return SW_EINVAL; }
    if (a3m && !a3m_bytes) { set_err("%s: A3M bytes without a place for their total", who); return SW_EINVAL; }
    if (a3m_cap < 0) { set_err("%s: a3m_cap = %lld is negative", who, (long long)a3m_cap); return SW_EINVAL; }
    return SW_OK;
}

// What sw_msa_filter_device and sw_msa_filter_host check: the query offsets (the rule of check_msa), top, the rule and the outputs.
int check_msa_filter(const char* who, const int64_t* qoffsets, int64_t nqueries, int64_t top, const void* cols, const sw_msa_filter* filter,
                     const void* hits, const void* hits_out, const void* keep) {
    if (!qoffsets) { set_err("%s: NULL query offsets", who); return SW_EINVAL; }
    if (nqueries < 0) { set_err("%s: negative query count", who); return SW_EINVAL; }
    if (qoffsets[0] < 0) { set_err("%s: qoffsets[0] = %lld is negative", who, (long long)qoffsets[0]); return SW_EINVAL; }
    for (int64_t q = 0; q < nqueries; ++q) {
        const int64_t len = qoffsets[q + 1] - qoffsets[q];
        if (len < 1 || len > kMaxDim) { set_err("%s: query %lld has length %lld, out of range 1..%lld", who, (long long)q, (long long)len, (long long)kMaxDim); return SW_EINVAL; }
    }
    if (top < 1 || top > SW_TOP_MAX) { set_err("%s: top = %lld is out of range 1..%d", who, (long long)top, SW_TOP_MAX); return SW_EINVAL; }
    if (!cols || !filter) { set_err("%s: NULL column rows or filter rule", who); return SW_EINVAL; }
    if (filter->max_ident_pct < 1 || filter->max_ident_pct > 101) { set_err("%s: max_ident_pct = %d is out of range 1..101", who, filter->max_ident_pct); return SW_EINVAL; }
    if (filter->min_cover_pct < 0 || filter->min_cover_pct > 100) { set_err("%s: min_cover_pct = %d is out of range 0..100", who, filter->min_cover_pct); return SW_EINVAL; }
    if (!keep && !hits_out) { set_err("%s: no output: the keep table and the filtered hit table are both NULL", who); return SW_EINVAL; }
    if (hits_out && !hits) { set_err("%s: a filtered hit table without the hit table it is made from", who); return SW_EINVAL; }
    return SW_OK;
}

// S[b * n + k] = sub[letters[b]][letters[k]]: the observed residue letters[b] plays the query letter.
void pssm_update_table(const sw_submat* sub, const char* letters, int n, int8_t* S) {
    for (int b = 0; b < n; ++b)
        for (int k = 0; k < n; ++k) S[b * n + k] = sub->s[(unsigned char)letters[b]][(unsigned char)letters[k]];
}

}  // namespace swh

namespace {

// The argument errors of sw_align_pssm_hits_host, restated: the checks of sw_host.cpp need the whole library behind them.
int check_host_args(const char* who, const int64_t* qoffsets, int64_t nqueries, const int64_t* offsets, int64_t ntargets, const sw_pssm_scoring* sc) {
    using swh::set_err;
    if (nqueries < 0 || ntargets < 0) { set_err("%s: negative query or target count", who); return SW_EINVAL; }
    if (offsets[0] < 0 || qoffsets[0] < 0) { set_err("%s: offsets[0] or qoffsets[0] is negative", who); return SW_EINVAL; }
    int64_t maxlen = 0, maxq = 0;
    if (int rc = check_target_lengths(who, offsets, ntargets, &maxlen)) return rc;
    for (int64_t q = 0; q < nqueries; ++q) {
        const int64_t len = qoffsets[q + 1] - qoffsets[q];
        if (len < 1 || len > kMaxDim) { set_err("%s: query %lld has length %lld, out of range 1..%lld", who, (long long)q, (long long)len, (long long)kMaxDim); return SW_EINVAL; }
        maxq = std::max(maxq, len);
    }
    if (!sc->letters) { set_err("%s: NULL letters", who); return SW_EINVAL; }
    if (sc->nletters < 1 || sc->nletters > 256) { set_err("%s: nletters = %d is out of range 1..256", who, sc->nletters); return SW_EINVAL; }
    if (sc->smax < 0 || sc->smax > 127) { set_err("%s: smax = %d is out of range 0..127", who, sc->smax); return SW_EINVAL; }
    if (sc->other < -128 || sc->other > sc->smax) { set_err("%s: other = %d is out of range -128..smax = %d", who, sc->other, sc->smax); return SW_EINVAL; }
    bool seen[256] = {};
    for (int k = 0; k < sc->nletters; ++k) {
        const int b = (unsigned char)sc->letters[k];
        if (seen[b]) { set_err("%s: letter 0x%02x is listed twice", who, b); return SW_EINVAL; }
        seen[b] = true;
    }
    if (sc->gap_open > 0 || sc->gap_extend > 0 || (int64_t)sc->gap_open + sc->gap_extend < -(1ll << 24)) {
        set_err("%s: gap_open and gap_extend must be <= 0 and their sum at least -2^24", who);
        return SW_EINVAL;
    }
    if ((int64_t)sc->smax * std::min(maxq, maxlen) >= (1ll << 24)) { set_err("%s: smax times min(longest query, longest target) reaches 2^24", who); return SW_EINVAL; }
    return SW_OK;
}

int64_t floor_div(int64_t a, int64_t b) {   // b > 0; C++ '/' truncates toward zero
    int64_t q = a / b;
    if (a % b != 0 && a < 0) --q;
    return q;
}

// The tables the three legs read, as their callers hand them over.
struct HitTables {
    const char* db; const int64_t* offsets; int64_t ntargets;
    const sw_hit* hits; const int64_t* nhits; int64_t top;
    const sw_alignment* aln; const char* ops; int64_t ops_cap;
    int64_t include_min;
};

// The entries of query q that count: nhits[q] clamped to 0..top, top without the counts.
int64_t query_hits(const HitTables& t, int64_t q) { return t.nhits ? std::clamp<int64_t>(t.nhits[q], 0, t.top) : t.top; }

// Entry e = q * top + r (r below the query's clamped count) of a query of qlen columns: is it a USED ENTRY?  Every index is compared,
// unsigned, before anything is read through it.  A used entry leaves its target's bytes and length.
bool entry_used(const HitTables& t, int64_t e, int64_t qlen, const unsigned char*& tb, int64_t& len) {
    const uint64_t tg = (uint64_t)t.hits[e].target;
    if (tg >= (uint64_t)t.ntargets) return false;
    const sw_alignment& a = t.aln[e];
    if (a.max_score < t.include_min || a.nops <= 0 || a.nops > t.ops_cap) return false;
    len = t.offsets[tg + 1] - t.offsets[tg];
    if ((uint64_t)a.q_begin > (uint64_t)qlen || (uint64_t)a.t_begin > (uint64_t)len) return false;
    tb = (const unsigned char*)t.db + t.offsets[tg];
    return true;
}

// THE WALK of a used entry: at_op(op, j, i) for its 'M', 'I' and 'D' ops in turn, j the column and i the target byte the op stands at
// (either may lie past its end: the caller compares); every other byte is passed over.
template <typename AtOp>
void walk_ops(const HitTables& t, int64_t e, AtOp at_op) {
    const sw_alignment& a = t.aln[e];
    const char* row = t.ops + e * t.ops_cap;
    int64_t j = a.q_begin, i = a.t_begin;
    for (int64_t o = 0; o < a.nops; ++o) {
        const char op = row[o];
        if (op != 'M' && op != 'I' && op != 'D') continue;
        at_op(op, j, i);
        j += op != 'D';
        i += op != 'I';
    }
}

// at(j, k) for every pair of column j with letters[k] that the used entries of query q make, entry by entry; begin(e) ahead of the
// pairs of the used entry e.
template <typename Begin, typename At>
void for_each_counted_pair(const HitTables& t, int64_t q, int64_t qlen, const int* code, Begin begin, At at) {
    const int64_t nh = query_hits(t, q);
    for (int64_t e = q * t.top; e < q * t.top + nh; ++e) {
        const unsigned char* tb;
        int64_t len;
        if (!entry_used(t, e, qlen, tb, len)) continue;
        begin(e);
        walk_ops(t, e, [&](char op, int64_t j, int64_t i) {
            if (op == 'M' && j < qlen && i < len && code[tb[i]] >= 0) at(j, code[tb[i]]);
        });
    }
}

// code[b]: the place of target byte b in a column, -1 where it has none
void letter_places(const sw_pssm_scoring* sc, int* code) {
    std::fill(code, code + 256, -1);
    for (int k = 0; k < sc->nletters; ++k) code[(unsigned char)sc->letters[k]] = k;
}

}  // namespace

extern "C" {

// The CPU leg of sw_db_pssm_from_hits: per query the counts of its used entries, walked op by op, then the rounded weighted mean.
// Everything is checked before the first byte is written.
int sw_pssm_from_hits_host(const int8_t* prior, const int64_t* qoffsets, int64_t nqueries, const char* db, const int64_t* offsets, int64_t ntargets,
                           const sw_pssm_scoring* scoring, const sw_pssm_update* upd, const sw_hit* hits, const int64_t* nhits, int64_t top,
                           const sw_alignment* aln, const char* ops, int64_t ops_cap, const int32_t* weights, int8_t* pssm_out, int32_t* counts) {
    const char* who = "sw_pssm_from_hits_host";
    if (!prior || !qoffsets || !db || !offsets || !scoring) { swh::set_err("%s: NULL pointer", who); return SW_EINVAL; }
    if (int rc = check_host_args(who, qoffsets, nqueries, offsets, ntargets, scoring)) return rc;
    if (int rc = swh::check_pssm_update(who, upd, top, hits, aln, ops, ops_cap, pssm_out, counts)) return rc;
    const HitTables t{db, offsets, ntargets, hits, nhits, top, aln, ops, ops_cap, upd->include_min_score};
    const int n = scoring->nletters;
    int code[256];
    letter_places(scoring, code);
    std::vector<int8_t> S((size_t)n * n);
    swh::pssm_update_table(upd->sub, scoring->letters, n, S.data());
    std::vector<int32_t> C;
    for (int64_t q = 0; q < nqueries; ++q) {
        const int64_t g0 = qoffsets[q], qlen = qoffsets[q + 1] - g0;
        C.assign((size_t)(qlen * n), 0);
        int32_t w = 1;
        for_each_counted_pair(t, q, qlen, code, [&](int64_t e) { w = weights ? std::clamp<int32_t>(weights[e], 0, 65535) : 1; },
                              [&](int64_t j, int k) { C[(size_t)(j * n + k)] += w; });
        if (counts) std::copy(C.begin(), C.end(), counts + (g0 - qoffsets[0]) * n);
        if (!pssm_out) continue;
        for (int64_t j = 0; j < qlen; ++j) {
            const int32_t* cj = C.data() + j * n;
            int64_t N = 0;
            for (int k = 0; k < n; ++k) N += cj[k];
            const int64_t den = (int64_t)upd->prior_weight + N;
            for (int k = 0; k < n; ++k) {
                const int64_t P = std::min<int>(prior[(g0 + j) * n + k], scoring->smax);
                int64_t v = P;
                if (den != 0) {
                    int64_t num = (int64_t)upd->prior_weight * P;
                    for (int b = 0; b < n; ++b) num += (int64_t)cj[b] * S[(size_t)b * n + k];
                    v = std::clamp<int64_t>(floor_div(2 * num + den, 2 * den), -128, 127);
                }
                pssm_out[(g0 + j) * n + k] = (int8_t)v;
            }
        }
    }
    return SW_OK;
}

// The CPU leg of sw_db_pssm_hit_weights: per query n[j][k] and k_j from one walk of its used entries, T_r and m_r from a second, then
// A_r, their sum and the rounded shares.  Everything is checked before the first weight is written.
int sw_pssm_hit_weights_host(const int64_t* qoffsets, int64_t nqueries, const char* db, const int64_t* offsets, int64_t ntargets,
                             const sw_pssm_scoring* scoring, const sw_pssm_weighting* weighting, const sw_hit* hits, const int64_t* nhits, int64_t top,
                             const sw_alignment* aln, const char* ops, int64_t ops_cap, int32_t* weights) {
    const char* who = "sw_pssm_hit_weights_host";
    if (!qoffsets || !db || !offsets || !scoring) { swh::set_err("%s: NULL pointer", who); return SW_EINVAL; }
    if (int rc = check_host_args(who, qoffsets, nqueries, offsets, ntargets, scoring)) return rc;
    if (int rc = swh::check_pssm_weighting(who, weighting, top, hits, aln, ops, ops_cap, weights)) return rc;
    const HitTables t{db, offsets, ntargets, hits, nhits, top, aln, ops, ops_cap, weighting->include_min_score};
    const int n = scoring->nletters;
    constexpr int64_t F = 1ll << 20;
    int code[256];
    letter_places(scoring, code);
    std::vector<int32_t> N, K;
    std::vector<int64_t> T((size_t)top), m((size_t)top), A((size_t)top);
    for (int64_t q = 0; q < nqueries; ++q) {
        const int64_t qlen = qoffsets[q + 1] - qoffsets[q];
        N.assign((size_t)(qlen * n), 0);
        K.assign((size_t)qlen, 0);
        std::fill(T.begin(), T.end(), 0);
        std::fill(m.begin(), m.end(), 0);
        for_each_counted_pair(t, q, qlen, code, [](int64_t) {}, [&](int64_t j, int k) { ++N[(size_t)(j * n + k)]; });
        for (int64_t j = 0; j < qlen; ++j)
            for (int k = 0; k < n; ++k) K[(size_t)j] += N[(size_t)(j * n + k)] > 0;
        int64_t cur = 0;
        for_each_counted_pair(t, q, qlen, code, [&](int64_t e) { cur = e - q * top; },
                              [&](int64_t j, int k) {
                                  T[(size_t)cur] += F / ((int64_t)K[(size_t)j] * N[(size_t)(j * n + k)]);
                                  ++m[(size_t)cur];
                              });
        int64_t U = 0, sum = 0;
        for (int64_t r = 0; r < top; ++r) {
            A[(size_t)r] = m[(size_t)r] > 0 ? T[(size_t)r] / m[(size_t)r] : 0;
            U += A[(size_t)r] > 0;
            sum += A[(size_t)r];
        }
        for (int64_t r = 0; r < top; ++r)
            weights[q * top + r] = sum > 0 ? (int32_t)std::min<int64_t>(65535, (2 * (int64_t)weighting->per_hit * U * A[(size_t)r] + sum) / (2 * sum)) : 0;
    }
    return SW_OK;
}

// The CPU leg of sw_db_msa_from_hits: entry by entry in (q, r) order, its ops walked one by one.  Everything is checked before the
// first byte is written.
int sw_msa_from_hits_host(const char* queries, const int64_t* qoffsets, int64_t nqueries, const char* db, const int64_t* offsets, int64_t ntargets,
                          int64_t include_min_score, const sw_hit* hits, const int64_t* nhits, int64_t top, const sw_alignment* aln, const char* ops,
                          int64_t ops_cap, char* cols, sw_msa_row* rows, char* a3m, int64_t a3m_cap, int64_t* a3m_bytes) {
    const char* who = "sw_msa_from_hits_host";
    if (!db || !offsets) { swh::set_err("%s: NULL pointer", who); return SW_EINVAL; }
    if (ntargets < 0 || offsets[0] < 0) { swh::set_err("%s: negative target count or offsets[0]", who); return SW_EINVAL; }
    int64_t longest = 0;
    if (int rc = check_target_lengths(who, offsets, ntargets, &longest)) return rc;
    if (int rc = swh::check_msa(who, qoffsets, nqueries, top, hits, aln, ops, ops_cap, cols, rows, a3m, a3m_cap, a3m_bytes)) return rc;
    const HitTables t{db, offsets, ntargets, hits, nhits, top, aln, ops, ops_cap, include_min_score};
    std::string row;   // the A3M row of the entry at hand
    int64_t off = 0;
    for (int64_t q = 0; q < nqueries; ++q) {
        const int64_t g0 = qoffsets[q], qlen = qoffsets[q + 1] - g0;
        const int64_t nh = query_hits(t, q);
        for (int64_t r = 0; r < top; ++r) {
            const int64_t e = q * top + r;
            char* crow = cols ? cols + (g0 - qoffsets[0]) * top + r * qlen : nullptr;
            if (crow) std::fill(crow, crow + qlen, '-');
            sw_msa_row out{off, 0, 0, 0, 0};
            const unsigned char* tb;
            int64_t len;
            if (r < nh && entry_used(t, e, qlen, tb, len)) {
                row.assign((size_t)aln[e].q_begin, '-');
                walk_ops(t, e, [&](char op, int64_t j, int64_t i) {
                    if (op == 'D') {
                        if (i < len && j <= qlen) {            // a valid insert
                            const unsigned char c = tb[i];
                            row += (char)(c >= 'A' && c <= 'Z' ? c + 32 : c);
                            ++out.ninsert;
                        }
                        return;
                    }
                    if (j >= qlen) return;                      // ('M' or 'I' behind the last column)
                    const bool pair = op == 'M' && i < len;
                    if (pair) {
                        if (crow) crow[j] = (char)tb[i];
                        ++out.nmatch;
                        out.nident += queries && (unsigned char)queries[g0 + j] == tb[i];
                    }
                    row += pair ? (char)tb[i] : '-';
                });
                row.append((size_t)(qlen + out.ninsert) - row.size(), '-');   // the columns behind the walk's end
                out.len = (int32_t)(qlen + out.ninsert);
                if (a3m && off + out.len <= a3m_cap) std::copy(row.begin(), row.end(), a3m + off);
            }
            if (rows) rows[e] = out;
            off += out.len;
        }
    }
    if (a3m_bytes) *a3m_bytes = off;
    return SW_OK;
}

// The CPU leg of sw_msa_filter_device: the rule of include/swhip.h restated, row by row in rank order; a row is compared with the rows
// kept before it only.  Everything is checked before the first byte is written; hits_out may be hits.
int sw_msa_filter_host(const char* cols, const char* queries, const int64_t* qoffsets, int64_t nqueries, int64_t top, const sw_msa_filter* filter,
                       const sw_hit* hits, sw_hit* hits_out, int32_t* keep, int64_t* nkept) {
    const char* who = "sw_msa_filter_host";
    if (int rc = swh::check_msa_filter(who, qoffsets, nqueries, top, cols, filter, hits, hits_out, keep)) return rc;
    const int32_t ident = filter->max_ident_pct, cover = filter->min_cover_pct;
    std::vector<int64_t> kept;   // the rows of the query at hand that are kept so far
    for (int64_t q = 0; q < nqueries; ++q) {
        const int64_t g0 = qoffsets[q], qlen = qoffsets[q + 1] - g0;
        const char* rows = cols + (g0 - qoffsets[0]) * top;
        kept.clear();
        for (int64_t r = 0; r < top; ++r) {
            const char* row = rows + r * qlen;
            int32_t n = 0, sameq = 0;
            int64_t lo = qlen, hi = 0;   // the row's letters lie in [lo, hi): nothing outside counts in same or sameq
            for (int64_t j = 0; j < qlen; ++j)
                if (row[j] != '-') { ++n; lo = std::min(lo, j); hi = j + 1; }
            if (queries)
                for (int64_t j = lo; j < hi; ++j) sameq += (row[j] != '-') & (row[j] == queries[g0 + j]);
            bool k = n >= 1 && (int64_t)100 * n >= (int64_t)cover * qlen && (!queries || 100 * sameq < ident * n);
            for (size_t i = 0; k && i < kept.size(); ++i) {
                const char* other = rows + kept[i] * qlen;
                int32_t same = 0;
                for (int64_t j = lo; j < hi; ++j) same += (row[j] != '-') & (row[j] == other[j]);
                k = 100 * same < ident * n;
            }
            if (k) kept.push_back(r);
            const int64_t e = q * top + r;
            if (keep) keep[e] = k;
            if (hits_out) {
                const sw_hit h = hits[e];
                hits_out[e] = sw_hit{k ? h.target : -1, h.max_pos, h.max_score};
            }
        }
        if (nkept) nkept[q] = (int64_t)kept.size();
    }
    return SW_OK;
}

// One query's A3M file (include/swhip.h states the layout); the text is built whole and written once.
int sw_write_a3m(const char* path, const char* qname, const char* query, int64_t qlen, const char* const* tnames, int64_t ntargets, const sw_hit* hits,
                 const sw_alignment* aln, const sw_msa_row* rows, int64_t top, const char* a3m, int64_t a3m_cap) {
    if (!path || !qname || !hits || !aln || !rows || !a3m || top < 1 || qlen < 1) { swh::set_err("sw_write_a3m: bad argument"); return SW_EINVAL; }
    std::string text;
    if (query) {
        text += '>'; text += qname; text += '\n';
        text.append(query, (size_t)qlen);
        text += '\n';
    }
    for (int64_t r = 0; r < top; ++r) {
        const sw_msa_row& w = rows[r];
        if (w.len <= 0 || w.off < 0 || w.off + w.len > a3m_cap) continue;
        const int64_t t = hits[r].target;
        if (t < 0 || t >= ntargets) { swh::set_err("sw_write_a3m: entry %lld names target %lld of %lld", (long long)r, (long long)t, (long long)ntargets); return SW_EINVAL; }
        const sw_alignment& a = aln[r];
        text += '>';
        text += tnames ? std::string(tnames[t]) : std::to_string(t);
        char buf[200];
        snprintf(buf, sizeof buf, " score=%lld q=%lld-%lld t=%lld-%lld ident=%d/%d\n", (long long)a.max_score, (long long)a.q_begin, (long long)a.q_end,
                 (long long)a.t_begin, (long long)a.t_end, w.nident, w.nmatch);
        text += buf;
        text.append(a3m + w.off, (size_t)w.len);
        text += '\n';
    }
    FILE* f = fopen(path, "wb");
    if (!f) { swh::set_err("sw_write_a3m: cannot open %s for writing", path); return SW_EINVAL; }
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    if (fclose(f) != 0 || !ok) { swh::set_err("sw_write_a3m: write error on %s", path); return SW_EINVAL; }
    return SW_OK;
}

}  // extern "C"
