// sw_host.cpp -- host-only parts of the C-ABI (no GPU needed): the reference's input generator,
// its wavefront indexing helpers and the host traceback.  Citations: /root/reference paths.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>
#include "sw_ctx.h"

namespace swh {
thread_local std::string g_err;
void set_err(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}

// glibc random_r TYPE_3 (x^31 + x^3 + 1) as used by rand(): 31-word state seeded by the
// Lehmer generator 16807 mod (2^31-1), 310 warm-up steps, outputs are state sums >> 1.
// The reference draws from libc rand() (serial_smithW.c:338,351); restating it keeps the
// generated sequences identical on any host libc.
class GlibcRand {
public:
    explicit GlibcRand(uint32_t seed) {
        int64_t w = seed ? seed : 1;
        st_[0] = (uint32_t)w;
        for (int i = 1; i < 31; ++i) {
            w = (16807 * w) % 2147483647;      // same value as glibc's Schrage form
            st_[i] = (uint32_t)w;
        }
        f_ = 3; r_ = 0;
        for (int i = 0; i < 310; ++i) (void)next();
    }
    int32_t next() {
        st_[f_] += st_[r_];
        const uint32_t out = st_[f_] >> 1;
        f_ = (f_ + 1 == 31) ? 0 : f_ + 1;
        r_ = (r_ + 1 == 31) ? 0 : r_ + 1;
        return (int32_t)out;
    }
private:
    uint32_t st_[31];
    int f_, r_;
};

// The argument rules every search call shares: query length, offsets[0], every target's length; reports the longest target and the
// number of non-empty ones.  kMaxDim: the 2^20 - 1 of swk::SW_MAX_DIM (40-bit indices).
int check_targets(const char* who, int64_t qlen, const int64_t* offsets, int64_t ntargets, int64_t* maxlen_out, int64_t* nonempty_out) {
    constexpr int64_t kMaxDim = swk::SW_MAX_DIM;
    if (qlen < 1 || qlen > kMaxDim) { set_err("%s: query length %lld out of range 1..%lld", who, (long long)qlen, (long long)kMaxDim); return SW_EINVAL; }
    if (offsets[0] < 0) { set_err("%s: offsets[0] = %lld is negative", who, (long long)offsets[0]); return SW_EINVAL; }
    int64_t maxlen = 0, nonempty = 0;
    for (int64_t k = 0; k < ntargets; ++k) {
        const int64_t len = offsets[k + 1] - offsets[k];
        if (len < 0) { set_err("%s: offsets decrease at target %lld", who, (long long)k); return SW_EINVAL; }
        if (len > kMaxDim) { set_err("%s: target %lld has length %lld (max %lld)", who, (long long)k, (long long)len, (long long)kMaxDim); return SW_EINVAL; }
        maxlen = std::max(maxlen, len);
        nonempty += len > 0;
    }
    *maxlen_out = maxlen;
    *nonempty_out = nonempty;
    return SW_OK;
}

// The scoring rules of the affine calls for a query of `qlen` against a longest target of `maxlen` (include/swhip.h).
constexpr int64_t kScoreLimit = 1ll << 24;
static int check_gap_costs(const char* who, int32_t gap_open, int32_t gap_extend) {
    if (gap_open > 0) { set_err("%s: gap_open must be <= 0 (got %d)", who, gap_open); return SW_EINVAL; }
    if (gap_extend > 0) { set_err("%s: gap_extend must be <= 0 (got %d)", who, gap_extend); return SW_EINVAL; }
    if ((int64_t)gap_open + (int64_t)gap_extend < -kScoreLimit) {
        set_err("%s: gap_open + gap_extend = %lld is below -2^24", who, (long long)gap_open + (long long)gap_extend);
        return SW_EINVAL;
    }
    return SW_OK;
}

static int check_affine_scoring(const char* who, const sw_affine* sc, int64_t qlen, int64_t maxlen) {
    if (int rc = check_gap_costs(who, sc->gap_open, sc->gap_extend)) return rc;
    int best = 0, bx = 0, by = 0;
    for (int x = 0; x < 256; ++x)
        for (int y = 0; y < 256; ++y)
            if (sc->sub->s[x][y] > best) { best = sc->sub->s[x][y]; bx = x; by = y; }
    if ((int64_t)best * std::min(qlen, maxlen) >= kScoreLimit) {
        set_err("%s: table entry s[%d][%d] = %d times min(query length %lld, longest target %lld) reaches 2^24 (the 24-bit score of the arg-max key)",
                who, bx, by, best, (long long)qlen, (long long)maxlen);
        return SW_EINVAL;
    }
    return SW_OK;
}

// The argument rules of the affine search (include/swhip.h), shared by the device and the host entry point.
int check_search_affine(const char* who, int64_t qlen, const int64_t* offsets, int64_t ntargets, const sw_affine* sc, int64_t* maxlen_out,
                        int64_t* nonempty_out) {
    if (!sc || !sc->sub) { set_err("%s: NULL scoring or substitution matrix", who); return SW_EINVAL; }
    int64_t maxlen = 0, nonempty = 0;
    if (int rc = check_targets(who, qlen, offsets, ntargets, &maxlen, &nonempty)) return rc;
    if (int rc = check_affine_scoring(who, sc, qlen, maxlen)) return rc;
    *maxlen_out = maxlen;
    *nonempty_out = nonempty;
    return SW_OK;
}

// The argument rules of a many-query search (sw_db_search_affine, sw_search_affine_multi_host): the query offsets, every query's
// length, and the scoring rules taken over the longest query against the database's longest target.  O(nqueries).
static int check_query_offsets(const char* who, const int64_t* qoffsets, int64_t nqueries, int64_t* maxq_out) {
    constexpr int64_t kMaxDim = swk::SW_MAX_DIM;
    if (nqueries < 0) { set_err("%s: negative query count", who); return SW_EINVAL; }
    if (qoffsets[0] < 0) { set_err("%s: qoffsets[0] = %lld is negative", who, (long long)qoffsets[0]); return SW_EINVAL; }
    int64_t maxq = 0;
    for (int64_t q = 0; q < nqueries; ++q) {
        const int64_t len = qoffsets[q + 1] - qoffsets[q];
        if (len < 0) { set_err("%s: qoffsets decrease at query %lld", who, (long long)q); return SW_EINVAL; }
        if (len < 1 || len > kMaxDim) { set_err("%s: query %lld has length %lld, out of range 1..%lld", who, (long long)q, (long long)len, (long long)kMaxDim); return SW_EINVAL; }
        maxq = std::max(maxq, len);
    }
    *maxq_out = maxq;
    return SW_OK;
}

int check_search_multi(const char* who, const int64_t* qoffsets, int64_t nqueries, int64_t longest_target, const sw_affine* sc, int64_t* maxq_out) {
    if (!qoffsets || !sc || !sc->sub) { set_err("%s: NULL query offsets, scoring or substitution matrix", who); return SW_EINVAL; }
    int64_t maxq = 0;
    if (int rc = check_query_offsets(who, qoffsets, nqueries, &maxq)) return rc;
    if (int rc = check_affine_scoring(who, sc, maxq, longest_target)) return rc;
    *maxq_out = maxq;
    return SW_OK;
}

// The argument rules of a many-query PSSM call (sw_db_search_pssm and its twins, sw_search_pssm_multi_host): the offsets as above, the
// scoring object, and the 24-bit bound that smax makes hold whatever the matrix holds.  O(nqueries) + O(nletters).  Builds the code
// table: code[x] = the place of target byte x in a column, 255 (>= nletters: `other`) for a byte that is not among the letters --
// with 256 letters every byte has a place and no code says `other`.
int check_search_pssm(const char* who, const int64_t* qoffsets, int64_t nqueries, int64_t longest_target, const sw_pssm_scoring* sc, int64_t* maxq_out,
                      unsigned char (&code)[256]) {
    if (!qoffsets || !sc || !sc->letters) { set_err("%s: NULL query offsets, scoring or letters", who); return SW_EINVAL; }
    int64_t maxq = 0;
    if (int rc = check_query_offsets(who, qoffsets, nqueries, &maxq)) return rc;
    if (sc->nletters < 1 || sc->nletters > 256) { set_err("%s: nletters = %d is out of range 1..256", who, sc->nletters); return SW_EINVAL; }
    if (sc->smax < 0 || sc->smax > 127) { set_err("%s: smax = %d is out of range 0..127", who, sc->smax); return SW_EINVAL; }
    if (sc->other < -128 || sc->other > sc->smax) { set_err("%s: other = %d is out of range -128..smax = %d", who, sc->other, sc->smax); return SW_EINVAL; }
    bool seen[256] = {};
    memset(code, 255, sizeof code);
    for (int k = 0; k < sc->nletters; ++k) {
        const int b = (unsigned char)sc->letters[k];
        if (seen[b]) { set_err("%s: letter 0x%02x is listed twice", who, b); return SW_EINVAL; }
        seen[b] = true;
        code[b] = (unsigned char)k;
    }
    if (int rc = check_gap_costs(who, sc->gap_open, sc->gap_extend)) return rc;
    if ((int64_t)sc->smax * std::min(maxq, longest_target) >= kScoreLimit) {
        set_err("%s: smax = %d times min(longest query %lld, longest target %lld) reaches 2^24 (the 24-bit score of the arg-max key)", who, sc->smax,
                (long long)maxq, (long long)longest_target);
        return SW_EINVAL;
    }
    *maxq_out = maxq;
    return SW_OK;
}

// What sw_db_prefilter_ungapped / sw_prefilter_ungapped_host check beyond check_search_multi (include/swhip.h).
int check_prefilter(const char* who, int64_t min_score, const void* pairs, int64_t pairs_cap, const void* npairs, const void* scores) {
    if (min_score < 1) { set_err("%s: min_score = %lld is below 1", who, (long long)min_score); return SW_EINVAL; }
    if (pairs_cap < 0) { set_err("%s: pairs_cap = %lld is negative", who, (long long)pairs_cap); return SW_EINVAL; }
    if (!pairs && pairs_cap > 0) { set_err("%s: the pair list is NULL with pairs_cap = %lld", who, (long long)pairs_cap); return SW_EINVAL; }
    if (!npairs && (pairs || !scores)) { set_err("%s: the pair count is NULL (allowed only for a call that asks for the scores alone)", who); return SW_EINVAL; }
    return SW_OK;
}

// What sw_align_affine_device / _host check beyond check_search_affine (include/swhip.h); reports the longest hit.
int check_align_affine(const char* who, const int64_t* offsets, int64_t ntargets, const int64_t* hits, int64_t nhits, const void* aln, const void* ops,
                       int64_t ops_cap, int64_t* maxhit_out) {
    if (nhits < 0) { set_err("%s: negative hit count", who); return SW_EINVAL; }
    if (nhits > 0 && !hits) { set_err("%s: hits is NULL with %lld hits", who, (long long)nhits); return SW_EINVAL; }
    if (!aln) { set_err("%s: the alignment array is NULL", who); return SW_EINVAL; }
    if (ops_cap < 0) { set_err("%s: ops_cap = %lld is negative", who, (long long)ops_cap); return SW_EINVAL; }
    if (!ops && ops_cap > 0) { set_err("%s: the ops buffer is NULL with ops_cap = %lld", who, (long long)ops_cap); return SW_EINVAL; }
    int64_t maxhit = 0;
    for (int64_t h = 0; h < nhits; ++h) {
        if (hits[h] < 0 || hits[h] >= ntargets) { set_err("%s: hits[%lld] = %lld is out of range 0..%lld", who, (long long)h, (long long)hits[h], (long long)ntargets - 1); return SW_EINVAL; }
        maxhit = std::max(maxhit, offsets[hits[h] + 1] - offsets[hits[h]]);
    }
    *maxhit_out = maxhit;
    return SW_OK;
}

// What sw_db_align_affine_hits / sw_align_affine_hits_host check beyond check_search_multi (include/swhip.h).
int check_align_hits(const char* who, int64_t top, const void* hits, const void* aln, const void* ops, int64_t ops_cap) {
    if (top < 1 || top > SW_TOP_MAX) { set_err("%s: top = %lld is out of range 1..%d", who, (long long)top, SW_TOP_MAX); return SW_EINVAL; }
    if (!hits) { set_err("%s: the hit table is NULL", who); return SW_EINVAL; }
    if (!aln) { set_err("%s: the alignment array is NULL", who); return SW_EINVAL; }
    if (ops_cap < 0) { set_err("%s: ops_cap = %lld is negative", who, (long long)ops_cap); return SW_EINVAL; }
    if (!ops && ops_cap > 0) { set_err("%s: the ops buffer is NULL with ops_cap = %lld", who, (long long)ops_cap); return SW_EINVAL; }
    return SW_OK;
}

inline char letter(int v) {  // serial_smithW.c:339-346
    switch (v) { case 0: return 'A'; case 2: return 'C'; case 3: return 'G'; default: return 'T'; }
}
}  // namespace swh

template <typename PT>
static int64_t traceback_t(PT* P, int64_t m, int64_t max_pos, int64_t* path, int64_t path_cap) {  // serial_smithW.c:262-277
    int64_t len = 0, pos = max_pos;
    for (int pr = P[pos]; pr > 0; pr = P[pos]) {
        P[pos] = (PT)(pr * SW_PATH);
        if (path && len < path_cap) path[len] = pos;
        ++len;
        pos -= (pr == SW_DIAGONAL) ? m + 1 : (pr == SW_UP) ? m : 1;
    }
    return len;
}

// Gotoh's recurrence of one query against targets, row by row with one row of H and E kept (include/swhip.h states it); -inf is a
// value no sum can reach from below (every E, F inside the matrix is at least gap_open + gap_extend >= -2^24).  s(j, y): the score of
// query column j (1-based) against target byte y -- a table entry for a sequence query, a PSSM entry for a matrix.
template <typename Score>
static void search_targets(Score s, int64_t qlen, const char* db, const int64_t* offsets, int64_t ntargets, int64_t go, int64_t ge, sw_result* results) {
    const int64_t M = qlen + 1;
    constexpr int64_t NEG = -(1ll << 40);
    std::vector<int64_t> Hrow((size_t)M), Erow((size_t)M);
    for (int64_t k = 0; k < ntargets; ++k) {
        const unsigned char* t = (const unsigned char*)db + offsets[k];
        const int64_t len = offsets[k + 1] - offsets[k];
        std::fill(Hrow.begin(), Hrow.end(), 0);
        std::fill(Erow.begin(), Erow.end(), NEG);
        int64_t best = 0, best_pos = 0;
        for (int64_t i = 1; i <= len; ++i) {
            const unsigned char y = t[i - 1];
            int64_t diag = 0, left = 0, F = NEG;       // H[i-1][j-1], H[i][j-1], F[i][j-1]
            for (int64_t j = 1; j <= qlen; ++j) {
                const int64_t up = Hrow[(size_t)j];
                const int64_t E = std::max(Erow[(size_t)j], up + go) + ge;
                F = std::max(F, left + go) + ge;
                const int64_t h = std::max<int64_t>({0, diag + s(j, y), E, F});
                Erow[(size_t)j] = E;
                Hrow[(size_t)j] = h;
                diag = up;
                left = h;
                if (h > best) { best = h; best_pos = i * M + j; }   // row-major scan, strict: the lowest index among equals
            }
        }
        results[k] = sw_result{best_pos, best, 0};
    }
}

// The same recurrence with one direction byte per cell (bits 0-1: where H came from, 0 nothing positive / 1 diagonal / 2 E / 3 F,
// compared in that order; bit 2: E[i][j] opened from H[i-1][j]; bit 3: F[i][j] opened from H[i][j-1]; opening wins a tie), then the
// walk of the canonical alignment (include/swhip.h) from the arg-max, for the targets hits[0 .. nhits) (none longer than maxhit).
template <typename Score>
static void align_targets(Score s, int64_t qlen, const char* db, const int64_t* offsets, const int64_t* hits, int64_t nhits, int64_t maxhit, int64_t go,
                          int64_t ge, sw_alignment* aln, char* ops, int64_t ops_cap) {
    const int64_t M = qlen + 1;
    constexpr int64_t NEG = -(1ll << 40);
    std::vector<int64_t> Hrow((size_t)M), Erow((size_t)M);
    std::vector<unsigned char> dir((size_t)(maxhit + 1) * (size_t)M);
    std::string rev;
    for (int64_t hx = 0; hx < nhits; ++hx) {
        const unsigned char* t = (const unsigned char*)db + offsets[hits[hx]];
        const int64_t len = offsets[hits[hx] + 1] - offsets[hits[hx]];
        std::fill(Hrow.begin(), Hrow.end(), 0);
        std::fill(Erow.begin(), Erow.end(), NEG);
        int64_t best = 0, best_pos = 0;
        for (int64_t i = 1; i <= len; ++i) {
            const unsigned char y = t[i - 1];
            unsigned char* d = dir.data() + i * M;
            int64_t diag = 0, left = 0, F = NEG;       // H[i-1][j-1], H[i][j-1], F[i][j-1]
            for (int64_t j = 1; j <= qlen; ++j) {
                const int64_t up = Hrow[(size_t)j];
                const bool eopen = up + go >= Erow[(size_t)j], fopen = left + go >= F;
                const int64_t E = std::max(Erow[(size_t)j], up + go) + ge;
                F = std::max(F, left + go) + ge;
                const int64_t dg = diag + s(j, y);
                const int64_t h = std::max<int64_t>({0, dg, E, F});
                d[j] = (unsigned char)((h == 0 ? 0 : h == dg ? 1 : h == E ? 2 : 3) | (eopen ? 4 : 0) | (fopen ? 8 : 0));
                Erow[(size_t)j] = E;
                Hrow[(size_t)j] = h;
                diag = up;
                left = h;
                if (h > best) { best = h; best_pos = i * M + j; }
            }
        }
        int64_t i = best_pos / M, j = best_pos % M;
        const int64_t i1 = i, j1 = j;
        rev.clear();
        int state = 0;                                 // 0: H, 2: E, 3: F
        while (best > 0) {
            const unsigned char c = dir[(size_t)(i * M + j)];
            if (state == 0) {
                if (i == 0 || j == 0 || (c & 3) == 0) break;
                if ((c & 3) == 1) { rev.push_back('M'); --i; --j; }
                else state = c & 3;
            } else if (state == 2) {
                rev.push_back('D');
                if (c & 4) state = 0;
                --i;
            } else {
                rev.push_back('I');
                if (c & 8) state = 0;
                --j;
            }
        }
        const int64_t nops = (int64_t)rev.size();
        aln[hx] = best > 0 ? sw_alignment{best_pos, best, j, i, j1, i1, nops} : sw_alignment{0, 0, 0, 0, 0, 0, 0};
        if (ops && nops <= ops_cap) std::reverse_copy(rev.begin(), rev.end(), ops + hx * ops_cap);
    }
}

// The score of a PSSM's column against a target byte (include/swhip.h): the clamped entry where the byte is among the letters.
struct PssmScore {
    const int8_t* col0;   // the query's first column
    const unsigned char* code; int64_t nletters, other, smax;
    int64_t operator()(int64_t j, unsigned char y) const {
        const int k = code[y];
        return k < nletters ? std::min<int64_t>(col0[(j - 1) * nletters + k], smax) : other;
    }
};

// One query's used hits through `align` into rows of their own, copied to their places; every other entry of the row is all zeros and
// its ops row is left alone (the rule of sw_db_align_affine_hits).  align(targets, n, maxhit, aln_rows, ops_rows, ops_cap), maxhit being
// the longest target the row lists: the direction matrix is sized by the hits, not by the database.
template <typename Align>
static void align_hit_row(Align align, int64_t q, const int64_t* offsets, int64_t ntargets, const sw_hit* hits, const int64_t* nhits, int64_t top,
                          sw_alignment* aln, char* ops, int64_t ops_cap) {
    std::vector<int64_t> targets, where;
    const int64_t used = nhits ? std::clamp<int64_t>(nhits[q], 0, top) : top;
    for (int64_t r = 0; r < top; ++r) {
        const uint64_t target = (uint64_t)hits[q * top + r].target;
        if (r < used && target < (uint64_t)ntargets) { targets.push_back((int64_t)target); where.push_back(q * top + r); }
        else aln[q * top + r] = sw_alignment{0, 0, 0, 0, 0, 0, 0};
    }
    if (targets.empty()) return;
    std::vector<sw_alignment> row(targets.size());
    std::vector<char> rows(ops ? targets.size() * (size_t)ops_cap : 0);
    int64_t maxhit = 0;
    for (int64_t t : targets) maxhit = std::max(maxhit, offsets[t + 1] - offsets[t]);
    align(targets.data(), (int64_t)targets.size(), maxhit, row.data(), ops ? rows.data() : nullptr, ops ? ops_cap : 0);
    for (size_t k = 0; k < targets.size(); ++k) {
        aln[where[k]] = row[k];
        if (ops && row[k].nops <= ops_cap) std::copy_n(rows.data() + k * (size_t)ops_cap, (size_t)row[k].nops, ops + where[k] * ops_cap);
    }
}

extern "C" {

const char* sw_last_error(void) { return swh::g_err.c_str(); }
const char* sw_version(void) { return "swhip 0.1 (gfx950)"; }

int sw_generate(int64_t cols, int64_t rows, uint32_t seed, char* a, char* b) {
    if (cols < 0 || rows < 0 || !a || !b) { swh::set_err("sw_generate: bad argument"); return SW_EINVAL; }
    swh::GlibcRand rng(seed);
    // generate() runs after m++, n++ (serial_smithW.c:91-92,129): cols+1 draws, then rows+1
    for (int64_t i = 0; i <= cols; ++i) a[i] = swh::letter(rng.next() % 4);
    for (int64_t i = 0; i <= rows; ++i) b[i] = swh::letter(rng.next() % 4);
    return SW_OK;
}

int64_t sw_nelement(int64_t i, int64_t m, int64_t n) {  // omp_smithW.c:260-275
    const int64_t lo = m < n ? m : n, hi = m < n ? n : m;
    if (i < lo) return i;
    if (i < hi) return lo - 1;
    return 2 * lo - i + (hi - lo) - 2;
}

void sw_first_diag_element(int64_t i, int64_t m, int64_t n, int64_t* si, int64_t* sj) {  // omp_smithW.c:282-291
    (void)m;
    const bool left_edge = i < n;
    if (si) *si = left_edge ? i : n - 1;
    if (sj) *sj = left_edge ? 1 : i - n + 2;
}

int sw_traceback_host_ex(void* P, int p_elem_bytes, int64_t cols, int64_t rows, int64_t max_pos, int64_t* path,
                         int64_t path_cap, int64_t* path_len) {
    const int64_t m = cols + 1;
    if (!P || cols < 0 || rows < 0 || max_pos < 0 || max_pos >= m * (rows + 1) || (p_elem_bytes != 4 && p_elem_bytes != 1)) {
        swh::set_err("sw_traceback_host: bad argument");
        return SW_EINVAL;
    }
    const int64_t len = p_elem_bytes == 4 ? traceback_t((int32_t*)P, m, max_pos, path, path_cap)
                                          : traceback_t((signed char*)P, m, max_pos, path, path_cap);
    if (path_len) *path_len = len;
    return SW_OK;
}
int sw_traceback_host(int32_t* P, int64_t cols, int64_t rows, int64_t max_pos, int64_t* path,
                      int64_t path_cap, int64_t* path_len) {
    return sw_traceback_host_ex(P, 4, cols, rows, max_pos, path, path_cap, path_len);
}

// Host fill for problems too small to be worth a launch (sw_align_auto): the reference recurrence itself, row-major
// (serial_smithW.c:141-145, 187-244).  Product code -- the oracle under oracle/ is test infrastructure and is never used here.
int sw_fill_cpu(const char* a, int64_t cols, const char* b, int64_t rows, const sw_scores* scores, int32_t* H, int32_t* P, sw_result* result) {
    static const sw_scores kDefault = {3, -3, -2};
    const sw_scores* sc = scores ? scores : &kDefault;
    if (cols < 0 || rows < 0 || !H || !P || !result || (cols > 0 && !a) || (rows > 0 && !b)) { swh::set_err("sw_fill_cpu: bad argument"); return SW_EINVAL; }
    const int64_t m = cols + 1;
    int64_t best_pos = 0; int32_t best = 0;
    for (int64_t j = 0; j < m; ++j) { H[j] = 0; P[j] = 0; }
    for (int64_t i = 1; i <= rows; ++i) {
        int32_t* h = H + i * m; const int32_t* hu = h - m; int32_t* p = P + i * m;
        h[0] = 0; p[0] = 0;
        const char bi = b[i - 1];
        for (int64_t j = 1; j < m; ++j) {
            const int32_t diag = hu[j - 1] + (a[j - 1] == bi ? sc->match : sc->mismatch), up = hu[j] + sc->gap, left = h[j - 1] + sc->gap;
            int32_t mx = 0, pr = SW_NONE;
            if (diag > mx) { mx = diag; pr = SW_DIAGONAL; }
            if (up > mx) { mx = up; pr = SW_UP; }
            if (left > mx) { mx = left; pr = SW_LEFT; }
            h[j] = mx; p[j] = pr;
            if (mx > best) { best = mx; best_pos = i * m + j; }
        }
    }
    result->max_pos = best_pos; result->max_score = best; result->path_len = 0;
    return SW_OK;
}

// FASTA reader: the step before the path when the input is a real sequence instead of generate()
// (SURVEY.md 8f-1).  '>' starts a record, ';' lines are comments, white space is dropped, letters are
// upper-cased; a file without any '>' line is one record.
int sw_read_fasta(const char* path, int64_t record, char* seq, int64_t cap, int64_t* len) {
    if (!path || record < 0 || !len || (seq && cap < 0)) { swh::set_err("sw_read_fasta: bad argument"); return SW_EINVAL; }
    FILE* f = fopen(path, "rb");
    if (!f) { swh::set_err("sw_read_fasta: cannot open %s", path); return SW_EINVAL; }
    int64_t cur = -1, n = 0;       // cur: index of the record being read (-1: before the first header)
    bool at_line_start = true, skip_line = false, found = false;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) {
        for (size_t i = 0; i < got; ++i) {
            const unsigned char ch = (unsigned char)buf[i];
            if (ch == '\n' || ch == '\r') { at_line_start = true; skip_line = false; continue; }
            if (at_line_start) {
                at_line_start = false;
                if (ch == '>') { ++cur; skip_line = true; if (cur == record) found = true; continue; }
                if (ch == ';') { skip_line = true; continue; }
                if (cur < 0) { cur = 0; if (record == 0) found = true; }   // headerless file: a single record
            }
            if (skip_line || cur != record || ch == ' ' || ch == '\t') continue;
            if (seq && n < cap) seq[n] = (char)((ch >= 'a' && ch <= 'z') ? ch - 32 : ch);
            ++n;
        }
        if (cur > record) break;
    }
    fclose(f);
    if (!found) { swh::set_err("sw_read_fasta: %s has no record %lld", path, (long long)record); return SW_EINVAL; }
    *len = n;
    return SW_OK;
}

// All records in one pass (the state machine of sw_read_fasta, every record kept): the database side of sw_search_device.
int sw_read_fasta_db(const char* path, char* seq, int64_t seq_cap, int64_t* offsets, int64_t offsets_cap, int64_t* nrecords, int64_t* total_len) {
    if (!path || !nrecords || !total_len || (seq && (seq_cap < 0 || !offsets || offsets_cap < 1))) {
        swh::set_err("sw_read_fasta_db: bad argument");
        return SW_EINVAL;
    }
    FILE* f = fopen(path, "rb");
    if (!f) { swh::set_err("sw_read_fasta_db: cannot open %s", path); return SW_EINVAL; }
    int64_t cur = -1, n = 0;       // cur: index of the record being read (-1: before the first header)
    bool at_line_start = true, skip_line = false, overflow = false;
    auto start_record = [&]() {    // record cur + 1 begins at byte n
        ++cur;
        if (seq) { if (cur < offsets_cap) offsets[cur] = n; else overflow = true; }
    };
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) {
        for (size_t i = 0; i < got; ++i) {
            const unsigned char ch = (unsigned char)buf[i];
            if (ch == '\n' || ch == '\r') { at_line_start = true; skip_line = false; continue; }
            if (at_line_start) {
                at_line_start = false;
                if (ch == '>') { start_record(); skip_line = true; continue; }
                if (ch == ';') { skip_line = true; continue; }
                if (cur < 0) start_record();   // headerless file: a single record
            }
            if (skip_line || ch == ' ' || ch == '\t') continue;
            if (seq) { if (n < seq_cap) seq[n] = (char)((ch >= 'a' && ch <= 'z') ? ch - 32 : ch); else overflow = true; }
            ++n;
        }
    }
    const bool err = ferror(f) != 0;
    fclose(f);
    if (err) { swh::set_err("sw_read_fasta_db: read error on %s", path); return SW_EINVAL; }
    *nrecords = cur + 1;
    *total_len = n;
    if (seq) {
        if (cur + 1 < offsets_cap) offsets[cur + 1] = n; else overflow = true;
        if (overflow) { swh::set_err("sw_read_fasta_db: buffers too small (%lld bytes, %lld records)", (long long)n, (long long)(cur + 1)); return SW_EINVAL; }
    }
    return SW_OK;
}

// ---- substitution matrices
void sw_submat_match(int match, int mismatch, sw_submat* out) {
    if (!out) return;
    const int8_t m = (int8_t)std::clamp(match, -128, 127), x = (int8_t)std::clamp(mismatch, -128, 127);
    for (int a = 0; a < 256; ++a)
        for (int b = 0; b < 256; ++b) out->s[a][b] = a == b ? m : x;
}

int sw_submat_from_letters(const char* letters, int n, const int8_t* scores, int other, sw_submat* out) {
    if (!letters || !scores || !out || n < 1 || n > 256) { swh::set_err("sw_submat_from_letters: bad argument"); return SW_EINVAL; }
    if (other < -128 || other > 127) { swh::set_err("sw_submat_from_letters: other = %d does not fit int8", other); return SW_EINVAL; }
    int at[256];
    std::fill(at, at + 256, -1);
    for (int i = 0; i < n; ++i) {
        const int b = (unsigned char)letters[i];
        if (at[b] >= 0) { swh::set_err("sw_submat_from_letters: letter 0x%02x is listed twice", b); return SW_EINVAL; }
        at[b] = i;
    }
    for (int a = 0; a < 256; ++a)
        for (int b = 0; b < 256; ++b) out->s[a][b] = (at[a] >= 0 && at[b] >= 0) ? scores[at[a] * n + at[b]] : (int8_t)other;
    return SW_OK;
}

// NCBI text format: '#' comments, a header line of letters, rows of a letter and n integers.
int sw_read_submat(const char* path, sw_submat* out) {
    if (!path || !out) { swh::set_err("sw_read_submat: bad argument"); return SW_EINVAL; }
    FILE* f = fopen(path, "rb");
    if (!f) { swh::set_err("sw_read_submat: cannot open %s", path); return SW_EINVAL; }
    std::string text;
    char buf[1 << 14];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    const bool err = ferror(f) != 0;
    fclose(f);
    if (err) { swh::set_err("sw_read_submat: read error on %s", path); return SW_EINVAL; }
    auto upper = [](unsigned char ch) { return (unsigned char)((ch >= 'a' && ch <= 'z') ? ch - 32 : ch); };
    std::string letters;             // the header's letters, in order
    std::string row_letters;         // the letter of every row read
    std::vector<int8_t> scores;      // rows read x n
    int lineno = 0, lo = 127;
    for (size_t pos = 0; pos < text.size();) {
        size_t end = text.find_first_of("\r\n", pos);
        if (end == std::string::npos) end = text.size();
        std::vector<std::string> tok;
        for (size_t i = pos; i < end;) {
            while (i < end && (text[i] == ' ' || text[i] == '\t')) ++i;
            size_t j = i;
            while (j < end && text[j] != ' ' && text[j] != '\t') ++j;
            if (j > i) tok.push_back(text.substr(i, j - i));
            i = j;
        }
        pos = end + 1;
        ++lineno;
        if (tok.empty() || tok[0][0] == '#') continue;
        if (letters.empty()) {       // the header
            for (const std::string& t : tok) {
                if (t.size() != 1) { swh::set_err("sw_read_submat: %s line %d: header entry '%s' is not one letter", path, lineno, t.c_str()); return SW_EINVAL; }
                const char ch = (char)upper((unsigned char)t[0]);
                if (letters.find(ch) != std::string::npos) { swh::set_err("sw_read_submat: %s line %d: letter '%c' is listed twice", path, lineno, ch); return SW_EINVAL; }
                letters.push_back(ch);
            }
            continue;
        }
        const size_t n = letters.size();
        if (tok[0].size() != 1 || letters.find((char)upper((unsigned char)tok[0][0])) == std::string::npos) {
            swh::set_err("sw_read_submat: %s line %d: row '%s' names no letter of the header", path, lineno, tok[0].c_str());
            return SW_EINVAL;
        }
        const char rl = (char)upper((unsigned char)tok[0][0]);
        if (row_letters.find(rl) != std::string::npos) { swh::set_err("sw_read_submat: %s line %d: row '%c' appears twice", path, lineno, rl); return SW_EINVAL; }
        if (tok.size() != n + 1) {
            swh::set_err("sw_read_submat: %s line %d: %zu entries in row '%c', the header has %zu letters", path, lineno, tok.size() - 1, rl, n);
            return SW_EINVAL;
        }
        for (size_t i = 1; i <= n; ++i) {
            char* endp = nullptr;
            const long v = strtol(tok[i].c_str(), &endp, 10);
            if (endp == tok[i].c_str() || *endp) { swh::set_err("sw_read_submat: %s line %d: '%s' is not an integer", path, lineno, tok[i].c_str()); return SW_EINVAL; }
            if (v < -128 || v > 127) { swh::set_err("sw_read_submat: %s line %d: entry %ld does not fit int8", path, lineno, v); return SW_EINVAL; }
            scores.push_back((int8_t)v);
            lo = std::min(lo, (int)v);
        }
        row_letters.push_back(rl);
    }
    const size_t n = letters.size();
    if (n == 0) { swh::set_err("sw_read_submat: %s has no header line", path); return SW_EINVAL; }
    if (row_letters.size() != n) { swh::set_err("sw_read_submat: %s has %zu rows for %zu letters", path, row_letters.size(), n); return SW_EINVAL; }
    // rows may come in any order: bring them into the header's
    std::vector<int8_t> ordered(n * n);
    for (size_t r = 0; r < n; ++r) {
        const size_t at = letters.find(row_letters[r]);
        std::copy(scores.begin() + (ptrdiff_t)(r * n), scores.begin() + (ptrdiff_t)((r + 1) * n), ordered.begin() + (ptrdiff_t)(at * n));
    }
    return sw_submat_from_letters(letters.data(), (int)n, ordered.data(), lo, out);
}

// The CPU leg of the affine search: Gotoh's recurrence row by row with one row of H and E kept (include/swhip.h states it); -inf is a
// value no sum can reach from below (every E, F inside the matrix is at least gap_open + gap_extend >= -2^24).
int sw_search_affine_host(const char* query, int64_t qlen, const char* db, const int64_t* offsets, int64_t ntargets, const sw_affine* scoring,
                          sw_result* results) {
    if (!query || !db || !offsets || !results || !scoring || ntargets < 0) { swh::set_err("sw_search_affine_host: NULL pointer or negative target count"); return SW_EINVAL; }
    int64_t maxlen = 0, nonempty = 0;
    if (int rc = swh::check_search_affine("sw_search_affine_host", qlen, offsets, ntargets, scoring, &maxlen, &nonempty)) return rc;
    const unsigned char* q = (const unsigned char*)query;
    const sw_submat* sub = scoring->sub;
    search_targets([=](int64_t j, unsigned char y) { return (int64_t)sub->s[q[j - 1]][y]; }, qlen, db, offsets, ntargets, scoring->gap_open, scoring->gap_extend,
                   results);
    return SW_OK;
}

// The CPU leg of sw_db_search_affine: sw_search_affine_host query after query into the query-major results.  Everything is checked
// before the first query runs, so an error leaves `results` untouched.
int sw_search_affine_multi_host(const char* queries, const int64_t* qoffsets, int64_t nqueries, const char* db, const int64_t* offsets, int64_t ntargets,
                                const sw_affine* scoring, sw_result* results) {
    if (!queries || !qoffsets || !db || !offsets || !results || !scoring || ntargets < 0) {
        swh::set_err("sw_search_affine_multi_host: NULL pointer or negative target count");
        return SW_EINVAL;
    }
    int64_t maxlen = 0, nonempty = 0, maxq = 0;
    if (int rc = swh::check_targets("sw_search_affine_multi_host", 1, offsets, ntargets, &maxlen, &nonempty)) return rc;
    if (int rc = swh::check_search_multi("sw_search_affine_multi_host", qoffsets, nqueries, maxlen, scoring, &maxq)) return rc;
    for (int64_t q = 0; q < nqueries; ++q)
        if (int rc = sw_search_affine_host(queries + qoffsets[q], qoffsets[q + 1] - qoffsets[q], db, offsets, ntargets, scoring, results + q * ntargets)) return rc;
    return SW_OK;
}

// The CPU leg of sw_db_search_affine_pairs: sw_search_affine_host for every listed pair, the query against that one target.  Everything
// is checked before the first pair, so an error leaves `results` untouched; an entry that names no query or no target gives {0, 0, 0}.
int sw_search_affine_pairs_host(const char* queries, const int64_t* qoffsets, int64_t nqueries, const char* db, const int64_t* offsets, int64_t ntargets,
                                const sw_affine* scoring, const sw_pair* pairs, int64_t npairs, sw_result* results) {
    if (!queries || !qoffsets || !db || !offsets || !scoring || ntargets < 0) {
        swh::set_err("sw_search_affine_pairs_host: NULL pointer or negative target count");
        return SW_EINVAL;
    }
    int64_t maxlen = 0, nonempty = 0, maxq = 0;
    if (int rc = swh::check_targets("sw_search_affine_pairs_host", 1, offsets, ntargets, &maxlen, &nonempty)) return rc;
    if (int rc = swh::check_search_multi("sw_search_affine_pairs_host", qoffsets, nqueries, maxlen, scoring, &maxq)) return rc;
    if (npairs < 0) { swh::set_err("sw_search_affine_pairs_host: negative pair count"); return SW_EINVAL; }
    if (npairs > 0 && (!pairs || !results)) { swh::set_err("sw_search_affine_pairs_host: NULL pairs or results with %lld pairs", (long long)npairs); return SW_EINVAL; }
    for (int64_t p = 0; p < npairs; ++p) {
        const uint64_t q = (uint64_t)pairs[p].query, k = (uint64_t)pairs[p].target;
        results[p] = sw_result{0, 0, 0};
        if (q >= (uint64_t)nqueries || k >= (uint64_t)ntargets) continue;
        if (int rc = sw_search_affine_host(queries + qoffsets[q], qoffsets[q + 1] - qoffsets[q], db, offsets + k, 1, scoring, results + p)) return rc;
    }
    return SW_OK;
}

// The CPU leg of sw_db_prefilter_ungapped: D[i][j] = max(0, D[i-1][j-1] + s) over one rolling row per pair, the list in ascending
// (query, target) order.  Everything is checked before the first pair, so an error leaves the outputs untouched.
int sw_prefilter_ungapped_host(const char* queries, const int64_t* qoffsets, int64_t nqueries, const char* db, const int64_t* offsets, int64_t ntargets,
                               const sw_submat* sub, int64_t min_score, sw_pair* pairs, int64_t pairs_cap, int64_t* npairs, int32_t* scores) {
    const char* who = "sw_prefilter_ungapped_host";
    if (!queries || !qoffsets || !db || !offsets || !sub || ntargets < 0) { swh::set_err("%s: NULL pointer or negative target count", who); return SW_EINVAL; }
    int64_t maxlen = 0, nonempty = 0, maxq = 0;
    if (int rc = swh::check_targets(who, 1, offsets, ntargets, &maxlen, &nonempty)) return rc;
    const sw_affine sc = {sub, 0, 0};
    if (int rc = swh::check_search_multi(who, qoffsets, nqueries, maxlen, &sc, &maxq)) return rc;
    if (int rc = swh::check_prefilter(who, min_score, pairs, pairs_cap, npairs, scores)) return rc;
    if (pairs) memset(pairs, 0xFF, (size_t)pairs_cap * sizeof(sw_pair));   // {-1, -1} behind the written entries
    int64_t n = 0;
    std::vector<int32_t> row((size_t)maxq + 1);
    for (int64_t q = 0; q < nqueries; ++q) {
        const unsigned char* qq = (const unsigned char*)queries + qoffsets[q];
        const int64_t qlen = qoffsets[q + 1] - qoffsets[q];
        for (int64_t k = 0; k < ntargets; ++k) {
            const unsigned char* t = (const unsigned char*)db + offsets[k];
            const int64_t len = offsets[k + 1] - offsets[k];
            std::fill(row.begin(), row.begin() + qlen + 1, 0);
            int32_t best = 0;
            for (int64_t i = 1; i <= len; ++i)
                for (int64_t c = qlen; c >= 1; --c) {   // from the highest column down: row[c - 1] still holds row i - 1
                    row[(size_t)c] = std::max<int32_t>(0, row[(size_t)c - 1] + sub->s[qq[c - 1]][t[i - 1]]);
                    best = std::max(best, row[(size_t)c]);
                }
            if (scores) scores[q * ntargets + k] = best;
            if (len > 0 && best >= min_score) {
                if (n < pairs_cap) pairs[n] = sw_pair{q, k};
                ++n;
            }
        }
    }
    if (npairs) *npairs = n;
    return SW_OK;
}

// The CPU leg of sw_db_search_affine_top: sw_search_affine_host query after query into one row, a sort of the qualifying targets by the
// rank order (max_score descending, then target ascending), the first `top` of them and the {-1, 0, 0} tail.
int sw_search_affine_multi_top_host(const char* queries, const int64_t* qoffsets, int64_t nqueries, const char* db, const int64_t* offsets, int64_t ntargets,
                                    const sw_affine* scoring, int64_t top, int64_t min_score, sw_hit* hits, int64_t* nhits) {
    if (!queries || !qoffsets || !db || !offsets || !scoring || ntargets < 0) {
        swh::set_err("sw_search_affine_multi_top_host: NULL pointer or negative target count");
        return SW_EINVAL;
    }
    int64_t maxlen = 0, nonempty = 0, maxq = 0;
    if (int rc = swh::check_targets("sw_search_affine_multi_top_host", 1, offsets, ntargets, &maxlen, &nonempty)) return rc;
    if (int rc = swh::check_search_multi("sw_search_affine_multi_top_host", qoffsets, nqueries, maxlen, scoring, &maxq)) return rc;
    if (top < 1 || top > SW_TOP_MAX) { swh::set_err("sw_search_affine_multi_top_host: top = %lld is out of range 1..%d", (long long)top, SW_TOP_MAX); return SW_EINVAL; }
    if (!hits || !nhits) { swh::set_err("sw_search_affine_multi_top_host: NULL hits or nhits"); return SW_EINVAL; }
    std::vector<sw_result> row((size_t)ntargets);
    std::vector<int64_t> order;
    for (int64_t q = 0; q < nqueries; ++q) {
        if (ntargets > 0)
            if (int rc = sw_search_affine_host(queries + qoffsets[q], qoffsets[q + 1] - qoffsets[q], db, offsets, ntargets, scoring, row.data())) return rc;
        order.clear();
        for (int64_t k = 0; k < ntargets; ++k)
            if (row[(size_t)k].max_score >= min_score) order.push_back(k);
        std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return row[(size_t)x].max_score > row[(size_t)y].max_score; });
        const int64_t n = std::min<int64_t>(top, (int64_t)order.size());
        for (int64_t i = 0; i < top; ++i)
            hits[q * top + i] = i < n ? sw_hit{order[(size_t)i], row[(size_t)order[(size_t)i]].max_pos, row[(size_t)order[(size_t)i]].max_score} : sw_hit{-1, 0, 0};
        nhits[q] = n;
    }
    return SW_OK;
}

// The CPU leg of sw_top_hits_pairs_device: the qualifying entries in a stable sort by (query, max_score modulo 2^24 descending, target) --
// stable, so entries equal in all three stay in list order --, then per query the first `top` of them and the {-1, 0, 0} tail.
int sw_top_hits_pairs_host(const sw_pair* pairs, const sw_result* results, int64_t npairs, int64_t nqueries, int64_t ntargets, int64_t top, int64_t min_score,
                           sw_hit* hits, int64_t* nhits) {
    const char* who = "sw_top_hits_pairs_host";
    if (!hits || !nhits) { swh::set_err("%s: NULL hits or nhits", who); return SW_EINVAL; }
    if (npairs < 0 || npairs >= (1ll << 31)) { swh::set_err("%s: npairs = %lld is negative or not below 2^31", who, (long long)npairs); return SW_EINVAL; }
    if (npairs > 0 && (!pairs || !results)) { swh::set_err("%s: NULL pairs or results with %lld pairs", who, (long long)npairs); return SW_EINVAL; }
    if (nqueries < 0) { swh::set_err("%s: negative query count", who); return SW_EINVAL; }
    if (ntargets < 0 || ntargets >= (1ll << 31)) { swh::set_err("%s: ntargets = %lld is negative or not below 2^31", who, (long long)ntargets); return SW_EINVAL; }
    if (top < 1 || top > SW_TOP_MAX) { swh::set_err("%s: top = %lld is out of range 1..%d", who, (long long)top, SW_TOP_MAX); return SW_EINVAL; }
    std::vector<int64_t> order;
    for (int64_t p = 0; p < npairs; ++p)
        if ((uint64_t)pairs[p].query < (uint64_t)nqueries && (uint64_t)pairs[p].target < (uint64_t)ntargets && results[p].max_score >= min_score) order.push_back(p);
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
        if (pairs[x].query != pairs[y].query) return pairs[x].query < pairs[y].query;
        const int64_t sx = results[x].max_score & 0xFFFFFF, sy = results[y].max_score & 0xFFFFFF;
        if (sx != sy) return sx > sy;
        return pairs[x].target < pairs[y].target;
    });
    size_t at = 0;
    for (int64_t q = 0; q < nqueries; ++q) {
        int64_t n = 0;
        for (; at < order.size() && pairs[order[at]].query == q; ++at, ++n)
            if (n < top) hits[q * top + n] = sw_hit{pairs[order[at]].target, results[order[at]].max_pos, results[order[at]].max_score};
        n = std::min(n, top);
        for (int64_t i = n; i < top; ++i) hits[q * top + i] = sw_hit{-1, 0, 0};
        nhits[q] = n;
    }
    return SW_OK;
}

// The CPU leg of sw_align_affine_device: align_targets (above) with the table's entry as the score of a cell.
int sw_align_affine_host(const char* query, int64_t qlen, const char* db, const int64_t* offsets, int64_t ntargets, const int64_t* hits, int64_t nhits,
                         const sw_affine* scoring, sw_alignment* aln, char* ops, int64_t ops_cap) {
    if (!query || !db || !offsets || !scoring || ntargets < 0) { swh::set_err("sw_align_affine_host: NULL pointer or negative target count"); return SW_EINVAL; }
    int64_t maxlen = 0, nonempty = 0, maxhit = 0;
    if (int rc = swh::check_search_affine("sw_align_affine_host", qlen, offsets, ntargets, scoring, &maxlen, &nonempty)) return rc;
    if (int rc = swh::check_align_affine("sw_align_affine_host", offsets, ntargets, hits, nhits, aln, ops, ops_cap, &maxhit)) return rc;
    const unsigned char* q = (const unsigned char*)query;
    const sw_submat* sub = scoring->sub;
    align_targets([=](int64_t j, unsigned char y) { return (int64_t)sub->s[q[j - 1]][y]; }, qlen, db, offsets, hits, nhits, maxhit, scoring->gap_open,
                  scoring->gap_extend, aln, ops, ops_cap);
    return SW_OK;
}

// The CPU leg of sw_db_align_affine_hits: per query the used entries of its row whose target lies inside the database go through
// align_targets in one call, into rows of their own, and are copied to their places (align_hit_row); every other entry is all zeros
// and its ops row is left alone.  Everything is checked before the first alignment.
int sw_align_affine_hits_host(const char* queries, const int64_t* qoffsets, int64_t nqueries, const char* db, const int64_t* offsets, int64_t ntargets,
                              const sw_affine* scoring, const sw_hit* hits, const int64_t* nhits, int64_t top, sw_alignment* aln, char* ops, int64_t ops_cap) {
    if (!queries || !qoffsets || !db || !offsets || !scoring || ntargets < 0) {
        swh::set_err("sw_align_affine_hits_host: NULL pointer or negative target count");
        return SW_EINVAL;
    }
    int64_t maxlen = 0, nonempty = 0, maxq = 0;
    if (int rc = swh::check_targets("sw_align_affine_hits_host", 1, offsets, ntargets, &maxlen, &nonempty)) return rc;
    if (int rc = swh::check_search_multi("sw_align_affine_hits_host", qoffsets, nqueries, maxlen, scoring, &maxq)) return rc;
    if (int rc = swh::check_align_hits("sw_align_affine_hits_host", top, hits, aln, ops, ops_cap)) return rc;
    const sw_submat* sub = scoring->sub;
    for (int64_t q = 0; q < nqueries; ++q) {
        const unsigned char* qq = (const unsigned char*)queries + qoffsets[q];
        const int64_t qlen = qoffsets[q + 1] - qoffsets[q];
        align_hit_row([&](const int64_t* targets, int64_t n, int64_t maxhit, sw_alignment* row, char* rows, int64_t cap) {
            align_targets([=](int64_t j, unsigned char y) { return (int64_t)sub->s[qq[j - 1]][y]; }, qlen, db, offsets, targets, n, maxhit, scoring->gap_open,
                          scoring->gap_extend, row, rows, cap);
        }, q, offsets, ntargets, hits, nhits, top, aln, ops, ops_cap);
    }
    return SW_OK;
}

// ---- position-specific scoring matrices (include/swhip.h)

// The CPU leg of sw_db_search_pssm: search_targets query after query into the query-major results, the score of a cell taken from the
// matrix.  Everything is checked before the first query runs, so an error leaves `results` untouched.
int sw_search_pssm_multi_host(const int8_t* pssm, const int64_t* qoffsets, int64_t nqueries, const char* db, const int64_t* offsets, int64_t ntargets,
                              const sw_pssm_scoring* scoring, sw_result* results) {
    const char* who = "sw_search_pssm_multi_host";
    if (!pssm || !qoffsets || !db || !offsets || !results || !scoring || ntargets < 0) { swh::set_err("%s: NULL pointer or negative target count", who); return SW_EINVAL; }
    int64_t maxlen = 0, nonempty = 0, maxq = 0;
    unsigned char code[256];
    if (int rc = swh::check_targets(who, 1, offsets, ntargets, &maxlen, &nonempty)) return rc;
    if (int rc = swh::check_search_pssm(who, qoffsets, nqueries, maxlen, scoring, &maxq, code)) return rc;
    for (int64_t q = 0; q < nqueries; ++q)
        search_targets(PssmScore{pssm + qoffsets[q] * scoring->nletters, code, scoring->nletters, scoring->other, scoring->smax}, qoffsets[q + 1] - qoffsets[q], db,
                       offsets, ntargets, scoring->gap_open, scoring->gap_extend, results + q * ntargets);
    return SW_OK;
}

// The CPU leg of sw_db_align_pssm_hits: sw_align_affine_hits_host with the score of a cell taken from the matrix.
int sw_align_pssm_hits_host(const int8_t* pssm, const int64_t* qoffsets, int64_t nqueries, const char* db, const int64_t* offsets, int64_t ntargets,
                            const sw_pssm_scoring* scoring, const sw_hit* hits, const int64_t* nhits, int64_t top, sw_alignment* aln, char* ops, int64_t ops_cap) {
    const char* who = "sw_align_pssm_hits_host";
    if (!pssm || !qoffsets || !db || !offsets || !scoring || ntargets < 0) { swh::set_err("%s: NULL pointer or negative target count", who); return SW_EINVAL; }
    int64_t maxlen = 0, nonempty = 0, maxq = 0;
    unsigned char code[256];
    if (int rc = swh::check_targets(who, 1, offsets, ntargets, &maxlen, &nonempty)) return rc;
    if (int rc = swh::check_search_pssm(who, qoffsets, nqueries, maxlen, scoring, &maxq, code)) return rc;
    if (int rc = swh::check_align_hits(who, top, hits, aln, ops, ops_cap)) return rc;
    for (int64_t q = 0; q < nqueries; ++q) {
        const PssmScore s{pssm + qoffsets[q] * scoring->nletters, code, scoring->nletters, scoring->other, scoring->smax};
        const int64_t qlen = qoffsets[q + 1] - qoffsets[q];
        align_hit_row([&](const int64_t* targets, int64_t n, int64_t maxhit, sw_alignment* row, char* rows, int64_t cap) {
            align_targets(s, qlen, db, offsets, targets, n, maxhit, scoring->gap_open, scoring->gap_extend, row, rows, cap);
        }, q, offsets, ntargets, hits, nhits, top, aln, ops, ops_cap);
    }
    return SW_OK;
}

// The PSSM that reproduces sequence queries under a table: column (q, j) holds the table's row of letter q[j] at the given letters.
int sw_pssm_from_queries(const char* queries, const int64_t* qoffsets, int64_t nqueries, const sw_submat* sub, const char* letters, int32_t nletters,
                         int8_t* out) {
    const char* who = "sw_pssm_from_queries";
    if (!queries || !qoffsets || !sub || !letters || !out || nqueries < 0) { swh::set_err("%s: NULL pointer or negative query count", who); return SW_EINVAL; }
    if (nletters < 1 || nletters > 256) { swh::set_err("%s: nletters = %d is out of range 1..256", who, nletters); return SW_EINVAL; }
    if (qoffsets[0] < 0) { swh::set_err("%s: qoffsets[0] = %lld is negative", who, (long long)qoffsets[0]); return SW_EINVAL; }
    for (int64_t q = 0; q < nqueries; ++q)
        if (qoffsets[q + 1] < qoffsets[q]) { swh::set_err("%s: qoffsets decrease at query %lld", who, (long long)q); return SW_EINVAL; }
    for (int64_t g = qoffsets[0]; g < qoffsets[nqueries]; ++g) {
        const int8_t* row = sub->s[(unsigned char)queries[g]];
        int8_t* col = out + (g - qoffsets[0]) * nletters;
        for (int k = 0; k < nletters; ++k) col[k] = row[(unsigned char)letters[k]];
    }
    return SW_OK;
}

}  // extern "C"
