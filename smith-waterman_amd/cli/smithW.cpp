// smithW -- host driver with the reference's command line (serial_smithW.c:71-180, omp_smithW.c:87-253):
//   smithW                  built-in 8x9 example (serial_smithW.c:105-125) + its known-answer checks
//   smithW <cols> <rows>    random DNA pair from the reference generator (seed 1 == serial_smithW.c)
//   smithW --fasta A.fa B.fa   real sequences: a = first record of A.fa (columns), b = first record of B.fa (rows)
//   smithW --search Q.fa DB.fa [--top K]   database search: a = record --record-a of Q.fa against every record of DB.fa (sw_search_device);
//                              prints the K best hits (default 10): rank, record, score, target_end, query_end (max_pos = target_end*(qlen+1)+query_end)
//     ... --matrix FILE --gap-open O --gap-extend E   substitution matrix (NCBI text format) and affine gaps (sw_search_affine_device): a gap of k
//                              letters scores O + k E; without --matrix the table is match / mismatch of --scores (signed bytes),
//                              without --gap-extend E = the gap of --scores; --gap-extend alone (O = 0) is the linear search with gap E
//     ... --all-queries       EVERY record of Q.fa through one prepared database handle and one call (sw_db_create / sw_db_search_affine): the
//                              hit block of --search once per query, each under a line "## query record <i> of <Q.fa>"; --top, --matrix,
//                              --gap-open, --gap-extend and --align (one sw_db_align_affine_hits call on the device hit table) as for one query.  The K best hits per
//                              query are selected on the device (sw_db_search_affine_top): only they are copied back
//     ... --min-score S       with --all-queries: only hits with a score of at least S are printed (fewer than K where fewer qualify)
//     ... --search-lanes 16|32  with --all-queries (and with --pssm): option "search_lanes" -- 16 runs two targets per wave on packed 16-bit lanes for
//                              every query whose scores fit them (include/swhip.h has the rule), 32 (the default) one target per wave; the output is
//                              the same byte for byte.  Not with --prefilter, --prefilter-hits or --pairs
//     ... --prefilter-hits S  with --all-queries: the blocks of --all-queries (--top, --min-score, --align as there), the hits selected among the pairs whose
//                              ungapped score is at least S: pre-filter, rescoring of the passing pairs and selection from that list in one call
//                              (sw_db_search_affine_top_prefiltered), a fraction of the full search's time; the elapsed line says how many pairs passed.
//                              More passing pairs than the list holds ("search_results_mib") is an error: raise S.  Not with --prefilter or --pairs.
//     ... --prefilter S       with --all-queries: the ungapped pre-filter (sw_db_prefilter_ungapped) and then the affine search of the pairs whose ungapped
//                              score reaches S (sw_db_search_affine_pairs on the filter's device list): one handle, one read-back; the passing pairs in
//                              ascending (query, target) order in the line format of --pairs with " ungapped=<U>" appended; S >= 1; not with --top,
//                              --min-score, --align, --pairs
//     ... --pairs FILE        a LIST of (query, target) pairs through one prepared handle and one call (sw_db_search_affine_pairs): FILE is text, one pair
//                              per line, "<query record> <target record>", 0-based; '#' lines and blank lines are skipped.  One line per pair in input
//                              order: query record, target record, the target's name, score, target_end, query_end (a pair outside the files: name "-",
//                              zeros).  --matrix, --gap-open, --gap-extend or --scores as for --all-queries; not with --all-queries, --top, --min-score, --align
//     ... --pairs-lanes 16|32  with --pairs or --prefilter-hits: option "search_pairs_lanes" -- 16 rescoring runs two listed pairs of a query per wave on
//                              packed 16-bit lanes for every query whose scores fit them (include/swhip.h has the rule), 32 (the default) one pair per
//                              wave; the printed lines are the same.  Nowhere else
//     ... --align             every printed hit is followed by its alignment (sw_align_affine_device; the canonical alignment of swhip.h), four lines:
//                                "align\t<q_begin>\t<q_end>\t<t_begin>\t<t_end>\t<nops>"   query [q_begin, q_end) against target [t_begin, t_end), 0-based, half open
//                                "Q <query letters, '-' where the target has letters of its own>"
//                                "  <'|' under equal letters, a space otherwise>"
//                                "T <target letters, '-' where the query has letters of its own>"
//                              on a linear search (no --matrix / --gap-open) the alignment is that of the table match / mismatch of --scores (signed
//                              bytes) with gap_open 0 and the gap of --scores: the reference's backtrack() path
//     ... --align-checkpoint  with --align: option "align_checkpoint" = 2 -- hits (with --all-queries: tables) whose whole direction matrices do not
//                              fit the workspace are aligned from checkpoint rows in bounded memory, in the same one call; the output is unchanged
//     ... --iterations N      with --all-queries or --pssm: N >= 1 rounds of search, alignment of the top hits and a new PSSM built from them on the device
//                              (sw_db_pssm_from_hits; --include-score S, default 1; --prior-weight W, default 10; --out-pssm PREFIX writes PREFIX.<query>.pssm);
//                              the hits and --align output are those of the last round; N = 1 is the search of today
//     ... --out-a3m PREFIX    with --all-queries or --pssm, --align, with or without --iterations: the query-anchored multiple alignment of the LAST round's
//                              aligned hits, built on the device (sw_db_msa_from_hits) and written per query to PREFIX.<query>.a3m (sw_write_a3m): for a
//                              sequence query its own record first (with --pssm there is NO query record: a matrix has no letters), then per hit whose
//                              score reaches --include-score ">name score=S q=b-e t=b-e ident=n/nmatch" and its A3M row -- one byte per query column,
//                              '-' where the hit has none, the target's inserted letters in lower case between them
//     ... --weight-hits P     with --iterations / --out-pssm: every round weights its aligned hits on the device before it builds the matrix
//                              (sw_db_pssm_hit_weights, Henikoff's position-based weights; per_hit = P within 1..65535, the round's --include-score):
//                              a family that fills the hit list no longer outvotes a distant homologue.  N[j] of the update then counts in units
//                              of P, so --prior-weight scales with it: --weight-hits 16 --prior-weight 160 is the balance of --prior-weight 10
//   smithW --search --pssm FILE DB.fa --gap-open O --gap-extend E [--top K] [--min-score S] [--align] [--search-lanes 16|32]
//                              the ONE query is a position-specific scoring matrix, PSI-BLAST's ASCII PSSM (sw_read_pssm), searched through a prepared
//                              handle (sw_db_search_pssm_top, sw_db_align_pssm_hits); the output is that of --all-queries for one record, the Q line of an
//                              alignment the matrix's consensus (per column the first letter with the largest entry)
// Extra flags: --seed N  --dump | --dump-labels (the header-row printers of omp_smithW.c)  --h64  --no-backtrack  --scores M X G  --record-a I  --record-b J
//   --gpus N | --devices 0,1,..   ONE matrix over several GPUs (row bands, sw_multi_*; an id may repeat)  --p8  int8 P
// The DP fill runs on the GPU through the C-ABI (include/swhip.h); stdout keeps the two
// "Elapsed time ..." lines the reference's run scripts grep for (readme.liao:12).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/swhip.h"

#define RESET "\033[0m"
#define BOLDRED "\033[1m\033[31m"

static double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
#define CHECK(call)                                                              \
    do {                                                                         \
        int rc_ = (call);                                                        \
        if (rc_ != SW_OK) {                                                      \
            fprintf(stderr, "smithW: %s -> %d: %s\n", #call, rc_, sw_last_error()); \
            return 1;                                                            \
        }                                                                        \
    } while (0)

// printMatrix / printPredecessorMatrix, serial_smithW.c:283-328
static void print_matrix(const std::vector<int32_t>& H, long long n, long long m) {
    for (long long i = 0; i < n; i++) {
        for (long long j = 0; j < m; j++) printf("%d\t", H[m * i + j]);
        printf("\n");
    }
}
static void print_pred(const std::vector<int32_t>& P, long long n, long long m) {
    for (long long i = 0; i < n; i++) {
        for (long long j = 0; j < m; j++) {
            const int v = P[m * i + j], av = v < 0 ? -v : v;
            const char* sym = av == SW_UP ? "↑ " : av == SW_LEFT ? "← " : av == SW_DIAGONAL ? "↖ " : "- ";
            if (v < 0) printf(BOLDRED "%s" RESET, sym); else printf("%s", sym);
        }
        printf("\n");
    }
}

// the labelled variants (sequence a as a header row, the letters of b in front of the rows), omp_smithW.c:426-483
static void print_matrix_labelled(const std::vector<int32_t>& H, long long n, long long m, const char* a, const char* b) {
    printf("-\t-\t");
    for (long long j = 0; j + 1 < m; j++) printf("%c\t", a[j]);
    printf("\n-\t");
    for (long long i = 0; i < n; i++) {
        if (i > 0) printf("%c\t", b[i - 1]);
        for (long long j = 0; j < m; j++) printf("%d\t", H[m * i + j]);
        printf("\n");
    }
}
static void print_pred_labelled(const std::vector<int32_t>& P, long long n, long long m, const char* a, const char* b) {
    printf("    ");
    for (long long j = 0; j + 1 < m; j++) printf("%c ", a[j]);
    printf("\n  ");
    for (long long i = 0; i < n; i++) {
        if (i > 0) printf("%c ", b[i - 1]);
        for (long long j = 0; j < m; j++) {
            const int v = P[m * i + j], av = v < 0 ? -v : v;
            const char* sym = av == SW_UP ? "↑ " : av == SW_LEFT ? "← " : av == SW_DIAGONAL ? "↖ " : "- ";
            if (v < 0) printf(BOLDRED "%s" RESET, sym); else printf("%s", sym);
        }
        printf("\n");
    }
}

// --search: one query record against every record of a FASTA database on the GPU, the best `top` hits by score (ties: lower record first)
// (`on`: --matrix or --gap-open was given, the search goes through the affine kernel; --gap-extend alone is a linear gap: sw_search_device)
struct AffineArgs { bool on = false; const char* matrix = nullptr; bool has_open = false, has_extend = false; int open = 0, extend = 0; };
// a whole decimal integer or nothing: "-x", "" and "3k" are errors, not 0 or 3
static bool parse_int(const char* flag, const char* text, int* out) {
    char* end = nullptr;
    const long v = strtol(text, &end, 10);
    if (end == text || *end || v < -(1l << 30) || v > (1l << 30)) { fprintf(stderr, "smithW: %s needs an integer, got \"%s\"\n", flag, text); return false; }
    *out = (int)v;
    return true;
}
// The best K targets of one row of results in rank order -- by score, ties: lower record first --, those below min_score left out.
static std::vector<sw_hit> rank_hits(const sw_result* res, int64_t nrec, long long K, long long min_score) {
    std::vector<int64_t> order;
    for (int64_t k = 0; k < nrec; ++k)
        if (res[(size_t)k].max_score >= min_score) order.push_back(k);
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return res[(size_t)x].max_score > res[(size_t)y].max_score; });
    order.resize((size_t)std::max(0ll, std::min(K, (long long)order.size())));
    std::vector<sw_hit> hits;
    for (int64_t k : order) hits.push_back(sw_hit{k, res[(size_t)k].max_pos, res[(size_t)k].max_score});
    return hits;
}

// The hit block of one query: the header line, its K hits in rank order and, with `align`, every hit's alignment: the K hits re-filled
// with directions and walked on the device here, or -- `done` given -- taken from the row of a call that aligned every query's hits
// (done_ops: that row's ops, done_cap bytes per hit).
static int print_hits(sw_ctx* ctx, const char* q, int64_t qlen, const void* d_q, const std::vector<char>& db, const void* d_db, const std::vector<int64_t>& offs,
                      int64_t nrec, int64_t total, const sw_hit* hits, long long K, bool align, const sw_affine& aff, const sw_alignment* done = nullptr,
                      const char* done_ops = nullptr, int64_t done_cap = 0) {
    std::vector<int64_t> order((size_t)K);
    for (long long i = 0; i < K; ++i) order[(size_t)i] = hits[i].target;
    // --align: the K hits re-filled with directions and walked on the device, ops of at most query + longest hit letters each
    std::vector<sw_alignment> aln((size_t)(align ? K : 0));
    std::vector<char> ops;
    int64_t ops_cap = 0;
    if (align && K > 0 && done) {
        std::copy(done, done + K, aln.begin());
        ops.assign(done_ops, done_ops + (size_t)K * (size_t)done_cap);
        ops_cap = done_cap;
    } else if (align && K > 0) {
        for (long long i = 0; i < K; ++i) ops_cap = std::max(ops_cap, qlen + offs[(size_t)order[(size_t)i] + 1] - offs[(size_t)order[(size_t)i]]);
        void *d_aln = nullptr, *d_ops = nullptr;
        CHECK(sw_device_malloc(ctx, (size_t)K * sizeof(sw_alignment), &d_aln));
        CHECK(sw_device_malloc(ctx, (size_t)K * (size_t)ops_cap, &d_ops));
        CHECK(sw_align_affine_device(ctx, (const char*)d_q, qlen, (const char*)d_db, offs.data(), nrec, order.data(), K, &aff, (sw_alignment*)d_aln, (char*)d_ops,
                                     ops_cap, nullptr));
        CHECK(sw_synchronize(ctx, nullptr));
        ops.resize((size_t)K * (size_t)ops_cap);
        CHECK(sw_memcpy_d2h(ctx, aln.data(), d_aln, (size_t)K * sizeof(sw_alignment)));
        CHECK(sw_memcpy_d2h(ctx, ops.data(), d_ops, ops.size()));
        (void)sw_device_free(ctx, d_aln); (void)sw_device_free(ctx, d_ops);
    }
    printf("# query %lld letters, %lld targets, %lld letters; rank\trecord\tscore\ttarget_end\tquery_end\n", (long long)qlen, (long long)nrec, (long long)total);
    for (long long i = 0; i < K; ++i) {
        const sw_hit& r = hits[i];
        const long long te = r.max_pos / (qlen + 1), qe = r.max_pos % (qlen + 1);
        printf("%lld\t%lld\t%lld\t%lld\t%lld\n", i + 1, (long long)order[(size_t)i], (long long)r.max_score, te, qe);
        if (!align) continue;
        const sw_alignment& a = aln[(size_t)i];
        printf("align\t%lld\t%lld\t%lld\t%lld\t%lld\n", (long long)a.q_begin, (long long)a.q_end, (long long)a.t_begin, (long long)a.t_end, (long long)a.nops);
        const char* t = db.data() + offs[(size_t)order[(size_t)i]];
        const char* op = ops.data() + (size_t)i * (size_t)ops_cap;
        std::string lq, lm, lt;
        int64_t qi = a.q_begin, ti = a.t_begin;
        for (int64_t k = 0; k < a.nops; ++k) {
            if (op[k] == 'M') { lq += q[(size_t)qi]; lt += t[ti]; lm += q[(size_t)qi] == t[ti] ? '|' : ' '; ++qi; ++ti; }
            else if (op[k] == 'I') { lq += q[(size_t)qi]; lt += '-'; lm += ' '; ++qi; }
            else { lq += '-'; lt += t[ti]; lm += ' '; ++ti; }
        }
        printf("Q %s\n  %s\nT %s\n", lq.c_str(), lm.c_str(), lt.c_str());
    }
    return 0;
}

static int search_main(const char* qpath, long long rec, const char* dbpath, long long top, const sw_scores& sc, const AffineArgs& af, bool align, bool align_ckpt) {
    int64_t qlen = 0, nrec = 0, total = 0;
    CHECK(sw_read_fasta(qpath, rec, nullptr, 0, &qlen));
    std::vector<char> q((size_t)qlen + 1);
    CHECK(sw_read_fasta(qpath, rec, q.data(), qlen, &qlen));
    CHECK(sw_read_fasta_db(dbpath, nullptr, 0, nullptr, 0, &nrec, &total));
    std::vector<char> db((size_t)total + 1);
    std::vector<int64_t> offs((size_t)nrec + 1, 0);
    CHECK(sw_read_fasta_db(dbpath, db.data(), total, offs.data(), nrec + 1, &nrec, &total));
    sw_ctx* ctx = nullptr;
    CHECK(sw_create(0, &ctx));
    if (align_ckpt) CHECK(sw_set_option(ctx, "align_checkpoint", 2));   // hits too large for whole direction matrices are aligned checkpointed
    void *d_q = nullptr, *d_db = nullptr, *d_res = nullptr;
    CHECK(sw_device_malloc(ctx, (size_t)qlen + 16, &d_q));
    CHECK(sw_device_malloc(ctx, (size_t)total + 16, &d_db));
    CHECK(sw_device_malloc(ctx, (size_t)(nrec > 0 ? nrec : 1) * sizeof(sw_result), &d_res));
    CHECK(sw_memcpy_h2d(ctx, d_q, q.data(), (size_t)qlen));
    if (total) CHECK(sw_memcpy_h2d(ctx, d_db, db.data(), (size_t)total));
    std::vector<sw_submat> sub(af.on || align ? 1 : 0);
    sw_affine aff = {nullptr, af.has_open ? af.open : 0, af.has_extend ? af.extend : sc.gap};
    if (af.on || align) {
        if (af.matrix) CHECK(sw_read_submat(af.matrix, sub.data()));
        else sw_submat_match(sc.match, sc.mismatch, sub.data());
        aff.sub = sub.data();
    }
    const double t0 = now_s();
    if (af.on) CHECK(sw_search_affine_device(ctx, (const char*)d_q, qlen, (const char*)d_db, offs.data(), nrec, &aff, (sw_result*)d_res, nullptr));
    else CHECK(sw_search_device(ctx, (const char*)d_q, qlen, (const char*)d_db, offs.data(), nrec, &sc, (sw_result*)d_res, nullptr));
    CHECK(sw_synchronize(ctx, nullptr));
    const double t1 = now_s();
    std::vector<sw_result> res((size_t)nrec);
    if (nrec) CHECK(sw_memcpy_d2h(ctx, res.data(), d_res, (size_t)nrec * sizeof(sw_result)));
    const std::vector<sw_hit> hits = rank_hits(res.data(), nrec, top, 0);
    if (int rc = print_hits(ctx, q.data(), qlen, d_q, db, d_db, offs, nrec, total, hits.data(), (long long)hits.size(), align, aff)) return rc;
    const double cells = (double)qlen * (double)total;
    printf("\nElapsed time for database search: %f (%.1f GCUPS)\n\n", t1 - t0, t1 > t0 ? cells / (t1 - t0) / 1e9 : 0.0);
    (void)sw_device_free(ctx, d_q); (void)sw_device_free(ctx, d_db); (void)sw_device_free(ctx, d_res);
    sw_destroy(ctx);
    return 0;
}

// --search --all-queries: every record of the query file against the database through ONE prepared handle and one call
// (sw_db_create / sw_db_search_affine_top); the hit block of --search once per query, each under a line that names the record.  The K
// best hits of every query are selected on the device and only they come back; more than SW_TOP_MAX hits per query go the long way:
// the whole table to the host and a sort of every row.  A linear search goes through the match / mismatch table of --scores with
// gap_open 0, which sw_search_device equals bit for bit.
// --prefilter-hits S (prefilter_hits > 0): sw_db_search_affine_top_prefiltered takes the place of sw_db_search_affine_top -- the hits are
// selected among the pairs whose ungapped score reaches S, on the device from the rescored pair list; everything else is the same.
static int search_all_main(const char* qpath, const char* dbpath, long long top, long long min_score, const sw_scores& sc, const AffineArgs& af, bool align,
                           bool align_ckpt, long long prefilter_hits = 0, int search_lanes = 32, int pairs_lanes = 32) {
    int64_t nq = 0, qtotal = 0, nrec = 0, total = 0;
    CHECK(sw_read_fasta_db(qpath, nullptr, 0, nullptr, 0, &nq, &qtotal));
    std::vector<char> qs((size_t)qtotal + 1);
    std::vector<int64_t> qoffs((size_t)nq + 1, 0);
    CHECK(sw_read_fasta_db(qpath, qs.data(), qtotal, qoffs.data(), nq + 1, &nq, &qtotal));
    CHECK(sw_read_fasta_db(dbpath, nullptr, 0, nullptr, 0, &nrec, &total));
    std::vector<char> db((size_t)total + 1);
    std::vector<int64_t> offs((size_t)nrec + 1, 0);
    CHECK(sw_read_fasta_db(dbpath, db.data(), total, offs.data(), nrec + 1, &nrec, &total));
    const long long K = std::max(0ll, std::min(top, (long long)nrec));
    const bool on_device = K <= SW_TOP_MAX;
    if (prefilter_hits > 0 && !on_device) {
        fprintf(stderr, "smithW: --prefilter-hits selects on the device: min(--top, records) = %lld is above %d\n", K, SW_TOP_MAX);
        return 2;
    }
    sw_ctx* ctx = nullptr;
    CHECK(sw_create(0, &ctx));
    // --align-checkpoint: a table the one call would refuse for its worst pair goes through it checkpointed instead of query by query
    if (align_ckpt) CHECK(sw_set_option(ctx, "align_checkpoint", 2));
    CHECK(sw_set_option(ctx, "search_lanes", search_lanes));
    CHECK(sw_set_option(ctx, "search_pairs_lanes", pairs_lanes));
    void *d_q = nullptr, *d_db = nullptr, *d_res = nullptr, *d_hits = nullptr, *d_nhits = nullptr, *d_npairs = nullptr;
    // the pair list of --prefilter-hits: every pair, or as many as "search_results_mib" lets the call hold (56 bytes each)
    const int64_t pairs_cap = std::min<int64_t>(nq * nrec, (sw_get_option(ctx, "search_results_mib") << 20) / 56);
    int64_t npassed = 0;
    CHECK(sw_device_malloc(ctx, sizeof(int64_t), &d_npairs));
    const size_t nres = on_device ? 1 : (size_t)std::max<int64_t>(1, nq * nrec), nhit = (size_t)std::max<int64_t>(1, nq * K);
    CHECK(sw_device_malloc(ctx, (size_t)qtotal + 16, &d_q));
    CHECK(sw_device_malloc(ctx, (size_t)total + 16, &d_db));
    CHECK(sw_device_malloc(ctx, nres * sizeof(sw_result), &d_res));
    CHECK(sw_device_malloc(ctx, nhit * sizeof(sw_hit), &d_hits));
    CHECK(sw_device_malloc(ctx, (size_t)std::max<int64_t>(1, nq) * sizeof(int64_t), &d_nhits));
    if (qtotal) CHECK(sw_memcpy_h2d(ctx, d_q, qs.data(), (size_t)qtotal));
    if (total) CHECK(sw_memcpy_h2d(ctx, d_db, db.data(), (size_t)total));
    std::vector<sw_submat> sub(1);
    sw_affine aff = {sub.data(), af.has_open ? af.open : 0, af.has_extend ? af.extend : sc.gap};
    if (af.matrix) CHECK(sw_read_submat(af.matrix, sub.data()));
    else sw_submat_match(sc.match, sc.mismatch, sub.data());
    sw_db* handle = nullptr;
    const double t0 = now_s();
    CHECK(sw_db_create(ctx, (const char*)d_db, offs.data(), nrec, &handle));
    const double t1 = now_s();
    if (!on_device) CHECK(sw_db_search_affine(ctx, handle, (const char*)d_q, qoffs.data(), nq, &aff, (sw_result*)d_res, nullptr));
    else if (K > 0 && prefilter_hits > 0)
        CHECK(sw_db_search_affine_top_prefiltered(ctx, handle, (const char*)d_q, qoffs.data(), nq, &aff, prefilter_hits, pairs_cap, K, min_score, (sw_hit*)d_hits,
                                                  (int64_t*)d_nhits, (int64_t*)d_npairs, nullptr));
    else if (K > 0) CHECK(sw_db_search_affine_top(ctx, handle, (const char*)d_q, qoffs.data(), nq, &aff, K, min_score, (sw_hit*)d_hits, (int64_t*)d_nhits, nullptr));
    CHECK(sw_synchronize(ctx, nullptr));
    const double t2 = now_s();
    if (K > 0 && prefilter_hits > 0) {
        CHECK(sw_memcpy_d2h(ctx, &npassed, d_npairs, sizeof npassed));
        if (npassed > pairs_cap) {   // the table was built from the pairs the list happened to keep: not a result
            fprintf(stderr, "smithW: --prefilter-hits %lld: %lld pairs pass the pre-filter, the list holds %lld: raise S\n", prefilter_hits, (long long)npassed,
                    (long long)pairs_cap);
            return 1;
        }
    }
    std::vector<sw_hit> hits(nhit);
    std::vector<int64_t> nhits((size_t)nq + 1, 0);
    if (on_device && K > 0 && nq > 0) {
        CHECK(sw_memcpy_d2h(ctx, hits.data(), d_hits, (size_t)(nq * K) * sizeof(sw_hit)));
        CHECK(sw_memcpy_d2h(ctx, nhits.data(), d_nhits, (size_t)nq * sizeof(int64_t)));
    }
    std::vector<sw_result> res(nres);
    if (!on_device && nq > 0) CHECK(sw_memcpy_d2h(ctx, res.data(), d_res, (size_t)(nq * nrec) * sizeof(sw_result)));
    // --align: the hits of every query in ONE call on the device table as the selection left it (sw_db_align_affine_hits), ops of at most
    // longest query + longest target letters each; a table of ops beyond 1 GiB, or one the call refuses, goes query by query instead (print_hits)
    std::vector<sw_alignment> aln;
    std::vector<char> ops;
    int64_t ops_cap = 0;
    if (align && on_device && K > 0 && nq > 0) {
        int64_t maxq = 0, longest = 0;
        for (int64_t i = 0; i < nq; ++i) maxq = std::max(maxq, qoffs[(size_t)i + 1] - qoffs[(size_t)i]);
        CHECK(sw_db_info(handle, nullptr, nullptr, &longest, nullptr));
        ops_cap = maxq + longest;
        const size_t n = (size_t)(nq * K);
        if ((double)n * (double)ops_cap <= (double)(1ll << 30)) {
            void *d_aln = nullptr, *d_ops = nullptr;
            CHECK(sw_device_malloc(ctx, n * sizeof(sw_alignment), &d_aln));
            CHECK(sw_device_malloc(ctx, n * (size_t)ops_cap, &d_ops));
            // the call refuses by the worst pair the table COULD name (longest target x longest query against "align_workspace_mib");
            // the hits of such a table may still fit one by one: those go query by query, as they always did (print_hits reports what is left)
            const int rc = sw_db_align_affine_hits(ctx, handle, (const char*)d_q, qoffs.data(), nq, &aff, (const sw_hit*)d_hits, (const int64_t*)d_nhits, K,
                                                   (sw_alignment*)d_aln, (char*)d_ops, ops_cap, nullptr);
            if (rc != SW_OK && rc != SW_EINVAL) CHECK(rc);
            if (rc == SW_EINVAL) fprintf(stderr, "smithW: the one alignment call on the hit table was refused (%s); aligning query by query\n", sw_last_error());
            if (rc == SW_OK) {
                CHECK(sw_synchronize(ctx, nullptr));
                aln.resize(n); ops.resize(n * (size_t)ops_cap);
                CHECK(sw_memcpy_d2h(ctx, aln.data(), d_aln, n * sizeof(sw_alignment)));
                CHECK(sw_memcpy_d2h(ctx, ops.data(), d_ops, ops.size()));
            }
            (void)sw_device_free(ctx, d_aln); (void)sw_device_free(ctx, d_ops);
        }
    }
    for (int64_t i = 0; i < nq; ++i) {
        printf("## query record %lld of %s\n", (long long)i, qpath);
        const std::vector<sw_hit> ranked = on_device ? std::vector<sw_hit>() : rank_hits(res.data() + i * nrec, nrec, K, min_score);
        const sw_hit* row = on_device ? hits.data() + i * K : ranked.data();
        const long long n = on_device ? (long long)nhits[(size_t)i] : (long long)ranked.size();
        if (int rc = print_hits(ctx, qs.data() + qoffs[(size_t)i], qoffs[(size_t)i + 1] - qoffs[(size_t)i], (const char*)d_q + qoffs[(size_t)i], db, d_db, offs, nrec,
                                total, row, n, align, aff, aln.empty() ? nullptr : aln.data() + i * K, aln.empty() ? nullptr : ops.data() + (size_t)(i * K) * (size_t)ops_cap,
                                ops_cap)) return rc;
    }
    const double cells = (double)qtotal * (double)total;
    if (prefilter_hits > 0)
        printf("\nElapsed time for database search: %f (%.1f GCUPS; %lld queries in one call, %lld of %lld pairs passed the pre-filter U >= %lld, handle prepared in %f)\n\n",
               t2 - t1, t2 > t1 ? cells / (t2 - t1) / 1e9 : 0.0, (long long)nq, (long long)npassed, (long long)(nq * nrec), prefilter_hits, t1 - t0);
    else
        printf("\nElapsed time for database search: %f (%.1f GCUPS; %lld queries in one call, handle prepared in %f)\n\n", t2 - t1,
               t2 > t1 ? cells / (t2 - t1) / 1e9 : 0.0, (long long)nq, t1 - t0);
    sw_db_free(handle);
    (void)sw_device_free(ctx, d_npairs);
    (void)sw_device_free(ctx, d_q); (void)sw_device_free(ctx, d_db); (void)sw_device_free(ctx, d_res);
    (void)sw_device_free(ctx, d_hits); (void)sw_device_free(ctx, d_nhits);
    sw_destroy(ctx);
    return 0;
}

// --search --pssm FILE DB.fa: ONE position-specific scoring matrix (PSI-BLAST's ASCII format, sw_read_pssm) as the one query against the
// database, through a prepared handle: sw_db_search_pssm_top (or, for more than SW_TOP_MAX hits, sw_db_search_pssm and a sort on the
// host) and, with --align, one sw_db_align_pssm_hits call on the device hit table.  The output is the output of --all-queries for a file
// of one record.  Bytes the matrix has no row entry for score the file's smallest entry (the rule of sw_read_submat) and smax is its
// largest one, so nothing is clamped; the query line of an alignment is the matrix's consensus: per column the first letter with the
// largest entry, '|' where the target has that letter.
static int search_pssm_main(const char* ppath, const char* dbpath, long long top, long long min_score, const AffineArgs& af, bool align, bool align_ckpt,
                            int search_lanes = 32) {
    char letters[256];
    int32_t nletters = 0;
    int64_t ncols = 0, nrec = 0, total = 0;
    CHECK(sw_read_pssm(ppath, letters, &nletters, nullptr, 0, &ncols));
    std::vector<int8_t> pssm((size_t)ncols * (size_t)nletters);
    CHECK(sw_read_pssm(ppath, letters, &nletters, pssm.data(), (int64_t)pssm.size(), &ncols));
    CHECK(sw_read_fasta_db(dbpath, nullptr, 0, nullptr, 0, &nrec, &total));
    std::vector<char> db((size_t)total + 1);
    std::vector<int64_t> offs((size_t)nrec + 1, 0);
    CHECK(sw_read_fasta_db(dbpath, db.data(), total, offs.data(), nrec + 1, &nrec, &total));
    const int lo = *std::min_element(pssm.begin(), pssm.end()), hi = *std::max_element(pssm.begin(), pssm.end());
    const sw_pssm_scoring scoring = {letters, nletters, std::min(lo, 0), std::max(hi, 0), af.has_open ? af.open : 0, af.has_extend ? af.extend : 0};
    std::string consensus((size_t)ncols, '?');
    for (int64_t g = 0; g < ncols; ++g) {
        const int8_t* col = pssm.data() + g * nletters;
        consensus[(size_t)g] = letters[std::max_element(col, col + nletters) - col];
    }
    const int64_t qoffs[2] = {0, ncols};
    const long long K = std::max(0ll, std::min(top, (long long)nrec));
    const bool on_device = K <= SW_TOP_MAX;
    if (align && !on_device) { fprintf(stderr, "smithW: --pssm --align aligns a device hit table: min(--top, records) = %lld is above %d\n", K, SW_TOP_MAX); return 2; }
    sw_ctx* ctx = nullptr;
    CHECK(sw_create(0, &ctx));
    if (align_ckpt) CHECK(sw_set_option(ctx, "align_checkpoint", 2));
    CHECK(sw_set_option(ctx, "search_lanes", search_lanes));
    void *d_pssm = nullptr, *d_db = nullptr, *d_res = nullptr, *d_hits = nullptr, *d_nhits = nullptr;
    const size_t nres = on_device ? 1 : (size_t)std::max<int64_t>(1, nrec), nhit = (size_t)std::max<long long>(1, K);
    CHECK(sw_device_malloc(ctx, pssm.size() + 16, &d_pssm));
    CHECK(sw_device_malloc(ctx, (size_t)total + 16, &d_db));
    CHECK(sw_device_malloc(ctx, nres * sizeof(sw_result), &d_res));
    CHECK(sw_device_malloc(ctx, nhit * sizeof(sw_hit), &d_hits));
    CHECK(sw_device_malloc(ctx, sizeof(int64_t), &d_nhits));
    CHECK(sw_memcpy_h2d(ctx, d_pssm, pssm.data(), pssm.size()));
    if (total) CHECK(sw_memcpy_h2d(ctx, d_db, db.data(), (size_t)total));
    sw_db* handle = nullptr;
    const double t0 = now_s();
    CHECK(sw_db_create(ctx, (const char*)d_db, offs.data(), nrec, &handle));
    const double t1 = now_s();
    if (!on_device) CHECK(sw_db_search_pssm(ctx, handle, (const int8_t*)d_pssm, qoffs, 1, &scoring, (sw_result*)d_res, nullptr));
    else if (K > 0) CHECK(sw_db_search_pssm_top(ctx, handle, (const int8_t*)d_pssm, qoffs, 1, &scoring, K, min_score, (sw_hit*)d_hits, (int64_t*)d_nhits, nullptr));
    CHECK(sw_synchronize(ctx, nullptr));
    const double t2 = now_s();
    std::vector<sw_hit> hits(nhit);
    int64_t nhits = 0;
    if (on_device && K > 0) {
        CHECK(sw_memcpy_d2h(ctx, hits.data(), d_hits, (size_t)K * sizeof(sw_hit)));
        CHECK(sw_memcpy_d2h(ctx, &nhits, d_nhits, sizeof nhits));
    } else if (!on_device) {
        std::vector<sw_result> res(nres);
        CHECK(sw_memcpy_d2h(ctx, res.data(), d_res, (size_t)nrec * sizeof(sw_result)));
        hits = rank_hits(res.data(), nrec, K, min_score);
        nhits = (int64_t)hits.size();
    }
    std::vector<sw_alignment> aln;
    std::vector<char> ops;
    int64_t ops_cap = 0;
    if (align && K > 0) {
        int64_t longest = 0;
        CHECK(sw_db_info(handle, nullptr, nullptr, &longest, nullptr));
        ops_cap = ncols + longest;
        void *d_aln = nullptr, *d_ops = nullptr;
        CHECK(sw_device_malloc(ctx, (size_t)K * sizeof(sw_alignment), &d_aln));
        CHECK(sw_device_malloc(ctx, (size_t)K * (size_t)ops_cap, &d_ops));
        CHECK(sw_db_align_pssm_hits(ctx, handle, (const int8_t*)d_pssm, qoffs, 1, &scoring, (const sw_hit*)d_hits, (const int64_t*)d_nhits, K, (sw_alignment*)d_aln,
                                    (char*)d_ops, ops_cap, nullptr));
        CHECK(sw_synchronize(ctx, nullptr));
        aln.resize((size_t)K); ops.resize((size_t)K * (size_t)ops_cap);
        CHECK(sw_memcpy_d2h(ctx, aln.data(), d_aln, aln.size() * sizeof(sw_alignment)));
        CHECK(sw_memcpy_d2h(ctx, ops.data(), d_ops, ops.size()));
        (void)sw_device_free(ctx, d_aln); (void)sw_device_free(ctx, d_ops);
    }
    printf("## query record 0 of %s\n", ppath);
    const sw_affine unused = {nullptr, 0, 0};   // (print_hits aligns nothing itself when it is given the rows of a call)
    if (int rc = print_hits(ctx, consensus.data(), ncols, nullptr, db, d_db, offs, nrec, total, hits.data(), (long long)nhits, align && K > 0, unused,
                            aln.empty() ? nullptr : aln.data(), aln.empty() ? nullptr : ops.data(), ops_cap)) return rc;
    const double cells = (double)ncols * (double)total;
    printf("\nElapsed time for database search: %f (%.1f GCUPS; 1 PSSM of %lld columns over %d letters, handle prepared in %f)\n\n", t2 - t1,
           t2 > t1 ? cells / (t2 - t1) / 1e9 : 0.0, (long long)ncols, nletters, t1 - t0);
    sw_db_free(handle);
    (void)sw_device_free(ctx, d_pssm); (void)sw_device_free(ctx, d_db); (void)sw_device_free(ctx, d_res);
    (void)sw_device_free(ctx, d_hits); (void)sw_device_free(ctx, d_nhits);
    sw_destroy(ctx);
    return 0;
}

// --iterations N (with --search Q.fa DB.fa --all-queries, or --search --pssm FILE DB.fa): an iterative search that stays on the device.
// Iteration 0 is the search of today: the sequence queries go through sw_pssm_from_queries (letters: the distinct bytes of the database
// and the queries, ascending; other / smax: the smallest / largest entry of the table over those letters, so nothing is clamped and the
// hits are those of --all-queries), a PSSM file is taken as it is (its letters, other and smax as for --pssm).  Every further iteration
// aligns the top hits (sw_db_align_pssm_hits), builds the next matrix from them with the iteration-0 matrix as prior
// (sw_db_pssm_from_hits: --prior-weight W, --include-score S; S: the table of --matrix, or of --scores where there is none, which is
// always the case with --pssm) and searches again (sw_db_search_pssm_top); the host reads nothing in between.  The hits printed, and
// with --align their alignments, are those of the LAST iteration, in the format of --all-queries; the query line of an alignment is the
// query's letters, for a PSSM file the consensus of the last matrix.  --out-pssm PREFIX writes the matrix the last search ran with, per
// query, to PREFIX.<query index>.pssm (sw_write_pssm).  --weight-hits P puts sw_db_pssm_hit_weights (per_hit = P, the same
// --include-score) between the alignment and the update of every round and hands its table to the update; 0: no weights, every hit counts 1.
static std::vector<std::string> fasta_names(const char* path);

static int search_iter_main(const char* qpath, const char* ppath, const char* dbpath, long long top, long long min_score, const sw_scores& sc, const AffineArgs& af,
                            bool align, bool align_ckpt, int search_lanes, long long iterations, long long include_score, long long prior_weight,
                            const char* out_pssm, long long weight_hits, const char* out_a3m) {
    int64_t nq = 0, qtotal = 0, nrec = 0, total = 0;
    CHECK(sw_read_fasta_db(dbpath, nullptr, 0, nullptr, 0, &nrec, &total));
    std::vector<char> db((size_t)total + 1);
    std::vector<int64_t> offs((size_t)nrec + 1, 0);
    CHECK(sw_read_fasta_db(dbpath, db.data(), total, offs.data(), nrec + 1, &nrec, &total));
    std::vector<sw_submat> sub(1);
    if (af.matrix) CHECK(sw_read_submat(af.matrix, sub.data()));
    else sw_submat_match(sc.match, sc.mismatch, sub.data());
    char letters[256];
    int32_t nletters = 0;
    std::vector<char> qs;                 // the query line of every query's alignments, back to back
    std::vector<int64_t> qoffs;
    std::vector<int8_t> pssm;             // iteration 0
    sw_pssm_scoring scoring = {letters, 0, 0, 0, af.has_open ? af.open : 0, af.has_extend ? af.extend : (ppath ? 0 : sc.gap)};
    if (ppath) {
        int64_t ncols = 0;
        CHECK(sw_read_pssm(ppath, letters, &nletters, nullptr, 0, &ncols));
        pssm.resize((size_t)ncols * (size_t)nletters);
        CHECK(sw_read_pssm(ppath, letters, &nletters, pssm.data(), (int64_t)pssm.size(), &ncols));
        nq = 1; qtotal = ncols;
        qoffs = {0, ncols};
        qs.assign((size_t)ncols, '?');
        scoring.other = std::min<int>(*std::min_element(pssm.begin(), pssm.end()), 0);
        scoring.smax = std::max<int>(*std::max_element(pssm.begin(), pssm.end()), 0);
    } else {
        CHECK(sw_read_fasta_db(qpath, nullptr, 0, nullptr, 0, &nq, &qtotal));
        qs.resize((size_t)qtotal + 1);
        qoffs.assign((size_t)nq + 1, 0);
        CHECK(sw_read_fasta_db(qpath, qs.data(), qtotal, qoffs.data(), nq + 1, &nq, &qtotal));
        bool seen[256] = {};
        for (int64_t i = 0; i < total; ++i) seen[(unsigned char)db[(size_t)i]] = true;
        for (int64_t i = 0; i < qtotal; ++i) seen[(unsigned char)qs[(size_t)i]] = true;
        for (int b = 0; b < 256; ++b)
            if (seen[b]) letters[nletters++] = (char)b;
        if (nletters == 0 || qtotal == 0) { fprintf(stderr, "smithW: --iterations needs queries and a database with letters\n"); return 2; }
        int lo = 0, hi = 0;
        for (int x = 0; x < nletters; ++x)
            for (int y = 0; y < nletters; ++y) {
                const int v = sub[0].s[(unsigned char)letters[x]][(unsigned char)letters[y]];
                lo = std::min(lo, v); hi = std::max(hi, v);
            }
        scoring.other = lo; scoring.smax = hi;
        pssm.resize((size_t)qtotal * (size_t)nletters);
        CHECK(sw_pssm_from_queries(qs.data(), qoffs.data(), nq, sub.data(), letters, nletters, pssm.data()));
        if (qoffs[0] != 0) { fprintf(stderr, "smithW: query offsets do not start at 0\n"); return 1; }
    }
    scoring.nletters = nletters;
    const long long K = std::max(0ll, std::min(top, (long long)nrec));
    if (K < 1 || K > SW_TOP_MAX) { fprintf(stderr, "smithW: --iterations / --out-pssm work on a device hit table: min(--top, records) = %lld is outside 1..%d\n", K, SW_TOP_MAX); return 2; }
    sw_ctx* ctx = nullptr;
    CHECK(sw_create(0, &ctx));
    if (align_ckpt) CHECK(sw_set_option(ctx, "align_checkpoint", 2));
    CHECK(sw_set_option(ctx, "search_lanes", search_lanes));
    void *d_prior = nullptr, *d_work = nullptr, *d_db = nullptr, *d_hits = nullptr, *d_nhits = nullptr, *d_aln = nullptr, *d_ops = nullptr, *d_weights = nullptr;
    const size_t n = (size_t)(nq * K);
    CHECK(sw_device_malloc(ctx, pssm.size() + 16, &d_prior));
    CHECK(sw_device_malloc(ctx, pssm.size() + 16, &d_work));
    CHECK(sw_device_malloc(ctx, (size_t)total + 16, &d_db));
    CHECK(sw_device_malloc(ctx, n * sizeof(sw_hit), &d_hits));
    CHECK(sw_device_malloc(ctx, (size_t)nq * sizeof(int64_t), &d_nhits));
    CHECK(sw_memcpy_h2d(ctx, d_prior, pssm.data(), pssm.size()));
    if (total) CHECK(sw_memcpy_h2d(ctx, d_db, db.data(), (size_t)total));
    sw_db* handle = nullptr;
    const double t0 = now_s();
    CHECK(sw_db_create(ctx, (const char*)d_db, offs.data(), nrec, &handle));
    int64_t maxq = 0, longest = 0;
    for (int64_t i = 0; i < nq; ++i) maxq = std::max(maxq, qoffs[(size_t)i + 1] - qoffs[(size_t)i]);
    CHECK(sw_db_info(handle, nullptr, nullptr, &longest, nullptr));
    const int64_t ops_cap = std::max<int64_t>(1, maxq + longest);
    if (iterations > 1 || align) {
        if ((double)n * (double)ops_cap > (double)(1ll << 32)) { fprintf(stderr, "smithW: the ops of %zu hits x %lld bytes pass 4 GiB: lower --top\n", n, (long long)ops_cap); return 2; }
        CHECK(sw_device_malloc(ctx, n * sizeof(sw_alignment), &d_aln));
        CHECK(sw_device_malloc(ctx, n * (size_t)ops_cap, &d_ops));
    }
    if (weight_hits > 0 && iterations > 1) CHECK(sw_device_malloc(ctx, n * sizeof(int32_t), &d_weights));
    const sw_pssm_update upd = {sub.data(), (int32_t)prior_weight, include_score};
    const sw_pssm_weighting weighting = {(int32_t)weight_hits, include_score};
    const double t1 = now_s();
    const int8_t* d_cur = (const int8_t*)d_prior;
    for (long long it = 0; it < iterations; ++it) {   // nothing below waits for the device or reads from it
        if (it > 0) {
            CHECK(sw_db_align_pssm_hits(ctx, handle, d_cur, qoffs.data(), nq, &scoring, (const sw_hit*)d_hits, (const int64_t*)d_nhits, K, (sw_alignment*)d_aln,
                                        (char*)d_ops, ops_cap, nullptr));
            if (d_weights)
                CHECK(sw_db_pssm_hit_weights(ctx, handle, qoffs.data(), nq, &scoring, &weighting, (const sw_hit*)d_hits, (const int64_t*)d_nhits, K,
                                             (const sw_alignment*)d_aln, (const char*)d_ops, ops_cap, (int32_t*)d_weights, nullptr));
            CHECK(sw_db_pssm_from_hits(ctx, handle, (const int8_t*)d_prior, qoffs.data(), nq, &scoring, &upd, (const sw_hit*)d_hits, (const int64_t*)d_nhits, K,
                                       (const sw_alignment*)d_aln, (const char*)d_ops, ops_cap, (const int32_t*)d_weights, (int8_t*)d_work, nullptr, nullptr));
            d_cur = (const int8_t*)d_work;
        }
        CHECK(sw_db_search_pssm_top(ctx, handle, d_cur, qoffs.data(), nq, &scoring, K, min_score, (sw_hit*)d_hits, (int64_t*)d_nhits, nullptr));
    }
    if (align)
        CHECK(sw_db_align_pssm_hits(ctx, handle, d_cur, qoffs.data(), nq, &scoring, (const sw_hit*)d_hits, (const int64_t*)d_nhits, K, (sw_alignment*)d_aln,
                                    (char*)d_ops, ops_cap, nullptr));
    // --out-a3m: the rows of the last round's tables, still on the device: one call for the row table and the size, one for the bytes
    void *d_qs = nullptr, *d_rows = nullptr, *d_a3m = nullptr, *d_a3m_bytes = nullptr;
    int64_t a3m_bytes = 0;
    if (out_a3m) {
        if (!ppath) {
            CHECK(sw_device_malloc(ctx, (size_t)qtotal + 16, &d_qs));
            CHECK(sw_memcpy_h2d(ctx, d_qs, qs.data(), (size_t)qtotal));
        }
        CHECK(sw_device_malloc(ctx, n * sizeof(sw_msa_row), &d_rows));
        CHECK(sw_device_malloc(ctx, sizeof(int64_t), &d_a3m_bytes));
        CHECK(sw_db_msa_from_hits(ctx, handle, (const char*)d_qs, qoffs.data(), nq, include_score, (const sw_hit*)d_hits, (const int64_t*)d_nhits, K,
                                  (const sw_alignment*)d_aln, (const char*)d_ops, ops_cap, nullptr, (sw_msa_row*)d_rows, nullptr, 0, (int64_t*)d_a3m_bytes, nullptr));
        CHECK(sw_synchronize(ctx, nullptr));
        CHECK(sw_memcpy_d2h(ctx, &a3m_bytes, d_a3m_bytes, sizeof a3m_bytes));
        CHECK(sw_device_malloc(ctx, (size_t)a3m_bytes + 16, &d_a3m));
        CHECK(sw_db_msa_from_hits(ctx, handle, (const char*)d_qs, qoffs.data(), nq, include_score, (const sw_hit*)d_hits, (const int64_t*)d_nhits, K,
                                  (const sw_alignment*)d_aln, (const char*)d_ops, ops_cap, nullptr, (sw_msa_row*)d_rows, (char*)d_a3m, a3m_bytes,
                                  (int64_t*)d_a3m_bytes, nullptr));
    }
    CHECK(sw_synchronize(ctx, nullptr));
    const double t2 = now_s();
    std::vector<sw_hit> hits(n);
    std::vector<int64_t> nhits((size_t)nq);
    std::vector<int8_t> last(pssm.size());
    CHECK(sw_memcpy_d2h(ctx, hits.data(), d_hits, n * sizeof(sw_hit)));
    CHECK(sw_memcpy_d2h(ctx, nhits.data(), d_nhits, (size_t)nq * sizeof(int64_t)));
    CHECK(sw_memcpy_d2h(ctx, last.data(), d_cur, last.size()));
    std::vector<sw_alignment> aln;
    std::vector<char> ops;
    if (align) {
        aln.resize(n); ops.resize(n * (size_t)ops_cap);
        CHECK(sw_memcpy_d2h(ctx, aln.data(), d_aln, n * sizeof(sw_alignment)));
        CHECK(sw_memcpy_d2h(ctx, ops.data(), d_ops, ops.size()));
    }
    if (ppath)   // the consensus of the last matrix: per column the first letter with the largest entry
        for (int64_t g = 0; g < qtotal; ++g) {
            const int8_t* col = last.data() + g * nletters;
            qs[(size_t)g] = letters[std::max_element(col, col + nletters) - col];
        }
    std::vector<sw_msa_row> msa_rows;
    std::vector<char> a3m;
    std::vector<std::string> tnames, qnames;
    std::vector<const char*> tname_ptrs;
    if (out_a3m) {
        msa_rows.resize(n); a3m.resize((size_t)a3m_bytes + 1);
        CHECK(sw_memcpy_d2h(ctx, msa_rows.data(), d_rows, n * sizeof(sw_msa_row)));
        if (a3m_bytes) CHECK(sw_memcpy_d2h(ctx, a3m.data(), d_a3m, (size_t)a3m_bytes));
        tnames = fasta_names(dbpath);
        tnames.resize((size_t)nrec, "-");
        for (const std::string& s : tnames) tname_ptrs.push_back(s.c_str());
        if (!ppath) qnames = fasta_names(qpath);
        qnames.resize((size_t)nq, "-");
    }
    const sw_affine unused = {nullptr, 0, 0};   // (print_hits aligns nothing itself when it is given the rows of a call)
    for (int64_t i = 0; i < nq; ++i) {
        printf("## query record %lld of %s\n", (long long)i, ppath ? ppath : qpath);
        if (int rc = print_hits(ctx, qs.data() + qoffs[(size_t)i], qoffs[(size_t)i + 1] - qoffs[(size_t)i], nullptr, db, d_db, offs, nrec, total, hits.data() + i * K,
                                (long long)nhits[(size_t)i], align, unused, align ? aln.data() + i * K : nullptr, align ? ops.data() + (size_t)(i * K) * (size_t)ops_cap : nullptr,
                                ops_cap)) return rc;
        if (out_pssm) {
            const std::string path = std::string(out_pssm) + "." + std::to_string((long long)i) + ".pssm";
            CHECK(sw_write_pssm(path.c_str(), letters, nletters, last.data() + qoffs[(size_t)i] * nletters, qoffs[(size_t)i + 1] - qoffs[(size_t)i],
                                qs.data() + qoffs[(size_t)i]));
        }
        if (out_a3m) {
            const std::string path = std::string(out_a3m) + "." + std::to_string((long long)i) + ".a3m";
            CHECK(sw_write_a3m(path.c_str(), qnames[(size_t)i].c_str(), ppath ? nullptr : qs.data() + qoffs[(size_t)i], qoffs[(size_t)i + 1] - qoffs[(size_t)i],
                               tname_ptrs.data(), nrec, hits.data() + i * K, aln.data() + i * K, msa_rows.data() + i * K, K, a3m.data(), a3m_bytes));
        }
    }
    const double cells = (double)qtotal * (double)total * (double)iterations;
    printf("\nElapsed time for database search: %f (%.1f GCUPS; %lld queries, %lld iterations on the device, handle prepared in %f)\n\n", t2 - t1,
           t2 > t1 ? cells / (t2 - t1) / 1e9 : 0.0, (long long)nq, iterations, t1 - t0);
    sw_db_free(handle);
    (void)sw_device_free(ctx, d_prior); (void)sw_device_free(ctx, d_work); (void)sw_device_free(ctx, d_db); (void)sw_device_free(ctx, d_hits);
    (void)sw_device_free(ctx, d_nhits);
    if (d_aln) (void)sw_device_free(ctx, d_aln);
    if (d_ops) (void)sw_device_free(ctx, d_ops);
    if (d_weights) (void)sw_device_free(ctx, d_weights);
    for (void* d : {d_qs, d_rows, d_a3m, d_a3m_bytes})
        if (d) (void)sw_device_free(ctx, d);
    sw_destroy(ctx);
    return 0;
}

// the first word of every record's header line, by the record rule of sw_read_fasta_db (a headerless record is "-")
static std::vector<std::string> fasta_names(const char* path) {
    std::vector<std::string> names;
    FILE* f = fopen(path, "rb");
    if (!f) return names;
    char line[1 << 12];
    bool whole = true;   // the previous fgets ended a line
    while (fgets(line, sizeof line, f)) {
        const bool start = whole;
        const size_t n = strlen(line);
        whole = n > 0 && (line[n - 1] == '\n' || line[n - 1] == '\r');
        if (!start || line[0] == ';' || line[0] == '\n' || line[0] == '\r') continue;
        if (line[0] == '>') { const size_t e = strcspn(line + 1, " \t\r\n"); names.push_back(e ? std::string(line + 1, e) : std::string("-")); }
        else if (names.empty()) names.push_back("-");
    }
    fclose(f);
    return names;
}

// --search --pairs FILE: the listed (query record, target record) pairs through ONE prepared handle and one call
// (sw_db_create / sw_db_search_affine_pairs), one output line per pair in input order.  A linear search goes through the match /
// mismatch table of --scores with gap_open 0, as --all-queries does.
static int search_pairs_main(const char* qpath, const char* dbpath, const char* ppath, const sw_scores& sc, const AffineArgs& af, int pairs_lanes = 32) {
    std::vector<sw_pair> pairs;
    {
        FILE* f = fopen(ppath, "r");
        if (!f) { fprintf(stderr, "smithW: --pairs: cannot open %s\n", ppath); return 2; }
        char line[512];
        for (long long ln = 1; fgets(line, sizeof line, f); ++ln) {
            if (!strchr(line, '\n') && !feof(f)) {   // (a line that does not fit the buffer would be counted twice)
                fprintf(stderr, "smithW: --pairs %s line %lld: longer than %zu bytes\n", ppath, ln, sizeof line - 2);
                fclose(f);
                return 2;
            }
            const char* t = line + strspn(line, " \t\r\n");
            if (*t == 0 || *t == '#') continue;
            char *e1 = nullptr, *e2 = nullptr;
            const long long q = strtoll(t, &e1, 10);
            const long long k = e1 != t ? strtoll(e1, &e2, 10) : 0;
            if (e1 == t || e2 == e1 || !strchr(" \t", *e1) || e2[strspn(e2, " \t\r\n")] != 0) {
                fprintf(stderr, "smithW: --pairs %s line %lld: expected \"<query record> <target record>\"\n", ppath, ln);
                fclose(f);
                return 2;
            }
            pairs.push_back(sw_pair{q, k});
        }
        fclose(f);
    }
    int64_t nq = 0, qtotal = 0, nrec = 0, total = 0;
    CHECK(sw_read_fasta_db(qpath, nullptr, 0, nullptr, 0, &nq, &qtotal));
    std::vector<char> qs((size_t)qtotal + 1);
    std::vector<int64_t> qoffs((size_t)nq + 1, 0);
    CHECK(sw_read_fasta_db(qpath, qs.data(), qtotal, qoffs.data(), nq + 1, &nq, &qtotal));
    CHECK(sw_read_fasta_db(dbpath, nullptr, 0, nullptr, 0, &nrec, &total));
    std::vector<char> db((size_t)total + 1);
    std::vector<int64_t> offs((size_t)nrec + 1, 0);
    CHECK(sw_read_fasta_db(dbpath, db.data(), total, offs.data(), nrec + 1, &nrec, &total));
    const std::vector<std::string> names = fasta_names(dbpath);
    if ((int64_t)names.size() != nrec) {   // the two readers must agree on the records, or a name would label another target
        fprintf(stderr, "smithW: --pairs: %s has %lld records but %zu header names\n", dbpath, (long long)nrec, names.size());
        return 1;
    }
    const int64_t np = (int64_t)pairs.size();
    sw_ctx* ctx = nullptr;
    CHECK(sw_create(0, &ctx));
    CHECK(sw_set_option(ctx, "search_pairs_lanes", pairs_lanes));
    void *d_q = nullptr, *d_db = nullptr, *d_pairs = nullptr, *d_res = nullptr;
    CHECK(sw_device_malloc(ctx, (size_t)qtotal + 16, &d_q));
    CHECK(sw_device_malloc(ctx, (size_t)total + 16, &d_db));
    CHECK(sw_device_malloc(ctx, (size_t)std::max<int64_t>(1, np) * sizeof(sw_pair), &d_pairs));
    CHECK(sw_device_malloc(ctx, (size_t)std::max<int64_t>(1, np) * sizeof(sw_result), &d_res));
    if (qtotal) CHECK(sw_memcpy_h2d(ctx, d_q, qs.data(), (size_t)qtotal));
    if (total) CHECK(sw_memcpy_h2d(ctx, d_db, db.data(), (size_t)total));
    if (np) CHECK(sw_memcpy_h2d(ctx, d_pairs, pairs.data(), (size_t)np * sizeof(sw_pair)));
    std::vector<sw_submat> sub(1);
    sw_affine aff = {sub.data(), af.has_open ? af.open : 0, af.has_extend ? af.extend : sc.gap};
    if (af.matrix) CHECK(sw_read_submat(af.matrix, sub.data()));
    else sw_submat_match(sc.match, sc.mismatch, sub.data());
    sw_db* handle = nullptr;
    const double t0 = now_s();
    CHECK(sw_db_create(ctx, (const char*)d_db, offs.data(), nrec, &handle));
    const double t1 = now_s();
    CHECK(sw_db_search_affine_pairs(ctx, handle, (const char*)d_q, qoffs.data(), nq, &aff, (const sw_pair*)d_pairs, np, (sw_result*)d_res, nullptr));
    CHECK(sw_synchronize(ctx, nullptr));
    const double t2 = now_s();
    std::vector<sw_result> res((size_t)np);
    if (np) CHECK(sw_memcpy_d2h(ctx, res.data(), d_res, (size_t)np * sizeof(sw_result)));
    printf("# %lld pairs of %lld queries and %lld targets; query\ttarget\tname\tscore\ttarget_end\tquery_end\n", (long long)np, (long long)nq, (long long)nrec);
    double cells = 0;
    for (int64_t p = 0; p < np; ++p) {
        const sw_pair& pr = pairs[(size_t)p];
        const bool qin = pr.query >= 0 && pr.query < nq, tin = pr.target >= 0 && pr.target < nrec;
        const long long M = qin ? qoffs[(size_t)pr.query + 1] - qoffs[(size_t)pr.query] + 1 : 1;
        const sw_result& r = res[(size_t)p];
        if (qin && tin) cells += (double)(M - 1) * (double)(offs[(size_t)pr.target + 1] - offs[(size_t)pr.target]);
        printf("%lld\t%lld\t%s\t%lld\t%lld\t%lld\n", (long long)pr.query, (long long)pr.target, tin && (size_t)pr.target < names.size() ? names[(size_t)pr.target].c_str() : "-",
               (long long)r.max_score, (long long)(r.max_pos / M), (long long)(r.max_pos % M));
    }
    printf("\nElapsed time for database search: %f (%.1f GCUPS; %lld pairs in one call, handle prepared in %f)\n\n", t2 - t1,
           t2 > t1 ? cells / (t2 - t1) / 1e9 : 0.0, (long long)np, t1 - t0);
    sw_db_free(handle);
    (void)sw_device_free(ctx, d_q); (void)sw_device_free(ctx, d_db); (void)sw_device_free(ctx, d_pairs); (void)sw_device_free(ctx, d_res);
    sw_destroy(ctx);
    return 0;
}

// --search --all-queries --prefilter S: the ungapped pre-filter (sw_db_prefilter_ungapped, U >= S) and the affine search of the pairs it
// lists (sw_db_search_affine_pairs over the whole list, its {-1, -1} tail included), through ONE prepared handle, back to back on the
// device; one read-back at the end brings the count, the list, the results and the ungapped scores.  The passing pairs are printed in
// ascending (query, target) order in the line format of --pairs, with " ungapped=<U>" appended.
static int search_prefilter_main(const char* qpath, const char* dbpath, long long min_u, const sw_scores& sc, const AffineArgs& af) {
    int64_t nq = 0, qtotal = 0, nrec = 0, total = 0;
    CHECK(sw_read_fasta_db(qpath, nullptr, 0, nullptr, 0, &nq, &qtotal));
    std::vector<char> qs((size_t)qtotal + 1);
    std::vector<int64_t> qoffs((size_t)nq + 1, 0);
    CHECK(sw_read_fasta_db(qpath, qs.data(), qtotal, qoffs.data(), nq + 1, &nq, &qtotal));
    CHECK(sw_read_fasta_db(dbpath, nullptr, 0, nullptr, 0, &nrec, &total));
    std::vector<char> db((size_t)total + 1);
    std::vector<int64_t> offs((size_t)nrec + 1, 0);
    CHECK(sw_read_fasta_db(dbpath, db.data(), total, offs.data(), nrec + 1, &nrec, &total));
    const std::vector<std::string> names = fasta_names(dbpath);
    if ((int64_t)names.size() != nrec) {
        fprintf(stderr, "smithW: --prefilter: %s has %lld records but %zu header names\n", dbpath, (long long)nrec, names.size());
        return 1;
    }
    // one device block for everything that comes back: the count (16 bytes), the list, the results, the ungapped scores
    const int64_t cap = nq * nrec;
    const size_t o_pairs = 16, o_res = o_pairs + (size_t)cap * sizeof(sw_pair), o_u = o_res + (size_t)cap * sizeof(sw_result),
                 out_bytes = o_u + (size_t)cap * sizeof(int32_t);
    sw_ctx* ctx = nullptr;
    CHECK(sw_create(0, &ctx));
    void *d_q = nullptr, *d_db = nullptr, *d_out = nullptr;
    CHECK(sw_device_malloc(ctx, (size_t)qtotal + 16, &d_q));
    CHECK(sw_device_malloc(ctx, (size_t)total + 16, &d_db));
    CHECK(sw_device_malloc(ctx, out_bytes, &d_out));
    if (qtotal) CHECK(sw_memcpy_h2d(ctx, d_q, qs.data(), (size_t)qtotal));
    if (total) CHECK(sw_memcpy_h2d(ctx, d_db, db.data(), (size_t)total));
    std::vector<sw_submat> sub(1);
    sw_affine aff = {sub.data(), af.has_open ? af.open : 0, af.has_extend ? af.extend : sc.gap};
    if (af.matrix) CHECK(sw_read_submat(af.matrix, sub.data()));
    else sw_submat_match(sc.match, sc.mismatch, sub.data());
    sw_pair* d_pairs = cap ? (sw_pair*)((char*)d_out + o_pairs) : nullptr;
    sw_result* d_res = cap ? (sw_result*)((char*)d_out + o_res) : nullptr;
    int32_t* d_u = cap ? (int32_t*)((char*)d_out + o_u) : nullptr;
    sw_db* handle = nullptr;
    const double t0 = now_s();
    CHECK(sw_db_create(ctx, (const char*)d_db, offs.data(), nrec, &handle));
    const double t1 = now_s();
    CHECK(sw_db_prefilter_ungapped(ctx, handle, (const char*)d_q, qoffs.data(), nq, sub.data(), min_u, d_pairs, cap, (int64_t*)d_out, d_u, nullptr));
    CHECK(sw_db_search_affine_pairs(ctx, handle, (const char*)d_q, qoffs.data(), nq, &aff, d_pairs, cap, d_res, nullptr));
    CHECK(sw_synchronize(ctx, nullptr));
    const double t2 = now_s();
    std::vector<char> out(out_bytes);
    CHECK(sw_memcpy_d2h(ctx, out.data(), d_out, out_bytes));
    int64_t np = 0;
    memcpy(&np, out.data(), sizeof np);
    const sw_pair* pairs = (const sw_pair*)(out.data() + o_pairs);
    const sw_result* res = (const sw_result*)(out.data() + o_res);
    const int32_t* u = (const int32_t*)(out.data() + o_u);
    std::vector<int64_t> order((size_t)np);
    for (int64_t p = 0; p < np; ++p) order[(size_t)p] = p;
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return pairs[a].query != pairs[b].query ? pairs[a].query < pairs[b].query : pairs[a].target < pairs[b].target; });
    printf("# %lld pairs of %lld queries and %lld targets pass the ungapped pre-filter at %lld; query\ttarget\tname\tscore\ttarget_end\tquery_end\n", (long long)np,
           (long long)nq, (long long)nrec, min_u);
    double cells = 0;
    for (int64_t i = 0; i < np; ++i) {
        const sw_pair& pr = pairs[order[(size_t)i]];
        const sw_result& r = res[order[(size_t)i]];
        const long long M = qoffs[(size_t)pr.query + 1] - qoffs[(size_t)pr.query] + 1;
        cells += (double)(M - 1) * (double)(offs[(size_t)pr.target + 1] - offs[(size_t)pr.target]);
        printf("%lld\t%lld\t%s\t%lld\t%lld\t%lld ungapped=%d\n", (long long)pr.query, (long long)pr.target, names[(size_t)pr.target].c_str(), (long long)r.max_score,
               (long long)(r.max_pos / M), (long long)(r.max_pos % M), u[pr.query * nrec + pr.target]);
    }
    printf("\nElapsed time for database search: %f (%.1f GCUPS over the rescored pairs; filter and %lld pairs in two calls, handle prepared in %f)\n\n", t2 - t1,
           t2 > t1 ? cells / (t2 - t1) / 1e9 : 0.0, (long long)np, t1 - t0);
    sw_db_free(handle);
    (void)sw_device_free(ctx, d_q); (void)sw_device_free(ctx, d_db); (void)sw_device_free(ctx, d_out);
    sw_destroy(ctx);
    return 0;
}

int main(int argc, char** argv) {
    long long cols = 8, rows = 9;
    bool builtin = true, dump = false, labels = false, h64 = false, backtrack = true, p8 = false;
    std::vector<int> devices;
    unsigned seed = 1;
    const char *fasta_a = nullptr, *fasta_b = nullptr;
    long long rec_a = 0, rec_b = 0;
    const char *search_q = nullptr, *search_db = nullptr;
    long long top = 10, min_score = 0, prefilter = 0, prefilter_hits = 0;
    bool has_min_score = false, has_top = false, has_prefilter = false, has_prefilter_hits = false;
    const char *pairs_path = nullptr, *pssm_path = nullptr;
    AffineArgs af;
    bool align = false, all_queries = false, align_ckpt = false;
    int search_lanes = 32, pairs_lanes = 32;
    bool has_search_lanes = false, has_pairs_lanes = false;
    int iterations = 1, include_score = 1, prior_weight = 10, weight_hits = 0;
    bool has_weight_hits = false;
    bool has_iter_flag = false;
    const char *out_pssm = nullptr, *out_a3m = nullptr;
    sw_scores sc = {3, -3, -2};
    int npos = 0;
    for (int ai = 1; ai < argc; ++ai) {
        std::string f = argv[ai];
        if (f[0] != '-' && npos < 2 && ai + (1 - npos) < argc) {   // <cols> <rows>, anywhere on the line
            (npos == 0 ? cols : rows) = strtoll(argv[ai], nullptr, 10);
            builtin = false;
            ++npos;
        }
        else if (f == "--dump") dump = true;
        else if (f == "--dump-labels") dump = labels = true;
        else if (f == "--h64") h64 = true;
        else if (f == "--no-backtrack") backtrack = false;
        else if (f == "--p8") p8 = true;
        else if (f == "--gpus" && ai + 1 < argc) { const int n = atoi(argv[++ai]); for (int g = 0; g < n; ++g) devices.push_back(g); }
        else if (f == "--devices" && ai + 1 < argc) { for (char* t = strtok(argv[++ai], ","); t; t = strtok(nullptr, ",")) devices.push_back(atoi(t)); }
        else if (f == "--fasta" && ai + 2 < argc) { fasta_a = argv[++ai]; fasta_b = argv[++ai]; builtin = false; }
        else if (f == "--search" && ai + 3 < argc && std::string(argv[ai + 1]) == "--pssm") { ai += 1; search_q = pssm_path = argv[++ai]; search_db = argv[++ai]; builtin = false; }
        else if (f == "--search" && ai + 2 < argc) { search_q = argv[++ai]; search_db = argv[++ai]; builtin = false; }
        else if (f == "--top" && ai + 1 < argc) { top = strtoll(argv[++ai], nullptr, 10); has_top = true; }
        else if (f == "--pairs" && ai + 1 < argc) pairs_path = argv[++ai];
        else if (f == "--min-score" && ai + 1 < argc) { int v = 0; if (!parse_int("--min-score", argv[++ai], &v)) return 2; min_score = v; has_min_score = true; }
        else if (f == "--prefilter" && ai + 1 < argc) { int v = 0; if (!parse_int("--prefilter", argv[++ai], &v)) return 2; prefilter = v; has_prefilter = true; }
        else if (f == "--prefilter-hits" && ai + 1 < argc) { int v = 0; if (!parse_int("--prefilter-hits", argv[++ai], &v)) return 2; prefilter_hits = v; has_prefilter_hits = true; }
        else if (f == "--search-lanes" && ai + 1 < argc) { if (!parse_int("--search-lanes", argv[++ai], &search_lanes)) return 2; has_search_lanes = true; }
        else if (f == "--pairs-lanes" && ai + 1 < argc) { if (!parse_int("--pairs-lanes", argv[++ai], &pairs_lanes)) return 2; has_pairs_lanes = true; }
        else if (f == "--iterations" && ai + 1 < argc) { if (!parse_int("--iterations", argv[++ai], &iterations)) return 2; has_iter_flag = true; }
        else if (f == "--include-score" && ai + 1 < argc) { if (!parse_int("--include-score", argv[++ai], &include_score)) return 2; has_iter_flag = true; }
        else if (f == "--prior-weight" && ai + 1 < argc) { if (!parse_int("--prior-weight", argv[++ai], &prior_weight)) return 2; has_iter_flag = true; }
        else if (f == "--out-pssm" && ai + 1 < argc) { out_pssm = argv[++ai]; has_iter_flag = true; }
        else if (f == "--out-a3m" && ai + 1 < argc) { out_a3m = argv[++ai]; has_iter_flag = true; }
        else if (f == "--weight-hits" && ai + 1 < argc) { if (!parse_int("--weight-hits", argv[++ai], &weight_hits)) return 2; has_weight_hits = true; }
        else if (f == "--matrix" && ai + 1 < argc) { af.matrix = argv[++ai]; af.on = true; }
        else if (f == "--gap-open" && ai + 1 < argc) { if (!parse_int("--gap-open", argv[++ai], &af.open)) return 2; af.has_open = af.on = true; }
        else if (f == "--gap-extend" && ai + 1 < argc) { if (!parse_int("--gap-extend", argv[++ai], &af.extend)) return 2; af.has_extend = true; }
        else if (f == "--align") align = true;
        else if (f == "--align-checkpoint") align_ckpt = true;
        else if (f == "--all-queries") all_queries = true;
        else if (f == "--record-a" && ai + 1 < argc) rec_a = strtoll(argv[++ai], nullptr, 10);
        else if (f == "--record-b" && ai + 1 < argc) rec_b = strtoll(argv[++ai], nullptr, 10);
        else if (f == "--seed" && ai + 1 < argc) seed = (unsigned)strtoul(argv[++ai], nullptr, 10);
        else if (f == "--scores" && ai + 3 < argc) { sc.match = atoi(argv[++ai]); sc.mismatch = atoi(argv[++ai]); sc.gap = atoi(argv[++ai]); }
        else { fprintf(stderr, "usage: smithW [<cols> <rows> | --fasta A.fa B.fa [--record-a I] [--record-b J] | --search QUERY.fa DB.fa [--record-a I] [--top K] [--all-queries [--min-score S] [--prefilter S | --prefilter-hits S [--pairs-lanes 16|32]] [--search-lanes 16|32]] [--pairs FILE [--pairs-lanes 16|32]] [--matrix FILE] [--gap-open O] [--gap-extend E] [--align [--align-checkpoint]] | --search --pssm FILE DB.fa --gap-open O --gap-extend E [--top K] [--min-score S] [--align] [--search-lanes 16|32] | with --all-queries or --pssm: [--iterations N] [--include-score S] [--prior-weight W] [--out-pssm PREFIX] [--align --out-a3m PREFIX: the A3M of the last round's hits per query, PREFIX.<query>.a3m; with --pssm it holds no query record] [--weight-hits P: Henikoff weights on the device, N[j] then counts in units of P, so scale --prior-weight with it]] [--seed N] [--dump | --dump-labels] [--h64] [--no-backtrack] [--scores M X G] [--gpus N | --devices 0,1,..] [--p8]\n"); return 2; }
    }
    if (npos == 1) { fprintf(stderr, "smithW: <cols> needs <rows>\n"); return 2; }
    if (align_ckpt && !(search_q && align)) { fprintf(stderr, "smithW: --align-checkpoint goes with --search --align\n"); return 2; }
    if (has_search_lanes) {   // the many-query search alone has the two kinds of lanes
        if (search_lanes != 16 && search_lanes != 32) { fprintf(stderr, "smithW: --search-lanes takes 16 or 32, got %d\n", search_lanes); return 2; }
        if (!pssm_path && !(search_q && all_queries)) { fprintf(stderr, "smithW: --search-lanes goes with --search --all-queries or --search --pssm\n"); return 2; }
        if (has_prefilter || has_prefilter_hits || pairs_path) { fprintf(stderr, "smithW: --search-lanes does not go with --prefilter / --prefilter-hits / --pairs\n"); return 2; }
    }
    if (has_pairs_lanes) {   // the rescoring of a pair list alone has this choice
        if (pairs_lanes != 16 && pairs_lanes != 32) { fprintf(stderr, "smithW: --pairs-lanes takes 16 or 32, got %d\n", pairs_lanes); return 2; }
        if (!search_q || pssm_path || !(pairs_path || has_prefilter_hits)) { fprintf(stderr, "smithW: --pairs-lanes goes with --search --pairs or --search --all-queries --prefilter-hits\n"); return 2; }
    }
    if (has_iter_flag) {   // the iterative search: many sequence queries, or one matrix
        if (!(search_q && (all_queries || pssm_path))) { fprintf(stderr, "smithW: --iterations / --include-score / --prior-weight / --out-pssm / --out-a3m go with --search --all-queries or --search --pssm\n"); return 2; }
        if (iterations < 1) { fprintf(stderr, "smithW: --iterations N needs N >= 1, got %d\n", iterations); return 2; }
        if (prior_weight < 0 || prior_weight > 65535) { fprintf(stderr, "smithW: --prior-weight W needs W within 0..65535, got %d\n", prior_weight); return 2; }
        if (has_prefilter || has_prefilter_hits || pairs_path) { fprintf(stderr, "smithW: --iterations does not go with --prefilter / --prefilter-hits / --pairs\n"); return 2; }
    }
    const bool iterate = iterations > 1 || out_pssm || out_a3m;   // (--iterations 1 alone is the search of today, through today's path)
    if (out_a3m && !align) { fprintf(stderr, "smithW: --out-a3m writes the alignment of the aligned hits: it goes with --align\n"); return 2; }
    if (has_weight_hits) {   // the weights feed the update of an iterative search and nothing else
        if (!(has_iter_flag && iterate)) { fprintf(stderr, "smithW: --weight-hits goes with --iterations N (N > 1) or --out-pssm\n"); return 2; }
        if (weight_hits < 1 || weight_hits > 65535) { fprintf(stderr, "smithW: --weight-hits P needs P within 1..65535, got %d\n", weight_hits); return 2; }
    }
    if (pssm_path) {   // the matrix is the query and the scoring at once
        if (af.matrix) { fprintf(stderr, "smithW: --pssm does not go with --matrix\n"); return 2; }
        if (all_queries) { fprintf(stderr, "smithW: --pssm does not go with --all-queries (the file is the one query)\n"); return 2; }
        if (pairs_path) { fprintf(stderr, "smithW: --pssm does not go with --pairs\n"); return 2; }
        if (has_prefilter || has_prefilter_hits) { fprintf(stderr, "smithW: --pssm does not go with --prefilter / --prefilter-hits\n"); return 2; }
        if (!af.has_open || !af.has_extend) { fprintf(stderr, "smithW: --pssm needs --gap-open O and --gap-extend E\n"); return 2; }
        if (iterate) {
            if (sc.match < -128 || sc.match > 127 || sc.mismatch < -128 || sc.mismatch > 127) { fprintf(stderr, "smithW: --pssm --iterations takes its table from --scores M X within -128..127, got %d %d\n", sc.match, sc.mismatch); return 2; }
            return search_iter_main(nullptr, pssm_path, search_db, top, min_score, sc, af, align, align_ckpt, search_lanes, iterations, include_score, prior_weight, out_pssm, weight_hits, out_a3m);
        }
        return search_pssm_main(pssm_path, search_db, top, min_score, af, align, align_ckpt, search_lanes);
    }
    if (search_q) {
        if (af.on && !af.matrix && (sc.match < -128 || sc.match > 127 || sc.mismatch < -128 || sc.mismatch > 127)) {   // (sw_submat_match would clamp them)
            fprintf(stderr, "smithW: --gap-open without --matrix needs --scores M X within -128..127 (a table of signed bytes), got %d %d\n", sc.match, sc.mismatch);
            return 2;
        }
        if (af.has_extend && !af.on) sc.gap = af.extend;   // --gap-extend alone: gap_open = 0 is the linear recurrence, and its kernel is the cheaper one
        if (align && !af.on && (sc.match < -128 || sc.match > 127 || sc.mismatch < -128 || sc.mismatch > 127)) {
            fprintf(stderr, "smithW: --align on a linear search needs --scores M X within -128..127 (a table of signed bytes), got %d %d\n", sc.match, sc.mismatch);
            return 2;
        }
        if (has_prefilter_hits) {
            if (!all_queries) { fprintf(stderr, "smithW: --prefilter-hits goes with --search --all-queries\n"); return 2; }
            if (has_prefilter) { fprintf(stderr, "smithW: --prefilter-hits does not go with --prefilter\n"); return 2; }
            if (pairs_path) { fprintf(stderr, "smithW: --prefilter-hits does not go with --pairs\n"); return 2; }
            if (prefilter_hits < 1) { fprintf(stderr, "smithW: --prefilter-hits S needs S >= 1, got %lld\n", prefilter_hits); return 2; }
        }
        if (has_prefilter) {
            if (!all_queries) { fprintf(stderr, "smithW: --prefilter goes with --search --all-queries\n"); return 2; }
            if (has_top) { fprintf(stderr, "smithW: --prefilter does not go with --top\n"); return 2; }
            if (has_min_score) { fprintf(stderr, "smithW: --prefilter does not go with --min-score\n"); return 2; }
            if (align) { fprintf(stderr, "smithW: --prefilter does not go with --align\n"); return 2; }
            if (pairs_path) { fprintf(stderr, "smithW: --prefilter does not go with --pairs\n"); return 2; }
            if (prefilter < 1) { fprintf(stderr, "smithW: --prefilter S needs S >= 1, got %lld\n", prefilter); return 2; }
            if (!af.matrix && (sc.match < -128 || sc.match > 127 || sc.mismatch < -128 || sc.mismatch > 127)) {
                fprintf(stderr, "smithW: --prefilter without --matrix needs --scores M X within -128..127 (a table of signed bytes), got %d %d\n", sc.match, sc.mismatch);
                return 2;
            }
            return search_prefilter_main(search_q, search_db, prefilter, sc, af);
        }
        if (pairs_path) {
            if (all_queries) { fprintf(stderr, "smithW: --pairs does not go with --all-queries\n"); return 2; }
            if (has_top) { fprintf(stderr, "smithW: --pairs does not go with --top\n"); return 2; }
            if (has_min_score) { fprintf(stderr, "smithW: --pairs does not go with --min-score\n"); return 2; }
            if (align) { fprintf(stderr, "smithW: --pairs does not go with --align\n"); return 2; }
            if (!af.matrix && (sc.match < -128 || sc.match > 127 || sc.mismatch < -128 || sc.mismatch > 127)) {
                fprintf(stderr, "smithW: --pairs without --matrix needs --scores M X within -128..127 (a table of signed bytes), got %d %d\n", sc.match, sc.mismatch);
                return 2;
            }
            return search_pairs_main(search_q, search_db, pairs_path, sc, af, pairs_lanes);
        }
        if (all_queries) {
            if (!af.matrix && (sc.match < -128 || sc.match > 127 || sc.mismatch < -128 || sc.mismatch > 127)) {
                fprintf(stderr, "smithW: --all-queries without --matrix needs --scores M X within -128..127 (a table of signed bytes), got %d %d\n", sc.match, sc.mismatch);
                return 2;
            }
            if (iterate) return search_iter_main(search_q, nullptr, search_db, top, min_score, sc, af, align, align_ckpt, search_lanes, iterations, include_score, prior_weight, out_pssm, weight_hits, out_a3m);
            return search_all_main(search_q, search_db, top, min_score, sc, af, align, align_ckpt, prefilter_hits, search_lanes, pairs_lanes);
        }
        if (has_min_score) { fprintf(stderr, "smithW: --min-score goes with --search --all-queries\n"); return 2; }
        return search_main(search_q, rec_a, search_db, top, sc, af, align, align_ckpt);
    }
    if (has_prefilter_hits) { fprintf(stderr, "smithW: --prefilter-hits goes with --search --all-queries\n"); return 2; }
    if (has_prefilter) { fprintf(stderr, "smithW: --prefilter goes with --search --all-queries\n"); return 2; }
    if (pairs_path) { fprintf(stderr, "smithW: --pairs goes with --search\n"); return 2; }
    if (all_queries) { fprintf(stderr, "smithW: --all-queries goes with --search\n"); return 2; }
    if (has_min_score) { fprintf(stderr, "smithW: --min-score goes with --search --all-queries\n"); return 2; }
    if (align) { fprintf(stderr, "smithW: --align goes with --search\n"); return 2; }
    if (af.on || af.has_extend) { fprintf(stderr, "smithW: --matrix / --gap-open / --gap-extend go with --search\n"); return 2; }
    if (fasta_a) {
        int64_t la = 0, lb = 0;
        CHECK(sw_read_fasta(fasta_a, rec_a, nullptr, 0, &la));
        CHECK(sw_read_fasta(fasta_b, rec_b, nullptr, 0, &lb));
        cols = la; rows = lb;
    }
    const long long m = cols + 1, n = rows + 1;
    std::vector<char> a(m + 1), b(n + 1);
    if (fasta_a) {
        int64_t la = 0, lb = 0;
        CHECK(sw_read_fasta(fasta_a, rec_a, a.data(), cols, &la));
        CHECK(sw_read_fasta(fasta_b, rec_b, b.data(), rows, &lb));
    } else if (builtin) { memcpy(b.data(), "GGTTGACTA", 9); memcpy(a.data(), "TGTTACGG", 8); }
    else CHECK(sw_generate(cols, rows, seed, a.data(), b.data()));
    if (dump) { if (builtin) printf("\n Using built-in data for testing .."); printf("\nMatrix[%lld][%lld]\n", rows, cols); }
    else {
        // the lines omp_smithW-v1-refinedOrig.cpp:119,138-142 print (there both matrices and both sequences are ints; here the
        // footprint is what is resident in HBM: H int32 | int64, P int32 | int8, one byte per letter)
        printf("Problem size: Matrix[%lld][%lld]\n", n, m);
        const unsigned long long sz = ((unsigned long long)(m + n) + (unsigned long long)m * n * ((h64 ? 8 : 4) + (p8 && !devices.empty() ? 1 : 4))) / 1024 / 1024;
        if (sz >= 1024) printf("Total memory footprint is:%llu GB\n", sz / 1024);
        else printf("Total memory footprint is:%llu MB\n", sz);
    }

    if (!devices.empty()) {
        // ---- one matrix over several GPUs: row bands, one band-resident launch per GPU, halo rows relayed over xGMI ----
        sw_multi* mh = nullptr;
        CHECK(sw_multi_create(devices.data(), (int)devices.size(), a.data(), cols, b.data(), rows, p8 ? 1 : 4, 1, &mh));
        sw_result res;
        CHECK(sw_multi_fill(mh, &sc, 64, &res));    // untimed: sizes the workspaces
        CHECK(sw_multi_fill(mh, &sc, 64, &res));
        printf("\nElapsed time for scoring matrix computation: %f\n\n", sw_multi_seconds(mh));
        double t0 = now_s();
        int64_t plen = 0;
        if (backtrack) CHECK(sw_multi_traceback(mh, &plen));
        printf("\nElapsed time for backtracking: %f\n\n", now_s() - t0);
        printf("maxPos = %lld, H[maxPos] = %lld, path length = %lld  (%d row bands)\n", (long long)res.max_pos, (long long)res.max_score,
               (long long)plen, sw_multi_nbands(mh));
        sw_multi_free(mh);
        return 0;
    }
    sw_ctx* ctx = nullptr;
    CHECK(sw_create(0, &ctx));
    const size_t cells = (size_t)m * (size_t)n;
    void *d_a, *d_b, *d_H, *d_P, *d_res;
    CHECK(sw_device_malloc(ctx, (size_t)cols + 16, &d_a));
    CHECK(sw_device_malloc(ctx, (size_t)rows + 16, &d_b));
    CHECK(sw_device_malloc(ctx, sizeof(sw_result), &d_res));
    CHECK(sw_memcpy_h2d(ctx, d_a, a.data(), (size_t)cols));
    CHECK(sw_memcpy_h2d(ctx, d_b, b.data(), (size_t)rows));
    // output matrices placed for speed (allocation is outside the reference's timer as well, serial_smithW.c:96-103,137)
    CHECK(sw_alloc_outputs(ctx, (const char*)d_a, cols, (const char*)d_b, rows, &sc, h64 ? 8 : 4, 4, cells >= (1u << 24) ? 0 : 1, &d_H, &d_P, nullptr));
    // one untimed call sizes the workspace (the reference's timer also excludes its allocations)
    CHECK(sw_fill_device(ctx, (const char*)d_a, cols, (const char*)d_b, rows, &sc, d_H, h64 ? 8 : 4, (int32_t*)d_P, nullptr, (sw_result*)d_res, nullptr));
    CHECK(sw_synchronize(ctx, nullptr));

    if (backtrack) {   // ... and loads the traceback kernel (first use of a kernel pays for its code object): a walk of nothing on a 1 x 1 matrix
        void *d_p1, *d_r1;
        CHECK(sw_device_malloc(ctx, 4 * sizeof(int32_t), &d_p1));
        CHECK(sw_device_malloc(ctx, sizeof(sw_result), &d_r1));
        const int32_t zeros[4] = {0, 0, 0, 0}; const sw_result r0 = {0, 0, 0};
        CHECK(sw_memcpy_h2d(ctx, d_p1, zeros, sizeof zeros));
        CHECK(sw_memcpy_h2d(ctx, d_r1, &r0, sizeof r0));
        CHECK(sw_traceback_device(ctx, (int32_t*)d_p1, 1, 1, 3, nullptr, 0, (sw_result*)d_r1, nullptr));
        CHECK(sw_synchronize(ctx, nullptr));
        sw_device_free(ctx, d_p1); sw_device_free(ctx, d_r1);
    }

    double t0 = now_s();
    CHECK(sw_fill_device(ctx, (const char*)d_a, cols, (const char*)d_b, rows, &sc, d_H, h64 ? 8 : 4, (int32_t*)d_P, nullptr, (sw_result*)d_res, nullptr));
    CHECK(sw_synchronize(ctx, nullptr));
    double t1 = now_s();
    printf("\nElapsed time for scoring matrix computation: %f\n\n", t1 - t0);
    sw_result res;
    CHECK(sw_memcpy_d2h(ctx, &res, d_res, sizeof res));
    if (res.path_len < 0) { fprintf(stderr, "smithW: device hand-off timed out\n"); return 1; }

    t0 = now_s();
    if (backtrack) {
        CHECK(sw_traceback_device(ctx, (int32_t*)d_P, cols, rows, res.max_pos, nullptr, 0, (sw_result*)d_res, nullptr));
        CHECK(sw_synchronize(ctx, nullptr));
        CHECK(sw_memcpy_d2h(ctx, &res, d_res, sizeof res));
    }
    t1 = now_s();
    printf("\nElapsed time for backtracking: %f\n\n", t1 - t0);
    printf("maxPos = %lld, H[maxPos] = %lld, path length = %lld\n", (long long)res.max_pos,
           (long long)res.max_score, (long long)res.path_len);

    int rc = 0;
    if (dump || builtin) {
        std::vector<int32_t> H(cells), P(cells);
        if (h64) {
            std::vector<int64_t> H8(cells);
            CHECK(sw_memcpy_d2h(ctx, H8.data(), d_H, cells * 8));
            for (size_t k = 0; k < cells; ++k) H[k] = (int32_t)H8[k];
        } else CHECK(sw_memcpy_d2h(ctx, H.data(), d_H, cells * 4));
        CHECK(sw_memcpy_d2h(ctx, P.data(), d_P, cells * 4));
        if (dump) { printf("\nSimilarity Matrix:\n"); if (labels) print_matrix_labelled(H, n, m, a.data(), b.data()); else print_matrix(H, n, m); }
        if (builtin) {
            // the reference's built-in checks: serial_smithW.c:162-166, omp_smithW-v1-refinedOrig.cpp:229-238
            const bool ok = H[m * n - 1] == 7 && res.max_pos == 69 && res.max_score == 13;
            printf("Verifying correctness using builtin data =%d\n", ok);
            if (!ok) rc = 1;
        }
        if (dump) { printf("\nPredecessor Matrix:\n"); if (labels) print_pred_labelled(P, n, m, a.data(), b.data()); else print_pred(P, n, m); }
    }
    sw_device_free(ctx, d_a); sw_device_free(ctx, d_b); sw_free_outputs(ctx, d_H, d_P); sw_device_free(ctx, d_res);
    sw_destroy(ctx);
    return rc;
}
