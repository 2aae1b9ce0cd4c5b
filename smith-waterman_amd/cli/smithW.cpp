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
//     ... --evalue E          with --all-queries or --pssm (also with --iterations): only hits whose E-value is at most E > 0 are printed, and every hit line
//                              ends in " E=<E-value>".  The E-values come from the scores of the search itself, per query: the search collects a histogram
//                              of every target's score by length class on the device (sw_db_search_affine_top_stats / sw_db_search_pssm_top_stats), the host
//                              fits the unrelated targets' line and spread to it (sw_score_fit_hist) and derives a score threshold per length class
//                              (sw_score_thresholds); a database too small for a fit (fewer than 30 targets) drops nothing and prints E=nan.  The histograms
//                              come to the host: 40 KiB per query and one synchronisation per round.  Not with --prefilter, --prefilter-hits or --pairs
//     ... --include-evalue E  with --iterations N (N > 1), in the place of --include-score: every round thresholds a COPY of its hit table by E-value on the
//                              device (sw_hits_threshold_device); the copy goes to the weights, the update and --out-a3m, the untouched table to the aligner
//                              and the printer
//     ... --score-shift N     with --evalue / --include-evalue: the histogram's bins are 2^N scores wide (0..16, default 0; 256 bins, the last one open)
//     ... --mask              with every --search mode: after the upload the database's low-complexity regions are masked on the device
//                              (sw_db_mask_low_complexity: SEG's first stage in integers) into a second buffer; the search, the selection, the statistics,
//                              the alignment and the PSSM update run on the MASKED copy, so printed alignments show the mask byte -- what was scored --,
//                              while --out-a3m writes its rows through the unmasked handle: the file carries the original letters.  One line on
//                              stderr says how many letters of how many targets were masked.  --mask-window W (2..64, default 12), --mask-trigger MB
//                              and --mask-extend MB (thousandths of a bit, defaults 2200 and 2500), --mask-byte C (default X), --mask-letters STR
//                              (the alphabet, default the 20 amino acids; every other byte is no letter)
//   smithW --search --pssm FILE DB.fa --gap-open O --gap-extend E [--top K] [--min-score S] [--align] [--search-lanes 16|32]
//                              the ONE query is a position-specific scoring matrix, PSI-BLAST's ASCII PSSM (sw_read_pssm), searched through a prepared
//                              handle (sw_db_search_pssm_top, sw_db_align_pssm_hits); the output is that of --all-queries for one record, the Q line of an
//                              alignment the matrix's consensus (per column the first letter with the largest entry)
// Extra flags: --seed N  --dump | --dump-labels (the header-row printers of omp_smithW.c)  --h64  --no-backtrack  --scores M X G  --record-a I  --record-b J
//   --gpus N | --devices 0,1,..   ONE matrix over several GPUs (row bands, sw_multi_*; an id may repeat)  --p8  int8 P
// The DP fill runs on the GPU through the C-ABI (include/swhip.h); stdout keeps the two
// "Elapsed time ..." lines the reference's run scripts grep for (readme.liao:12).
#include <chrono>
#include "cli_parts.h"

#define RESET "\033[0m"
#define BOLDRED "\033[1m\033[31m"

static double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

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
// a whole decimal integer or nothing: "-x", "" and "3k" are errors, not 0 or 3
static bool parse_int(const char* flag, const char* text, int* out) {
    char* end = nullptr;
    const long v = strtol(text, &end, 10);
    if (end == text || *end || v < -(1l << 30) || v > (1l << 30)) { fprintf(stderr, "smithW: %s needs an integer, got \"%s\"\n", flag, text); return false; }
    *out = (int)v;
    return true;
}
// ... and a whole decimal number
static bool parse_real(const char* flag, const char* text, double* out) {
    char* end = nullptr;
    const double v = strtod(text, &end);
    if (end == text || *end) { fprintf(stderr, "smithW: %s needs a number, got \"%s\"\n", flag, text); return false; }
    *out = v;
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

// The hit block of one query: the header line, its K hits in rank order and, with `align`, every hit's alignment: the row `done` of a
// call that aligned every query's hits or -- `done` empty -- the K hits re-filled with directions and walked on the device here.
// --evalue: `keep` says which of the K hits are printed (the ranks count those), `fit` gives every printed line its " E=" field.
static void print_hits(sw_ctx* ctx, const char* q, int64_t qlen, const char* d_q, const Db& db, const DeviceBuffer& d_db, const sw_hit* hits, long long K, bool align,
                       const sw_affine& aff, const AlignedHits& done = AlignedHits(), const int32_t* keep = nullptr, const sw_score_fit* fit = nullptr) {
    std::vector<int64_t> order((size_t)K);
    for (long long i = 0; i < K; ++i) order[(size_t)i] = hits[i].target;
    AlignedHits here;   // --align without `done`: ops of at most query + longest hit letters each
    if (align && K > 0 && done.empty()) {
        int64_t ops_cap = 0;
        for (long long i = 0; i < K; ++i) ops_cap = std::max(ops_cap, qlen + db.len(order[(size_t)i]));
        DeviceBuffer d_aln(ctx, (size_t)K * sizeof(sw_alignment)), d_ops(ctx, (size_t)K * (size_t)ops_cap);
        CHECK(sw_align_affine_device(ctx, d_q, qlen, d_db.as<const char>(), db.offsets.data(), db.nrec, order.data(), K, &aff, d_aln.as<sw_alignment>(),
                                     d_ops.as<char>(), ops_cap, nullptr));
        CHECK(sw_synchronize(ctx, nullptr));
        here = download_aligned(d_aln, d_ops, (size_t)K, ops_cap);
    }
    const AlignedHits& got = done.empty() ? here : done;
    printf("# query %lld letters, %lld targets, %lld letters; rank\trecord\tscore\ttarget_end\tquery_end\n", (long long)qlen, (long long)db.nrec, (long long)db.total);
    long long rank = 0;
    for (long long i = 0; i < K; ++i) {
        if (keep && !keep[i]) continue;
        const sw_hit& r = hits[i];
        const long long te = r.max_pos / (qlen + 1), qe = r.max_pos % (qlen + 1);
        printf("%lld\t%lld\t%lld\t%lld\t%lld", ++rank, (long long)order[(size_t)i], (long long)r.max_score, te, qe);
        if (fit) printf(" E=%.2e", sw_score_evalue(fit, db.len(order[(size_t)i]), r.max_score));
        printf("\n");
        if (!align) continue;
        const sw_alignment& a = got.aln[(size_t)i];
        printf("align\t%lld\t%lld\t%lld\t%lld\t%lld\n", (long long)a.q_begin, (long long)a.q_end, (long long)a.t_begin, (long long)a.t_end, (long long)a.nops);
        const char* t = db.record(order[(size_t)i]);
        const char* op = got.ops_of(i);
        std::string lq, lm, lt;
        int64_t qi = a.q_begin, ti = a.t_begin;
        for (int64_t k = 0; k < a.nops; ++k) {
            if (op[k] == 'M') { lq += q[(size_t)qi]; lt += t[ti]; lm += q[(size_t)qi] == t[ti] ? '|' : ' '; ++qi; ++ti; }
            else if (op[k] == 'I') { lq += q[(size_t)qi]; lt += '-'; lm += ' '; ++qi; }
            else { lq += '-'; lt += t[ti]; lm += ' '; ++ti; }
        }
        printf("Q %s\n  %s\nT %s\n", lq.c_str(), lm.c_str(), lt.c_str());
    }
}

// --search: one query record against every record of a FASTA database on the GPU, the best --top hits by score (ties: lower record first)
static int search_main(const Options& o) {
    sw_scores sc = o.sc;
    if (o.af.has_extend && !o.af.on) sc.gap = o.af.extend;   // --gap-extend alone: gap_open = 0 is the linear recurrence, and its kernel is the cheaper one
    int64_t qlen = 0;
    CHECK(sw_read_fasta(o.search_q, o.rec_a, nullptr, 0, &qlen));
    std::vector<char> q((size_t)qlen + 1);
    CHECK(sw_read_fasta(o.search_q, o.rec_a, q.data(), qlen, &qlen));
    const Db db = read_db(o.search_db);
    Context ctx(0);
    if (o.align_ckpt) CHECK(sw_set_option(ctx, "align_checkpoint", 2));   // hits too large for whole direction matrices are aligned checkpointed
    DeviceBuffer d_q(ctx, q.data(), (size_t)qlen), d_db(ctx, db.letters.data(), (size_t)db.total), d_res(ctx, (size_t)(db.nrec > 0 ? db.nrec : 1) * sizeof(sw_result));
    const MaskedDb masked(ctx, o.mask, db, d_db);   // --mask: the search, the alignment and the printer see the masked copy from here on
    const Scoring s(o.af, sc);   // (a linear search without --align does not look at it)
    const double t0 = now_s();
    if (o.af.on) CHECK(sw_search_affine_device(ctx, d_q.as<const char>(), qlen, masked.buffer().as<const char>(), db.offsets.data(), db.nrec, &s.aff, d_res.as<sw_result>(), nullptr));
    else CHECK(sw_search_device(ctx, d_q.as<const char>(), qlen, masked.buffer().as<const char>(), db.offsets.data(), db.nrec, &sc, d_res.as<sw_result>(), nullptr));
    CHECK(sw_synchronize(ctx, nullptr));
    const double t1 = now_s();
    std::vector<sw_result> res((size_t)db.nrec);
    d_res.download(res.data(), (size_t)db.nrec * sizeof(sw_result));
    const std::vector<sw_hit> hits = rank_hits(res.data(), db.nrec, o.top, 0);
    print_hits(ctx, q.data(), qlen, d_q.as<const char>(), masked.db(), masked.buffer(), hits.data(), (long long)hits.size(), o.align, s.aff);
    print_elapsed(t1 - t0, (double)qlen * (double)db.total, nullptr);
    return 0;
}

// --search --all-queries: every record of the query file against the database through ONE prepared handle and one call
// (sw_db_create / sw_db_search_affine_top); the hit block of --search once per query, each under a line that names the record.  The K
// best hits of every query are selected on the device and only they come back; more than SW_TOP_MAX hits per query go the long way:
// the whole table to the host and a sort of every row.  A linear search goes through the match / mismatch table of --scores with
// gap_open 0, which sw_search_device equals bit for bit.
// --prefilter-hits S (prefilter_hits > 0): sw_db_search_affine_top_prefiltered takes the place of sw_db_search_affine_top -- the hits are
// selected among the pairs whose ungapped score reaches S, on the device from the rescored pair list; everything else is the same.
static int search_all_main(const Options& o) {
    const Db qs = read_db(o.search_q), db = read_db(o.search_db);
    const int64_t nq = qs.nrec, nrec = db.nrec;
    const long long K = std::max(0ll, std::min(o.top, (long long)nrec));
    const bool on_device = K <= SW_TOP_MAX, prefiltered = K > 0 && o.prefilter_hits > 0;
    if (o.prefilter_hits > 0 && !on_device) {
        fprintf(stderr, "smithW: --prefilter-hits selects on the device: min(--top, records) = %lld is above %d\n", K, SW_TOP_MAX);
        return 2;
    }
    if (o.has_evalue && !on_device) {
        fprintf(stderr, "smithW: --evalue takes its histogram inside the search that selects on the device: min(--top, records) = %lld is above %d\n", K, SW_TOP_MAX);
        return 2;
    }
    Context ctx(0);
    // --align-checkpoint: a table the one call would refuse for its worst pair goes through it checkpointed instead of query by query
    if (o.align_ckpt) CHECK(sw_set_option(ctx, "align_checkpoint", 2));
    CHECK(sw_set_option(ctx, "search_lanes", o.search_lanes));
    CHECK(sw_set_option(ctx, "search_pairs_lanes", o.pairs_lanes));
    // the pair list of --prefilter-hits: every pair, or as many as "search_results_mib" lets the call hold (56 bytes each)
    const int64_t pairs_cap = std::min<int64_t>(nq * nrec, (sw_get_option(ctx, "search_results_mib") << 20) / 56);
    int64_t npassed = 0;
    const size_t nres = on_device ? 1 : (size_t)std::max<int64_t>(1, nq * nrec), nhit = (size_t)std::max<int64_t>(1, nq * K);
    DeviceBuffer d_npairs(ctx, sizeof(int64_t)), d_q(ctx, qs.letters.data(), (size_t)qs.total), d_db(ctx, db.letters.data(), (size_t)db.total),
        d_res(ctx, nres * sizeof(sw_result)), d_hits(ctx, nhit * sizeof(sw_hit)), d_nhits(ctx, (size_t)std::max<int64_t>(1, nq) * sizeof(int64_t));
    const MaskedDb masked(ctx, o.mask, db, d_db);   // --mask: the search, the alignment and the printer see the masked copy from here on
    const Scoring s(o.af, o.sc);
    ScoreStats stats;   // --evalue: the histograms of the search
    if (o.has_evalue && K > 0) stats.alloc(ctx, nq, o.score_shift);
    DbHandle handle;
    const double t0 = now_s();
    handle.create(ctx, masked.buffer(), db.offsets, nrec);
    const double t1 = now_s();
    if (!on_device) CHECK(sw_db_search_affine(ctx, handle, d_q.as<const char>(), qs.offsets.data(), nq, &s.aff, d_res.as<sw_result>(), nullptr));
    else if (stats)
        CHECK(sw_db_search_affine_top_stats(ctx, handle, d_q.as<const char>(), qs.offsets.data(), nq, &s.aff, K, o.min_score, d_hits.as<sw_hit>(), d_nhits.as<int64_t>(),
                                            o.score_shift, stats.d_hist.as<uint32_t>(), nullptr));
    else if (prefiltered)
        CHECK(sw_db_search_affine_top_prefiltered(ctx, handle, d_q.as<const char>(), qs.offsets.data(), nq, &s.aff, o.prefilter_hits, pairs_cap, K, o.min_score,
                                                  d_hits.as<sw_hit>(), d_nhits.as<int64_t>(), d_npairs.as<int64_t>(), nullptr));
    else if (K > 0)
        CHECK(sw_db_search_affine_top(ctx, handle, d_q.as<const char>(), qs.offsets.data(), nq, &s.aff, K, o.min_score, d_hits.as<sw_hit>(), d_nhits.as<int64_t>(), nullptr));
    CHECK(sw_synchronize(ctx, nullptr));
    const double t2 = now_s();
    if (prefiltered) {
        d_npairs.download(&npassed, sizeof npassed);
        if (npassed > pairs_cap) {   // the table was built from the pairs the list happened to keep: not a result
            fprintf(stderr, "smithW: --prefilter-hits %lld: %lld pairs pass the pre-filter, the list holds %lld: raise S\n", o.prefilter_hits, (long long)npassed,
                    (long long)pairs_cap);
            return 1;
        }
    }
    std::vector<sw_hit> hits(nhit);
    std::vector<int64_t> nhits((size_t)nq + 1, 0);
    if (on_device && K > 0) {
        d_hits.download(hits.data(), (size_t)(nq * K) * sizeof(sw_hit));
        d_nhits.download(nhits.data(), (size_t)nq * sizeof(int64_t));
    }
    std::vector<sw_result> res(nres);
    if (!on_device) d_res.download(res.data(), (size_t)(nq * nrec) * sizeof(sw_result));
    std::vector<int32_t> keep;   // --evalue: the hits at or above the threshold of their length class
    if (stats) {
        stats.fit_last_search();
        keep.resize(nhit);
        CHECK(sw_hits_threshold_host(db.offsets.data(), nrec, stats.thresholds(o.evalue), nq, K, hits.data(), nhits.data(), nullptr, keep.data(), nullptr));
    }
    // --align: the hits of every query in ONE call on the device table as the selection left it (sw_db_align_affine_hits), ops of at most
    // longest query + longest target letters each; a table of ops beyond 1 GiB, or one the call refuses, goes query by query instead (print_hits)
    AlignedHits aligned;
    if (o.align && on_device && K > 0 && nq > 0) {
        const int64_t ops_cap = qs.longest() + handle.longest();
        const size_t n = (size_t)(nq * K);
        if ((double)n * (double)ops_cap <= (double)(1ll << 30)) {
            DeviceBuffer d_aln(ctx, n * sizeof(sw_alignment)), d_ops(ctx, n * (size_t)ops_cap);
            // the call refuses by the worst pair the table COULD name (longest target x longest query against "align_workspace_mib");
            // the hits of such a table may still fit one by one: those go query by query, as they always did (print_hits reports what is left)
            const int rc = sw_db_align_affine_hits(ctx, handle, d_q.as<const char>(), qs.offsets.data(), nq, &s.aff, d_hits.as<const sw_hit>(), d_nhits.as<const int64_t>(),
                                                   K, d_aln.as<sw_alignment>(), d_ops.as<char>(), ops_cap, nullptr);
            if (rc != SW_OK && rc != SW_EINVAL) fail("sw_db_align_affine_hits", rc);
            if (rc == SW_EINVAL) fprintf(stderr, "smithW: the one alignment call on the hit table was refused (%s); aligning query by query\n", sw_last_error());
            if (rc == SW_OK) {
                CHECK(sw_synchronize(ctx, nullptr));
                aligned = download_aligned(d_aln, d_ops, n, ops_cap);
            }
        }
    }
    for (int64_t i = 0; i < nq; ++i) {
        printf("## query record %lld of %s\n", (long long)i, o.search_q);
        const std::vector<sw_hit> ranked = on_device ? std::vector<sw_hit>() : rank_hits(res.data() + i * nrec, nrec, K, o.min_score);
        const sw_hit* row = on_device ? hits.data() + i * K : ranked.data();
        const long long n = on_device ? (long long)nhits[(size_t)i] : (long long)ranked.size();
        print_hits(ctx, qs.record(i), qs.len(i), d_q.as<const char>() + qs.offsets[(size_t)i], masked.db(), masked.buffer(), row, n, o.align, s.aff, aligned.only_row(i, K),
                   stats ? keep.data() + i * K : nullptr, stats ? &stats.fit[(size_t)i] : nullptr);
    }
    const double cells = (double)qs.total * (double)db.total;
    if (o.prefilter_hits > 0)
        print_elapsed(t2 - t1, cells, "; %lld queries in one call, %lld of %lld pairs passed the pre-filter U >= %lld, handle prepared in %f", (long long)nq,
                      (long long)npassed, (long long)(nq * nrec), o.prefilter_hits, t1 - t0);
    else print_elapsed(t2 - t1, cells, "; %lld queries in one call, handle prepared in %f", (long long)nq, t1 - t0);
    return 0;
}

// --search --pssm FILE DB.fa: ONE position-specific scoring matrix (PSI-BLAST's ASCII format, sw_read_pssm) as the one query against the
// database, through a prepared handle: sw_db_search_pssm_top (or, for more than SW_TOP_MAX hits, sw_db_search_pssm and a sort on the
// host) and, with --align, one sw_db_align_pssm_hits call on the device hit table.  The output is the output of --all-queries for a file
// of one record; the query line of an alignment is the matrix's consensus, '|' where the target has that letter.
static int search_pssm_main(const Options& o) {
    Pssm m;
    read_pssm_file(o.pssm_path, &m);
    const Db db = read_db(o.search_db);
    const int64_t ncols = m.ncols, nrec = db.nrec;
    const sw_pssm_scoring scoring = {m.letters, m.nletters, m.other, m.smax, o.af.has_open ? o.af.open : 0, o.af.has_extend ? o.af.extend : 0};
    const std::string query = consensus(m, m.matrix.data(), ncols);
    const int64_t qoffs[2] = {0, ncols};
    const long long K = std::max(0ll, std::min(o.top, (long long)nrec));
    const bool on_device = K <= SW_TOP_MAX, align = o.align && K > 0;
    if (o.align && !on_device) { fprintf(stderr, "smithW: --pssm --align aligns a device hit table: min(--top, records) = %lld is above %d\n", K, SW_TOP_MAX); return 2; }
    if (o.has_evalue && !on_device) {
        fprintf(stderr, "smithW: --evalue takes its histogram inside the search that selects on the device: min(--top, records) = %lld is above %d\n", K, SW_TOP_MAX);
        return 2;
    }
    Context ctx(0);
    if (o.align_ckpt) CHECK(sw_set_option(ctx, "align_checkpoint", 2));
    CHECK(sw_set_option(ctx, "search_lanes", o.search_lanes));
    const size_t nres = on_device ? 1 : (size_t)std::max<int64_t>(1, nrec), nhit = (size_t)std::max<long long>(1, K);
    DeviceBuffer d_pssm(ctx, m.matrix.data(), m.matrix.size()), d_db(ctx, db.letters.data(), (size_t)db.total), d_res(ctx, nres * sizeof(sw_result)),
        d_hits(ctx, nhit * sizeof(sw_hit)), d_nhits(ctx, sizeof(int64_t));
    const MaskedDb masked(ctx, o.mask, db, d_db);   // --mask: the search, the alignment and the printer see the masked copy from here on
    ScoreStats stats;   // --evalue: the histogram of the search
    if (o.has_evalue && K > 0) stats.alloc(ctx, 1, o.score_shift);
    DbHandle handle;
    const double t0 = now_s();
    handle.create(ctx, masked.buffer(), db.offsets, nrec);
    const double t1 = now_s();
    if (!on_device) CHECK(sw_db_search_pssm(ctx, handle, d_pssm.as<const int8_t>(), qoffs, 1, &scoring, d_res.as<sw_result>(), nullptr));
    else if (stats)
        CHECK(sw_db_search_pssm_top_stats(ctx, handle, d_pssm.as<const int8_t>(), qoffs, 1, &scoring, K, o.min_score, d_hits.as<sw_hit>(), d_nhits.as<int64_t>(), o.score_shift,
                                          stats.d_hist.as<uint32_t>(), nullptr));
    else if (K > 0) CHECK(sw_db_search_pssm_top(ctx, handle, d_pssm.as<const int8_t>(), qoffs, 1, &scoring, K, o.min_score, d_hits.as<sw_hit>(), d_nhits.as<int64_t>(), nullptr));
    CHECK(sw_synchronize(ctx, nullptr));
    const double t2 = now_s();
    std::vector<sw_hit> hits(nhit);
    int64_t nhits = 0;
    if (on_device && K > 0) {
        d_hits.download(hits.data(), (size_t)K * sizeof(sw_hit));
        d_nhits.download(&nhits, sizeof nhits);
    } else if (!on_device) {
        std::vector<sw_result> res(nres);
        d_res.download(res.data(), (size_t)nrec * sizeof(sw_result));
        hits = rank_hits(res.data(), nrec, K, o.min_score);
        nhits = (int64_t)hits.size();
    }
    AlignedHits aligned;
    if (align) {
        const int64_t ops_cap = ncols + handle.longest();
        DeviceBuffer d_aln(ctx, (size_t)K * sizeof(sw_alignment)), d_ops(ctx, (size_t)K * (size_t)ops_cap);
        CHECK(sw_db_align_pssm_hits(ctx, handle, d_pssm.as<const int8_t>(), qoffs, 1, &scoring, d_hits.as<const sw_hit>(), d_nhits.as<const int64_t>(), K,
                                    d_aln.as<sw_alignment>(), d_ops.as<char>(), ops_cap, nullptr));
        CHECK(sw_synchronize(ctx, nullptr));
        aligned = download_aligned(d_aln, d_ops, (size_t)K, ops_cap);
    }
    std::vector<int32_t> keep;   // --evalue: the hits at or above the threshold of their length class
    if (stats) {
        stats.fit_last_search();
        keep.resize(nhit);
        CHECK(sw_hits_threshold_host(db.offsets.data(), nrec, stats.thresholds(o.evalue), 1, K, hits.data(), &nhits, nullptr, keep.data(), nullptr));
    }
    printf("## query record 0 of %s\n", o.pssm_path);
    const sw_affine unused = {nullptr, 0, 0};   // (print_hits aligns nothing itself when it is given the rows of a call)
    print_hits(ctx, query.data(), ncols, nullptr, masked.db(), masked.buffer(), hits.data(), (long long)nhits, align, unused, aligned, stats ? keep.data() : nullptr,
               stats ? stats.fit.data() : nullptr);
    print_elapsed(t2 - t1, (double)ncols * (double)db.total, "; 1 PSSM of %lld columns over %d letters, handle prepared in %f", (long long)ncols, m.nletters, t1 - t0);
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
// --evalue / --include-evalue: every search is the _top_stats call.  With --include-evalue a round that feeds an update or the A3M waits
// for its search, fits the histograms on the host and thresholds a COPY of the hit table on the device (sw_hits_threshold_device): the
// copy goes to the weights, the update and --out-a3m with include_min_score at its minimum, the untouched table to the aligner and the
// printer.  That is the one synchronisation per round this path adds.
static int search_iter_main(const Options& o) {
    const char *ppath = o.pssm_path, *qpath = o.search_q;   // (with --pssm the two are the one file)
    const Db db = read_db(o.search_db);
    const Scoring s(o.af, o.sc);
    Pssm m;    // iteration 0
    Db qs;     // the query line of every query's alignments, back to back
    if (ppath) {
        read_pssm_file(ppath, &m);
        qs.nrec = 1; qs.total = m.ncols;
        qs.offsets = {0, m.ncols};
        qs.letters.assign((size_t)m.ncols, '?');
    } else {
        qs = read_db(qpath);
        bool seen[256] = {};
        for (int64_t i = 0; i < db.total; ++i) seen[(unsigned char)db.letters[(size_t)i]] = true;
        for (int64_t i = 0; i < qs.total; ++i) seen[(unsigned char)qs.letters[(size_t)i]] = true;
        for (int b = 0; b < 256; ++b)
            if (seen[b]) m.letters[m.nletters++] = (char)b;
        if (m.nletters == 0 || qs.total == 0) { fprintf(stderr, "smithW: --iterations needs queries and a database with letters\n"); return 2; }
        for (int x = 0; x < m.nletters; ++x)
            for (int y = 0; y < m.nletters; ++y) {
                const int v = s.sub.s[(unsigned char)m.letters[x]][(unsigned char)m.letters[y]];
                m.other = std::min(m.other, v); m.smax = std::max(m.smax, v);
            }
        m.matrix.resize((size_t)qs.total * (size_t)m.nletters);
        CHECK(sw_pssm_from_queries(qs.letters.data(), qs.offsets.data(), qs.nrec, &s.sub, m.letters, m.nletters, m.matrix.data()));
        if (qs.offsets[0] != 0) { fprintf(stderr, "smithW: query offsets do not start at 0\n"); return 1; }
    }
    const sw_pssm_scoring scoring = {m.letters, m.nletters, m.other, m.smax, o.af.has_open ? o.af.open : 0, o.af.has_extend ? o.af.extend : (ppath ? 0 : o.sc.gap)};
    const int64_t nq = qs.nrec, nrec = db.nrec, *qoffs = qs.offsets.data();
    const long long K = std::max(0ll, std::min(o.top, (long long)nrec));
    if (K < 1 || K > SW_TOP_MAX) { fprintf(stderr, "smithW: --iterations / --out-pssm work on a device hit table: min(--top, records) = %lld is outside 1..%d\n", K, SW_TOP_MAX); return 2; }
    Context ctx(0);
    if (o.align_ckpt) CHECK(sw_set_option(ctx, "align_checkpoint", 2));
    CHECK(sw_set_option(ctx, "search_lanes", o.search_lanes));
    const size_t n = (size_t)(nq * K);
    DeviceBuffer d_prior(ctx, m.matrix.data(), m.matrix.size()), d_work(ctx, m.matrix.size() + 16), d_db(ctx, db.letters.data(), (size_t)db.total),
        d_hits(ctx, n * sizeof(sw_hit)), d_nhits(ctx, (size_t)nq * sizeof(int64_t)), d_aln, d_ops, d_weights;
    const MaskedDb masked(ctx, o.mask, db, d_db);   // --mask: the search, the alignment and the printer see the masked copy from here on
    DbHandle handle;
    const double t0 = now_s();
    handle.create(ctx, masked.buffer(), db.offsets, nrec);
    const int64_t ops_cap = std::max<int64_t>(1, qs.longest() + handle.longest());
    if (o.iterations > 1 || o.align) {
        if ((double)n * (double)ops_cap > (double)(1ll << 32)) { fprintf(stderr, "smithW: the ops of %zu hits x %lld bytes pass 4 GiB: lower --top\n", n, (long long)ops_cap); return 2; }
        d_aln.alloc(ctx, n * sizeof(sw_alignment));
        d_ops.alloc(ctx, n * (size_t)ops_cap);
    }
    if (o.weight_hits > 0 && o.iterations > 1) d_weights.alloc(ctx, n * sizeof(int32_t));
    ScoreStats stats;
    DeviceBuffer d_included;   // --include-evalue: the thresholded copy of the hit table
    if (o.stats()) stats.alloc(ctx, nq, o.score_shift);
    if (o.has_include_evalue) d_included.alloc(ctx, n * sizeof(sw_hit));
    const sw_hit* d_use = o.has_include_evalue ? d_included.as<const sw_hit>() : d_hits.as<const sw_hit>();   // what the weights, the update and the A3M read
    const int64_t include_min = o.has_include_evalue ? INT64_MIN : (int64_t)o.include_score;
    const sw_pssm_update upd = {&s.sub, (int32_t)o.prior_weight, include_min};
    const sw_pssm_weighting weighting = {(int32_t)o.weight_hits, include_min};
    const double t1 = now_s();
    const DeviceBuffer* cur = &d_prior;   // the matrix the search runs with
    for (long long it = 0; it < o.iterations; ++it) {   // nothing below waits for the device or reads from it
        if (it > 0) {
            CHECK(sw_db_align_pssm_hits(ctx, handle, cur->as<const int8_t>(), qoffs, nq, &scoring, d_hits.as<const sw_hit>(), d_nhits.as<const int64_t>(), K,
                                        d_aln.as<sw_alignment>(), d_ops.as<char>(), ops_cap, nullptr));
            if (d_weights)
                CHECK(sw_db_pssm_hit_weights(ctx, handle, qoffs, nq, &scoring, &weighting, d_use, d_nhits.as<const int64_t>(), K,
                                             d_aln.as<const sw_alignment>(), d_ops.as<const char>(), ops_cap, d_weights.as<int32_t>(), nullptr));
            CHECK(sw_db_pssm_from_hits(ctx, handle, d_prior.as<const int8_t>(), qoffs, nq, &scoring, &upd, d_use, d_nhits.as<const int64_t>(), K,
                                       d_aln.as<const sw_alignment>(), d_ops.as<const char>(), ops_cap, d_weights.as<const int32_t>(), d_work.as<int8_t>(), nullptr, nullptr));
            cur = &d_work;
        }
        if (stats)
            CHECK(sw_db_search_pssm_top_stats(ctx, handle, cur->as<const int8_t>(), qoffs, nq, &scoring, K, o.min_score, d_hits.as<sw_hit>(), d_nhits.as<int64_t>(),
                                              o.score_shift, stats.d_hist.as<uint32_t>(), nullptr));
        else CHECK(sw_db_search_pssm_top(ctx, handle, cur->as<const int8_t>(), qoffs, nq, &scoring, K, o.min_score, d_hits.as<sw_hit>(), d_nhits.as<int64_t>(), nullptr));
        if (o.has_include_evalue && (it + 1 < o.iterations || o.out_a3m)) {   // this round's table feeds an update or the A3M
            CHECK(sw_synchronize(ctx, nullptr));
            stats.fit_last_search();
            stats.thresholds(o.include_evalue);
            CHECK(sw_hits_threshold_device(ctx, handle, stats.d_thr.as<const int64_t>(), nq, K, d_hits.as<const sw_hit>(), d_nhits.as<const int64_t>(),
                                           d_included.as<sw_hit>(), nullptr, nullptr, nullptr));
        }
    }
    if (o.align)
        CHECK(sw_db_align_pssm_hits(ctx, handle, cur->as<const int8_t>(), qoffs, nq, &scoring, d_hits.as<const sw_hit>(), d_nhits.as<const int64_t>(), K,
                                    d_aln.as<sw_alignment>(), d_ops.as<char>(), ops_cap, nullptr));
    // --out-a3m: the rows of the last round's tables, still on the device: one call for the row table and the size, one for the bytes
    // (through the handle over the letters as they were read: ops and offsets do not depend on letters, so with --mask the file keeps the original ones)
    DeviceBuffer d_qs, d_rows, d_a3m, d_a3m_bytes;
    int64_t a3m_bytes = 0;
    if (o.out_a3m) {
        if (!ppath) d_qs.alloc(ctx, qs.letters.data(), (size_t)qs.total);
        d_rows.alloc(ctx, n * sizeof(sw_msa_row));
        d_a3m_bytes.alloc(ctx, sizeof(int64_t));
        CHECK(sw_db_msa_from_hits(ctx, masked.original(handle), d_qs.as<const char>(), qoffs, nq, include_min, d_use, d_nhits.as<const int64_t>(), K,
                                  d_aln.as<const sw_alignment>(), d_ops.as<const char>(), ops_cap, nullptr, d_rows.as<sw_msa_row>(), nullptr, 0, d_a3m_bytes.as<int64_t>(),
                                  nullptr));
        CHECK(sw_synchronize(ctx, nullptr));
        d_a3m_bytes.download(&a3m_bytes, sizeof a3m_bytes);
        d_a3m.alloc(ctx, (size_t)a3m_bytes + 16);
        CHECK(sw_db_msa_from_hits(ctx, masked.original(handle), d_qs.as<const char>(), qoffs, nq, include_min, d_use, d_nhits.as<const int64_t>(), K,
                                  d_aln.as<const sw_alignment>(), d_ops.as<const char>(), ops_cap, nullptr, d_rows.as<sw_msa_row>(), d_a3m.as<char>(), a3m_bytes,
                                  d_a3m_bytes.as<int64_t>(), nullptr));
    }
    CHECK(sw_synchronize(ctx, nullptr));
    const double t2 = now_s();
    std::vector<sw_hit> hits(n);
    std::vector<int64_t> nhits((size_t)nq);
    std::vector<int8_t> last(m.matrix.size());
    d_hits.download(hits.data(), n * sizeof(sw_hit));
    d_nhits.download(nhits.data(), (size_t)nq * sizeof(int64_t));
    cur->download(last.data(), last.size());
    const AlignedHits aligned = o.align ? download_aligned(d_aln, d_ops, n, ops_cap) : AlignedHits();
    std::vector<sw_hit> used;    // --include-evalue with --out-a3m: the table the A3M rows were made from
    std::vector<int32_t> keep;   // --evalue: the hits at or above the threshold of their length class
    if (o.has_include_evalue && o.out_a3m) { used.resize(n); d_included.download(used.data(), n * sizeof(sw_hit)); }
    if (o.has_evalue) {
        stats.fit_last_search();
        keep.resize(n);
        CHECK(sw_hits_threshold_host(db.offsets.data(), nrec, stats.thresholds(o.evalue), nq, K, hits.data(), nhits.data(), nullptr, keep.data(), nullptr));
    }
    if (ppath) {   // the consensus of the last matrix
        const std::string c = consensus(m, last.data(), qs.total);
        std::copy(c.begin(), c.end(), qs.letters.begin());
    }
    std::vector<sw_msa_row> msa_rows;
    std::vector<char> a3m;
    std::vector<std::string> tnames, qnames;
    std::vector<const char*> tname_ptrs;
    if (o.out_a3m) {
        msa_rows.resize(n); a3m.resize((size_t)a3m_bytes + 1);
        d_rows.download(msa_rows.data(), n * sizeof(sw_msa_row));
        d_a3m.download(a3m.data(), (size_t)a3m_bytes);
        tnames = fasta_names(o.search_db);
        tnames.resize((size_t)nrec, "-");
        for (const std::string& t : tnames) tname_ptrs.push_back(t.c_str());
        if (!ppath) qnames = fasta_names(qpath);
        qnames.resize((size_t)nq, "-");
    }
    const sw_affine unused = {nullptr, 0, 0};   // (print_hits aligns nothing itself when it is given the rows of a call)
    for (int64_t i = 0; i < nq; ++i) {
        printf("## query record %lld of %s\n", (long long)i, qpath);
        print_hits(ctx, qs.record(i), qs.len(i), nullptr, masked.db(), masked.buffer(), hits.data() + i * K, (long long)nhits[(size_t)i], o.align, unused, aligned.only_row(i, K),
                   o.has_evalue ? keep.data() + i * K : nullptr, o.has_evalue ? &stats.fit[(size_t)i] : nullptr);
        if (o.out_pssm) {
            const std::string path = std::string(o.out_pssm) + "." + std::to_string((long long)i) + ".pssm";
            CHECK(sw_write_pssm(path.c_str(), m.letters, m.nletters, last.data() + qoffs[i] * m.nletters, qs.len(i), qs.record(i)));
        }
        if (o.out_a3m) {
            const std::string path = std::string(o.out_a3m) + "." + std::to_string((long long)i) + ".a3m";
            CHECK(sw_write_a3m(path.c_str(), qnames[(size_t)i].c_str(), ppath ? nullptr : qs.record(i), qs.len(i), tname_ptrs.data(), nrec,
                               (used.empty() ? hits : used).data() + i * K,
                               aligned.row(i, K), msa_rows.data() + i * K, K, a3m.data(), a3m_bytes));
        }
    }
    print_elapsed(t2 - t1, (double)qs.total * (double)db.total * (double)o.iterations, "; %lld queries, %lld iterations on the device, handle prepared in %f", (long long)nq,
                  (long long)o.iterations, t1 - t0);
    return 0;
}

// the list of --pairs: one "<query record> <target record>" per line, 0-based; '#' lines and blank lines are skipped
static int read_pairs(const char* path, std::vector<sw_pair>* pairs) {
    FILE* f = fopen(path, "r");
    if (!f) { fprintf(stderr, "smithW: --pairs: cannot open %s\n", path); return 2; }
    char line[512];
    int rc = 0;
    for (long long ln = 1; !rc && fgets(line, sizeof line, f); ++ln) {
        if (!strchr(line, '\n') && !feof(f)) {   // (a line that does not fit the buffer would be counted twice)
            fprintf(stderr, "smithW: --pairs %s line %lld: longer than %zu bytes\n", path, ln, sizeof line - 2);
            rc = 2;
            continue;
        }
        const char* t = line + strspn(line, " \t\r\n");
        if (*t == 0 || *t == '#') continue;
        char *e1 = nullptr, *e2 = nullptr;
        const long long q = strtoll(t, &e1, 10);
        const long long k = e1 != t ? strtoll(e1, &e2, 10) : 0;
        if (e1 == t || e2 == e1 || !strchr(" \t", *e1) || e2[strspn(e2, " \t\r\n")] != 0) {
            fprintf(stderr, "smithW: --pairs %s line %lld: expected \"<query record> <target record>\"\n", path, ln);
            rc = 2;
            continue;
        }
        pairs->push_back(sw_pair{q, k});
    }
    fclose(f);
    return rc;
}

// --search --pairs FILE: the listed (query record, target record) pairs through ONE prepared handle and one call
// (sw_db_create / sw_db_search_affine_pairs), one output line per pair in input order.  A linear search goes through the match /
// mismatch table of --scores with gap_open 0, as --all-queries does.
static int search_pairs_main(const Options& o) {
    std::vector<sw_pair> pairs;
    if (int rc = read_pairs(o.pairs_path, &pairs)) return rc;
    const Db qs = read_db(o.search_q), db = read_db(o.search_db);
    const std::vector<std::string> names = target_names("--pairs", o.search_db, db);
    const int64_t np = (int64_t)pairs.size(), nq = qs.nrec, nrec = db.nrec;
    Context ctx(0);
    CHECK(sw_set_option(ctx, "search_pairs_lanes", o.pairs_lanes));
    DeviceBuffer d_q(ctx, qs.letters.data(), (size_t)qs.total), d_db(ctx, db.letters.data(), (size_t)db.total),
        d_pairs(ctx, (size_t)std::max<int64_t>(1, np) * sizeof(sw_pair)), d_res(ctx, (size_t)std::max<int64_t>(1, np) * sizeof(sw_result));
    const MaskedDb masked(ctx, o.mask, db, d_db);   // --mask: the search, the alignment and the printer see the masked copy from here on
    d_pairs.upload(pairs.data(), (size_t)np * sizeof(sw_pair));
    const Scoring s(o.af, o.sc);
    DbHandle handle;
    const double t0 = now_s();
    handle.create(ctx, masked.buffer(), db.offsets, nrec);
    const double t1 = now_s();
    CHECK(sw_db_search_affine_pairs(ctx, handle, d_q.as<const char>(), qs.offsets.data(), nq, &s.aff, d_pairs.as<const sw_pair>(), np, d_res.as<sw_result>(), nullptr));
    CHECK(sw_synchronize(ctx, nullptr));
    const double t2 = now_s();
    std::vector<sw_result> res((size_t)np);
    d_res.download(res.data(), (size_t)np * sizeof(sw_result));
    printf("# %lld pairs of %lld queries and %lld targets; query\ttarget\tname\tscore\ttarget_end\tquery_end\n", (long long)np, (long long)nq, (long long)nrec);
    double cells = 0;
    for (int64_t p = 0; p < np; ++p) {
        const sw_pair& pr = pairs[(size_t)p];
        const bool qin = pr.query >= 0 && pr.query < nq, tin = pr.target >= 0 && pr.target < nrec;
        const long long M = qin ? qs.len(pr.query) + 1 : 1;
        if (qin && tin) cells += (double)(M - 1) * (double)db.len(pr.target);
        print_pair(pr.query, pr.target, tin ? names[(size_t)pr.target].c_str() : "-", res[(size_t)p], M);
    }
    print_elapsed(t2 - t1, cells, "; %lld pairs in one call, handle prepared in %f", (long long)np, t1 - t0);
    return 0;
}

// --search --all-queries --prefilter S: the ungapped pre-filter (sw_db_prefilter_ungapped, U >= S) and the affine search of the pairs it
// lists (sw_db_search_affine_pairs over the whole list, its {-1, -1} tail included), through ONE prepared handle, back to back on the
// device; one read-back at the end brings the count, the list, the results and the ungapped scores.  The passing pairs are printed in
// ascending (query, target) order in the line format of --pairs, with " ungapped=<U>" appended.
static int search_prefilter_main(const Options& o) {
    const Db qs = read_db(o.search_q), db = read_db(o.search_db);
    const std::vector<std::string> names = target_names("--prefilter", o.search_db, db);
    const int64_t nq = qs.nrec, nrec = db.nrec;
    // one device block for everything that comes back: the count (16 bytes), the list, the results, the ungapped scores
    const int64_t cap = nq * nrec;
    const size_t o_pairs = 16, o_res = o_pairs + (size_t)cap * sizeof(sw_pair), o_u = o_res + (size_t)cap * sizeof(sw_result),
                 out_bytes = o_u + (size_t)cap * sizeof(int32_t);
    Context ctx(0);
    DeviceBuffer d_q(ctx, qs.letters.data(), (size_t)qs.total), d_db(ctx, db.letters.data(), (size_t)db.total), d_out(ctx, out_bytes);
    const MaskedDb masked(ctx, o.mask, db, d_db);   // --mask: the search, the alignment and the printer see the masked copy from here on
    const Scoring s(o.af, o.sc);
    sw_pair* d_pairs = cap ? (sw_pair*)(d_out.as<char>() + o_pairs) : nullptr;
    sw_result* d_res = cap ? (sw_result*)(d_out.as<char>() + o_res) : nullptr;
    int32_t* d_u = cap ? (int32_t*)(d_out.as<char>() + o_u) : nullptr;
    DbHandle handle;
    const double t0 = now_s();
    handle.create(ctx, masked.buffer(), db.offsets, nrec);
    const double t1 = now_s();
    CHECK(sw_db_prefilter_ungapped(ctx, handle, d_q.as<const char>(), qs.offsets.data(), nq, &s.sub, o.prefilter, d_pairs, cap, d_out.as<int64_t>(), d_u, nullptr));
    CHECK(sw_db_search_affine_pairs(ctx, handle, d_q.as<const char>(), qs.offsets.data(), nq, &s.aff, d_pairs, cap, d_res, nullptr));
    CHECK(sw_synchronize(ctx, nullptr));
    const double t2 = now_s();
    std::vector<char> out(out_bytes);
    d_out.download(out.data(), out_bytes);
    int64_t np = 0;
    memcpy(&np, out.data(), sizeof np);
    const sw_pair* pairs = (const sw_pair*)(out.data() + o_pairs);
    const sw_result* res = (const sw_result*)(out.data() + o_res);
    const int32_t* u = (const int32_t*)(out.data() + o_u);
    std::vector<int64_t> order((size_t)np);
    for (int64_t p = 0; p < np; ++p) order[(size_t)p] = p;
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return pairs[a].query != pairs[b].query ? pairs[a].query < pairs[b].query : pairs[a].target < pairs[b].target; });
    printf("# %lld pairs of %lld queries and %lld targets pass the ungapped pre-filter at %lld; query\ttarget\tname\tscore\ttarget_end\tquery_end\n", (long long)np,
           (long long)nq, (long long)nrec, o.prefilter);
    double cells = 0;
    for (int64_t i = 0; i < np; ++i) {
        const sw_pair& pr = pairs[order[(size_t)i]];
        const long long M = qs.len(pr.query) + 1;
        cells += (double)(M - 1) * (double)db.len(pr.target);
        print_pair(pr.query, pr.target, names[(size_t)pr.target].c_str(), res[order[(size_t)i]], M, &u[pr.query * nrec + pr.target]);
    }
    print_elapsed(t2 - t1, cells, " over the rescored pairs; filter and %lld pairs in two calls, handle prepared in %f", (long long)np, t1 - t0);
    return 0;
}

// The command line into `o`; 0, or 2 after the usage line or the message of a value that is no integer.
static int parse_options(int argc, char** argv, Options& o) {
    for (int ai = 1; ai < argc; ++ai) {
        const std::string f = argv[ai];
        const auto flag = [&](const char* name, int values) { return f == name && ai + values < argc; };   // the flag, and its values follow
        const auto integer = [&](int* out) { const char* name = argv[ai]; return parse_int(name, argv[++ai], out); };
        const auto real = [&](double* out) { const char* name = argv[ai]; return parse_real(name, argv[++ai], out); };
        int v = 0;
        if (f[0] != '-' && o.npos < 2 && ai + (1 - o.npos) < argc) {   // <cols> <rows>, anywhere on the line
            (o.npos == 0 ? o.cols : o.rows) = strtoll(argv[ai], nullptr, 10);
            o.builtin = false;
            ++o.npos;
        }
        else if (f == "--dump") o.dump = true;
        else if (f == "--dump-labels") o.dump = o.labels = true;
        else if (f == "--h64") o.h64 = true;
        else if (f == "--no-backtrack") o.backtrack = false;
        else if (f == "--p8") o.p8 = true;
        else if (flag("--gpus", 1)) { const int n = atoi(argv[++ai]); for (int g = 0; g < n; ++g) o.devices.push_back(g); }
        else if (flag("--devices", 1)) { for (char* t = strtok(argv[++ai], ","); t; t = strtok(nullptr, ",")) o.devices.push_back(atoi(t)); }
        else if (flag("--fasta", 2)) { o.fasta_a = argv[++ai]; o.fasta_b = argv[++ai]; o.builtin = false; }
        else if (flag("--search", 3) && std::string(argv[ai + 1]) == "--pssm") { ai += 1; o.search_q = o.pssm_path = argv[++ai]; o.search_db = argv[++ai]; o.builtin = false; }
        else if (flag("--search", 2)) { o.search_q = argv[++ai]; o.search_db = argv[++ai]; o.builtin = false; }
        else if (flag("--top", 1)) { o.top = strtoll(argv[++ai], nullptr, 10); o.has_top = true; }
        else if (flag("--pairs", 1)) o.pairs_path = argv[++ai];
        else if (flag("--min-score", 1)) { if (!integer(&v)) return 2; o.min_score = v; o.has_min_score = true; }
        else if (flag("--prefilter", 1)) { if (!integer(&v)) return 2; o.prefilter = v; o.has_prefilter = true; }
        else if (flag("--prefilter-hits", 1)) { if (!integer(&v)) return 2; o.prefilter_hits = v; o.has_prefilter_hits = true; }
        else if (flag("--search-lanes", 1)) { if (!integer(&o.search_lanes)) return 2; o.has_search_lanes = true; }
        else if (flag("--pairs-lanes", 1)) { if (!integer(&o.pairs_lanes)) return 2; o.has_pairs_lanes = true; }
        else if (flag("--iterations", 1)) { if (!integer(&o.iterations)) return 2; o.has_iter_flag = true; }
        else if (flag("--include-score", 1)) { if (!integer(&o.include_score)) return 2; o.has_iter_flag = o.has_include_score = true; }
        else if (flag("--evalue", 1)) { if (!real(&o.evalue)) return 2; o.has_evalue = true; }
        else if (flag("--include-evalue", 1)) { if (!real(&o.include_evalue)) return 2; o.has_include_evalue = true; }
        else if (flag("--score-shift", 1)) { if (!integer(&o.score_shift)) return 2; o.has_score_shift = true; }
        else if (f == "--mask") o.mask.on = true;
        else if (flag("--mask-window", 1)) { if (!integer(&o.mask.window)) return 2; o.mask.has_sub = true; }
        else if (flag("--mask-trigger", 1)) { if (!integer(&o.mask.trigger)) return 2; o.mask.has_sub = true; }
        else if (flag("--mask-extend", 1)) { if (!integer(&o.mask.extend)) return 2; o.mask.has_sub = true; }
        else if (flag("--mask-byte", 1)) { o.mask.byte = argv[++ai]; o.mask.has_sub = true; }
        else if (flag("--mask-letters", 1)) { o.mask.letters = argv[++ai]; o.mask.has_sub = true; }
        else if (flag("--prior-weight", 1)) { if (!integer(&o.prior_weight)) return 2; o.has_iter_flag = true; }
        else if (flag("--out-pssm", 1)) { o.out_pssm = argv[++ai]; o.has_iter_flag = true; }
        else if (flag("--out-a3m", 1)) { o.out_a3m = argv[++ai]; o.has_iter_flag = true; }
        else if (flag("--weight-hits", 1)) { if (!integer(&o.weight_hits)) return 2; o.has_weight_hits = true; }
        else if (flag("--matrix", 1)) { o.af.matrix = argv[++ai]; o.af.on = true; }
        else if (flag("--gap-open", 1)) { if (!integer(&o.af.open)) return 2; o.af.has_open = o.af.on = true; }
        else if (flag("--gap-extend", 1)) { if (!integer(&o.af.extend)) return 2; o.af.has_extend = true; }
        else if (f == "--align") o.align = true;
        else if (f == "--align-checkpoint") o.align_ckpt = true;
        else if (f == "--all-queries") o.all_queries = true;
        else if (flag("--record-a", 1)) o.rec_a = strtoll(argv[++ai], nullptr, 10);
        else if (flag("--record-b", 1)) o.rec_b = strtoll(argv[++ai], nullptr, 10);
        else if (flag("--seed", 1)) o.seed = (unsigned)strtoul(argv[++ai], nullptr, 10);
        else if (flag("--scores", 3)) { o.sc.match = atoi(argv[++ai]); o.sc.mismatch = atoi(argv[++ai]); o.sc.gap = atoi(argv[++ai]); }
        else { fprintf(stderr, "usage: smithW [<cols> <rows> | --fasta A.fa B.fa [--record-a I] [--record-b J] | --search QUERY.fa DB.fa [--record-a I] [--top K] [--all-queries [--min-score S] [--prefilter S | --prefilter-hits S [--pairs-lanes 16|32]] [--search-lanes 16|32]] [--pairs FILE [--pairs-lanes 16|32]] [--matrix FILE] [--gap-open O] [--gap-extend E] [--align [--align-checkpoint]] | --search --pssm FILE DB.fa --gap-open O --gap-extend E [--top K] [--min-score S] [--align] [--search-lanes 16|32] | with --all-queries or --pssm: [--iterations N] [--include-score S] [--prior-weight W] [--out-pssm PREFIX] [--align --out-a3m PREFIX: the A3M of the last round's hits per query, PREFIX.<query>.a3m; with --pssm it holds no query record] [--weight-hits P: Henikoff weights on the device, N[j] then counts in units of P, so scale --prior-weight with it]] [--seed N] [--dump | --dump-labels] [--h64] [--no-backtrack] [--scores M X G] [--gpus N | --devices 0,1,..] [--p8]\n"); return 2; }
    }
    return 0;
}

// the reference's own run: one DP fill and its backtrack, on one GPU or as row bands over several
static int fill_main(const Options& o) {
    long long cols = o.cols, rows = o.rows;
    const bool builtin = o.builtin, dump = o.dump, labels = o.labels, h64 = o.h64, backtrack = o.backtrack, p8 = o.p8;
    const std::vector<int>& devices = o.devices;
    const sw_scores sc = o.sc;
    if (o.fasta_a) {
        int64_t la = 0, lb = 0;
        CHECK(sw_read_fasta(o.fasta_a, o.rec_a, nullptr, 0, &la));
        CHECK(sw_read_fasta(o.fasta_b, o.rec_b, nullptr, 0, &lb));
        cols = la; rows = lb;
    }
    const long long m = cols + 1, n = rows + 1;
    std::vector<char> a(m + 1), b(n + 1);
    if (o.fasta_a) {
        int64_t la = 0, lb = 0;
        CHECK(sw_read_fasta(o.fasta_a, o.rec_a, a.data(), cols, &la));
        CHECK(sw_read_fasta(o.fasta_b, o.rec_b, b.data(), rows, &lb));
    } else if (builtin) { memcpy(b.data(), "GGTTGACTA", 9); memcpy(a.data(), "TGTTACGG", 8); }
    else CHECK(sw_generate(cols, rows, o.seed, a.data(), b.data()));
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
    Context ctx(0);
    const size_t cells = (size_t)m * (size_t)n;
    DeviceBuffer d_a(ctx, (size_t)cols + 16), d_b(ctx, (size_t)rows + 16), d_res(ctx, sizeof(sw_result));
    void *d_H, *d_P;   // (placed by sw_alloc_outputs: released by sw_free_outputs at the end of a run that got there)
    d_a.upload(a.data(), (size_t)cols);
    d_b.upload(b.data(), (size_t)rows);
    // output matrices placed for speed (allocation is outside the reference's timer as well, serial_smithW.c:96-103,137)
    CHECK(sw_alloc_outputs(ctx, d_a.as<const char>(), cols, d_b.as<const char>(), rows, &sc, h64 ? 8 : 4, 4, cells >= (1u << 24) ? 0 : 1, &d_H, &d_P, nullptr));
    // one untimed call sizes the workspace (the reference's timer also excludes its allocations)
    CHECK(sw_fill_device(ctx, d_a.as<const char>(), cols, d_b.as<const char>(), rows, &sc, d_H, h64 ? 8 : 4, (int32_t*)d_P, nullptr, d_res.as<sw_result>(), nullptr));
    CHECK(sw_synchronize(ctx, nullptr));

    if (backtrack) {   // ... and loads the traceback kernel (first use of a kernel pays for its code object): a walk of nothing on a 1 x 1 matrix
        DeviceBuffer d_p1(ctx, 4 * sizeof(int32_t)), d_r1(ctx, sizeof(sw_result));
        const int32_t zeros[4] = {0, 0, 0, 0}; const sw_result r0 = {0, 0, 0};
        d_p1.upload(zeros, sizeof zeros);
        d_r1.upload(&r0, sizeof r0);
        CHECK(sw_traceback_device(ctx, d_p1.as<int32_t>(), 1, 1, 3, nullptr, 0, d_r1.as<sw_result>(), nullptr));
        CHECK(sw_synchronize(ctx, nullptr));
    }

    double t0 = now_s();
    CHECK(sw_fill_device(ctx, d_a.as<const char>(), cols, d_b.as<const char>(), rows, &sc, d_H, h64 ? 8 : 4, (int32_t*)d_P, nullptr, d_res.as<sw_result>(), nullptr));
    CHECK(sw_synchronize(ctx, nullptr));
    double t1 = now_s();
    printf("\nElapsed time for scoring matrix computation: %f\n\n", t1 - t0);
    sw_result res;
    d_res.download(&res, sizeof res);
    if (res.path_len < 0) { fprintf(stderr, "smithW: device hand-off timed out\n"); return 1; }

    t0 = now_s();
    if (backtrack) {
        CHECK(sw_traceback_device(ctx, (int32_t*)d_P, cols, rows, res.max_pos, nullptr, 0, d_res.as<sw_result>(), nullptr));
        CHECK(sw_synchronize(ctx, nullptr));
        d_res.download(&res, sizeof res);
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
    sw_free_outputs(ctx, d_H, d_P);
    return rc;
}

typedef int (*Mode)(const Options&);   // one of the *_main above; none: the command line was refused
static Mode refuse(const char* message, ...) {
    va_list ap;
    va_start(ap, message);
    fputs("smithW: ", stderr);
    vfprintf(stderr, message, ap);
    fputc('\n', stderr);
    va_end(ap);
    return nullptr;
}
// match / mismatch of --scores become a table of signed bytes (sw_submat_match would clamp them): `who` needs them within -128..127
static bool byte_scores(const sw_scores& sc, const char* who, const char* wants = "needs --scores M X within -128..127 (a table of signed bytes)") {
    if (sc.match >= -128 && sc.match <= 127 && sc.mismatch >= -128 && sc.mismatch <= 127) return true;
    refuse("%s %s, got %d %d", who, wants, sc.match, sc.mismatch);
    return false;
}
// Which flags go together: the mode to run, or nullptr after one line on stderr.  The order of the checks decides which line a
// command that breaks several rules gets (tests/test_cli_usage_host.py holds it).
static Mode check_options(const Options& o) {
    const AffineArgs& af = o.af;
    const bool any_prefilter = o.has_prefilter || o.has_prefilter_hits, many = o.search_q && o.all_queries;
    if (o.npos == 1) return refuse("<cols> needs <rows>");
    if (o.align_ckpt && !(o.search_q && o.align)) return refuse("--align-checkpoint goes with --search --align");
    if (o.has_search_lanes) {   // the many-query search alone has the two kinds of lanes
        if (o.search_lanes != 16 && o.search_lanes != 32) return refuse("--search-lanes takes 16 or 32, got %d", o.search_lanes);
        if (!o.pssm_path && !many) return refuse("--search-lanes goes with --search --all-queries or --search --pssm");
        if (any_prefilter || o.pairs_path) return refuse("--search-lanes does not go with --prefilter / --prefilter-hits / --pairs");
    }
    if (o.has_pairs_lanes) {   // the rescoring of a pair list alone has this choice
        if (o.pairs_lanes != 16 && o.pairs_lanes != 32) return refuse("--pairs-lanes takes 16 or 32, got %d", o.pairs_lanes);
        if (!o.search_q || o.pssm_path || !(o.pairs_path || o.has_prefilter_hits)) return refuse("--pairs-lanes goes with --search --pairs or --search --all-queries --prefilter-hits");
    }
    if (const std::string why = score_stats_rule(o); !why.empty()) return refuse("%s", why.c_str());   // (the rules stand in cli_parts.h)
    if (const std::string why = mask_rule(o); !why.empty()) return refuse("%s", why.c_str());          // (likewise)
    if (o.has_iter_flag) {   // the iterative search: many sequence queries, or one matrix
        if (!(o.search_q && (o.all_queries || o.pssm_path))) return refuse("--iterations / --include-score / --prior-weight / --out-pssm / --out-a3m go with --search --all-queries or --search --pssm");
        if (o.iterations < 1) return refuse("--iterations N needs N >= 1, got %d", o.iterations);
        if (o.prior_weight < 0 || o.prior_weight > 65535) return refuse("--prior-weight W needs W within 0..65535, got %d", o.prior_weight);
        if (any_prefilter || o.pairs_path) return refuse("--iterations does not go with --prefilter / --prefilter-hits / --pairs");
    }
    if (o.out_a3m && !o.align) return refuse("--out-a3m writes the alignment of the aligned hits: it goes with --align");
    if (o.has_weight_hits) {   // the weights feed the update of an iterative search and nothing else
        if (!(o.has_iter_flag && o.iterate())) return refuse("--weight-hits goes with --iterations N (N > 1) or --out-pssm");
        if (o.weight_hits < 1 || o.weight_hits > 65535) return refuse("--weight-hits P needs P within 1..65535, got %d", o.weight_hits);
    }
    if (o.pssm_path) {   // the matrix is the query and the scoring at once
        if (af.matrix) return refuse("--pssm does not go with --matrix");
        if (o.all_queries) return refuse("--pssm does not go with --all-queries (the file is the one query)");
        if (o.pairs_path) return refuse("--pssm does not go with --pairs");
        if (any_prefilter) return refuse("--pssm does not go with --prefilter / --prefilter-hits");
        if (!af.has_open || !af.has_extend) return refuse("--pssm needs --gap-open O and --gap-extend E");
        if (!o.iterate()) return search_pssm_main;
        return byte_scores(o.sc, "--pssm --iterations", "takes its table from --scores M X within -128..127") ? search_iter_main : nullptr;
    }
    if (o.search_q) {
        if (af.on && !af.matrix && !byte_scores(o.sc, "--gap-open without --matrix")) return nullptr;
        if (o.align && !af.on && !byte_scores(o.sc, "--align on a linear search")) return nullptr;
    }
    // from here on a flag without --search is refused by its first rule
    if (o.has_prefilter_hits) {
        if (!many) return refuse("--prefilter-hits goes with --search --all-queries");
        if (o.has_prefilter) return refuse("--prefilter-hits does not go with --prefilter");
        if (o.pairs_path) return refuse("--prefilter-hits does not go with --pairs");
        if (o.prefilter_hits < 1) return refuse("--prefilter-hits S needs S >= 1, got %lld", o.prefilter_hits);
    }
    if (o.has_prefilter) {
        if (!many) return refuse("--prefilter goes with --search --all-queries");
        if (o.has_top) return refuse("--prefilter does not go with --top");
        if (o.has_min_score) return refuse("--prefilter does not go with --min-score");
        if (o.align) return refuse("--prefilter does not go with --align");
        if (o.pairs_path) return refuse("--prefilter does not go with --pairs");
        if (o.prefilter < 1) return refuse("--prefilter S needs S >= 1, got %lld", o.prefilter);
        return af.matrix || byte_scores(o.sc, "--prefilter without --matrix") ? search_prefilter_main : nullptr;
    }
    if (o.pairs_path) {
        if (!o.search_q) return refuse("--pairs goes with --search");
        if (o.all_queries) return refuse("--pairs does not go with --all-queries");
        if (o.has_top) return refuse("--pairs does not go with --top");
        if (o.has_min_score) return refuse("--pairs does not go with --min-score");
        if (o.align) return refuse("--pairs does not go with --align");
        return af.matrix || byte_scores(o.sc, "--pairs without --matrix") ? search_pairs_main : nullptr;
    }
    if (o.all_queries) {
        if (!o.search_q) return refuse("--all-queries goes with --search");
        if (!af.matrix && !byte_scores(o.sc, "--all-queries without --matrix")) return nullptr;
        return o.iterate() ? search_iter_main : search_all_main;
    }
    if (o.has_min_score) return refuse("--min-score goes with --search --all-queries");
    if (o.search_q) return search_main;
    if (o.align) return refuse("--align goes with --search");
    if (af.on || af.has_extend) return refuse("--matrix / --gap-open / --gap-extend go with --search");
    return fill_main;
}

int main(int argc, char** argv) {
    Options o;
    if (int rc = parse_options(argc, argv, o)) return rc;
    const Mode mode = check_options(o);
    try { return mode ? mode(o) : 2; }
    catch (const Exit& e) { return e.status; }   // a failed call: what the mode held is released by now
}
