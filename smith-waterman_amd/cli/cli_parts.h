// The parts the modes of smithW.cpp are built from (DESIGN.md "The CLI's shared parts"): the owners of the C-ABI's resources, the
// loaders of the input files, the one read-back of aligned hits, the two printers and the options main() parses.  Host code only;
// smithW.cpp is the one translation unit that includes it.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/swhip.h"

// A failed C-ABI call ends the run with status 1 from wherever it stands: fail() prints the line and throws, main() catches.  The
// owners below release what the run holds on the way out -- buffers and handle before the context, by the order of their declarations.
struct Exit { int status; };
[[noreturn]] static void fail(const char* call, int rc) {
    fprintf(stderr, "smithW: %s -> %d: %s\n", call, rc, sw_last_error());
    throw Exit{1};
}
#define CHECK(call)                         \
    do {                                    \
        const int rc_ = (call);             \
        if (rc_ != SW_OK) fail(#call, rc_); \
    } while (0)

// ---- owners: not copyable; the destructors ignore statuses and launch nothing (sw_device_free is hipFree, which waits for the device)
struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy&) = delete;
    NoCopy& operator=(const NoCopy&) = delete;
};
struct Context : NoCopy {
    sw_ctx* p = nullptr;
    explicit Context(int device) { CHECK(sw_create(device, &p)); }
    ~Context() { sw_destroy(p); }
    operator sw_ctx*() const { return p; }
};

struct DeviceBuffer : NoCopy {
    sw_ctx* ctx = nullptr;
    void* p = nullptr;
    DeviceBuffer() = default;   // nothing yet: alloc() where the mode's story has it
    DeviceBuffer(sw_ctx* c, size_t bytes) { alloc(c, bytes); }
    // letters or a matrix as the kernels read them: the bytes and the 16 bytes of padding the C-ABI asks for behind them
    DeviceBuffer(sw_ctx* c, const void* src, size_t bytes) { alloc(c, src, bytes); }
    ~DeviceBuffer() { if (p) (void)sw_device_free(ctx, p); }
    void alloc(sw_ctx* c, size_t bytes) { ctx = c; CHECK(sw_device_malloc(ctx, bytes, &p)); }
    void alloc(sw_ctx* c, const void* src, size_t bytes) { alloc(c, bytes + 16); upload(src, bytes); }
    template <class T> T* as() const { return (T*)p; }
    explicit operator bool() const { return p != nullptr; }
    void upload(const void* src, size_t bytes) const { if (bytes) CHECK(sw_memcpy_h2d(ctx, p, src, bytes)); }
    void download(void* dst, size_t bytes) const { if (bytes) CHECK(sw_memcpy_d2h(ctx, dst, p, bytes)); }
};

struct DbHandle : NoCopy {
    sw_db* p = nullptr;
    DbHandle() = default;       // create() inside the mode's timed region
    ~DbHandle() { sw_db_free(p); }
    void create(sw_ctx* ctx, const DeviceBuffer& d_db, const std::vector<int64_t>& offsets, int64_t nrec) {
        CHECK(sw_db_create(ctx, d_db.as<const char>(), offsets.data(), nrec, &p));
    }
    operator sw_db*() const { return p; }
    int64_t longest() const { int64_t n = 0; CHECK(sw_db_info(p, nullptr, nullptr, &n, nullptr)); return n; }
};

// ---- loaders
// every record of a FASTA file back to back: a database, or a file of queries
struct Db {
    std::vector<char> letters;
    std::vector<int64_t> offsets;
    int64_t nrec = 0, total = 0;
    int64_t len(int64_t i) const { return offsets[(size_t)i + 1] - offsets[(size_t)i]; }
    const char* record(int64_t i) const { return letters.data() + offsets[(size_t)i]; }
    int64_t longest() const { int64_t n = 0; for (int64_t i = 0; i < nrec; ++i) n = std::max(n, len(i)); return n; }
};
static Db read_db(const char* path) {
    Db d;
    CHECK(sw_read_fasta_db(path, nullptr, 0, nullptr, 0, &d.nrec, &d.total));
    d.letters.resize((size_t)d.total + 1);
    d.offsets.assign((size_t)d.nrec + 1, 0);
    CHECK(sw_read_fasta_db(path, d.letters.data(), d.total, d.offsets.data(), d.nrec + 1, &d.nrec, &d.total));
    return d;
}

// PSI-BLAST's ASCII PSSM.  Bytes the matrix has no row entry for score the file's smallest entry (the rule of sw_read_submat) and smax
// is its largest one, so nothing is clamped.
struct Pssm {
    char letters[256];
    int32_t nletters = 0;
    std::vector<int8_t> matrix;
    int64_t ncols = 0;
    int other = 0, smax = 0;
};
static void read_pssm_file(const char* path, Pssm* m) {   // (filled in place: a sw_pssm_scoring points at m->letters)
    CHECK(sw_read_pssm(path, m->letters, &m->nletters, nullptr, 0, &m->ncols));
    m->matrix.resize((size_t)m->ncols * (size_t)m->nletters);
    CHECK(sw_read_pssm(path, m->letters, &m->nletters, m->matrix.data(), (int64_t)m->matrix.size(), &m->ncols));
    m->other = std::min<int>(*std::min_element(m->matrix.begin(), m->matrix.end()), 0);
    m->smax = std::max<int>(*std::max_element(m->matrix.begin(), m->matrix.end()), 0);
}
// the query line of a matrix's alignments: per column the first letter with the largest entry
static std::string consensus(const Pssm& m, const int8_t* matrix, int64_t ncols) {
    std::string s((size_t)ncols, '?');
    for (int64_t g = 0; g < ncols; ++g) {
        const int8_t* col = matrix + g * m.nletters;
        s[(size_t)g] = m.letters[std::max_element(col, col + m.nletters) - col];
    }
    return s;
}

// (`on`: --matrix or --gap-open was given, the search goes through the affine kernel; --gap-extend alone is a linear gap: sw_search_device)
struct AffineArgs { bool on = false; const char* matrix = nullptr; bool has_open = false, has_extend = false; int open = 0, extend = 0; };
// the table of --matrix, or match / mismatch of --scores, and the gaps that go with it; aff.sub points at sub, so it stays where it is
struct Scoring : NoCopy {
    sw_submat sub;
    sw_affine aff;
    Scoring(const AffineArgs& af, const sw_scores& sc) : aff{&sub, af.has_open ? af.open : 0, af.has_extend ? af.extend : sc.gap} {
        if (af.matrix) CHECK(sw_read_submat(af.matrix, &sub));
        else sw_submat_match(sc.match, sc.mismatch, &sub);
    }
};

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
// ... of a database whose lines name their targets: the two readers must agree on the records, or a name would label another target
static std::vector<std::string> target_names(const char* flag, const char* path, const Db& db) {
    std::vector<std::string> names = fasta_names(path);
    if ((int64_t)names.size() != db.nrec) {
        fprintf(stderr, "smithW: %s: %s has %lld records but %zu header names\n", flag, path, (long long)db.nrec, names.size());
        throw Exit{1};
    }
    return names;
}

// ---- --mask: the low-complexity mask of the database (sw_db_mask_low_complexity) and what the command line says about its rule
struct MaskArgs {
    bool on = false, has_sub = false;        // --mask; any of the sub-flags
    int window = 12, trigger = 2200, extend = 2500;
    const char *byte = "X", *letters = "ACDEFGHIKLMNPQRSTVWY";
    sw_mask_params params() const {
        sw_mask_params mp;
        memset(&mp, 0, sizeof mp);
        mp.window = window; mp.trigger_mbits = trigger; mp.extend_mbits = extend;
        mp.nletters = (int32_t)std::min<size_t>(strlen(letters), 32);
        memcpy(mp.letters, letters, (size_t)mp.nletters);
        mp.mask_byte = (unsigned char)byte[0];
        return mp;
    }
};
// After the upload: the masked copy of the database in a second buffer, its letters on the host (what --align prints is what was
// scored) and the handle over the UNMASKED bytes, through which --out-a3m writes the original letters.  Without --mask it is the
// database as it was read and uploaded.  One line on stderr says what was masked.
struct MaskedDb : NoCopy {
    const Db& plain;
    const DeviceBuffer& d_plain;
    bool on;
    Db host;
    DeviceBuffer d_masked;
    DbHandle unmasked;
    MaskedDb(sw_ctx* ctx, const MaskArgs& m, const Db& db, const DeviceBuffer& d_db) : plain(db), d_plain(d_db), on(m.on) {
        if (!on) return;
        const sw_mask_params mp = m.params();
        const size_t nrec = (size_t)std::max<int64_t>(1, db.nrec);
        unmasked.create(ctx, d_db, db.offsets, db.nrec);
        d_masked.alloc(ctx, (size_t)db.total + 16);
        DeviceBuffer d_n(ctx, nrec * sizeof(int64_t));
        CHECK(sw_db_mask_low_complexity(ctx, unmasked, &mp, d_masked.as<char>(), d_n.as<int64_t>(), nullptr));
        CHECK(sw_synchronize(ctx, nullptr));
        host = db;
        d_masked.download(host.letters.data(), (size_t)db.total);
        std::vector<int64_t> n(nrec, 0);
        d_n.download(n.data(), (size_t)db.nrec * sizeof(int64_t));
        long long letters = 0, targets = 0;
        for (int64_t i = 0; i < db.nrec; ++i) { letters += n[(size_t)i]; targets += n[(size_t)i] > 0; }
        fprintf(stderr, "smithW: --mask: %lld letters of %lld targets masked (of %lld letters, %lld targets)\n", letters, targets, (long long)db.total, (long long)db.nrec);
    }
    const Db& db() const { return on ? host : plain; }
    const DeviceBuffer& buffer() const { return on ? d_masked : d_plain; }
    sw_db* original(sw_db* searched) const { return on ? unmasked.p : searched; }   // the handle that holds the letters as they were read
};

// ---- the alignments of a table of hits on the host: K entries per row, ops_cap bytes of ops per entry
struct AlignedHits {
    std::vector<sw_alignment> aln;
    std::vector<char> ops;
    int64_t ops_cap = 0;
    bool empty() const { return aln.empty(); }
    const sw_alignment* row(int64_t i, int64_t K) const { return aln.data() + i * K; }
    const char* ops_of(int64_t entry) const { return ops.data() + (size_t)entry * (size_t)ops_cap; }
    // row i alone, as a table of one row (an empty table has empty rows)
    AlignedHits only_row(int64_t i, int64_t K) const {
        AlignedHits r;
        if (empty()) return r;
        r.aln.assign(row(i, K), row(i, K) + K);
        r.ops.assign(ops_of(i * K), ops_of((i + 1) * K));
        r.ops_cap = ops_cap;
        return r;
    }
};
static AlignedHits download_aligned(const DeviceBuffer& d_aln, const DeviceBuffer& d_ops, size_t n, int64_t ops_cap) {
    AlignedHits a;
    a.aln.resize(n); a.ops.resize(n * (size_t)ops_cap); a.ops_cap = ops_cap;
    d_aln.download(a.aln.data(), n * sizeof(sw_alignment));
    d_ops.download(a.ops.data(), a.ops.size());
    return a;
}

// ---- the statistics of a many-query search (--evalue, --include-evalue): the score histograms the _top_stats calls fill on the
// device, and what the host makes of them once per round -- 40 KiB per query come back, the fit and the thresholds are O(queries)
struct ScoreStats : NoCopy {
    int64_t nq = 0;
    int shift = 0;
    DeviceBuffer d_hist, d_thr;
    std::vector<uint32_t> hist;
    std::vector<sw_score_fit> fit;
    std::vector<int64_t> thr;
    void alloc(sw_ctx* ctx, int64_t queries, int score_shift) {
        nq = queries; shift = score_shift;
        const size_t cells = (size_t)std::max<int64_t>(1, nq) * SW_HIST_CLASSES * SW_HIST_BINS;
        d_hist.alloc(ctx, cells * sizeof(uint32_t));
        d_thr.alloc(ctx, (size_t)std::max<int64_t>(1, nq) * SW_HIST_CLASSES * sizeof(int64_t));
        hist.resize(cells); fit.resize((size_t)std::max<int64_t>(1, nq)); thr.resize((size_t)std::max<int64_t>(1, nq) * SW_HIST_CLASSES);
    }
    explicit operator bool() const { return (bool)d_hist; }
    // the stream has been synchronised: the histograms of the last search come to the host and are fitted
    void fit_last_search() {
        d_hist.download(hist.data(), (size_t)nq * SW_HIST_CLASSES * SW_HIST_BINS * sizeof(uint32_t));
        CHECK(sw_score_fit_hist(hist.data(), nq, shift, fit.data()));
    }
    // ... and the thresholds of `evalue` under that fit, on the host and in d_thr
    const int64_t* thresholds(double evalue) {
        CHECK(sw_score_thresholds(fit.data(), nq, evalue, thr.data()));
        d_thr.upload(thr.data(), (size_t)nq * SW_HIST_CLASSES * sizeof(int64_t));
        return thr.data();
    }
};

// ---- printers
// the line the run scripts grep for: seconds, GCUPS of `cells`, then the mode's own detail inside the parentheses ("; ...", or none)
__attribute__((format(printf, 3, 4))) static void print_elapsed(double seconds, double cells, const char* detail, ...) {
    printf("\nElapsed time for database search: %f (%.1f GCUPS", seconds, seconds > 0 ? cells / seconds / 1e9 : 0.0);
    va_list ap;
    va_start(ap, detail);
    if (detail) vprintf(detail, ap);
    va_end(ap);
    printf(")\n\n");
}
// one pair of --pairs / --prefilter: the result of query record q (M - 1 letters) against target record t; `ungapped`: the suffix of --prefilter
static void print_pair(long long q, long long t, const char* name, const sw_result& r, long long M, const int32_t* ungapped = nullptr) {
    printf("%lld\t%lld\t%s\t%lld\t%lld\t%lld", q, t, name, (long long)r.max_score, (long long)(r.max_pos / M), (long long)(r.max_pos % M));
    if (ungapped) printf(" ungapped=%d", *ungapped);
    printf("\n");
}

// ---- what main() parses; every mode takes it whole
struct Options {
    long long cols = 8, rows = 9;
    int npos = 0;
    bool builtin = true, dump = false, labels = false, h64 = false, backtrack = true, p8 = false;
    std::vector<int> devices;
    unsigned seed = 1;
    const char *fasta_a = nullptr, *fasta_b = nullptr;
    long long rec_a = 0, rec_b = 0;
    const char *search_q = nullptr, *search_db = nullptr, *pairs_path = nullptr, *pssm_path = nullptr;
    long long top = 10, min_score = 0, prefilter = 0, prefilter_hits = 0;
    bool has_min_score = false, has_top = false, has_prefilter = false, has_prefilter_hits = false;
    AffineArgs af;
    bool align = false, all_queries = false, align_ckpt = false;
    int search_lanes = 32, pairs_lanes = 32;
    bool has_search_lanes = false, has_pairs_lanes = false;
    int iterations = 1, include_score = 1, prior_weight = 10, weight_hits = 0;
    bool has_weight_hits = false, has_iter_flag = false, has_include_score = false;
    double evalue = 0, include_evalue = 0;   // --evalue E: report by E-value; --include-evalue E: include in the next round by E-value
    bool has_evalue = false, has_include_evalue = false, has_score_shift = false;
    int score_shift = 0;
    const char *out_pssm = nullptr, *out_a3m = nullptr;
    MaskArgs mask;
    sw_scores sc = {3, -3, -2};
    bool iterate() const { return iterations > 1 || out_pssm || out_a3m; }   // (--iterations 1 alone is the search of today, through today's path)
    bool stats() const { return has_evalue || has_include_evalue; }
};

// Which command lines the statistics flags go with: the message of the first rule broken, or none.  (tests/test_cli_score_stats_host.py
// holds every one; main() prints it as it prints its own.)
static std::string score_stats_rule(const Options& o) {
    char msg[256] = "";
    const auto say = [&](const char* fmt, auto... v) { snprintf(msg, sizeof msg, fmt, v...); return std::string(msg); };
    if (!o.stats() && !o.has_score_shift) return "";
    if (o.has_evalue && !(o.evalue > 0)) return say("--evalue E needs E > 0, got %g", o.evalue);
    if (o.has_include_evalue && !(o.include_evalue > 0)) return say("--include-evalue E needs E > 0, got %g", o.include_evalue);
    if (o.score_shift < 0 || o.score_shift > SW_HIST_SHIFT_MAX) return say("--score-shift N needs N within 0..%d, got %d", SW_HIST_SHIFT_MAX, o.score_shift);
    if (!o.stats()) return "--score-shift goes with --evalue or --include-evalue";
    if (o.has_prefilter || o.has_prefilter_hits || o.pairs_path)
        return "--evalue / --include-evalue do not go with --prefilter / --prefilter-hits / --pairs (the fit needs every score, not a censored sample)";
    if (!(o.search_q && (o.all_queries || o.pssm_path))) return "--evalue / --include-evalue go with --search --all-queries or --search --pssm";
    if (o.has_include_evalue && o.has_include_score) return "--include-evalue does not go with --include-score";
    if (o.has_include_evalue && o.iterations < 2) return "--include-evalue goes with --iterations N (N > 1)";
    return "";
}

// Which command lines --mask and its sub-flags go with, and the values they take: the message of the first rule broken, or none.
// (tests/test_cli_mask_host.py holds every one; main() prints it as it prints its own.)
static std::string mask_rule(const Options& o) {
    char msg[256] = "";
    const auto say = [&](const char* fmt, auto... v) { snprintf(msg, sizeof msg, fmt, v...); return std::string(msg); };
    const MaskArgs& m = o.mask;
    if (!m.on && !m.has_sub) return "";
    if (!m.on) return "--mask-window / --mask-trigger / --mask-extend / --mask-byte / --mask-letters go with --mask";
    if (!o.search_q) return "--mask goes with --search";
    if (m.window < 2 || m.window > 64) return say("--mask-window W needs W within 2..64, got %d", m.window);
    if (m.trigger < 0) return say("--mask-trigger MB needs MB >= 0 (thousandths of a bit), got %d", m.trigger);
    if (m.extend < m.trigger) return say("--mask-extend MB needs MB >= the trigger's %d, got %d", m.trigger, m.extend);
    if (strlen(m.byte) != 1) return say("--mask-byte C takes one character, got \"%s\"", m.byte);
    const size_t n = strlen(m.letters);
    if (n < 1 || n > 32) return say("--mask-letters STR takes 1..32 letters, got %d", (int)n);
    for (size_t i = 0; i < n; ++i)
        if (memchr(m.letters, m.letters[i], i)) return say("--mask-letters names '%c' twice", m.letters[i]);
    return "";
}
