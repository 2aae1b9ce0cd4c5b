// sw_score_stats.cpp -- the host side of the search statistics (include/swhip.h states the rules): the CPU legs of the score
// histogram (sw_score_hist_host) and of the thresholds of a hit table (sw_hits_threshold_host), the argument checks they share with
// the device calls, and the ONE implementation of what follows the histogram: the fit (sw_score_fit_hist), the E-value
// (sw_score_evalue) and the thresholds (sw_score_thresholds), in double, O(nqueries x 10 240).  Plain C++ that needs nothing of the
// library but the header and the error text.
#include <cmath>
#include <cstring>
#include <algorithm>
#include <limits>
#include "../../include/swhip.h"

namespace swh {   // sw_host.cpp
void set_err(const char* fmt, ...);
// (shared with sw_api_search.hip through sw_ctx.h, not exported by the library)
__attribute__((visibility("hidden"))) int check_score_hist(const char* who, const void* results, int64_t nqueries, int64_t ntargets, int shift, const void* hist);
__attribute__((visibility("hidden"))) int check_hits_threshold(const char* who, const void* thresholds, int64_t nqueries, int64_t ntargets, int64_t top,
                                                               const void* hits, const void* hits_out, const void* keep);
}  // namespace swh

namespace {

constexpr int64_t kMaxDim = (1 << 20) - 1;   // swk::SW_MAX_DIM (this file does not see the kernels' header)
constexpr int kClasses = SW_HIST_CLASSES, kBins = SW_HIST_BINS, kCells = kClasses * kBins;
constexpr double kEulerGamma = 0.57721566490153286061;
const double kPiOverSqrt6 = 3.14159265358979323846 / std::sqrt(6.0);

// The half-octave class of a length >= 1 and the bin of a score: the rule of include/swhip.h (swk::score_class, swk::score_bin).
int length_class(int64_t len) {
    if (len < 2) return 0;
    const int e = 63 - __builtin_clzll((unsigned long long)len);
    return 2 * e + (int)((len >> (e - 1)) & 1);
}
int score_bin(int64_t v, int shift) { return (int)std::min<int64_t>(std::max<int64_t>(v, 0) >> shift, kBins - 1); }

int check_target_lengths(const char* who, const int64_t* offsets, int64_t ntargets) {
    for (int64_t k = 0; k < ntargets; ++k) {
        const int64_t len = offsets[k + 1] - offsets[k];
        if (len < 0 || len > kMaxDim) { swh::set_err("%s: target %lld has length %lld, out of range 0..%lld", who, (long long)k, (long long)len, (long long)kMaxDim); return SW_EINVAL; }
    }
    return SW_OK;
}

// One weighted least-squares line through the cells of a query's histogram, bin 255 left out; `prev`: the fit whose z drops cells, or NULL.
struct Line { double a = 0, b = 0, sigma = 0, W = 0; };
Line fit_line(const uint32_t* h, double scale, double mid, const Line* prev) {
    const bool trim = prev && prev->sigma > 0;
    auto weight = [&](int c, int s) -> double {
        const uint32_t n = h[c * kBins + s];
        if (!n || !trim) return (double)n;
        const double z = (s * scale + mid - prev->a - prev->b * c) / prev->sigma;
        return z > 5.0 || z < -4.0 ? 0.0 : (double)n;
    };
    Line l;
    double sx = 0, sy = 0;
    for (int c = 0; c < kClasses; ++c)
        for (int s = 0; s < kBins - 1; ++s) {
            const double w = weight(c, s);
            l.W += w; sx += w * c; sy += w * (s * scale + mid);
        }
    if (!(l.W > 0)) return l;
    const double mx = sx / l.W, my = sy / l.W;
    double sxx = 0, sxy = 0;
    for (int c = 0; c < kClasses; ++c)
        for (int s = 0; s < kBins - 1; ++s) {
            const double w = weight(c, s);
            sxx += w * (c - mx) * (c - mx); sxy += w * (c - mx) * (s * scale + mid - my);
        }
    l.b = sxx > 0 ? sxy / sxx : 0.0;
    l.a = my - l.b * mx;
    double srr = 0;
    for (int c = 0; c < kClasses; ++c)
        for (int s = 0; s < kBins - 1; ++s) {
            const double r = s * scale + mid - l.a - l.b * c;
            srr += weight(c, s) * r * r;
        }
    l.sigma = l.W > 2 ? std::sqrt(srr / (l.W - 2)) : 0.0;
    return l;
}

// The E-value of `score` against a target of class c under a valid fit.
double class_evalue(const sw_score_fit& f, int c, int64_t score) {
    const double z = ((double)score - f.a - f.b * c) / f.sigma;
    return (double)f.n_db * -std::expm1(-std::exp(-kPiOverSqrt6 * z - kEulerGamma));
}

}  // namespace

namespace swh {

// What sw_score_hist_device and sw_score_hist_host check alike.
int check_score_hist(const char* who, const void* results, int64_t nqueries, int64_t ntargets, int shift, const void* hist) {
    if (!results || !hist) { set_err("%s: NULL result table or histogram", who); return SW_EINVAL; }
    if (nqueries < 0 || ntargets < 0) { set_err("%s: negative query or target count", who); return SW_EINVAL; }
    if (shift < 0 || shift > SW_HIST_SHIFT_MAX) { set_err("%s: shift = %d is out of range 0..%d", who, shift, SW_HIST_SHIFT_MAX); return SW_EINVAL; }
    if (ntargets >= (1ll << 31)) { set_err("%s: %lld targets, the histogram takes fewer than 2^31", who, (long long)ntargets); return SW_EINVAL; }
    return SW_OK;
}

// What sw_hits_threshold_device and sw_hits_threshold_host check alike.
int check_hits_threshold(const char* who, const void* thresholds, int64_t nqueries, int64_t ntargets, int64_t top, const void* hits, const void* hits_out,
                         const void* keep) {
    if (!thresholds || !hits) { set_err("%s: NULL thresholds or hit table", who); return SW_EINVAL; }
    if (nqueries < 0 || ntargets < 0) { set_err("%s: negative query or target count", who); return SW_EINVAL; }
    if (ntargets >= (1ll << 31)) { set_err("%s: %lld targets, a hit table takes fewer than 2^31", who, (long long)ntargets); return SW_EINVAL; }
    if (top < 1 || top > SW_TOP_MAX) { set_err("%s: top = %lld is out of range 1..%d", who, (long long)top, SW_TOP_MAX); return SW_EINVAL; }
    if (!keep && !hits_out) { set_err("%s: no output: the keep table and the thresholded hit table are both NULL", who); return SW_EINVAL; }
    return SW_OK;
}

}  // namespace swh

extern "C" {

// The CPU leg of sw_score_hist_device: the rule restated, target by target.  Everything is checked before the first counter is written.
int sw_score_hist_host(const sw_result* results, int64_t nqueries, const int64_t* offsets, int64_t ntargets, int shift, uint32_t* hist) {
    const char* who = "sw_score_hist_host";
    if (!offsets) { swh::set_err("%s: NULL offsets", who); return SW_EINVAL; }
    if (int rc = swh::check_score_hist(who, results, nqueries, ntargets, shift, hist)) return rc;
    if (int rc = check_target_lengths(who, offsets, ntargets)) return rc;
    if (nqueries > 0) std::memset(hist, 0, (size_t)nqueries * kCells * sizeof(uint32_t));
    for (int64_t q = 0; q < nqueries; ++q)
        for (int64_t k = 0; k < ntargets; ++k) {
            const int64_t len = offsets[k + 1] - offsets[k];
            if (len < 1) continue;
            ++hist[(q * kClasses + length_class(len)) * kBins + score_bin(results[q * ntargets + k].max_score, shift)];
        }
    return SW_OK;
}

// The fit of include/swhip.h: a first round over every cell below bin 255, then three rounds that each start from the full counts and
// leave out the cells whose z under the round before is > 5 or < -4 (not cumulative; a round without a positive sigma drops nothing).
int sw_score_fit_hist(const uint32_t* hist, int64_t nqueries, int shift, sw_score_fit* fit) {
    const char* who = "sw_score_fit_hist";
    if (!hist || !fit) { swh::set_err("%s: NULL histogram or fit", who); return SW_EINVAL; }
    if (nqueries < 0) { swh::set_err("%s: negative query count", who); return SW_EINVAL; }
    if (shift < 0 || shift > SW_HIST_SHIFT_MAX) { swh::set_err("%s: shift = %d is out of range 0..%d", who, shift, SW_HIST_SHIFT_MAX); return SW_EINVAL; }
    const double scale = (double)(1ll << shift), mid = (scale - 1.0) / 2.0;
    for (int64_t q = 0; q < nqueries; ++q) {
        const uint32_t* h = hist + q * kCells;
        sw_score_fit f;
        std::memset(&f, 0, sizeof f);
        f.shift = shift;
        for (int c = 0; c < kClasses; ++c) {
            for (int s = 0; s < kBins; ++s) f.n_db += h[c * kBins + s];
            f.n_censored += h[c * kBins + kBins - 1];
        }
        Line l = fit_line(h, scale, mid, nullptr);
        for (int round = 0; round < 3; ++round) {
            const Line prev = l;
            l = fit_line(h, scale, mid, &prev);
        }
        f.a = l.a; f.b = l.b; f.sigma = l.sigma;
        f.n_fit = (int64_t)l.W;
        f.valid = l.W >= 30 && l.sigma > 0;
        fit[q] = f;
    }
    return SW_OK;
}

// E = n_db (1 - exp(-exp(-(pi / sqrt 6) z - gamma))); 1 - exp(-x) is taken as -expm1(-x), which keeps the small E-values of real hits.
double sw_score_evalue(const sw_score_fit* fit, int64_t target_len, int64_t score) {
    if (!fit || !fit->valid || target_len < 1) return std::numeric_limits<double>::quiet_NaN();
    return class_evalue(*fit, length_class(target_len), score);
}

// T[q][c]: the smallest integer score whose E-value in class c is <= evalue.  The closed form gives it up to the rounding of its last
// step; the two loops then hold it against sw_score_evalue itself, so that E(T) <= evalue < E(T - 1) holds as computed.
int sw_score_thresholds(const sw_score_fit* fit, int64_t nqueries, double evalue, int64_t* thresholds) {
    const char* who = "sw_score_thresholds";
    if (!fit || !thresholds) { swh::set_err("%s: NULL fit or thresholds", who); return SW_EINVAL; }
    if (nqueries < 0) { swh::set_err("%s: negative query count", who); return SW_EINVAL; }
    if (!(evalue > 0)) { swh::set_err("%s: the E-value must be above 0", who); return SW_EINVAL; }
    for (int64_t q = 0; q < nqueries; ++q) {
        const sw_score_fit& f = fit[q];
        int64_t* t = thresholds + q * kClasses;
        if (!f.valid || evalue >= (double)f.n_db) { std::fill(t, t + kClasses, (int64_t)0); continue; }
        const double z0 = -(std::log(-std::log1p(-evalue / (double)f.n_db)) + kEulerGamma) / kPiOverSqrt6;
        for (int c = 0; c < kClasses; ++c) {
            int64_t v = (int64_t)std::ceil(f.a + f.b * c + f.sigma * z0);
            for (int i = 0; i < 4 && class_evalue(f, c, v - 1) <= evalue; ++i) --v;
            for (int i = 0; i < 4 && !(class_evalue(f, c, v) <= evalue); ++i) ++v;
            t[c] = v;
        }
    }
    return SW_OK;
}

// The CPU leg of sw_hits_threshold_device.  Everything is checked before the first byte is written; hits_out may be hits.
int sw_hits_threshold_host(const int64_t* offsets, int64_t ntargets, const int64_t* thresholds, int64_t nqueries, int64_t top, const sw_hit* hits,
                           const int64_t* nhits, sw_hit* hits_out, int32_t* keep, int64_t* nkept) {
    const char* who = "sw_hits_threshold_host";
    if (!offsets) { swh::set_err("%s: NULL offsets", who); return SW_EINVAL; }
    if (int rc = swh::check_hits_threshold(who, thresholds, nqueries, ntargets, top, hits, hits_out, keep)) return rc;
    if (int rc = check_target_lengths(who, offsets, ntargets)) return rc;
    for (int64_t q = 0; q < nqueries; ++q) {
        const int64_t n = nhits ? std::clamp<int64_t>(nhits[q], 0, top) : top;
        int64_t kept = 0;
        for (int64_t r = 0; r < top; ++r) {
            const int64_t e = q * top + r;
            const sw_hit h = hits[e];
            int32_t k = 0;
            if (r < n && (uint64_t)h.target < (uint64_t)ntargets) {
                const int64_t len = offsets[h.target + 1] - offsets[h.target];
                if (len >= 1) k = h.max_score >= thresholds[q * kClasses + length_class(len)];
            }
            if (keep) keep[e] = k;
            if (hits_out) hits_out[e] = sw_hit{k ? h.target : -1, h.max_pos, h.max_score};
            kept += k;
        }
        if (nkept) nkept[q] = kept;
    }
    return SW_OK;
}

}  // extern "C"
