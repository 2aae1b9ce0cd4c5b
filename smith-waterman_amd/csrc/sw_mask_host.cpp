// sw_mask_host.cpp -- the CPU leg of the low-complexity mask (sw_mask_low_complexity_host; include/swhip.h states the rule) and the
// check of sw_mask_params it shares with the device call, which also turns the two entropy bounds into the integers the windows are
// compared with.  The leg restates the rule as it is written: window by window, the counts afresh for every start.  Plain C++ that
// needs nothing of the library but the header, the table and the error text.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../include/swhip.h"
#include "sw_mask_table.h"

namespace swh {
void set_err(const char* fmt, ...);
__attribute__((visibility("hidden"))) int check_mask_params(const char* who, const sw_mask_params* mp, int32_t* bound1, int32_t* bound2, unsigned char (&cls)[256]);
}  // namespace swh
using swh::set_err;

namespace {
constexpr int64_t kG[SW_MASK_WINDOW_MAX + 1] = {SW_MASK_G_LITERALS};
constexpr unsigned char kNoLetter = 32;
}  // namespace

namespace swh {

// What both legs check of the rule; *bound1 and *bound2 receive min(floor(K x W x 65536 / 1000), G[W]) -- D never exceeds G[W], so the
// clamp changes no comparison and the bounds fit int32 --, cls the class 0..31 of every byte, 32 for a no-letter.
int check_mask_params(const char* who, const sw_mask_params* mp, int32_t* bound1, int32_t* bound2, unsigned char (&cls)[256]) {
    if (!mp) { set_err("%s: NULL pointer", who); return SW_EINVAL; }
    if (mp->window < 2 || mp->window > SW_MASK_WINDOW_MAX) { set_err("%s: window = %d is out of range 2..%d", who, mp->window, SW_MASK_WINDOW_MAX); return SW_EINVAL; }
    if (mp->trigger_mbits < 0 || mp->extend_mbits < mp->trigger_mbits) {
        set_err("%s: the bounds must hold 0 <= trigger_mbits <= extend_mbits (got %lld, %lld)", who, (long long)mp->trigger_mbits, (long long)mp->extend_mbits);
        return SW_EINVAL;
    }
    const int64_t unit = (int64_t)mp->window * 65536;
    if (mp->extend_mbits > INT64_MAX / unit) { set_err("%s: extend_mbits = %lld x window x 65536 leaves 64 bits", who, (long long)mp->extend_mbits); return SW_EINVAL; }
    if (mp->nletters < 1 || mp->nletters > 32) { set_err("%s: nletters = %d is out of range 1..32", who, mp->nletters); return SW_EINVAL; }
    memset(cls, kNoLetter, sizeof cls);
    for (int k = 0; k < mp->nletters; ++k) {
        if (cls[mp->letters[k]] != kNoLetter) { set_err("%s: the letter with byte value %d is named twice", who, (int)mp->letters[k]); return SW_EINVAL; }
        cls[mp->letters[k]] = (unsigned char)k;
    }
    const int64_t b1 = mp->trigger_mbits * unit / 1000, b2 = mp->extend_mbits * unit / 1000, top = kG[mp->window];
    *bound1 = (int32_t)(b1 < top ? b1 : top);
    *bound2 = (int32_t)(b2 < top ? b2 : top);
    return SW_OK;
}

}  // namespace swh

int sw_mask_low_complexity_host(const char* seq, const int64_t* offsets, int64_t ntargets, const sw_mask_params* params, char* out, int64_t* nmasked) {
    const char* who = "sw_mask_low_complexity_host";
    if (!seq || !offsets || !params || !out || ntargets < 0) { set_err("%s: NULL pointer or negative target count", who); return SW_EINVAL; }
    if (out == seq) { set_err("%s: in place (out == seq) is refused", who); return SW_EINVAL; }
    int32_t bound1, bound2;
    unsigned char cls[256];
    if (int rc = swh::check_mask_params(who, params, &bound1, &bound2, cls)) return rc;
    if (offsets[0] < 0) { set_err("%s: offsets[0] = %lld is negative", who, (long long)offsets[0]); return SW_EINVAL; }
    for (int64_t t = 0; t < ntargets; ++t)
        if (offsets[t + 1] < offsets[t]) { set_err("%s: the offsets decrease at target %lld", who, (long long)t); return SW_EINVAL; }
    const int W = params->window;
    std::vector<unsigned char> low1, low2, masked;
    for (int64_t t = 0; t < ntargets; ++t) {
        const int64_t len = offsets[t + 1] - offsets[t];
        const unsigned char* s = (const unsigned char*)seq + offsets[t];
        const int64_t starts = len - W + 1;                          // the starts i with i + W <= len
        masked.assign((size_t)len, 0);
        if (starts > 0) {
            low1.assign((size_t)starts, 0);
            low2.assign((size_t)starts, 0);
            for (int64_t i = 0; i < starts; ++i) {
                int count[32] = {};
                bool valid = true;
                for (int x = 0; x < W; ++x) {
                    const unsigned char c = cls[s[i + x]];
                    if (c == kNoLetter) valid = false; else ++count[c];
                }
                if (!valid) continue;
                int64_t sum = 0;
                for (int k = 0; k < 32; ++k) sum += kG[count[k]];
                const int64_t D = kG[W] - sum;
                low1[(size_t)i] = D <= bound1;
                low2[(size_t)i] = D <= bound2;
            }
            for (int64_t i = 0; i < starts;) {                       // the runs of low2
                if (!low2[(size_t)i]) { ++i; continue; }
                int64_t e = i;
                bool triggered = false;
                for (; e < starts && low2[(size_t)e]; ++e) triggered |= low1[(size_t)e] != 0;
                if (triggered)
                    for (int64_t p = i; p < e - 1 + W; ++p) masked[(size_t)p] = 1;
                i = e;
            }
        }
        int64_t n = 0;
        char* o = out + offsets[t];
        for (int64_t p = 0; p < len; ++p) {
            o[p] = masked[(size_t)p] ? (char)params->mask_byte : (char)s[p];
            n += masked[(size_t)p];
        }
        if (nmasked) nmasked[t] = n;
    }
    return SW_OK;
}
