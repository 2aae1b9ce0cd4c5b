// Drives sw_read_pssm (smith-waterman_amd/csrc/sw_pssm_read.cpp) over one file, for tests/test_pssm_host.py: the two-call pattern with
// heap buffers of EXACTLY the sizes the first call reports, so that a write past either of them is a sanitizer error.  Built with
// -fsanitize=address,undefined.  Prints "nletters ncols sum-of-entries letters" and returns 0, or the error text and returns 3.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "../include/swhip.h"

namespace swh {   // the library's error text (sw_host.cpp there)
static std::string g_err;
void set_err(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}
}  // namespace swh

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::vector<char> letters(256);
    int32_t nletters = 0;
    int64_t ncols = 0;
    if (sw_read_pssm(argv[1], letters.data(), &nletters, nullptr, 0, &ncols) != SW_OK) {
        printf("%s\n", swh::g_err.c_str());
        return 3;
    }
    std::vector<int8_t> pssm((size_t)ncols * (size_t)nletters);
    // one byte short first: refused, nothing written
    if (!pssm.empty() && sw_read_pssm(argv[1], letters.data(), &nletters, pssm.data(), (int64_t)pssm.size() - 1, &ncols) != SW_EINVAL) return 4;
    if (sw_read_pssm(argv[1], letters.data(), &nletters, pssm.data(), (int64_t)pssm.size(), &ncols) != SW_OK) {
        printf("%s\n", swh::g_err.c_str());
        return 3;
    }
    long long sum = 0;
    for (int8_t v : pssm) sum += v;
    printf("%d %lld %lld %.*s\n", nletters, (long long)ncols, sum, nletters, letters.data());
    return 0;
}
