// Drives sw_pssm_from_hits_host (smith-waterman_amd/csrc/sw_hits_host.cpp) and sw_write_pssm (.../sw_pssm_read.cpp) for tests/test_pssm_hits_host.py over tables
// NO alignment call would write -- targets -1 and ntargets, counts below 0 and above top, nops 0 and ops_cap + 1, q_begin / t_begin out
// of range, op bytes 0x00 / 0xFF, walks that run past qlen and len, weights out of range -- with every buffer a heap block of EXACTLY
// its size, so that a read or write past one is a sanitizer error.  Built with -fsanitize=address,undefined.  argv[1]: a file to write.
// Prints "ok <sum of the matrix> <sum of the counts>" and returns 0; any other return is a failure.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

static uint32_t g_state = 12345;
static uint32_t rnd() { g_state = g_state * 1664525u + 1013904223u; return g_state >> 8; }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const char letters[] = "ACDEFGHIKLMNPQRSTVWY";
    const int n = 20;
    const int64_t qlens[] = {1, 63, 64, 65, 257}, nq = 5, top = 18, cap = 150, front = 3;
    const int64_t tlens[] = {0, 1, 64, 65, 300}, nt = 5;
    std::vector<int64_t> qoffs(nq + 1), offs(nt + 1);
    qoffs[0] = front;
    for (int64_t q = 0; q < nq; ++q) qoffs[q + 1] = qoffs[q] + qlens[q];
    offs[0] = 0;                                         // the database block starts AT its first target: a read in front of it is an error
    for (int64_t t = 0; t < nt; ++t) offs[t + 1] = offs[t] + tlens[t];
    std::vector<char> db((size_t)offs[nt]);
    for (char& x : db) x = rnd() % 8 ? letters[rnd() % n] : (char)(rnd() & 0xFF);
    static sw_submat sub;
    for (int x = 0; x < 256; ++x)
        for (int y = 0; y < 256; ++y) sub.s[x][y] = (int8_t)((int)(rnd() % 21) - 10);
    // the prior block holds the queries' columns and nothing behind them; the front columns are part of the layout
    std::vector<int8_t> prior((size_t)(qoffs[nq] * n)), out((size_t)(qoffs[nq] * n), 0x55);
    for (int8_t& v : prior) v = (int8_t)((int)(rnd() % 41) - 20);
    std::vector<int32_t> counts((size_t)((qoffs[nq] - front) * n), 0x55555555);
    std::vector<sw_hit> hits((size_t)(nq * top));
    std::vector<sw_alignment> aln((size_t)(nq * top));
    std::vector<char> ops((size_t)(nq * top * cap));
    std::vector<int32_t> w((size_t)(nq * top));
    std::vector<int64_t> nhits = {-5, top + 7, top, top - 1, top};
    for (int64_t e = 0; e < nq * top; ++e) {
        const int64_t q = e / top;
        const int what = (int)(e % 9);
        hits[e] = {(int64_t)(rnd() % nt), 0, 0};
        aln[e] = {0, (int64_t)(rnd() % 100), (int64_t)(rnd() % (qlens[q] + 1)), (int64_t)(rnd() % 2), 0, 0, (int64_t)(1 + rnd() % cap)};
        for (int64_t o = 0; o < cap; ++o) ops[e * cap + o] = "MMMID"[rnd() % 5];
        w[e] = (int32_t)(rnd() % 5) - 1;
        if (what == 0) hits[e].target = -1;
        if (what == 1) hits[e].target = nt;
        if (what == 2) aln[e].nops = 0;
        if (what == 3) aln[e].nops = cap + 1;
        if (what == 4) aln[e].q_begin = qlens[q] + 1;
        if (what == 5) for (int64_t o = 0; o < cap; o += 2) ops[e * cap + o] = o % 4 ? (char)0xFF : (char)0x00;
        if (what == 6) { aln[e].nops = cap; memset(&ops[e * cap], 'M', (size_t)cap); w[e] = 70000; }   // past qlen and len
        if (what == 7) aln[e].t_begin = -1;
    }
    const sw_pssm_scoring sc = {letters, n, -4, 11, -10, -1};
    const sw_pssm_update upd = {&sub, 3, 10};
    if (sw_pssm_from_hits_host(prior.data(), qoffs.data(), nq, db.data(), offs.data(), nt, &sc, &upd, hits.data(), nhits.data(), top, aln.data(), ops.data(), cap,
                               w.data(), out.data(), counts.data()) != SW_OK) {
        printf("%s\n", swh::g_err.c_str());
        return 3;
    }
    for (int64_t g = 0; g < front * n; ++g)
        if (out[g] != 0x55) return 4;                    // the unused front columns stay
    // in place, counts only, matrix only: the same bytes
    std::vector<int8_t> inplace = prior;
    if (sw_pssm_from_hits_host(inplace.data(), qoffs.data(), nq, db.data(), offs.data(), nt, &sc, &upd, hits.data(), nhits.data(), top, aln.data(), ops.data(), cap,
                               w.data(), inplace.data(), nullptr) != SW_OK) return 5;
    if (memcmp(inplace.data() + front * n, out.data() + front * n, (size_t)((qoffs[nq] - front) * n)) != 0) return 6;
    std::vector<int32_t> again(counts.size());
    if (sw_pssm_from_hits_host(prior.data(), qoffs.data(), nq, db.data(), offs.data(), nt, &sc, &upd, hits.data(), nhits.data(), top, aln.data(), ops.data(), cap,
                               w.data(), nullptr, again.data()) != SW_OK || again != counts) return 7;
    // refusals write nothing
    if (sw_pssm_from_hits_host(prior.data(), qoffs.data(), nq, db.data(), offs.data(), nt, &sc, &upd, hits.data(), nhits.data(), top, aln.data(), ops.data(), cap,
                               w.data(), nullptr, nullptr) != SW_EINVAL) return 8;
    // the writer, and the reader on what it wrote
    std::vector<char> cons((size_t)(qoffs[nq] - front), 'Q');
    if (sw_write_pssm(argv[1], letters, n, out.data() + front * n, qoffs[nq] - front, cons.data()) != SW_OK) { printf("%s\n", swh::g_err.c_str()); return 9; }
    std::vector<char> lt(256);
    int32_t nl = 0;
    int64_t ncols = 0;
    if (sw_read_pssm(argv[1], lt.data(), &nl, nullptr, 0, &ncols) != SW_OK || nl != n || ncols != qoffs[nq] - front) return 10;
    std::vector<int8_t> back((size_t)(ncols * nl));
    if (sw_read_pssm(argv[1], lt.data(), &nl, back.data(), (int64_t)back.size(), &ncols) != SW_OK) return 11;
    if (memcmp(back.data(), out.data() + front * n, back.size()) != 0 || memcmp(lt.data(), letters, (size_t)n) != 0) return 12;
    if (sw_write_pssm(argv[1], "A\x01", 2, out.data(), 1, nullptr) != SW_EINVAL) return 13;
    long long s0 = 0, s1 = 0;
    for (size_t g = (size_t)(front * n); g < out.size(); ++g) s0 += out[g];
    for (int32_t v : counts) s1 += v;
    printf("ok %lld %lld\n", s0, s1);
    return 0;
}
