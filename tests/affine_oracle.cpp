// The independent checker of the affine search (tests/test_search_affine_host.py, tests/test_search_affine_gpu.py): a naive
// three-matrix Gotoh written from the recurrence alone, sharing no code with the library.
//
//   H[0][j] = H[i][0] = 0, E[0][j] = F[i][0] = -inf
//   E[i][j] = max(E[i-1][j], H[i-1][j] + go) + ge
//   F[i][j] = max(F[i][j-1], H[i][j-1] + go) + ge
//   H[i][j] = max(0, H[i-1][j-1] + S[q[j-1]][t[i-1]], E[i][j], F[i][j])
//   max_score = max H, max_pos = min{i (qlen + 1) + j : H[i][j] = max H} if max H > 0 else 0
//
// With Hm / Em / Fm given ((len + 1) x (qlen + 1) int64 each) the whole matrices are kept and handed back; without them the three
// matrices keep two rows each (the same loop, rows taken modulo 2), so that a 200 000-row target needs no gigabytes.
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {
constexpr int64_t NEG_INF = INT64_MIN / 4;   // no sum of the recurrence gets near it from either side
int64_t max2(int64_t a, int64_t b) { return a > b ? a : b; }
}  // namespace

extern "C" int affine_oracle_pair(const uint8_t* q, int64_t qlen, const uint8_t* t, int64_t len, const int8_t* S /* 256 x 256 */, int64_t go,
                                  int64_t ge, int64_t* max_score, int64_t* max_pos, int64_t* Hm, int64_t* Em, int64_t* Fm) {
    const int64_t M = qlen + 1;
    const bool full = Hm && Em && Fm;
    std::vector<int64_t> h2, e2, f2;
    if (!full) {
        h2.assign((size_t)(2 * M), 0);
        e2.assign((size_t)(2 * M), NEG_INF);
        f2.assign((size_t)(2 * M), NEG_INF);
    }
    int64_t* H = full ? Hm : h2.data();
    int64_t* E = full ? Em : e2.data();
    int64_t* F = full ? Fm : f2.data();
    auto row = [&](int64_t i) { return (full ? i : (i & 1)) * M; };
    for (int64_t j = 0; j <= qlen; ++j) {
        H[row(0) + j] = 0;
        E[row(0) + j] = NEG_INF;
        F[row(0) + j] = NEG_INF;
    }
    int64_t best = 0, pos = 0;
    for (int64_t i = 1; i <= len; ++i) {
        const int64_t r = row(i), p = row(i - 1);
        H[r] = 0;
        E[r] = NEG_INF;
        F[r] = NEG_INF;
        for (int64_t j = 1; j <= qlen; ++j) {
            E[r + j] = max2(E[p + j], H[p + j] + go) + ge;
            F[r + j] = max2(F[r + j - 1], H[r + j - 1] + go) + ge;
            const int64_t d = H[p + j - 1] + S[(int64_t)q[j - 1] * 256 + t[i - 1]];
            H[r + j] = max2(max2(0, d), max2(E[r + j], F[r + j]));
            if (H[r + j] > best) {
                best = H[r + j];
                pos = i * M + j;
            }
        }
    }
    *max_score = best;
    *max_pos = pos;
    return 0;
}

// every target of a packed database: res[k] = {max_pos, max_score, 0}
extern "C" int affine_oracle_search(const uint8_t* q, int64_t qlen, const uint8_t* db, const int64_t* offsets, int64_t ntargets, const int8_t* S,
                                    int64_t go, int64_t ge, int64_t* res) {
    for (int64_t k = 0; k < ntargets; ++k) {
        int64_t score = 0, pos = 0;
        affine_oracle_pair(q, qlen, db + offsets[k], offsets[k + 1] - offsets[k], S, go, ge, &score, &pos, nullptr, nullptr, nullptr);
        res[3 * k] = pos;
        res[3 * k + 1] = score;
        res[3 * k + 2] = 0;
    }
    return 0;
}
