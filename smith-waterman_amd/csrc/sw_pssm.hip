// sw_pssm.hip -- the query profiles of a position-specific scoring matrix (sw_db_search_pssm and its twins, gfx950).
//
// Every kernel of the many-query family scores a cell by one byte of a query's profile, prof[x][c]: query column c against target byte x
// (257 x qpad bytes, sw_search_multi.hip).  sw_search_profile_submat_multi fills it from the query's letters and a 256 x 256 table; the
// kernel below fills the same layout from a PSSM, and nothing behind the profile can tell the two apart.
//
// The PSSM is column-major -- column g is the nletters bytes at pssm + g * nletters, byte k of it scores the target byte letters[k] --
// and the profile is row-major, one row per byte value: the kernel is a transposition through the LDS.
//   * A tile is 256 adjacent query columns: 256 * nletters adjacent bytes of the PSSM (at most 64 KiB), at any byte address.  The
//     workgroup reads every byte of it ONCE, 256 adjacent bytes per step, clamps it to smax and stores it to the LDS.
//   * It then writes the 257 rows of the tile: thread c the byte of column c, 256 adjacent bytes of one row per step (the stores of
//     sw_search_profile_submat_multi).  Row x reads byte code[x] of every column, code[] being the call's 256-byte table from a target
//     byte to its place in a column; a code >= nletters says the byte is not among the letters: the row is `other`.  x is uniform in the
//     workgroup: code[x] is read with a vector load at a uniform address and made a scalar (readfirstlane), the choice is scalar.
//   * LDS layout: column c takes `stride` dwords, byte k of it in dword k / 4.  The 32 lanes of a half-wave read the same k of 32
//     adjacent columns, so their bank is (c * stride + k / 4) mod 32 (ds_read_u8: 32 banks of 4 bytes): with an ODD stride the 32
//     banks are distinct.  stride = ceil(nletters / 4) | 1; only 253..256 letters would pass 64 KiB that way (65 dwords), so there the
//     stride stays 64 and dword d of column c lies at d ^ (c & 31) instead: bank (d ^ c) mod 32, distinct again.
//     The fill's byte stores go to 256 adjacent bytes spread over 256 / nletters columns; their conflicts are bounded by the same
//     argument and the fill is a 257th of the LDS traffic.
// Bounds: a tile's reads are [first column * nletters, (last column + 1) * nletters) of the query's own columns, nothing else; the
// stores are the stores of sw_search_profile_submat_multi, inside 257 x qpad bytes at prof_off.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"

namespace swk {

// The profiles of the table entries tab[0 .. nq) from a PSSM: for entry t, prof[prof_off + x * qpad + c] = s(qstart + c, x) for x < 256,
// c < qlen, with s(g, x) = min(pssm[g * nletters + code[x]], smax) where code[x] < nletters and `other` elsewhere; row 256 (PAD) and
// columns >= qlen: -1.  Every query is cut into `parts` interleaved shares of whole tiles, dealt to the workgroups in turn.
// Dynamic LDS: 1024 * (nletters > 252 ? 64 : ceil(nletters / 4) | 1) bytes.
__global__ void __launch_bounds__(256) sw_search_profile_pssm_multi(const signed char* __restrict__ pssm, const MultiQuery* __restrict__ tab, int64_t nq, int parts,
                                                                    signed char* __restrict__ prof, const unsigned char* __restrict__ code, int nletters,
                                                                    int other, int smax) {
    extern __shared__ unsigned int lds_dw[];
    signed char* lds = (signed char*)lds_dw;
    const bool swz = nletters > 252;
    const int stride = swz ? 64 : (((nletters + 3) >> 2) | 1);       // dwords per column
    const int tid = (int)threadIdx.x;
    // where the bytes tid, tid + 256, ... of a tile lie: (column of the tile, place in the column), stepped without a division
    const int col0 = tid / nletters, k0 = tid - col0 * nletters, dcol = 256 / nletters, dk = 256 - dcol * nletters;
    for (int64_t job = blockIdx.x; job < nq * parts; job += gridDim.x) {
        const MultiQuery d = tab[job / parts];
        const int part = (int)(job % parts), ntiles = (d.qlen + 255) >> 8;
        signed char* out = prof + d.prof_off;
        for (int tile = part; tile < (d.qpad >> 8); tile += parts) {
            const int c0 = tile << 8, c = c0 + tid;
            if (tile < ntiles) {
                const int cols = min(256, d.qlen - c0), nbytes = cols * nletters;
                const signed char* src = pssm + (d.qstart + c0) * (int64_t)nletters;
                __syncthreads();                                     // the last tile's rows have been read
                for (int i = tid, col = col0, k = k0; i < nbytes; i += 256) {
                    const int dw = col * stride + (swz ? (k >> 2) ^ (col & 31) : (k >> 2));
                    lds[(dw << 2) + (k & 3)] = (signed char)min((int)src[i], smax);
                    col += dcol; k += dk;
                    if (k >= nletters) { k -= nletters; ++col; }
                }
                __syncthreads();
            }
            const bool live = c < d.qlen;
            for (int x = 0; x < SW_SEARCH_ROWS; ++x) {
                int v = -1;
                if (x < 256 && live) {
                    const int k = __builtin_amdgcn_readfirstlane((int)code[x]);   // (a vector load at a uniform address: tell the compiler it is a scalar)
                    v = other;
                    if (k < nletters) {
                        const int dw = tid * stride + (swz ? (k >> 2) ^ (tid & 31) : (k >> 2));
                        v = lds[(dw << 2) + (k & 3)];
                    }
                }
                out[(int64_t)x * d.qpad + c] = (signed char)v;
            }
        }
    }
}

}  // namespace swk
