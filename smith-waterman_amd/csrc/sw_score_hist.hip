// sw_score_hist.hip -- the statistics of a many-query search on the device (include/swhip.h states the rules): the score histogram of a
// query-major result table (sw_score_hist_device and, chunk by chunk, sw_db_search_affine_top_stats / sw_db_search_pssm_top_stats) and
// the thresholds of a hit table (sw_hits_threshold_device).
//
//   sw_score_hist      one workgroup per work item of swp::plan_score_hist: a query and a slice of the targets.  The workgroup zeroes
//                      `copies` histograms of 40 x 256 counters in LDS, its threads walk the slice -- max_score of the row, 8 of every 24
//                      bytes, and the target's two offsets --, and add 1 to cell (class(len), bin(score)) of the copy of their wave
//                      with an LDS integer add.  The flush adds the non-zero cells, summed over the copies, to the query's global
//                      histogram with one vector atomic add per cell.  Integer sums: the bytes do not depend on the order of the adds.
//                      The unrelated scores of a query fall into a few dozen cells, so the lanes of one LDS instruction collide: they
//                      are serialised inside that instruction, at worst one add per lane and clock, which a CU still outruns the HBM
//                      with.  An empty target is counted nowhere.
//   sw_hits_threshold  one workgroup per query: thread t takes the entries t, t + 256, ...; keep is the used-entry test (count, target
//                      compared unsigned before any load through it, non-empty) and max_score >= thresholds[q][class(len)].
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"

namespace swk {

constexpr int kCells = swp::kScoreHistClasses * swp::kScoreHistBins;
static_assert(kCells % 256 == 0);

__global__ void __launch_bounds__(256) sw_score_hist(ScoreHistParams p) {
    extern __shared__ unsigned int sh_hist[];                        // copies x kCells
    const int tid = (int)threadIdx.x;
    const int ncell = p.copies * kCells;
    unsigned int* mine = sh_hist + ((tid >> 6) % p.copies) * kCells; // the copy of this thread's wave
    for (int64_t w = blockIdx.x; w < p.items; w += gridDim.x) {
        const int64_t q = w / p.slices_per_query, s = w % p.slices_per_query;
        const int64_t lo = s * p.slice, hi = min(p.ntargets, lo + p.slice);
        __syncthreads();                                             // (the item before has been flushed)
        for (int i = tid; i < ncell; i += 256) sh_hist[i] = 0;
        __syncthreads();
        const sw_result* row = p.results + q * p.ntargets;
        for (int64_t k = lo + tid; k < hi; k += 256) {
            const int64_t len = p.offsets[k + 1] - p.offsets[k];
            if (len < 1) continue;
            const int c = min(score_class(len), swp::kScoreHistClasses - 1);   // (a handle's targets are below 2^20 letters: class <= 39)
            atomicAdd(&mine[c * swp::kScoreHistBins + score_bin(row[k].max_score, p.shift)], 1u);
        }
        __syncthreads();
        unsigned int* g = p.hist + q * kCells;
        for (int i = tid; i < kCells; i += 256) {
            unsigned int n = sh_hist[i];
            for (int c = 1; c < p.copies; ++c) n += sh_hist[c * kCells + i];
            if (n) atomicAdd(&g[i], n);
        }
    }
}

__global__ void __launch_bounds__(256) sw_hits_threshold(HitsThresholdParams p) {
    __shared__ int part[4];
    const int tid = (int)threadIdx.x;
    for (int64_t q = blockIdx.x; q < p.nq; q += gridDim.x) {
        int64_t n = p.top;
        if (p.nhits) { n = p.nhits[q]; n = n < 0 ? 0 : n > p.top ? p.top : n; }
        const int64_t* thr = p.thresholds + q * swp::kScoreHistClasses;
        int kept = 0;
        for (int64_t r = tid; r < p.top; r += 256) {
            const int64_t e = q * p.top + r;
            const sw_hit h = p.hits[e];
            int k = 0;
            if (r < n && (uint64_t)h.target < (uint64_t)p.ntargets) {
                const int64_t len = p.offsets[h.target + 1] - p.offsets[h.target];
                if (len >= 1) k = h.max_score >= thr[min(score_class(len), swp::kScoreHistClasses - 1)];
            }
            if (p.keep) p.keep[e] = k;
            if (p.hits_out) p.hits_out[e] = sw_hit{k ? h.target : -1, h.max_pos, h.max_score};
            kept += k;
        }
        if (p.nkept) {   // (uniform)
            for (int d = 32; d; d >>= 1) kept += __shfl_down(kept, d);
            __syncthreads();                                         // (the query before has been read)
            if ((tid & 63) == 0) part[tid >> 6] = kept;
            __syncthreads();
            if (tid == 0) p.nkept[q] = (int64_t)part[0] + part[1] + part[2] + part[3];
        }
    }
}

}  // namespace swk
