// sw_kernels.h -- shared declarations between the HIP kernels and the C-ABI host code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/swhip.h"
#include "sw_plan.h"   // (SW_SEARCH_ROWS, SearchItem, MultiQuery)

namespace swk {

// packed arg-max key: (score << 40) | (2^40-1 - linear_index); atomicMax picks the highest
// score and, among equals, the LOWEST linear index (the serial scan's rule, serial_smithW.c:240-242)
constexpr unsigned long long SW_KEY_IDX_MASK = (1ull << 40) - 1;
constexpr int64_t SW_MAX_DIM = (1 << 20) - 1; // rows/cols limit: 20-bit row tags, 40-bit indices

struct FillParams {
    int64_t cols, rows, M;     // M = row stride of H/P in elements (cols + 1 for a whole matrix)
    void* H;                   // HT[(rows+1)*M]
    int32_t* P;                // int32[(rows+1)*M]
    const int32_t* top;        // optional halo row (cols+1), NULL = zeros
    const int32_t* left;       // systolic: optional halo column (rows+1 H values of the column left of the tile), NULL = zeros
    int32_t* right;            // systolic: optional output, H of the tile's last column (rows+1)
    int npairs;                // systolic: independent problems in this launch (batch), 1 otherwise
    int store_hp;              // (unused; H / P are written when their pointers are non-NULL)
    int64_t a_pstride, b_pstride, bpad_pstride, hp_pstride, edge_pstride;  // per-pair strides (elements)
    int32_t mm, xm, ngap;      // match-2*gap, mismatch-2*gap, -gap  (G-space constants)
    unsigned long long* edge;  // [nstrips][rows+1] {tag,value} granules
    unsigned int tag_base;     // epoch << 20
    unsigned long long* result_key;
    unsigned int* abort_flag;
    int phi_base;              // systolic: >= 0 -> fast producers, phi = phi_base - s; < 0 -> generic
    int bfront;                // systolic: index of b[0] inside bpad / bpad16
    const unsigned short* bpad16;
    const unsigned char* bpad8;          // sw_systolic2: zero-padded byte copy of b, same layout as bpad16 (b[0] at index bfront)
    unsigned long long* dbg;   // optional: per strip {start, end} s_memrealtime stamps of its producer (experiments)
    int p_bytes;               // bytes per P element: 4 (reference layout) or 1 (compact, systolic engine only)
    int store_nt;              // systolic: streaming (nt) H/P stores
    int xcd_order;             // systolic: neighbouring strip groups on one XCD
    int pace_ps;               // systolic: strip 0 releases one row per pace_ps picoseconds (0 = unpaced)
    int debug_flags;           // development aids: swk::DebugFlag (sw_debug.h)
    int nstrips;               // strip_scan: ceil(cols/64); systolic: ceil(cols/63)
    // band-resident launch (systolic; multi-GPU row bands): the halo row arrives / leaves as 8-byte
    // {tag, H value} granules, one per column, while the kernel runs
    const unsigned long long* top_gran;  // cols+1 granules of the row above (polled per strip), or NULL
    unsigned long long* bot_gran;        // cols+1 granules of the band's last row (written per strip), or NULL
    unsigned int* bot_done;              // optional [nstrips]: set to bot_tag (system scope, after a release) once the strip's bottom granules are written
    unsigned int top_tag, bot_tag;
    unsigned int top_wait_ticks;         // patience of the top-halo poll in 100 MHz ticks / 2^10
    // "perm" producer (systolic; alphabets of at most 7 letters, scores that fit a signed byte): the substitution
    // scores of 16 steps come from 4 v_perm_b32 over a per-lane profile, every G value carries `gbias` (8-bit launch
    // tag << 24 | 2^16), and lane 63 stores its own results as self-validating 4-byte values
    const unsigned char* bcode;          // padded copy of b as letter codes 0..6 (7 = outside the sequence), layout as bpad
    const unsigned char* atab;           // [256] letter code of every byte value; [256..259] = number of letters (uint32)
    unsigned int* edge4;                 // [nstrips][e4stride] lane-63 values indexed by the producer's local step - 1
    int64_t e4stride, edge4_pstride;
    unsigned int gbias;                  // 0 = perm path not eligible on the host side (score range)
    int skip_if_perm;                    // sw_systolic: leave when the perm path applies (sw_systolic2 was launched for that case)
    int h_bytes;                         // sw_systolic2: bytes per H element (4 or 8); sw_systolic carries it as a template parameter
    int scout_double;                    // sw_systolic2: the first scout_double scout workgroups carry two strips, the others one
    int nscout;                          // sw_systolic2: workgroups 0..nscout-1 only run the chain (two strips each) and leave the edge columns to the others
    int filler_hop_ps, filler_tau_ps, filler_bw_gbs;    // sw_systolic2 behind scouts: pacing of the fillers (sw_systolic2.inc), 0 = none
    int xcd_mode;                        // sw_systolic2: 256 workgroups, roles dealt per XCD (workgroup i on XCD i % 8; nscout = scout workgroups in all)
    // one launch per fill (round 4): the preparation and the finalisation of a fill are the prologue / epilogue of sw_systolic2 itself
    unsigned int* sync;                  // per context, all zero between launches: [0] arrivals at the prologue's grid barrier, [1] workgroups that have
                                         // left, [2] the letter count the prologue found (kept for the fall-back kernel), [8..15] presence map of the byte values
    unsigned char* priv;                 // per workgroup: a zero-padded copy of b and its letter codes ([bpad8 | bcode], bpad_pstride bytes each)
    int64_t priv_stride;                 // bytes between two workgroups' copies
    unsigned short* bpad16_w;            // writable views of the shared padded copies (the prologue of workgroup 0 fills them when the fall-back kernel has to run)
    unsigned char* bpad8_w; unsigned char* bcode_w; unsigned char* atab_w;
    sw_result* result;                   // != NULL: the last workgroup to leave writes the result and re-arms key / abort flag / sync for the next launch
    int skip_row0;                       // prologue: row 0 of H / P is not this launch's to clear (a band's halo row)
    // column tiles of one matrix, one launch each (round 4: matrices too wide for scout workgroups beside one filler per strip)
    const int32_t* tile_left;            // H of the column left of this tile's first column, row r at tile_left[r * M] (the previous tile wrote it); NULL: zeros
    int64_t idx_off;                     // added to the linear index of the arg-max (the tile's first column: indices of the whole matrix)
    int final_launch;                    // the epilogue reports and re-arms the key (earlier tiles only accumulate into it)
    const unsigned char* alpha_a;        // what the prologue scans for letters: the WHOLE a (every tile must decide alike who fills)
    int64_t alpha_cols;
    // split strips (round 4, xcd_mode 1): from strip split_from on, the filler of a strip writes only the 16-row blocks below split_blk and
    // the strip's SCOUT -- a workgroup with rings and consumers like a filler -- writes the rest (sw_systolic2.inc); 0 = off
    int split_blk, split_from;
    int split_extra;                     // 1: the last strip has a scout workgroup too (it writes that strip's lower blocks; nobody reads its edge)
    int filler_end_steps;                // pacing: the steps of the filler that ends last (a split one), 0 = every filler runs all steps
    int filler_full_steps;               // pacing: steps of a whole strip (what the bandwidth bound is computed with)
    // strip geometry of sw_systolic2: strip s spans the columns s2w * s + 1 .. s2w * s + 126 (63 lanes x 2); s2w = 126: the strips tile the
    // matrix; s2w = 110: neighbouring strips OVERLAP by 16 columns, so that every 64-byte line of a matrix row lies wholly inside some
    // strip and can be stored by ONE instruction of that strip (whole-line stores: sw_systolic2.inc).  0 is taken as 126.
    int s2w;
    int scan_all;                        // sw_systolic2 prologue: 1 = every workgroup scans all letters itself, no grid barrier (the planner decides)
};
constexpr int SW_XTAB_OFF = 448;         // atab + 448: unsigned int[256], XCD + 1 of every workgroup of the running sw_systolic2 launch (0: not there yet)
constexpr int SW_PERM_PAD = -100;        // score of any cell outside the sequences (perm producer)

// sw_batch.hip: one pair per wave (BASELINE config 5)
struct BatchParams {
    const unsigned char* a; int64_t a_pstride, cols;
    const unsigned char* bcode; int64_t bcode_pstride; int bfront;   // padded letter codes of b (sw_batch_codes)
    int64_t rows, npairs;
    const unsigned char* atab;       // letter code of every byte value; [256..259] = number of letters
    int32_t* H; void* P;             // either may be NULL; pair k at element offset k * hp_pstride
    int64_t hp_pstride;
    int match, mismatch, ngap;       // plain scores (H-space), ngap = -gap
    int* bnd; int64_t bnd_pstride;   // boundary column between strips (only when cols > 64 * C), ints per pair
    sw_result* results;
    int debug;                       // bit 0: drop the H / P stores (timing experiments only)
};
__global__ void sw_batch_codes(const unsigned char* b, int64_t rows, int64_t b_pstride, unsigned char* bcode, int64_t per, int front,
                               const unsigned int* part, int npart, unsigned char* atab, int64_t npairs);
template <int C, int PB>
__global__ void sw_batch_wave(BatchParams p);
template <bool LE4, bool K12, bool PB1>
__global__ void sw_batch_wave16(BatchParams p);   // two pairs per wave on packed 16-bit lanes (score + exact maxPos; PB1: int8 P too)

// sw_search.hip: one query against many targets of any length (database search)
struct SearchParams {
    const unsigned char* db;             // the targets back to back
    const SearchItem* items; int64_t nitems;
    const signed char* prof; int64_t qpad;   // SW_SEARCH_ROWS x qpad profile (sw_search_profile), qpad = strips * 64 * C
    int64_t qlen;
    int match, mismatch, ngap;           // plain scores, ngap = -gap
    int* bnd; int64_t bnd_per;           // per resident wave: boundary column between strips (ints), only when qlen > 64 * C
    unsigned int* counter;               // next item (zero at launch)
    sw_result* results;                  // caller's order
};
__global__ void sw_search_profile(const unsigned char* q, int64_t qlen, int64_t qpad, signed char* prof, int match, int mismatch, int wide);
template <int C, bool WIDE>
__global__ void sw_search_wave(SearchParams p);

// sw_search_affine.hip: the same search with a substitution matrix and affine gaps
struct SearchAffineParams {
    const unsigned char* db;             // the targets back to back
    const SearchItem* items; int64_t nitems;
    const signed char* prof; int64_t qpad;   // SW_SEARCH_ROWS x qpad profile (sw_search_profile_submat), qpad = strips * 64 * C
    int64_t qlen;
    int ge, goe;                         // gap_extend, gap_open + gap_extend (both <= 0)
    int* bnd; int64_t bnd_per;           // per resident wave: boundary pairs (H, F) between strips (ints), only when qlen > 64 * C
    unsigned int* counter;               // next item (zero at launch)
    sw_result* results;                  // caller's order
};
__global__ void sw_search_profile_submat(const unsigned char* q, int64_t qlen, int64_t qpad, signed char* prof, const signed char* sub);
template <int C>
__global__ void sw_search_affine_wave(SearchAffineParams p);

// sw_search_multi.hip: many queries against a prepared database, one launch per class of queries (columns per lane)
struct SearchMultiParams {
    const unsigned char* db;             // the targets back to back
    const SearchItem* items;             // the handle's schedule: every non-empty target, longest first
    int64_t rank0;                       // the first target rank of this launch
    const MultiQuery* queries;           // the launch's queries (entries of the call's table)
    unsigned int nq;                     // ... how many: item w = (rank0 + w / nq, w % nq)
    int64_t nitems;                      // nq * target ranks of the launch, below 2^31
    const signed char* prof;             // the group's profiles (sw_search_profile_submat_multi), query t at its prof_off
    int64_t ntargets;                    // row stride of the results
    int ge, goe;                         // gap_extend, gap_open + gap_extend (both <= 0)
    int* bnd; int64_t bnd_per;           // per resident wave: boundary pairs (H, F) between strips (ints), only when a query has more than one strip
    unsigned int* counter;               // next item (zero at launch)
    sw_result* results;                  // query-major, nqueries x ntargets, the caller's order
};
__global__ void sw_search_profile_submat_multi(const unsigned char* q, const MultiQuery* tab, int64_t nq, int parts, signed char* prof, const signed char* sub);
template <int C>
__global__ void sw_search_affine_multi_wave(SearchMultiParams p);

// sw_search_multi16.hip: the same search with two targets per wave on packed 16-bit lanes ("search_lanes" = 16); the launches and the
// queries that may run here are swp::plan_search_multi_lanes's
struct SearchMultiPackedParams {
    const unsigned char* db;             // the targets back to back
    const SearchItem* items;             // the handle's schedule: every non-empty target, longest first
    int64_t rank0, nranks;               // the target ranks of this launch: rank0 is even, an odd nranks leaves the last rank without a partner
    const MultiQuery* queries;           // the launch's queries (entries of the call's table)
    unsigned int nq;                     // ... how many: item w = (ranks rank0 + 2 (w / nq) and the next, w % nq)
    int64_t nitems;                      // nq * ceil(nranks / 2), below 2^31
    const signed char* prof;             // the group's profiles, query t at its prof_off
    int64_t ntargets;                    // row stride of the results
    int ge, goe;                         // gap_extend, gap_open + gap_extend (both <= 0, gap_open + 2 gap_extend >= -32768)
    int* bnd; int64_t bnd_per;           // per resident wave: boundary pairs (H, F) of both targets between strips (ints), as SearchMultiParams
    unsigned int* counter;               // next item (zero at launch)
    sw_result* results;                  // query-major, nqueries x ntargets, the caller's order
};
template <int C>
__global__ void sw_search_multi_pk_wave(SearchMultiPackedParams p);

// sw_pssm.hip: the same profiles from a position-specific scoring matrix (sw_db_search_pssm and its twins)
__global__ void sw_search_profile_pssm_multi(const signed char* pssm, const MultiQuery* tab, int64_t nq, int parts, signed char* prof, const unsigned char* code,
                                             int nletters, int other, int smax);
// ... its dynamic LDS: 256 columns of an odd number of dwords each (sw_pssm.hip says why), at most 64 KiB
constexpr unsigned sw_pssm_profile_lds_bytes(int nletters) { return 1024u * (nletters > 252 ? 64u : (unsigned)(((nletters + 3) >> 2) | 1)); }

// What every kernel that reads a hit table's alignments takes (sw_pssm_walk.h holds the used-entry rule and the walks over it).
struct HitTables {
    const int64_t* qoffs; int64_t nqueries;      // device copy of the caller's nqueries + 1 offsets
    const unsigned char* db; const int64_t* offsets; int64_t ntargets;   // the handle's bytes and its ntargets + 1 offsets on the device
    const sw_hit* hits; const int64_t* nhits; int64_t top;               // the caller's tables, as the alignment calls take and leave them
    const sw_alignment* aln; const char* ops; int64_t ops_cap;
    int64_t include_min;                         // entries that score less are not used
};

// sw_pssm_hits.hip: the next iteration's PSSM from a hit table, its alignments and their ops (sw_db_pssm_from_hits).  One workgroup per
// (query, tile of columns) as swp::plan_pssm_hits cuts them; dynamic LDS: the plan's lds_bytes.
struct PssmHitsParams {
    HitTables t;
    const signed char* prior; signed char* out;  // the layout of d_pssm; out may be NULL, or prior itself
    int* counts;                                 // (qoffsets[nqueries] - qoffsets[0]) x nletters, or NULL
    const signed char* S;                        // nletters x nletters: S[b * nletters + k] = sub[letters[b]][letters[k]]
    const unsigned char* code;                   // 256 bytes: target byte -> its place in a column, 255 where it has none (swh::check_search_pssm)
    const int* weights;                          // nqueries x top, or NULL: every weight 1
    int64_t tiles_per_query, col0;               // col0 = qoffsets[0]: counts start at the first query's first column
    int nletters, stride, tile_cols, smax, prior_weight;
};
__global__ void sw_pssm_from_hits(PssmHitsParams p);

// sw_pssm_weights.hip: the position-based weights of a hit table's entries (sw_db_pssm_hit_weights).  sw_pssm_weights_tile: one workgroup
// per (query, tile of columns) with the tiles and the dynamic LDS of swp::plan_pssm_weights (those of plan_pssm_hits);
// sw_pssm_weights_finish: one workgroup of 256 threads per query, static LDS.
struct PssmWeightsParams {
    HitTables t;
    const unsigned char* code;                   // 256 bytes: target byte -> its place in a column, 255 where it has none
    unsigned long long* acc;                     // nqueries x top, zero before the tile launch: T_r + (m_r << 40)
    int* weights;                                // nqueries x top: every entry is written
    int64_t tiles_per_query;
    int nletters, stride, tile_cols, per_hit;
};
__global__ void sw_pssm_weights_tile(PssmWeightsParams p);
__global__ void sw_pssm_weights_finish(PssmWeightsParams p);

// sw_msa_hits.hip: the query-anchored alignment of a hit table's entries (sw_db_msa_from_hits), as swp::plan_msa_hits cuts it.
// sw_msa_cols: one workgroup per (query, slice of entries), the column rows and every field of a sw_msa_row but `off`;
// sw_msa_scan_chunks / sw_msa_scan_top: the exclusive scan of `len` in chunks of swp::kMsaScanChunk entries and over the chunks' sums;
// sw_msa_rows: one wave per entry, its final `off` and its A3M row.
struct MsaHitsParams {
    HitTables t;
    const unsigned char* queries;                // the query letters at qoffs[q] + j, or NULL (PSSM queries): nident = 0
    unsigned char* cols;                        // (qoffsets[nqueries] - qoffsets[0]) x top bytes, or NULL
    sw_msa_row* rows;                            // nqueries x top, or NULL
    unsigned char* a3m; int64_t a3m_cap;         // a3m_cap bytes, or NULL
    int64_t* a3m_bytes;                          // the true total (with rows)
    int64_t* chunk_off;                          // workspace: per scan chunk its sum, then its exclusive offset
    int64_t entries, chunks;                     // entries = nqueries x top; chunks of swp::kMsaScanChunk entries
    int64_t slices_per_query, slice_entries, col0;   // col0 = qoffsets[0]: cols start at the first query's first column
};
__global__ void sw_msa_cols(MsaHitsParams p);
__global__ void sw_msa_scan_chunks(MsaHitsParams p);
__global__ void sw_msa_scan_top(MsaHitsParams p);
__global__ void sw_msa_rows(MsaHitsParams p);

// sw_msa_filter.hip: the filter of the column rows (sw_msa_filter_device), as swp::plan_msa_filter cuts it, for the queries
// q0 .. q0 + nq - 1 of one chunk.  sw_msa_filter_pairs: one workgroup per (query, tile), the bit planes of the workspace;
// sw_msa_filter_greedy: one workgroup per query, keep in rank order and the outputs.
struct MsaFilterParams {
    const unsigned char* cols;                   // the column rows of sw_db_msa_from_hits
    const unsigned char* queries;                // the query letters at qoffs[q] + j, or NULL: no row is compared with the query
    const int64_t* qoffs; int64_t col0;          // device copy of the offsets; col0 = qoffsets[0]: cols start at the first query's first column
    int64_t q0, nq;                              // the chunk's queries
    int64_t top, blocks, tiles_per_query, query_words;
    unsigned long long* ws;                      // nq x query_words: query q's planes at (q - q0) x query_words
    int max_ident_pct, min_cover_pct;
    const sw_hit* hits; sw_hit* hits_out;        // nqueries x top, or NULL together / hits_out alone NULL
    int* keep;                                   // nqueries x top, or NULL
    int64_t* nkept;                              // nqueries, or NULL
};
__global__ void sw_msa_filter_pairs(MsaFilterParams p);
__global__ void sw_msa_filter_greedy(MsaFilterParams p);

// sw_score_hist.hip: the score histogram of a query-major result table (sw_score_hist_device and the _top_stats searches), as
// swp::plan_score_hist cuts it, and the thresholds of a hit table (sw_hits_threshold_device), one workgroup per query.
// score_class / score_bin are the rule of include/swhip.h, shared by both kernels.
__host__ __device__ inline int score_class(int64_t len) {   // len >= 1
    if (len < 2) return 0;
    const int e = 63 - __builtin_clzll((unsigned long long)len);
    return 2 * e + (int)((len >> (e - 1)) & 1);
}
__host__ __device__ inline int score_bin(int64_t v, int shift) {
    const int64_t b = (v > 0 ? v : 0) >> shift;
    return b < 255 ? (int)b : 255;
}
struct ScoreHistParams {
    const sw_result* results;                    // nq x ntargets, query-major
    const int64_t* offsets;                      // the handle's ntargets + 1 offsets
    int64_t ntargets, nq;
    int64_t slices_per_query, slice, items;
    int shift, copies;
    unsigned int* hist;                          // nq x 40 x 256, zeroed on the stream before the launch
};
__global__ void sw_score_hist(ScoreHistParams p);
struct HitsThresholdParams {
    const int64_t* offsets; int64_t ntargets;    // the handle's offsets
    const int64_t* thresholds;                   // nq x 40
    int64_t nq, top;
    const sw_hit* hits; const int64_t* nhits;    // nq x top; nq or NULL
    sw_hit* hits_out; int* keep; int64_t* nkept; // each may be NULL
};
__global__ void sw_hits_threshold(HitsThresholdParams p);

// sw_mask.hip: the low-complexity mask of a handle's bytes (sw_db_mask_low_complexity), flat over the positions 0 .. letters - 1 of the
// concatenated targets (position p is byte offs[0] + p) in the tiles of swp::plan_mask.  sw_mask_windows: low1 / low2 bits and a
// summary per tile; sw_mask_carries: one workgroup, the carry word of every tile; sw_mask_apply: the mask bits and the bytes;
// sw_mask_count: the masked positions per target.
struct MaskParams {
    const unsigned char* in; unsigned char* out; // the handle's bytes and the masked copy, both indexed like d_db
    const int64_t* offs; int64_t ntargets;       // the handle's ntargets + 1 offsets on the device
    int64_t base, letters, tiles;                // offs[0]; offs[ntargets] - offs[0]; tiles of swp::kMaskTile positions
    unsigned long long *low1, *low2, *mask;      // tiles x 64 words each: bit p % 64 of word p / 64 is position p
    unsigned int *summary, *carry;               // per tile
    int window, bound1, bound2, gw;              // W; D <= bound1 is low1, D <= bound2 is low2; gw = G[W]
    int nletters; unsigned char letters_[32];    // the alphabet: class k is letters_[k]
    unsigned int mask_byte;
    int64_t* nmasked;                            // ntargets, or NULL
};
__global__ void sw_mask_windows(MaskParams p);
__global__ void sw_mask_carries(MaskParams p);
__global__ void sw_mask_apply(MaskParams p);
__global__ void sw_mask_count(MaskParams p);

// sw_search_pairs.hip: the scores of a device list of (query, target) pairs (sw_db_search_affine_pairs).  Per (chunk of the list, group
// of queries) two binning launches turn the usable pairs into work items, one list per class, heaviest bucket first
// (swp::plan_search_pairs); one launch of sw_search_affine_pairs_wave<C> per class scores them.
struct SearchPairItem { int64_t start, out; int32_t len, entry; };   // first byte in db, index in d_results (= in d_pairs), length, entry of the call's query table
constexpr int SW_SP_CLASSES = swp::kSearchPairsKernels, SW_SP_BUCKETS = swp::kSearchPairsBuckets;
struct SearchPairsList { unsigned int n, first; };   // a class's list: its items and where it starts in the item buffer (the scatter launch writes it)
// the control words of a (chunk, group), zero before its binning: per (class, bucket) the items counted and the scatter's cursor, per
// class its list and the work counter of its launch
struct SearchPairsCtl {
    unsigned int count[SW_SP_CLASSES][SW_SP_BUCKETS], cursor[SW_SP_CLASSES][SW_SP_BUCKETS];
    SearchPairsList list[SW_SP_CLASSES];
    unsigned int work[SW_SP_CLASSES];
};
struct SearchPairsBinParams {
    const sw_pair* pairs;                        // the caller's list
    int64_t p0, np;                              // the chunk: pairs p0 .. p0 + np - 1
    const int64_t* offsets; int64_t ntargets;    // the handle's ntargets + 1 offsets on the device
    const MultiQuery* queries;                   // the call's table (what an item's `entry` counts from)
    const int32_t* entry_of; int64_t nqueries;   // query index -> its entry of the table
    int64_t cls_q0[SW_SP_CLASSES + 1];           // the group: class k = entries cls_q0[k] .. cls_q0[k + 1] - 1 of the table
    SearchPairsCtl* ctl;
    SearchPairItem* items;                       // np at most
};
template <bool SCATTER>
__global__ void sw_search_pairs_bin(SearchPairsBinParams p);
struct SearchPairsParams {
    const unsigned char* db;             // the targets back to back
    const SearchPairItem* items;         // the (chunk, group)'s item buffer: the classes' lists back to back
    const SearchPairsList* list;         // this class's list (SearchPairsCtl::list[k])
    const MultiQuery* queries;           // the call's table
    const signed char* prof;             // the group's profiles, query t at its prof_off
    int ge, goe;                         // gap_extend, gap_open + gap_extend (both <= 0)
    int* bnd; int64_t bnd_per;           // per resident wave: boundary pairs (H, F) between strips (ints), only when a query of the class has more than one strip
    unsigned int* counter;               // next item (zero at launch)
    sw_result* results;                  // npairs, the order of the caller's list
};
template <int C>
__global__ void sw_search_affine_pairs_wave(SearchPairsParams p);

// sw_search_pairs16.hip: the same call with two pairs of one query per wave on packed 16-bit lanes ("search_pairs_lanes" = 16), for the
// groups that hold packed queries (swp::plan_search_pairs_lanes).  Per (chunk, group) three binning launches -- count, scan, scatter --
// pair the listed pairs of a packed query inside a bucket into two-pair items and keep the lists of the other queries as
// sw_search_pairs_bin makes them; sw_search_pairs_pk_wave<C> scores the two-pair items of a class.
struct SearchPairItem2 { SearchPairItem half[2]; };   // half 0 is never empty; an empty half 1 has len = 0 (the scan launch writes it)
// the control words of a (chunk, group) at the head of the cell workspace, zero before its binning; behind them
// (swp::kSearchPairsCellsHead bytes from the start) the cells' counts, cursors -- zero too -- and bases, `cells` words each
struct SearchPairsPackedCtl {
    SearchPairsList list[SW_SP_CLASSES];         // a class's two-pair items: how many, and the first one's index in the item buffer
    unsigned int work[SW_SP_CLASSES];            // the work counters of the packed launches
    unsigned int base32[SW_SP_CLASSES][SW_SP_BUCKETS];   // where the 32-bit items of a (class, bucket) start, in SearchPairItem units
};
static_assert(sizeof(SearchPairsPackedCtl) <= swp::kSearchPairsCellsHead);
struct SearchPairsPackedBinParams {
    SearchPairsBinParams bin;                    // what sw_search_pairs_bin takes; bin.items: the item buffer of the (chunk, group)
    int64_t pk_q1[SW_SP_CLASSES];                // class k: the entries bin.cls_q0[k] .. pk_q1[k] - 1 run packed
    int64_t cells;                               // SW_SP_BUCKETS x packed entries of the group
    SearchPairsPackedCtl* pk;                    // the head of the cell workspace
    unsigned long long* total;                   // two-pair items of the call so far ("last_search_pairs_packed_items")
};
template <bool SCATTER>
__global__ void sw_search_pairs_pk_bin(SearchPairsPackedBinParams p);
__global__ void sw_search_pairs_pk_scan(SearchPairsPackedBinParams p);
struct SearchPairsPackedParams {
    const unsigned char* db;             // the targets back to back
    const SearchPairItem2* items;        // the (chunk, group)'s item buffer: the classes' two-pair lists back to back at its start
    const SearchPairsList* list;         // this class's list (SearchPairsPackedCtl::list[k])
    const MultiQuery* queries;           // the call's table
    const signed char* prof;             // the group's profiles, query t at its prof_off
    int ge, goe;                         // gap_extend, gap_open + gap_extend (both <= 0, gap_open + 2 gap_extend >= -32768)
    int* bnd; int64_t bnd_per;           // per resident wave: boundary pairs (H, F) of both halves between strips (ints), as SearchPairsParams
    unsigned int* counter;               // next item (zero at launch)
    sw_result* results;                  // npairs, the order of the caller's list
};
template <int C>
__global__ void sw_search_pairs_pk_wave(SearchPairsPackedParams p);

// sw_prefilter.hip: the ungapped pre-filter (sw_db_prefilter_ungapped): the best gapless local score U of every (query, target) pair and
// the list of the pairs with U >= min_score.  The items and the launches are swp::plan_prefilter's.
struct PrefilterCtl {                    // the control words of a call
    unsigned int work;                   // next item of the launch in flight (zero at launch)
    unsigned int cursor;                 // passing pairs of the launch in flight (zero at launch)
    long long total;                     // passing pairs of the launches before it
};
struct PrefilterParams {
    const unsigned char* db;             // the targets back to back
    const SearchItem* items;             // the handle's schedule: every non-empty target, longest first
    int64_t rank0, nranks;               // the target ranks of this launch
    const MultiQuery* queries;           // the launch's queries (entries of the call's table)
    unsigned int nq;                     // ... how many: item w = (w / nq, w % nq); w / nq counts ranks, or rank PAIRS in the packed kernel
    int64_t nitems;                      // below 2^31
    const signed char* prof;             // the group's profiles (sw_search_profile_submat_multi), query t at its prof_off
    int64_t ntargets;                    // row stride of the scores
    int* bnd; int64_t bnd_per;           // per resident wave: two boundary columns of one int per row, only when a query has more than one strip
    PrefilterCtl* ctl;
    int min_score;
    sw_pair* pairs; int64_t pairs_cap;   // the list: slot total + cursor, stored where it lies below pairs_cap
    int32_t* scores;                     // optional: query-major, nqueries x ntargets
};
__global__ void sw_prefilter_commit(PrefilterCtl* ctl, int64_t* npairs, int first);
template <int C>
__global__ void sw_prefilter_wave(PrefilterParams p);
template <int C>
__global__ void sw_prefilter_wave16(PrefilterParams p);   // two targets of a query per wave on packed 16-bit lanes

// sw_search_top.hip: the best `top` targets of every row of a query-major result table (swp::plan_search_top has the geometry)
struct TopState {                        // of one row, between the launches of a radix select
    unsigned long long prefix;           // the digits found so far, highest first; after the last pass: the key of rank `top`
    unsigned int want;                   // rank still looked for among the keys that carry the prefix
    unsigned int all;                    // 1: fewer than `top` targets qualify, every one of them is a hit
    unsigned int count;                  // compaction: keys written so far
    unsigned int n;                      // hits of the row: min(top, qualifying targets), known after the first pass
};
struct TopParams {
    const sw_result* results;            // query-major, nq rows of ntargets
    int64_t ntargets;
    unsigned int nq;
    unsigned int wgs_row; int64_t slice; // workgroup w of a row reads the targets [w * slice, min(ntargets, (w + 1) * slice))
    int tbits;                           // key = score << tbits | (2^tbits - 1 - target)
    int shift, bits, first;              // this pass's digit; first: the pass with the highest bits (no prefix yet)
    int64_t top, min_score;
    unsigned int* hist;                  // per row 2^swp::kTopDigitBits bins, zero between the passes
    TopState* state;                     // per row
    sw_hit* hits; int64_t* nhits;        // nq x top, nq
    int selected;                        // sw_top_sort: 1 = the row's keys lie compacted at the start of its hits (state has their number)
};
__global__ void sw_top_hist(TopParams p);
__global__ void sw_top_scan(TopParams p);
__global__ void sw_top_compact(TopParams p);
__global__ void sw_top_sort(TopParams p);

// sw_top_pairs.hip: the best `top` entries of every query of a scored pair list (swp::plan_top_pairs has the geometry)
struct TopPairsParams {
    const sw_pair* pairs; const sw_result* results;   // the list and its results, entry for entry; only read
    int64_t npairs, nqueries, ntargets;
    int64_t slice;                       // count, scatter: workgroup w reads the entries [w * slice, min(npairs, (w + 1) * slice))
    int tbits;                           // key = score << tbits | (2^tbits - 1 - target)
    int64_t top, min_score;
    unsigned int T;                      // streaming sort: items kept between rounds, pow2ceil(top)
    unsigned int* cnt;                   // per query: qualifying entries (count), then the next free slot of its segment (scan, scatter)
    unsigned int* offs;                  // nqueries + 1: where the segment of a query starts
    unsigned long long* keys; unsigned int* pos;   // the segments: key and list position of every qualifying entry
    sw_hit* hits; int64_t* nhits;        // nqueries x top, nqueries
};
template <bool LDS>
__global__ void sw_top_pairs_count(TopPairsParams p);
__global__ void sw_top_pairs_scan(TopPairsParams p);
template <bool LDS>
__global__ void sw_top_pairs_scatter(TopPairsParams p);
template <int ITEMS, bool STREAM>
__global__ void sw_top_pairs_sort(TopPairsParams p);

// sw_align_affine.hip: the alignment of chosen hits under affine scoring (direction fill + walk, one wave per hit)
struct AlignAffineParams {
    const unsigned char* db;             // the targets back to back
    const SearchItem* items; int64_t nitems;   // the hits, longest first: first byte in db, index in the caller's `hits`, length
    const signed char* prof; int64_t qpad;   // SW_SEARCH_ROWS x qpad profile (sw_search_profile_submat), qpad = strips * 64 * C
    int64_t qlen;
    int ge, goe;                         // gap_extend, gap_open + gap_extend (both <= 0)
    int* bnd; int64_t bnd_per;           // per slot: boundary pairs (H, F) between strips (ints), only when qlen > 64 * C
    unsigned int* counter;               // next item (zero at launch)
    unsigned char* dir; int64_t slot_bytes, nslots;   // per slot: the direction matrix, row stride qpad (longest hit x qpad bytes, below 2^31)
    sw_alignment* aln;                   // caller's order
    char* ops; int64_t ops_cap;          // caller's order, ops_cap bytes per hit; NULL: coordinates only
    unsigned long long* stamps;          // optional timing aid: [0] += ticks in fills, [1] += ticks in walks (100 MHz clock)
};
template <int C>
__global__ void sw_align_affine_wave(AlignAffineParams p);

// sw_align_hits.hip: the alignments of the hits of many queries, straight from a device hit table (sw_db_align_affine_hits).  Two binning
// launches turn the used entries of a group's rows into work items, one list per (class, tier) (swp::plan_align_hits); one launch of
// sw_align_hits_wave<C> per list aligns them.
struct AlignHitItem { int64_t start, out; int32_t len, entry; };   // first byte in db, index in d_aln (q * top + r), length, entry of the group's query table
constexpr int SW_AH_CLASSES = swp::kAlignHitsKernels, SW_AH_TIERS = swp::kAlignHitsTiers;
// the control words of a group, zero before its binning: per list the items counted, the scatter's cursor and the work counter of its launch
struct AlignHitsCtl { unsigned int count[SW_AH_CLASSES][SW_AH_TIERS], cursor[SW_AH_CLASSES][SW_AH_TIERS], work[SW_AH_CLASSES][SW_AH_TIERS]; };
struct AlignHitsBinParams {
    const sw_hit* hits; const int64_t* nhits;    // the caller's table (nqueries x top) and counts (or NULL: every entry is used)
    int64_t top;
    const int64_t* offsets; int64_t ntargets;    // the handle's ntargets + 1 offsets on the device
    const MultiQuery* queries;                   // the group's entries of the call's table, by class
    int64_t nq;
    int64_t cls_q0[SW_AH_CLASSES + 1];           // class k: entries cls_q0[k] .. cls_q0[k + 1] - 1 of `queries`, items from cls_q0[k] * top on
    int ntiers[SW_AH_CLASSES]; int64_t bound[SW_AH_CLASSES][SW_AH_TIERS];   // ascending bounds of the class's tiers (bytes of a direction matrix)
    int log_band[SW_AH_CLASSES];                 // 0: an item takes len x qpad bytes; else swp::align_ckpt_slot_bytes at 2^log_band rows (sw_align_ckpt.hip)
    AlignHitsCtl* ctl;
    AlignHitItem* items;                         // nq * top at most
    sw_alignment* aln;                           // entries that yield the zero alignment are written here
    unsigned int* filled;                        // SCATTER: += the lists of this group that received items (zero before the call's first group)
};
template <bool SCATTER>
__global__ void sw_align_hits_bin(AlignHitsBinParams p);
struct AlignHitsParams {
    const unsigned char* db;             // the targets back to back
    const AlignHitItem* items;           // the class's part of the group's list: its tiers back to back, smallest first
    const unsigned int* counts;          // the class's counts per tier (AlignHitsCtl::count[k]): this list starts behind the lower tiers'
    int tier;
    const MultiQuery* queries;           // the group's entries of the call's table (what an item's `entry` counts from)
    const signed char* prof;             // the group's profiles, query t at its prof_off
    int ge, goe;                         // gap_extend, gap_open + gap_extend (both <= 0)
    int* bnd; int64_t bnd_per;           // per slot: boundary pairs (H, F) between strips (ints), only when a query of the class has more than one strip
    unsigned int* counter;               // next item (zero at launch)
    unsigned char* dir; int64_t slot_bytes, nslots;   // per slot: a direction matrix of the tier's size (below 2^31), row stride = the item's qpad
    sw_alignment* aln;                   // nqueries x top
    char* ops; int64_t ops_cap;          // nqueries x top rows of ops_cap bytes; NULL: coordinates only
};
template <int C>
__global__ void sw_align_hits_wave(AlignHitsParams p);

// sw_align_ckpt.hip: the same alignments in bounded memory ("align_checkpoint"): a slot holds one band of 2^log_band rows of direction
// bytes and, behind it, a checkpoint row per band boundary (swp::align_ckpt_slot_bytes; swp::plan_align_ckpt, plan_align_hits_ckpt)
struct AlignCkptParams {                 // the hits of one query, from the host-built list: AlignAffineParams and the band
    const unsigned char* db;
    const SearchItem* items; int64_t nitems;
    const signed char* prof; int64_t qpad;
    int64_t qlen;
    int ge, goe;
    int* bnd; int64_t bnd_per;           // per slot: boundary pairs (H, F) between the strips of ONE BAND (ints), only when qlen > 64 * C
    unsigned int* counter;
    unsigned char* dir; int64_t slot_bytes, nslots;   // per slot and hit: min(2^log_band, len) x qpad direction bytes, then the checkpoint rows
    int log_band;
    sw_alignment* aln;
    char* ops; int64_t ops_cap;
    unsigned long long* stamps;          // optional timing aid, three words: += ticks in the sweep, in the walk, in the walk's re-fills
};
template <int C>
__global__ void sw_align_ckpt_wave(AlignCkptParams p);
struct AlignHitsCkptParams {             // the items of a device hit table, from the lists of sw_align_hits_bin: AlignHitsParams and the band
    const unsigned char* db;
    const AlignHitItem* items;
    const unsigned int* counts;
    int tier;
    const MultiQuery* queries;
    const signed char* prof;
    int ge, goe;
    int* bnd; int64_t bnd_per;
    unsigned int* counter;
    unsigned char* dir; int64_t slot_bytes, nslots;   // per slot: room for a band of 2^log_band rows x the item's qpad and its checkpoint rows
    int log_band;
    sw_alignment* aln;
    char* ops; int64_t ops_cap;
};
template <int C>
__global__ void sw_align_hits_ckpt_wave(AlignHitsCkptParams p);

template <typename HT, int B>
__global__ void sw_strip_scan(const unsigned char* a, const unsigned char* b, FillParams p);
template <typename HT, int NS, int NC>
__global__ void sw_systolic(const unsigned char* a, const unsigned char* b, const unsigned char* bpad, FillParams p);
__global__ void sw_wipe_u32(unsigned int* buf, size_t n);
template <int NC, bool OV>
__global__ void sw_systolic2(const unsigned char* a, const unsigned char* b, FillParams p);
__global__ void sw_prep_scan(const unsigned char* a, int64_t cols, int64_t a_pstride, const unsigned char* b, int64_t rows, int64_t b_pstride, int64_t npairs,
                             unsigned int* part);
__global__ void sw_prep_code(const unsigned char* b, int64_t rows, int64_t front, int64_t b_pstride, unsigned char* bpad, unsigned short* bpad16,
                             unsigned char* bcode, const unsigned int* part, int npart, unsigned char* atab, int64_t per, int npad, void* H, int h_bytes,
                             void* P, int p_bytes, int64_t M, int64_t rows1, int skip_row0, unsigned long long* key);
__global__ void sw_xcc_probe(unsigned int* xcc_of_block);
__global__ void sw_prep_reduce(unsigned int* part, int npart);
__global__ void sw_finalize(const unsigned long long* key, const unsigned int* abort_flag, sw_result* res, int n);
template <typename PT>
__global__ void sw_traceback_wave(PT* P, int64_t M, int64_t rows1, int64_t pstride, int64_t start_pos, int64_t* paths, int64_t cap, sw_result* res,
                                  int64_t* stop, unsigned int* pathbits);
template <typename T> __global__ void sw_row_checksums(const T* X, int64_t m, unsigned long long* cs);
__global__ void sw_widen_p8(const signed char* P8, int32_t* P32, size_t n);
// 2-bit predecessor matrix (4 codes per byte) + path bitmap (1 bit per cell): sw_kernels.hip, sw_traceback.hip
struct P2Cells { unsigned char v; };     // tag type: sw_traceback_wave<P2Cells> walks a packed matrix
template <typename PT> __global__ void sw_pack_p2(const PT* P, unsigned char* P2, unsigned int* bits, size_t n);
__global__ void sw_unpack_p2(const unsigned char* P2, const unsigned int* bits, int32_t* P32, size_t n);

}  // namespace swk
