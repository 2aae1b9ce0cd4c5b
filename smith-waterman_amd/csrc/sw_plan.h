// sw_plan.h -- the planners: every policy decision of one fill (kernel, workgroup shape, perm producer, strip geometry, column
// tiles, scouts, roles per XCD, split strips, filler pacing, store kind), of one batch call (one pair or two pairs per wave, columns
// per lane, pairs per launch, the kernel of every launch) and of one database search (columns per lane, profile kind, grid, schedule;
// plan_search_affine for the affine-gap search) and of one alignment call (plan_align_affine: columns per lane, slots, grid, order of the
// hits; plan_align_hits: groups, size tiers and slots for a device hit table), and the workspace sizes they need, as pure functions of
// the job, the device and the options.  Plain C++ (no HIP include): sw_api_fill.hip and sw_api_search.hip carry a plan out,
// tests/test_fill_plan.py and tests/test_batch_plan.py check the policy on a CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "sw_debug.h"
#include "sw_mask_table.h"

namespace swk {   // shared with the search kernels (sw_kernels.h)

constexpr int SW_SEARCH_ROWS = 257;      // profile rows: one per byte value + PAD (the letter of every row outside a target)
struct SearchItem { int64_t start, idx, len; };   // a target in schedule order: first byte in db, index in the caller's order, length
// A query of a many-query search (sw_search_multi.hip), one entry of the call's device table: where its profile starts in the group's
// profile workspace, its first byte in the caller's query buffer, its row of the query-major results, its length, its profile row
// length (strips * 64 * C) and its strips at the C of its class.
struct MultiQuery { int64_t prof_off, qstart, row; int32_t qlen, qpad, nstrips, pad; };

}  // namespace swk

namespace swp {

struct PlanJob {
    int64_t cols = 0, rows = 0, npairs = 1;
    bool full_stride = true;                 // row stride == cols + 1
    int h_elem_bytes = 4, p_elem_bytes = 4;  // 4 / 8; 4 / 1
    bool has_H = true, has_P = true;         // which matrices are written
    bool has_top = false;                    // halo row in (a tile or a band)
    bool has_left = false, has_right = false;            // halo column in / out (a tile of a wider matrix)
    bool has_top_gran = false, has_bot_gran = false;     // band-resident launch: halo row in / last row out as granules
    bool has_result = true;                  // a result pointer the one-launch fill can write (batches keep their own keys)
    int64_t total_rows = 0;                  // band: rows of the whole matrix (bounds the scores a halo can carry)
    int reserve_cus = 0;                     // CUs left free for other kernels
    bool h_aligned = true, p_aligned = true; // d_H 16-byte (int64 H) / 8-byte aligned, d_P 8-byte aligned: whole-line stores possible
    int match = 3, mismatch = -3, gap = -2;
    float pair_ratio = 0.f;                  // store probe's two-stream / one-stream time of the H / P pair (~1.4: two classes of the HBM, ~2: one); 0: unknown
};

// sw_search_wave<C, WIDE> for C = 4, 8, 16: its index in kSearch (sw_api_search.hip, which checks its order against it at compile time)
constexpr int kSearchKernels = 6;
constexpr int search_kernel_index(int C, bool wide) { return 2 * (C / 8) + wide; }

struct DeviceFacts {
    int num_cus = 256;
    bool xcd_round_robin = false;            // workgroup i of a launch runs on XCD i % 8 (8 XCDs of 32 CUs)
    int s2_per_cu = 0;                       // occupancy of sw_systolic2 at 768 threads (workgroups per CU)
    int search_per_cu[kSearchKernels] = {};  // occupancy of every sw_search_wave instantiation at 256 threads
};

struct PlanOptions {   // the sw_set_option values the policy reads (include/swhip.h)
    int64_t engine = 0, strips_per_group = 0, consumers = 0, importers = 0, max_blocks = 0, waves_per_block = 4, store_policy = 0;
    int64_t s2w = 0, xcd_chain = 0, split_blk = 0, split_from = 0;
    int64_t filler_hop_ps = 2400000, filler_tau_ps = 25000, filler_bw_gbs = 4200;
    int64_t probe_foreign_pairs = 0, debug_flags = 0;
};

// one launch of the two-column kernel (a column tile, or the whole matrix)
struct TilePlan {
    int64_t c0 = 0, cols = 0, strips = 0;    // first column, columns, strips
    int grid = 0, nscout = 0, scout_double = 0, xcd_mode = 0;
    int split_blk = 0, split_from = 0, split_extra = 0, filler_end_steps = 0, filler_full_steps = 0;
    int filler_hop_ps = 0, filler_tau_ps = 0, filler_bw_gbs = 0;
    int store_nt = 0;
    int consumers = 0;                       // consumer waves: the kernel's instantiation
    int scan_all = 0;                        // prologue: every workgroup scans all letters itself (no grid barrier); the same in every tile
};

// tiles of at most 160 strips of at least 110 columns: cols <= SW_MAX_DIM gives at most 60
constexpr int kMaxTiles = 64;

struct FillPlan {
    int engine = 0;                          // 0: systolic (sw_systolic / sw_systolic2), 1: sw_strip_scan
    int64_t S = 0;                           // strips of the one-column kernel (sw_strip_scan: of 64 columns)
    int store_nt = 0;                        // streaming H / P stores
    // sw_systolic (also enqueued behind the two-column kernel: the fall-back for alphabets it cannot take)
    int NS = 0, NC = 0, importers = 0, threads = 0;
    int grid = 0;                            // before the occupancy cap
    bool fast = false;                       // fast producers (phi_base = S - 1)
    int64_t bfront = 0, per = 0;             // padded copies of b: index of b[0], elements per pair
    bool perm = false;                       // perm producer eligible on the host side
    int64_t e4stride = 0;
    // sw_systolic2: one launch per tile, each writes the result when it is the last (a fused fill: no sw_finalize behind it)
    bool two_cols = false;
    int W2 = 126;                            // strip width: 126 (strips tile the matrix) or 110 (overlapping strips, compiled in)
    int64_t ntile = 1, tstrips = 0;
    TilePlan tile[kMaxTiles];
    int64_t priv_stride = 0;
    // workspaces: edge granules, padded b (bytes), perm edge values, per-workgroup copies of b (bytes)
    size_t edge_need = 0, cb_need = 0, edge4_need = 0, priv_need = 0;
    // the output matrices, in bytes, and whether the pair's class of the HBM decides the strip geometry and is to be probed
    size_t h_bytes = 0, p_bytes = 0;
    bool probe_pair_class = false;
};

FillPlan plan_fill(const PlanJob& job, const DeviceFacts& dev, const PlanOptions& opt);

// The prologue of the two-column kernel finds the alphabet either by a scan shared among the workgroups and one grid barrier, or by
// every workgroup scanning all cols + rows letters for itself (no atomics in memory, no barrier).  The second is cheaper while the
// letters are few: up to this many (sw_plan.cpp says where the figure comes from).
constexpr int64_t kScanAllLetters = 48 * 1024;

// ---- batches of independent pairs (sw_batch_device_ex): one pair per wave (sw_batch_wave), two on packed 16-bit lanes (sw_batch_wave16),
// or the single-pair machinery in chunks (the fall-back)
struct BatchJob {
    int64_t cols = 0, rows = 0, npairs = 1;
    bool has_H = true, has_P = true;
    int p_elem_bytes = 4;                    // 4 / 1
    int match = 3, mismatch = -3, gap = -2;
};

struct BatchPlan {
    bool wave = false;                       // one pair per wave may run (scores, pair size, debug bit 16); the letter count decides on the device
    int C = 0;                               // columns per lane
    int64_t nstrips = 0;                     // strips of 64 C columns one wave sweeps after each other
    int front = 0;                           // padded letter codes of b: index of b[0] ...
    int64_t per = 0;                         // ... and bytes per pair
    int64_t bnd_per = 0;                     // boundary column between strips, ints per pair (0: one strip)
    int64_t chunk = 0;                       // pairs per launch
    int64_t grid = 0;                        // workgroups of a chunk at one pair per wave (sw_get_option "last_grid")
    int scan_blocks = 0, codes_blocks = 0;   // sw_prep_scan blocks; sw_batch_codes blocks per pair
    bool fits16 = false, k12 = false, packed16 = false;   // two pairs per wave: scores of 15 bits; keyed arg-max: 12 bits; taken
    size_t bcodes_need = 0, bnd_need = 0;    // workspaces: padded letter codes (bytes), boundary columns (ints)
    int64_t single_chunk = 0;                // the fall-back: pairs per launch (= arg-max keys of the workspace)
};

BatchPlan plan_batch(const BatchJob& job, const PlanOptions& opt);

// The batch kernels: their indices in kBatch (sw_api_fill.hip, which checks its order against them at compile time).  sw_batch_wave<C, PB> for
// C = 4, 8, 16 and PB = 0, 1, 4 first, then sw_batch_wave16<LE4, K12, PB1> (two pairs per wave) from kBatchWave16 on.
constexpr int kBatchWave16 = 9, kBatchKernels = 17;
constexpr int batch_wave_index(int C, int pb) { return 3 * (C / 8) + (pb == 4 ? 2 : pb); }
constexpr int batch_wave16_index(bool le4, bool k12, bool pb1) { return kBatchWave16 + 4 * le4 + 2 * k12 + pb1; }
// The kernel of a chunk of n pairs, given the letter count of the batch and the bytes of a P element (0: no P); -1: the batch has to
// run on the fall-back.
int batch_kernel(const BatchPlan& plan, unsigned nletters, int64_t n, int p_bytes);

// ---- database search (sw_search_device): one query against many targets of any length
struct SearchJob {
    int64_t qlen = 0, maxlen = 0;            // query length, longest target
    int64_t ntargets = 0;                    // non-empty targets
    int match = 3, mismatch = -3, gap = -2;
};

struct SearchPlan {
    int C = 0;                               // query columns per lane
    bool wide = false;                       // scores beyond a signed byte: the selector profile
    int kernel = 0;                          // index of sw_search_wave<C, wide> (kSearchKernels)
    int64_t nstrips = 0, qpad = 0;           // strips of 64 C columns; profile row length
    int64_t bnd_per = 0;                     // per resident wave: boundary column between strips (ints), 0: one strip
    int64_t grid = 0;                        // persistent workgroups of 4 waves
    int prof_blocks = 0;                     // sw_search_profile blocks
    size_t prof_need = 0, bnd_need = 0;      // workspaces: profile (bytes), boundary columns (ints)
};

SearchPlan plan_search(const SearchJob& job, const DeviceFacts& dev);

// ---- database search with a substitution matrix and affine gaps (sw_search_affine_device): sw_search_affine_wave<C> for C = 4, 8, 16,
// its index in kSearchAffine (sw_api_search.hip, which checks its order against it at compile time)
constexpr int kSearchAffineKernels = 3;
constexpr int search_affine_kernel_index(int C) { return C / 8; }

struct SearchAffineJob {
    int64_t qlen = 0, maxlen = 0;            // query length, longest target
    int64_t ntargets = 0;                    // non-empty targets
    int num_cus = 256;
    int per_cu[kSearchAffineKernels] = {};   // occupancy of every sw_search_affine_wave instantiation at 256 threads (workgroups per CU)
};

struct SearchAffinePlan {
    int C = 0;                               // query columns per lane
    int kernel = 0;                          // index of sw_search_affine_wave<C> (kSearchAffineKernels)
    int64_t nstrips = 0, qpad = 0;           // strips of 64 C columns; profile row length
    int bnd_row_ints = 0;                    // ints per row of a boundary column: H and F
    int64_t bnd_per = 0;                     // per resident wave: boundary column between strips (ints), 0: one strip
    int64_t grid = 0;                        // persistent workgroups of 4 waves
    int prof_blocks = 0;                     // sw_search_profile_submat blocks
    size_t prof_need = 0, bnd_need = 0;      // workspaces: profile (bytes), boundary columns (ints)
};

SearchAffinePlan plan_search_affine(const SearchAffineJob& job);

// ---- many queries against a prepared database (sw_db_search_affine): sw_search_affine_multi_wave<C> for C = 4, 8, 16, its index in
// kSearchMulti (sw_api_search.hip, which checks its order against it at compile time).
// Classes: a query gets the columns per lane plan_search_affine gives it alone; the queries of a class share a launch.
// Groups: consecutive queries whose profiles (257 x qpad bytes each, back to back) fit the budget; one query alone may exceed it.
// Items: work item w of a launch is the pair (target rank rank0 + w / nq, table entry q0 + w % nq): all the class's queries against the
// longest target first, then against the next -- the long pairs start first whatever the mix of query lengths; a launch ends where
// its items would pass kMultiMaxItems (the work counter is 32 bits wide), the next one goes on with the following target ranks.
constexpr int kSearchMultiKernels = 3;
constexpr int search_multi_kernel_index(int C) { return C / 8; }
constexpr int64_t kMultiMaxItems = (1ll << 31) - 1;

struct SearchMultiJob {
    const int64_t* qlens = nullptr;          // length of every query, input order
    int64_t nqueries = 0;
    int64_t longest = 0, nonempty = 0;       // of the handle: longest target, non-empty targets
    int num_cus = 256;
    int per_cu[kSearchMultiKernels] = {};    // occupancy of every sw_search_affine_multi_wave instantiation at 256 threads (workgroups per CU)
    int64_t budget_bytes = 256ll << 20;      // "search_profile_mib": the profiles of a group may take this much
    int64_t max_items = kMultiMaxItems;      // (tests lower it)
};

struct MultiGroup { int64_t q0 = 0, nq = 0, prof_bytes = 0; };   // the queries q0 .. q0 + nq - 1 = the table entries q0 .. q0 + nq - 1, by class
struct MultiLaunch {
    int group = 0, C = 0, kernel = 0;        // kernel: index of sw_search_affine_multi_wave<C> (kSearchMultiKernels)
    int64_t q0 = 0, nq = 0;                  // its queries: entries q0 .. q0 + nq - 1 of the table
    int64_t rank0 = 0, nranks = 0;           // its targets: ranks rank0 .. rank0 + nranks - 1 of the handle's schedule
    int64_t items = 0;                       // nq * nranks <= max_items
    int64_t bnd_per = 0;                     // per resident wave: boundary pairs between strips (ints), 0: every query has one strip
    int64_t grid = 0;                        // persistent workgroups of 4 waves: min(resident waves, items) waves
};

struct SearchMultiPlan {
    std::vector<swk::MultiQuery> table;      // one entry per query (qstart is left 0: the caller's offsets); per group sorted by class, input order within
    std::vector<MultiGroup> group;
    std::vector<MultiLaunch> launch;         // in the order they are enqueued: group after group
    size_t prof_need = 0, bnd_need = 0;      // workspaces: profiles of the largest group (bytes), boundary columns (ints)
};

SearchMultiPlan plan_search_multi(const SearchMultiJob& job);

// ---- a device list of (query, target) pairs against a prepared database (sw_db_search_affine_pairs; sw_search_pairs.hip):
// sw_search_affine_pairs_wave<C> for C = 4, 8, 16, its index in kSearchPairs (sw_api_search.hip, which checks its order against it at
// compile time).  The host knows the queries and the handle's longest target, neither the pairs nor the targets they name.
// Queries: the table and the groups are plan_search_multi's, entry for entry, so sw_search_profile_submat_multi fills a group's profiles
// as it does there; entry_of[q] is the table entry of query q (the device gets from a pair's query to its entry through it).
// Chunks: the list is taken in consecutive chunks of at most `chunk` pairs ("search_pairs_chunk"); chunk i holds the pairs
// [i * chunk, min(npairs, (i + 1) * chunk)).  That bounds the item workspace (24 bytes per pair of a chunk) and keeps every count,
// cursor and work counter inside 32 bits.
// Launches: every (chunk, group) gets a count launch, a scatter launch and one score launch per class present in the group -- `launch`
// holds those of one chunk, group after group; a score launch runs min(resident waves, pairs of the chunk) waves in workgroups of four
// (search_pairs_grid), fewer where the boundary columns would pass kSearchBndBytes.  The kernel reads its list's length on the device.
// Order inside a class's list: heaviest first.  An item's bucket is floor(log2(len x qpad)) -- at most kSearchPairsBuckets of them, since
// len < 2^20 and qpad <= 2^20 --, the list holds bucket after bucket from the heaviest down, and the one launch of a class starts
// with its longest pairs (the short tail of DESIGN 9c).  Order inside a bucket comes from an atomic and is free.
constexpr int kSearchPairsKernels = 3;
constexpr int search_pairs_kernel_index(int C) { return C / 8; }
constexpr int kSearchPairsBuckets = 41;
constexpr int64_t kSearchPairsChunk = 1ll << 22;     // the default chunk: 24 bytes of list each (96 MiB), the bound of kAlignHitsMaxItems
constexpr int64_t kSearchPairsChunkMax = (1ll << 31) - 1;
constexpr int search_pairs_bucket(int64_t len, int64_t qpad) { return 63 - __builtin_clzll((unsigned long long)(len * qpad)); }   // len, qpad >= 1

struct SearchPairsJob {
    const int64_t* qlens = nullptr;          // length of every query, input order
    int64_t nqueries = 0, npairs = 0;
    int64_t longest = 0;                     // of the handle: longest target
    int num_cus = 256;
    int per_cu[kSearchPairsKernels] = {};    // occupancy of every sw_search_affine_pairs_wave instantiation at 256 threads (workgroups per CU)
    int64_t budget_bytes = 256ll << 20;      // "search_profile_mib": the profiles of a group may take this much
    int64_t chunk = kSearchPairsChunk;       // "search_pairs_chunk"
};

struct PairsGroup {
    int64_t q0 = 0, nq = 0, prof_bytes = 0;  // as MultiGroup
    int64_t cls_q0[kSearchPairsKernels + 1] = {};   // class k: the table entries cls_q0[k] .. cls_q0[k + 1] - 1
};
struct PairsLaunch {                         // the score launch of a class of a group, the same in every chunk but for its grid
    int group = 0, C = 0, kernel = 0;        // kernel: index of sw_search_affine_pairs_wave<C> (kSearchPairsKernels)
    int64_t q0 = 0, nq = 0;                  // its queries: entries q0 .. q0 + nq - 1 of the table
    int64_t bnd_per = 0;                     // per resident wave: boundary pairs between strips (ints), 0: every query of the class has one strip
    int64_t max_grid = 0;                    // workgroups of 4 waves the device (and the boundary workspace) holds
};
constexpr int64_t search_pairs_grid(const PairsLaunch& l, int64_t chunk_pairs) {   // min(resident waves, pairs of the chunk) waves
    const int64_t g = (chunk_pairs + 3) / 4 < l.max_grid ? (chunk_pairs + 3) / 4 : l.max_grid;
    return g < 1 ? 1 : g;
}

struct SearchPairsPlan {
    std::vector<swk::MultiQuery> table;      // as SearchMultiPlan::table
    std::vector<int32_t> entry_of;           // per query: its entry of the table
    std::vector<PairsGroup> group;
    std::vector<PairsLaunch> launch;         // the score launches of ONE chunk in the order they are enqueued: group after group
    int64_t chunk = 0, nchunks = 0;          // pairs of a full chunk; chunks of the call
    int64_t launches = 0;                    // kernel launches of the call: per group a profile launch, per (chunk, group) two binning launches and its score launches
    size_t prof_need = 0, bnd_need = 0, items_need = 0;   // workspaces: profiles of the largest group (bytes), boundary columns (ints), items (bytes)
    int64_t chunk_p0(int64_t i) const { return i * chunk; }
    int64_t chunk_pairs(int64_t i, int64_t npairs) const { return npairs - i * chunk < chunk ? npairs - i * chunk : chunk; }
};

SearchPairsPlan plan_search_pairs(const SearchPairsJob& job);

// ---- the ungapped pre-filter of a many-query search (sw_db_prefilter_ungapped; sw_prefilter.hip): sw_prefilter_wave<C> (32-bit lanes,
// one target per wave) and sw_prefilter_wave16<C> (packed 16-bit lanes, two targets per wave) for C = 4, 8, 16, their index in
// kPrefilter (sw_api_search.hip, which checks its order against it at compile time).
// Queries: the groups, the classes and every table entry are plan_search_multi's (the profiles lie where they lie there, so
// sw_search_profile_submat_multi fills them unchanged); inside a (group, class) the entries of the queries that run packed come first,
// input order within either part.
// Packed: a query runs on 16-bit lanes where max_entry x min(qlen, longest target) <= kPrefilterPackedMax (max_entry: the largest
// table entry, at least 0): no score of any of its pairs leaves int16.  lanes = 32 ("prefilter_lanes") sends every query to 32-bit lanes.
// Launches: per (group, class) the packed queries and the others get launches of their own, cut by target ranks where the items would
// pass max_items (the work counter and the cursor of the list are 32 bits wide).  A 32-bit launch has nq x nranks items; item w is
// (rank rank0 + w / nq, entry q0 + w % nq).  A packed launch has nq x ceil(nranks / 2) items; item w runs the ranks rank0 + 2 (w / nq)
// and, if it lies inside the launch, the next one -- rank0 is even, and only the last launch of a class can hold an odd last rank.
// Boundary: per resident wave two columns of one int per row, sized by the handle's longest target; 0 where every query has one strip.
constexpr int kPrefilterKernels = 6;
constexpr int prefilter_kernel_index(int C, bool packed) { return 2 * (C / 8) + (packed ? 1 : 0); }
constexpr int64_t kPrefilterPackedMax = 32767;
constexpr bool prefilter_packed(int64_t max_entry, int64_t qlen, int64_t longest, int lanes) {
    return lanes != 32 && (max_entry < 0 ? 0 : max_entry) * (qlen < longest ? qlen : longest) <= kPrefilterPackedMax;
}

struct PrefilterJob {
    const int64_t* qlens = nullptr;          // length of every query, input order
    int64_t nqueries = 0;
    int64_t longest = 0, nonempty = 0;       // of the handle: longest target, non-empty targets
    int num_cus = 256;
    int per_cu[kPrefilterKernels] = {};      // occupancy of every instantiation at 256 threads (workgroups per CU)
    int64_t budget_bytes = 256ll << 20;      // "search_profile_mib"
    int64_t max_items = kMultiMaxItems;      // (tests lower it)
    int max_entry = 0;                       // the largest entry of the substitution table
    int lanes = 0;                           // "prefilter_lanes": 0 the planner decides, 32 never packed
};

struct PrefilterLaunch {
    int group = 0, C = 0, kernel = 0;        // kernel: prefilter_kernel_index(C, packed)
    bool packed = false;
    int64_t q0 = 0, nq = 0;                  // its queries: entries q0 .. q0 + nq - 1 of the table
    int64_t rank0 = 0, nranks = 0;           // its targets: ranks rank0 .. rank0 + nranks - 1 of the handle's schedule
    int64_t items = 0;                       // nq * nranks, packed: nq * ceil(nranks / 2); <= max_items
    int64_t bnd_per = 0;                     // per resident wave: boundary ints, 0: every query of the launch has one strip
    int64_t grid = 0;                        // persistent workgroups of 4 waves: min(resident waves, items) waves
};

struct PrefilterPlan {
    std::vector<swk::MultiQuery> table;      // as SearchMultiPlan::table, but for the order inside a (group, class)
    std::vector<MultiGroup> group;
    std::vector<PrefilterLaunch> launch;     // in the order they are enqueued: group after group
    int64_t packed_launches = 0;
    size_t prof_need = 0, bnd_need = 0;      // workspaces: profiles of the largest group (bytes), boundary columns (ints)
};

PrefilterPlan plan_prefilter(const PrefilterJob& job);

// ---- the many-query search with a choice of lanes ("search_lanes"; sw_search_multi16.hip): sw_search_multi_pk_wave<C> for C = 4, 8, 16
// runs two targets of a query per wave on packed 16-bit lanes; its index in kSearchMultiPacked (sw_api_search.hip, which checks its
// order against it at compile time) is search_multi_kernel_index(C).
// Queries: the groups, the classes and every table entry are plan_search_multi's for the 32-bit kernels' occupancy, whatever the lanes
// (the profiles lie where they lie there); inside a (group, class) the entries of the queries that run packed come first, input order
// within either part.
// Packed: under lanes = 16 a query runs on 16-bit lanes where
//     max(max_entry, 0) x min(qlen, longest target) <= kPrefilterPackedMax   and   gap_open + 2 gap_extend >= kSearchPackedGapMin
// (max_entry: the largest entry of the table, or a PSSM's smax) -- the header of sw_search_multi16.hip proves that no half wraps under
// them -- and where the packed kernel of its class fits a CU (16 columns per lane: kAffineC16MinPerCu workgroups, as the 32-bit
// kernel).  Every other query runs on the 32-bit kernel inside the same call; lanes = 32 sends every query there, and then the launches
// are plan_search_multi's, field for field.
// Launches: as plan_prefilter's.  Per (group, class) the packed queries and the others get launches of their own, cut by target ranks
// where the items would pass max_items.  A packed launch has nq x ceil(nranks / 2) items; item w runs the ranks rank0 + 2 (w / nq) and,
// if it lies inside the launch, the next one, against entry q0 + w % nq -- rank0 is even, and only the last launch of a class can hold
// an odd last rank.  Its boundary workspace per resident wave is that of the 32-bit launch of the same queries.
constexpr int64_t kSearchPackedGapMin = -32768;
constexpr bool search_multi_packed(int64_t max_entry, int64_t qlen, int64_t longest, int64_t gap_open, int64_t gap_extend, int lanes) {
    return lanes == 16 && gap_open + 2 * gap_extend >= kSearchPackedGapMin &&
           (max_entry < 0 ? 0 : max_entry) * (qlen < longest ? qlen : longest) <= kPrefilterPackedMax;
}

struct SearchMultiLanesJob : SearchMultiJob {    // per_cu: of the 32-bit kernels, as there
    int packed_per_cu[kSearchMultiKernels] = {}; // occupancy of every sw_search_multi_pk_wave instantiation at 256 threads (workgroups per CU)
    int max_entry = 0;                       // the largest entry of the substitution table; a PSSM's smax
    int gap_open = 0, gap_extend = 0;
    int lanes = 32;                          // "search_lanes": 32 never packed, 16 packed where a query is eligible
};

struct MultiLanesLaunch : MultiLaunch {      // kernel: index in kSearchMulti, packed: in kSearchMultiPacked; items packed: nq * ceil(nranks / 2)
    bool packed = false;
};

struct SearchMultiLanesPlan {
    std::vector<swk::MultiQuery> table;      // as SearchMultiPlan::table, but for the order inside a (group, class)
    std::vector<MultiGroup> group;
    std::vector<MultiLanesLaunch> launch;    // in the order they are enqueued: group after group
    int64_t packed_launches = 0;
    size_t prof_need = 0, bnd_need = 0;      // workspaces: profiles of the largest group (bytes), boundary columns (ints)
};

SearchMultiLanesPlan plan_search_multi_lanes(const SearchMultiLanesJob& job);

// ---- the pair list with a choice of lanes ("search_pairs_lanes"; sw_search_pairs16.hip): sw_search_pairs_pk_wave<C> for C = 4, 8, 16
// runs two listed pairs of one query per wave on packed 16-bit lanes; its index in kSearchPairsPacked (sw_api_search.hip, which checks
// its order against it at compile time) is search_pairs_kernel_index(C).  The relation to plan_search_pairs is the relation of
// plan_search_multi_lanes to plan_search_multi.
// Queries: the groups, the classes, the chunks and every table entry are plan_search_pairs's for the 32-bit kernels' occupancy,
// whatever the lanes; inside a (group, class) the entries of the queries that run packed come first, input order within either part,
// and entry_of follows.  Packed: search_multi_packed's rule against the HANDLE's longest target -- a conservative bound for a list,
// which may name shorter targets only -- and the packed kernel of the class fits a CU (16 columns per lane: kAffineC16MinPerCu).
// lanes = 32 sends every query to the 32-bit kernel, and then the plan is plan_search_pairs's, field for field.
// Cells: the device pairs the listed pairs of a packed query inside a bucket.  A group's cells are (packed entry, bucket), laid out
// class after class, inside a class the heaviest bucket first, inside a bucket entry after entry (search_pairs_cell): a prefix sum in
// that order gives every cell its place in the list of two-pair items.  A cell of n pairs takes ceil(n / 2) items.
// Items: np pairs in `cells` cells make at most search_pairs_packed_items_max(np, cells) = min(np, floor((np + cells) / 2)) two-pair
// items -- every cell holds at most one item with an empty half, and no more items than pairs --, and the bound is met (cells of one
// pair each, the rest in one cell).  A two-pair item takes twice a pair's item (2 x 24 bytes), and the 32-bit items of the (chunk,
// group) lie behind the two-pair items: every pair takes 24 bytes wherever it goes and every empty half another 24, one per cell at
// most and no more than there are pairs, so a chunk of `most` pairs needs 24 x min(2 most, most + cells) bytes where a group has packed
// queries; items_need is the largest of these and the 24 x most of plan_search_pairs.  cells_need: the counters of the largest
// group's cells (count, cursor, base: 4 bytes each) behind kSearchPairsCellsHead bytes of control words.
// Launches: a group WITHOUT packed queries is plan_search_pairs's: two binning launches per chunk and a score launch per class.  A group
// with packed queries gets three binning launches per chunk (count, scan, scatter) and per class a packed score launch (if the class has
// packed queries) followed by a 32-bit one (if it has others), both with the boundary workspace of the class.
constexpr int64_t kSearchPairsCellsHead = 1024;
constexpr int64_t search_pairs_packed_items_max(int64_t np, int64_t cells) { return np < (np + cells) / 2 ? np : (np + cells) / 2; }
// bytes of the item workspace for a (chunk, group) of np pairs with `cells` cells: 24 per pair and 24 per empty half
constexpr int64_t search_pairs_lanes_item_bytes(int64_t np, int64_t cells) { return 24 * (2 * np < np + cells ? 2 * np : np + cells); }
// the cell of (entry t of class k, bucket b): cell0 = cells of the classes before, npk = packed entries of the class, t0 = its first entry
constexpr int64_t search_pairs_cell(int64_t cell0, int64_t npk, int64_t t0, int64_t t, int b) { return cell0 + (int64_t)(kSearchPairsBuckets - 1 - b) * npk + (t - t0); }

struct SearchPairsLanesJob : SearchPairsJob {    // per_cu: of the 32-bit kernels, as there
    int packed_per_cu[kSearchPairsKernels] = {}; // occupancy of every sw_search_pairs_pk_wave instantiation at 256 threads (workgroups per CU)
    int max_entry = 0;                       // the largest entry of the substitution table
    int gap_open = 0, gap_extend = 0;
    int lanes = 32;                          // "search_pairs_lanes": 32 never packed, 16 packed where a query is eligible
};

struct PairsLanesGroup : PairsGroup {
    int64_t pk_q1[kSearchPairsKernels] = {}; // class k: its packed entries are cls_q0[k] .. pk_q1[k] - 1, the others pk_q1[k] .. cls_q0[k + 1] - 1
    int64_t cells = 0;                       // kSearchPairsBuckets x packed entries of the group
};
struct PairsLanesLaunch : PairsLaunch {      // kernel: index in kSearchPairs, packed: in kSearchPairsPacked; q0, nq: its part of the class
    bool packed = false;
};
// workgroups of a score launch for a chunk of `chunk_pairs` pairs: a packed launch has at most items_max(chunk_pairs, cells) items
constexpr int64_t search_pairs_lanes_grid(const PairsLanesLaunch& l, int64_t chunk_pairs, int64_t cells) {
    return search_pairs_grid(l, l.packed ? search_pairs_packed_items_max(chunk_pairs, cells) : chunk_pairs);
}

struct SearchPairsLanesPlan {
    std::vector<swk::MultiQuery> table;      // as SearchPairsPlan::table, but for the order inside a (group, class)
    std::vector<int32_t> entry_of;           // per query: its entry of the table
    std::vector<PairsLanesGroup> group;
    std::vector<PairsLanesLaunch> launch;    // the score launches of ONE chunk in the order they are enqueued: group after group, class after class, packed first
    int64_t chunk = 0, nchunks = 0;          // as SearchPairsPlan
    int64_t launches = 0;                    // kernel launches of the call: per group a profile launch, per (chunk, group) its binning and score launches
    int64_t packed_launches = 0;             // ... the packed score launches among them
    size_t prof_need = 0, bnd_need = 0, items_need = 0;   // workspaces as SearchPairsPlan
    size_t cells_need = 0;                   // the cell workspace (bytes), 0 without a packed query
    int64_t chunk_p0(int64_t i) const { return i * chunk; }
    int64_t chunk_pairs(int64_t i, int64_t npairs) const { return npairs - i * chunk < chunk ? npairs - i * chunk : chunk; }
};

SearchPairsLanesPlan plan_search_pairs_lanes(const SearchPairsLanesJob& job);

// ---- the best `top` targets of every row of a query-major result table (sw_top_hits_device, sw_db_search_affine_top; sw_search_top.hip).
// Key: a target's key is score << tbits | (2^tbits - 1 - target) with tbits = ceil(log2 ntargets): unique per target, and plain integer
// order of the keys is the rank order (score descending, target ascending).  nbits = 24 + tbits bits of a key can differ.
// Kernels: rows of at most kTopMax targets are sorted whole by one workgroup (kernel 0).  Longer rows (kernel 1) are radix-selected:
// `npasses` digit passes from the top bit down, pass p over the `bits` bits from `shift` on, find the key of rank `top`; every pass is a
// histogram launch of wgs_row workgroups per row -- workgroup w of a row reads the targets [w * slice, min(ntargets, (w + 1) * slice)) --
// and a one-workgroup-per-row scan; a compaction launch of the same shape gathers the keys at or above it, and kernel 0's sort orders them.
// Chunks: consecutive queries whose rows (24 bytes per target) fit the budget, at most kTopChunkQueries of them (that bounds the
// histograms), at least one -- a row larger than the budget is a chunk of its own.
constexpr int64_t kTopMax = 4096;            // SW_TOP_MAX (include/swhip.h): the keys one workgroup sorts in LDS
constexpr int kTopDigitBits = 11;            // widest digit of a pass: 2048 bins of 4 bytes in LDS and per row in the workspace
constexpr int kTopMaxPasses = 5;             // ceil((24 + 31) / kTopDigitBits)
constexpr int64_t kTopChunkQueries = 4096;
constexpr int64_t kTopMinSlice = 4096;       // a workgroup of 256 threads takes at least 16 targets per thread

struct SearchTopJob {
    int64_t nqueries = 0, ntargets = 0, top = 1;
    int64_t budget_bytes = 1ll << 30;        // "search_results_mib": the rows of a chunk may take this much
    int num_cus = 256;
    int per_cu = 8;                          // occupancy of the histogram kernel at 256 threads (workgroups per CU)
};

struct TopChunk { int64_t q0 = 0, nq = 0; };
struct TopPass { int shift = 0, bits = 0; };
struct SearchTopPlan {
    int kernel = 0;                          // 0: every row is sorted whole, 1: radix select, then the sort of the selected keys
    std::vector<TopChunk> chunk;             // in order, every query once
    int64_t chunk_queries = 0;               // queries of the largest chunk
    int tbits = 0, nbits = 24;               // bits of a key's target field; bits of a key that can differ
    int npasses = 0;                         // kernel 1: digit passes, highest bits first
    TopPass pass[kTopMaxPasses];
    int64_t wgs_row = 1, slice = 0;          // kernel 1: workgroups per row and the targets each one reads
    size_t results_need = 0;                 // workspaces: result rows of the largest chunk (sw_result elements) ...
    size_t hist_need = 0, state_need = 0;    // ... kernel 1: histogram bins (uint32) and per-row states of the largest chunk
};

SearchTopPlan plan_search_top(const SearchTopJob& job);

// ---- the best `top` entries of every query of a scored PAIR LIST (sw_top_hits_pairs_device; sw_top_pairs.hip).  The list is neither
// sorted nor grouped, so the selection first groups it: a count launch (qualifying entries per query), a one-workgroup scan (segment
// offsets), a scatter launch (every qualifying entry's sort item -- the key above, 8 bytes, beside its list position, 4 bytes -- into
// its query's segment), then one workgroup per query orders its segment by (key descending, position ascending) and writes the row.
// Count and scatter: `grid` workgroups of 256 threads, workgroup w over the entries [w * slice, min(npairs, (w + 1) * slice)).  Up to
// kTopPairsLdsQueries queries (`lds`) a workgroup counts its slice in an LDS histogram and touches global memory with one vector atomic
// per (workgroup, query) that occurs in it -- a list has far more entries than queries, and one global atomic per entry on a few
// addresses serialises; beyond that many queries the addresses are many and every entry takes its own atomic.
// Sort: `items` sort items of LDS per workgroup.  Kernel 0 (npairs <= kTopMax: every segment fits) sorts a segment whole.  Kernel 1
// streams a longer segment: the best T = pow2ceil(top) items so far stay in front, the next items - T entries of the segment are
// loaded behind them, the whole is sorted and the first T kept.  items = max(kTopMax, 2 T): 4096 (48 KiB) up to top = 2048, 8192
// (96 KiB) above, so a round takes in at least as many new entries as it keeps.
constexpr int64_t kTopPairsLdsQueries = 8192;   // 32 KiB of LDS counters
constexpr int64_t kTopPairsMinSlice = 4096;     // a workgroup of 256 threads takes at least 16 entries per thread
constexpr int64_t kTopPairsSortGrid = 1 << 16;  // the sort's workgroups walk the queries in strides of at most this many
constexpr int kTopPairsKernels = 3;
constexpr int top_pairs_kernel_index(int64_t items, bool stream) { return stream ? (items > kTopMax ? 2 : 1) : 0; }

struct TopPairsJob {
    int64_t npairs = 0, nqueries = 0, ntargets = 0, top = 1;
    int num_cus = 256;
};

struct TopPairsPlan {
    const char* refused = nullptr;           // not NULL: the call is SW_EINVAL for this reason, nothing else of the plan is set
    int tbits = 0;                           // bits of a key's target field: ceil(log2 ntargets)
    bool lds = false;                        // count and scatter aggregate per workgroup in LDS
    int64_t grid = 0, slice = 0;             // count and scatter: workgroups and the entries each one reads (0 workgroups: an empty list)
    int kernel = 0;                          // 0: every segment is sorted whole, 1: the streaming form ("last_top_pairs_kernel")
    int64_t T = 1, items = kTopMax;          // the sort: items kept between rounds, sort items of LDS
    int sort_kernel = 0;                     // index of sw_top_pairs_sort<items, stream> (kTopPairsKernels)
    int64_t sort_grid = 0;
    int launches = 0;                        // kernel launches of the call ("last_top_pairs_launches")
    size_t keys_need = 0, pos_need = 0;      // workspaces: keys (uint64) and positions (uint32) of the segments, npairs each ...
    size_t seg_need = 0;                     // ... and per query a count / cursor and an offset (uint32): 2 * (nqueries + 1)
    int64_t segment_bytes = 0;               // 12 * npairs: what the segments take (at most 16 bytes per entry)
};

TopPairsPlan plan_top_pairs(const TopPairsJob& job);

// The workspace of sw_db_search_affine_top_prefiltered: list and results (16 + 24 bytes per entry) beside the segments above.
constexpr int64_t kTopPrefilteredEntryBytes = 56;
constexpr int64_t top_prefiltered_cap(int64_t budget_bytes) { return budget_bytes / kTopPrefilteredEntryBytes; }

// ---- the next iteration's PSSM from aligned hits (sw_db_pssm_from_hits; sw_pssm_hits.hip).  One workgroup of 256 threads per (query,
// tile of tile_cols columns); a tile's int32 counts lie in LDS, `stride` dwords per column behind the 256-byte table from a target byte
// to its place in a column.
// Stride: (nletters + 1) | 1 -- one spare dword per column for its sum N[j], and odd, so that the same letter of adjacent columns (what
// the lanes of a run of 'M' touch) falls into different banks.
// LDS: kPssmHitsLdsBytes, the 64 KiB every workgroup may take without opting in; two workgroups per CU keep their waves apart.  That
// holds 604 columns of 25 letters and 63 columns of 256 letters.
// Tile: every workgroup of a query walks the ops of all the query's hits up to the end of its tile, so tiles are as wide as spreading
// the call over the device allows -- the columns of the call over two workgroups per CU, in whole chunks of 64 columns (a chunk of ops
// advances at most 64 columns), at least 64 -- and at most what the LDS holds or the longest query needs.
// Grid: queries x tiles of the LONGEST query (a shorter query's surplus workgroups return at once), walked in strides of at most
// kPssmHitsGridMax workgroups.
constexpr int64_t kPssmHitsLdsBytes = 64 << 10;
constexpr int64_t kPssmHitsCodeBytes = 256;
constexpr int64_t kPssmHitsGridMax = 1 << 20;

struct PssmHitsJob {
    const int64_t* qlens = nullptr;          // length of every query, input order
    int64_t nqueries = 0;
    int nletters = 1;                        // 1..256
    int num_cus = 256;
};

struct PssmHitsPlan {
    int stride = 0;                          // dwords per column in LDS
    int tile_cols = 0;                       // columns per workgroup
    int64_t max_cols = 0;                    // ... and the most the LDS holds
    int64_t tiles_per_query = 0;             // tiles of the longest query
    int64_t grid = 0;                        // workgroups (0: no query)
    unsigned lds_bytes = 0;                  // dynamic LDS of a workgroup
    int launches = 0;                        // kernel launches of the call ("last_pssm_hits_launches")
};

PssmHitsPlan plan_pssm_hits(const PssmHitsJob& job);

// ---- the position-based weights of aligned hits (sw_db_pssm_hit_weights; sw_pssm_weights.hip).  Two launches.  The first keeps a
// tile's int32 counts, then its terms, in the LDS layout of the update above -- the spare dword of a column holds k_j in the place of
// N[j] --, so its tiles, stride, grid and LDS are plan_pssm_hits' for the same queries and letters: `tiles`.  The tiles of an entry add
// their share to the entry's 64-bit accumulator in the workspace (kPssmWeightsAccBytes per entry, nqueries x top of them, zeroed by a
// memset before the launch).  The second launch runs one workgroup of 256 threads per query, walked in strides of at most
// kPssmHitsGridMax workgroups, with the query's top <= SW_TOP_MAX values A_r in static LDS.
constexpr int64_t kPssmWeightsAccBytes = 8;

struct PssmWeightsJob {
    PssmHitsJob queries;                     // the queries, the letters and the device, as for the update
    int64_t top = 1;                         // 1..SW_TOP_MAX
};

struct PssmWeightsPlan {
    PssmHitsPlan tiles;                      // the first launch (tiles.launches counts that launch alone)
    int64_t finish_grid = 0;                 // workgroups of the second launch (0: no query)
    int64_t acc_entries = 0, acc_bytes = 0;  // the accumulators
    int launches = 0;                        // kernel launches of the call ("last_pssm_weights_launches")
};

PssmWeightsPlan plan_pssm_weights(const PssmWeightsJob& job);

// ---- the query-anchored alignment of aligned hits (sw_db_msa_from_hits; sw_msa_hits.hip).  Up to four launches of 256 threads.
// Launch A (column rows and the rows' counts): one workgroup per (query, slice of slice_entries entries r), its four waves taking the
// slice's entries round robin.  A slice is the call's nqueries x top entries over kMsaHitsWgsPerCu workgroups per CU, in whole rounds of
// the four waves, at least one round and at most the rounds `top` takes; the slices of a query cover 0 .. top - 1 exactly once.
// Grid: queries x slices, walked in strides of at most kPssmHitsGridMax workgroups.
// Launch B (with rows only; the exclusive scan of the rows' lengths), two levels: scan_chunks chunks of kMsaScanChunk entries, one
// workgroup each (walked in strides of at most kPssmHitsGridMax), leave their sums in the workspace (8 bytes per chunk); ONE workgroup
// scans those sums kMsaScanChunk at a time in top_rounds rounds.  scan_levels: 1 where one chunk holds every entry (the second level
// then only carries the total out), else 2.
// Launch C (with rows only): one wave per entry, four to a workgroup, walked in strides of at most kPssmHitsGridMax workgroups.
constexpr int64_t kMsaScanChunk = 256;
constexpr int64_t kMsaHitsWgsPerCu = 8;

struct MsaHitsJob {
    int64_t nqueries = 0, top = 1;           // top: 1..SW_TOP_MAX
    int num_cus = 256;
    bool rows = true;                        // the A3M side is asked for (d_rows): launches B and C
};

struct MsaHitsPlan {
    int64_t entries = 0;                     // nqueries x top
    int64_t slice_entries = 0, slices_per_query = 0, cols_grid = 0;   // launch A (grid 0: no query)
    int64_t scan_chunks = 0, scan_grid = 0;  // launch B, first level (0: no rows)
    int64_t top_rounds = 0;                  // ... second level: rounds of its one workgroup
    int scan_levels = 0;
    int64_t rows_grid = 0;                   // launch C
    int64_t sums_bytes = 0;                  // the workspace: one int64 per chunk
    int launches = 0;                        // kernel launches of the call ("last_msa_hits_launches")
};

MsaHitsPlan plan_msa_hits(const MsaHitsJob& job);

// ---- the filter of a hit alignment (sw_msa_filter_device; sw_msa_filter.hip).  Two launches of 256 threads per chunk of queries.
// Rows go in blocks of kMsaFilterTile = 64: `blocks` per query.  Per query the workspace holds blocks + 1 planes of blocks x 64 64-bit
// words: word r of plane c has bit i set where row r is redundant to row 64 c + i (planes c <= r / 64 only; bit i of a word on the
// diagonal only for 64 c + i < r), word r of the last plane is the row's own test (cover, query).  A plane is indexed by the row, so
// the 64 lanes of a wave store and load neighbouring words.
// Pair launch: one workgroup per (query, tile); tile t of the tiles_per_query = blocks (blocks + 1) / 2 is (row block rb, compared
// block cb <= rb) in row-major order of the triangle (msa_filter_tile); every pair r' < r lies in exactly one tile, (r / 64, r' / 64).
// The tiles on the diagonal also compare their rows with the query.  A tile takes its rows kMsaFilterChunkCols columns at a time.
// Greedy launch: one workgroup per query.
// Chunks: queries_per_chunk queries, as many as fit budget_bytes ("msa_filter_workspace_mib"), at least one -- one query is never
// refused --, so the workspace holds at most max(budget_bytes, one query's bytes).  Grids: walked in strides of at most
// kPssmHitsGridMax workgroups.
constexpr int64_t kMsaFilterTile = 64;
constexpr int64_t kMsaFilterChunkCols = 64;
constexpr int64_t msa_filter_query_words(int64_t top) {
    const int64_t blocks = (top + kMsaFilterTile - 1) / kMsaFilterTile;
    return (blocks + 1) * blocks * kMsaFilterTile;
}
constexpr int64_t kMsaFilterMinMib = (8 * msa_filter_query_words(4096) + (1 << 20) - 1) >> 20;   // one query of top 4096: 3
// tile t -> (rb, cb), cb <= rb: t = rb (rb + 1) / 2 + cb
constexpr void msa_filter_tile(int64_t t, int& rb, int& cb) {
    int r = 0;
    while ((int64_t)(r + 1) * (r + 2) / 2 <= t) ++r;
    rb = r;
    cb = (int)(t - (int64_t)r * (r + 1) / 2);
}

struct MsaFilterJob {
    int64_t nqueries = 0, top = 1;           // top: 1..SW_TOP_MAX
    int64_t budget_bytes = 256ll << 20;      // "msa_filter_workspace_mib"
};

struct MsaFilterPlan {
    int64_t blocks = 0;                      // row blocks of a query
    int64_t tiles_per_query = 0;             // the triangle with its diagonal; the diagonal tiles take the query column
    int chunk_cols = 0;                      // columns a tile stages at a time
    int64_t query_words = 0, query_bytes = 0;   // a query's share of the workspace
    int64_t queries_per_chunk = 0, chunks = 0;
    int64_t workspace_bytes = 0;             // queries_per_chunk queries
    int64_t pair_grid = 0, greedy_grid = 0;  // of a whole chunk (0: no query)
    int64_t last_queries = 0, last_pair_grid = 0, last_greedy_grid = 0;   // of the last chunk
    int launches = 0;                        // kernel launches of the call ("last_msa_filter_launches")
};

MsaFilterPlan plan_msa_filter(const MsaFilterJob& job);

// ---- the score histogram of a result table (sw_score_hist_device, the _top_stats searches; sw_score_hist.hip).  One launch of 256
// threads per call or chunk.  A query's histogram is kScoreHistClasses x kScoreHistBins uint32 counters, 40 KiB; a workgroup keeps
// `copies` private ones in LDS (wave w adds into copy w % copies), so copies x 40 KiB <= the CU's 160 KiB.  Work item w of the
// nqueries x slices_per_query is (query w / slices_per_query, targets [s x slice, min(ntargets, (s + 1) x slice)) with s = w %
// slices_per_query): every target of every query lies in exactly one item.  Slices: as many as give every CU kScoreHistWgsPerCu
// workgroups, but no slice below kScoreHistMinSlice targets -- zeroing and flushing 10 240 counters costs a workgroup as much as 40
// targets per thread -- and at most kScoreHistMaxSlices, which bounds the adds into one global counter.  The grid is walked in strides
// of at most kPssmHitsGridMax workgroups.
constexpr int kScoreHistClasses = 40;        // SW_HIST_CLASSES: half octaves of the target's length, lengths below 2^20
constexpr int kScoreHistBins = 256;          // SW_HIST_BINS
constexpr int64_t kScoreHistCells = (int64_t)kScoreHistClasses * kScoreHistBins;
constexpr int64_t kScoreHistLdsMax = 160 << 10;
constexpr int64_t kScoreHistMinSlice = 4096;
constexpr int64_t kScoreHistMaxSlices = 1024;
constexpr int kScoreHistWgsPerCu = 4;

struct ScoreHistJob {
    int64_t nqueries = 0, ntargets = 0;
    int num_cus = 256;
    int copies = 0;                          // "score_hist_copies": 0 = the planner's choice, or 1 / 2 / 4 LDS copies per workgroup
};

struct ScoreHistPlan {
    int64_t slices_per_query = 0, slice = 0; // (0: nothing to count)
    int64_t items = 0, grid = 0;             // nqueries x slices_per_query work items; workgroups launched
    int copies = 0; int64_t lds_bytes = 0;   // LDS histograms of a workgroup and their bytes (dynamic LDS of the launch)
    int launches = 0;
};

ScoreHistPlan plan_score_hist(const ScoreHistJob& job);

// ---- the thresholds of a hit table (sw_hits_threshold_device; sw_score_hist.hip): one workgroup of 256 threads per query.
struct HitsThresholdPlan { int64_t grid = 0; int launches = 0; };
HitsThresholdPlan plan_hits_threshold(int64_t nqueries);

// ---- the low-complexity mask of a database (sw_db_mask_low_complexity; sw_mask.hip).  The work is FLAT over the `letters` concatenated
// bytes of the handle, whatever the targets' lengths: the last W - 1 starts of every target are invalid, so a run of low windows never
// crosses a target's end and a position needs no target index, only to know where targets end.  Tile i of the `tiles` holds the
// positions [i x kMaskTile, min(letters, (i + 1) x kMaskTile)): every position lies in exactly one tile.  A workgroup of 256 threads
// takes a tile (the grids are walked in strides of at most kPssmHitsGridMax workgroups); a lane of the window launch owns
// kMaskStartsPerLane consecutive starts, so its 16 bits of an array are one half-word and need no ballot.  A tile stages its bytes and
// a halo of W - 1 behind them.  The workspace holds per tile kMaskTileWords 64-bit words of each of three bit arrays -- low1, low2,
// masked; bit p % 64 of word p / 64 is position p -- then one 32-bit summary and one 32-bit carry word per tile: every word of the
// tiles at hand is written by the call before it is read, so nothing of an earlier call is seen.  Launches: windows, carries (one
// workgroup, every thread a contiguous share of the tiles), apply, and -- only with d_nmasked -- count, 256 targets per workgroup.
constexpr int64_t kMaskTile = 4096;
constexpr int kMaskStartsPerLane = 16;
constexpr int64_t kMaskTileWords = kMaskTile / 64;
constexpr int kMaskCarryThreads = 1024;          // the one workgroup of the carry launch
constexpr int kMaskCountTargets = 256;           // targets of a workgroup of the count launch: one per thread
constexpr int kMaskCountLaneWords = 8;           // ... which counts a target of up to this many words alone; a longer one takes the whole wave
constexpr int kMaskG[SW_MASK_WINDOW_MAX + 1] = {SW_MASK_G_LITERALS};   // (sw_mask_table.h; the driver hands G[W] to the kernel)
static_assert(kMaskTile == 256 * kMaskStartsPerLane, "a workgroup of 256 lanes covers a tile");

struct MaskJob {
    int64_t letters = 0, ntargets = 0;       // of the handle
    int window = 12;                         // 2..64
    bool count = true;                       // d_nmasked is given
};

struct MaskPlan {
    int64_t tile = kMaskTile; int starts_per_lane = kMaskStartsPerLane; int halo = 0;   // halo: W - 1 bytes staged behind a tile
    int64_t tiles = 0, words = 0;            // words of ONE bit array: tiles x kMaskTileWords
    int64_t low1_off = 0, low2_off = 0, mask_off = 0, summary_off = 0, carry_off = 0;   // byte offsets into the workspace
    int64_t workspace_bytes = 0;
    int64_t window_grid = 0, carry_grid = 0, apply_grid = 0, count_grid = 0;   // (0: not launched)
    int launches = 0;                        // kernel launches of the call ("last_mask_launches")
};

MaskPlan plan_mask(const MaskJob& job);

// ---- alignment of chosen hits under affine scoring (sw_align_affine_device): sw_align_affine_wave<C> for C = 4, 8, 16, its index in
// kAlignAffine (sw_api_search.hip, which checks its order against it at compile time)
constexpr int kAlignAffineKernels = 3;
constexpr int align_affine_kernel_index(int C) { return C / 8; }

struct AlignAffineJob {
    int64_t qlen = 0, maxhit = 0;            // query length, longest hit
    int64_t nhits = 0;
    int num_cus = 256;
    int per_cu[kAlignAffineKernels] = {};    // occupancy of every sw_align_affine_wave instantiation at 256 threads (workgroups per CU)
    int64_t budget_bytes = 1ll << 30;        // "align_workspace_mib": the direction workspace may take this much
};

struct AlignAffinePlan {
    bool fits = false;                       // one hit's direction matrix fits the budget (and a buffer descriptor: below 2^31 bytes)
    int C = 0;                               // query columns per lane
    int kernel = 0;                          // index of sw_align_affine_wave<C> (kAlignAffineKernels)
    int64_t nstrips = 0, qpad = 0;           // strips of 64 C columns; profile row length = row stride of a direction matrix
    int64_t bnd_per = 0;                     // per slot: boundary column between strips (ints: H and F per row), 0: one strip
    int64_t slot_bytes = 0;                  // direction matrix of a slot: longest hit x qpad
    int64_t slots = 0;                       // waves at work, each with its own slot: min(hits, resident waves, budget / slot_bytes)
    int64_t grid = 0;                        // workgroups of 4 waves
    int prof_blocks = 0;                     // sw_search_profile_submat blocks
    size_t prof_need = 0, bnd_need = 0, dir_need = 0;   // workspaces: profile (bytes), boundary columns (ints), directions (bytes)
};

AlignAffinePlan plan_align_affine(const AlignAffineJob& job);

// ---- alignment of the hits of many queries, taken from a device table (sw_db_align_affine_hits; sw_align_hits.hip):
// sw_align_hits_wave<C> for C = 4, 8, 16, its index in kAlignHits (sw_api_search.hip, which checks its order against it at compile time).
// The host knows the queries and the handle's longest target, not the targets a table names; it plans for every target the table could name.
// Groups: consecutive queries whose profiles fit the profile budget (plan_search_multi's rule; one query alone may exceed it) and whose
// entries -- queries x top, each at most one work item -- stay within max_items: that bounds the item list of a group.  The table of a
// group is laid out by class (columns per lane) like plan_search_multi's, the profiles in table order.
// Tiers: per class of a group at most kAlignHitsTiers sizes of a direction matrix.  The top tier is the worst case of the class in that
// group, longest target x the class's largest padded query length; every lower tier is kAlignHitsTierRatio times smaller, as long as it
// stays at or above kAlignHitsTierFloor bytes.  An item of len x qpad bytes goes to the smallest tier that holds it (the binning kernels
// decide by the same bounds, which they get from this plan).
// Launches: one per (class, tier) of a group, largest tier first.  The launches of a call follow each other in the stream, so every
// launch has the direction workspace to itself: slots x slot_bytes of ONE launch stay within the budget; slots are at least 1, at most
// the resident waves of the kernel, at most the entries of the class (no list is longer), and at most what the boundary columns allow
// (kSearchBndBytes, as in plan_align_affine; a tier's rows are bounded by its size over two strips' width).
// Fits: the call's worst case, longest target x the padded length of the longest query, fits the budget and a buffer descriptor.
constexpr int kAlignHitsKernels = 3;
constexpr int align_hits_kernel_index(int C) { return C / 8; }
constexpr int kAlignHitsTiers = 4;
constexpr int64_t kAlignHitsTierRatio = 4;
constexpr int64_t kAlignHitsTierFloor = 32 << 10;
constexpr int64_t kAlignHitsMaxItems = 1 << 22;      // entries of a group: 24 bytes of list each (96 MiB)

struct AlignHitsJob {
    const int64_t* qlens = nullptr;          // length of every query, input order
    int64_t nqueries = 0, top = 1;
    int64_t longest = 0;                     // of the handle: longest target
    int num_cus = 256;
    int per_cu[kAlignHitsKernels] = {};      // occupancy of every sw_align_hits_wave instantiation at 256 threads (workgroups per CU)
    int64_t profile_budget_bytes = 256ll << 20;   // "search_profile_mib"
    int64_t budget_bytes = 1ll << 30;        // "align_workspace_mib": the direction workspace may take this much
    int64_t max_items = kAlignHitsMaxItems;  // (tests lower it)
};

struct AlignHitsClass {
    int64_t q0 = 0, nq = 0;                  // its queries: entries q0 .. q0 + nq - 1 of the table
    int64_t item0 = 0, entries = 0;          // its part of the group's item list: first item, nq * top items at most
    int64_t qpad = 0, nstrips = 0;           // the largest padded query length and the most strips among its queries
    int ntiers = 0;                          // 0: no query of this class in the group
    int log_band = 0;                        // plan_align_hits_ckpt: band height 2^log_band rows, the bounds are align_ckpt_slot_bytes (0: len x qpad)
    int64_t bound[kAlignHitsTiers] = {};     // ascending: tier t holds the items of at most bound[t] bytes (and more than bound[t - 1])
};
struct AlignHitsGroup {
    int64_t q0 = 0, nq = 0, prof_bytes = 0;  // the queries q0 .. q0 + nq - 1 = the table entries q0 .. q0 + nq - 1, by class
    AlignHitsClass cls[kAlignHitsKernels];
};
struct AlignHitsLaunch {
    int group = 0, C = 0, kernel = 0, tier = 0;
    int log_band = 0;                        // plan_align_hits_ckpt: the class's band height, 2^log_band rows (0: whole matrices)
    int64_t slot_bytes = 0, slots = 0;       // the tier's bound; waves at work, each with its own slot
    int64_t bnd_per = 0;                     // per slot: boundary pairs between strips (ints), 0: every query of the class has one strip
    int64_t grid = 0;                        // workgroups of 4 waves
};

struct AlignHitsPlan {
    bool fits = false;
    int64_t worst_qpad = 0, worst_bytes = 0; // the padded length of the longest query; longest target x that
    std::vector<swk::MultiQuery> table;      // as SearchMultiPlan::table
    std::vector<AlignHitsGroup> group;
    std::vector<AlignHitsLaunch> launch;     // in the order they are enqueued: group after group, per class the largest tier first
    int64_t tiers = 0, slots = 0;            // tiers planned (= launches) and the sum of their slots
    size_t prof_need = 0, bnd_need = 0, dir_need = 0, items_need = 0;   // workspaces: profiles (bytes), boundary columns (ints), directions (bytes), items
};

AlignHitsPlan plan_align_hits(const AlignHitsJob& job);

// ---- checkpointed alignment ("align_checkpoint"; sw_align_ckpt.hip): the same alignments from a slot that holds ONE band of B rows
// of direction bytes and a checkpoint row (H and E of every column, 8 bytes each) per band boundary, instead of len x qpad bytes.
// B is a power of two in [kAlignCkptMinRows, kAlignCkptMaxRows]; len <= B is one band, no checkpoint: the whole-matrix layout.
constexpr int64_t kAlignCkptMinRows = 64, kAlignCkptMaxRows = 1 << 20;
// The planner's own choice never goes below this: a band pays the 63 steps of lane skew whatever its height -- 20 % of its steps at
// 256 rows, 50 % at 64.  Reasoned from that ratio, not measured.  ("align_checkpoint_rows" may force less: the tests do.)
constexpr int64_t kAlignCkptFloorRows = 256;
constexpr int64_t kAlignSlotLimit = (1ll << 31) - 256;   // a slot is addressed through buffer descriptors with 32-bit offsets

// Bytes of a slot for a hit of `len` rows (an empty hit counts as one row) against a query padded to qpad, at band height B.  The one
// statement of the layout: the planners size by it, the binning kernels sort by it, sw_align_ckpt.hip lays a slot out by it.
constexpr int64_t align_ckpt_slot_bytes(int64_t len, int64_t qpad, int64_t B) {
    const int64_t rows = len < 1 ? 1 : len;
    return qpad * ((rows < B ? rows : B) + 8 * ((rows + B - 1) / B - 1));
}

// "align_checkpoint": 0 whole matrices, 1 checkpointed, 2 checkpointed for exactly the calls that 0 would refuse for size.
constexpr bool align_use_ckpt(int64_t mode, bool whole_fits) { return mode == 1 || (mode == 2 && !whole_fits); }

// The band height for hits of at most `len` rows: forced_rows if not 0 (a power of two in range: the caller has checked); otherwise
// the power of two at or above kAlignCkptFloorRows that makes the slot smallest -- more slots, more hits in flight --, the larger one
// among equals.  fits: that slot is within the budget and kAlignSlotLimit (no admissible B gives a smaller one).
struct AlignCkptBand {
    int64_t rows = 0; int log_rows = 0;
    int64_t slot_bytes = 0;
    bool fits = false;
};
AlignCkptBand align_ckpt_band(int64_t len, int64_t qpad, int64_t forced_rows, int64_t budget_bytes);

struct AlignCkptJob : AlignAffineJob {       // per_cu: of the sw_align_ckpt_wave instantiations
    int64_t band_rows = 0;                   // "align_checkpoint_rows": 0 = the planner's choice
};
struct AlignCkptPlan : AlignAffinePlan {     // slot_bytes: align_ckpt_slot_bytes of the longest hit; bnd_per: of one band's rows
    int64_t band_rows = 0; int log_band = 0;
};
AlignCkptPlan plan_align_ckpt(const AlignCkptJob& job);

// The hit-table call, checkpointed: plan_align_hits with another size function.  Every class of a group gets one band height, chosen
// for the handle's longest target and the class's largest padded query; its top tier is the slot of that worst case, the lower tiers
// follow by kAlignHitsTierRatio / kAlignHitsTierFloor, and an item goes to the smallest tier that holds align_ckpt_slot_bytes(its
// length, its query's qpad, the class's band).  A boundary column is a band's.  Fits: the worst case's smallest slot fits; worst_bytes
// is that slot.  per_cu: of the sw_align_hits_ckpt_wave instantiations.
struct AlignHitsCkptJob : AlignHitsJob {
    int64_t band_rows = 0;                   // "align_checkpoint_rows": 0 = the planner's choice
};
AlignHitsPlan plan_align_hits_ckpt(const AlignHitsCkptJob& job);

// The order of the hits: by decreasing length, ties in the caller's order; items[k].idx is the position in `hits` (empty hits are kept:
// they get their all-zero alignment from the kernel like any other).
void align_schedule(const int64_t* offsets, const int64_t* hits, int64_t nhits, swk::SearchItem* items);

// The schedule: the non-empty targets of offsets[0 .. ntargets], by decreasing length, ties in input order, written to items.
void search_schedule(const int64_t* offsets, int64_t ntargets, swk::SearchItem* items);

}  // namespace swp
