// sw_ctx.h -- what the files of the C-ABI driver share (library-internal): the context, the per-device launch order, the workspace
// helpers and the prototypes of the library-internal functions.  sw_api.hip (context, options, traceback), sw_api_fill.hip (fills and
// batches), sw_api_search.hip (the search family) and sw_place.hip (the output allocator) carry the plans of sw_plan.cpp out on it.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <iterator>
#include <map>
#include <mutex>
#include "sw_kernels.h"
#include "sw_plan.h"

#define SW_HIDDEN __attribute__((visibility("hidden")))   // shared among the driver's files without joining the library's exported symbols
namespace swh {   // sw_host.cpp
void set_err(const char* fmt, ...);
int check_search_affine(const char* who, int64_t qlen, const int64_t* offsets, int64_t ntargets, const sw_affine* sc, int64_t* maxlen_out,
                        int64_t* nonempty_out);
int check_align_affine(const char* who, const int64_t* offsets, int64_t ntargets, const int64_t* hits, int64_t nhits, const void* aln, const void* ops,
                       int64_t ops_cap, int64_t* maxhit_out);
int check_search_multi(const char* who, const int64_t* qoffsets, int64_t nqueries, int64_t longest_target, const sw_affine* sc, int64_t* maxq_out);
SW_HIDDEN int check_search_pssm(const char* who, const int64_t* qoffsets, int64_t nqueries, int64_t longest_target, const sw_pssm_scoring* sc,
                                int64_t* maxq_out, unsigned char (&code)[256]);
int check_prefilter(const char* who, int64_t min_score, const void* pairs, int64_t pairs_cap, const void* npairs, const void* scores);
int check_align_hits(const char* who, int64_t top, const void* hits, const void* aln, const void* ops, int64_t ops_cap);
SW_HIDDEN int check_pssm_update(const char* who, const sw_pssm_update* upd, int64_t top, const void* hits, const void* aln, const void* ops, int64_t ops_cap,
                                const void* out, const void* counts);                                 // sw_hits_host.cpp
SW_HIDDEN int check_pssm_weighting(const char* who, const sw_pssm_weighting* wt, int64_t top, const void* hits, const void* aln, const void* ops,
                                   int64_t ops_cap, const void* weights);                             // sw_hits_host.cpp
SW_HIDDEN int check_msa(const char* who, const int64_t* qoffsets, int64_t nqueries, int64_t top, const void* hits, const void* aln, const void* ops,
                        int64_t ops_cap, const void* cols, const void* rows, const void* a3m, int64_t a3m_cap, const void* a3m_bytes);   // sw_hits_host.cpp
SW_HIDDEN int check_msa_filter(const char* who, const int64_t* qoffsets, int64_t nqueries, int64_t top, const void* cols, const sw_msa_filter* filter,
                               const void* hits, const void* hits_out, const void* keep);            // sw_hits_host.cpp
SW_HIDDEN int check_score_hist(const char* who, const void* results, int64_t nqueries, int64_t ntargets, int shift, const void* hist);   // sw_score_stats.cpp
SW_HIDDEN int check_hits_threshold(const char* who, const void* thresholds, int64_t nqueries, int64_t ntargets, int64_t top, const void* hits,
                                   const void* hits_out, const void* keep);                          // sw_score_stats.cpp
SW_HIDDEN int check_mask_params(const char* who, const sw_mask_params* mp, int32_t* bound1, int32_t* bound2, unsigned char (&cls)[256]);   // sw_mask_host.cpp
SW_HIDDEN void pssm_update_table(const sw_submat* sub, const char* letters, int n, int8_t* S);        // sw_hits_host.cpp
SW_HIDDEN int check_targets(const char* who, int64_t qlen, const int64_t* offsets, int64_t ntargets, int64_t* maxlen_out, int64_t* nonempty_out);
}
using swh::set_err;
extern "C" {
int sw_place_pair_ratio(void* d_X, size_t xbytes, void* d_Y, size_t ybytes, float* ratio, float* ms_together);   // sw_place.hip
int sw_traceback_stop_device(sw_ctx* c, void* d_P, int p_elem_bytes, int64_t cols, int64_t rows, int64_t max_pos, sw_result* d_result, int64_t* d_stop,
                             void* stream);   // sw_api.hip
int sw_fill_band_reserve(sw_ctx* c, int64_t cols, int64_t rows, int64_t total_rows, const sw_scores* scores, int h_elem_bytes, int p_elem_bytes, int want_h,
                         void* stream);       // sw_api_fill.hip
}

#define HIP_TRY(expr)                                                                 \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess) {                                                       \
            set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return SW_EDEVICE;                                                        \
        }                                                                             \
    } while (0)

// Fills of one device are serialised.  The systolic kernel's workgroups spin on hand-offs from other workgroups, so
// every workgroup of a launch must be resident; two fills in flight on one device (two contexts, or one context on
// two streams) could each hold part of the CUs and wait for the rest forever.  Launches therefore happen under a
// per-device lock, and a fill enqueued on a different stream than the previous one first waits (on the device, not
// the host) for everything enqueued on that previous stream.
struct DevState {
    std::mutex mu;
    bool any = false;
    hipStream_t last_stream = nullptr;
    hipEvent_t ev = nullptr;
    int concurrent_ok = 0;   // set while band launches that partition the CUs explicitly are being enqueued
};
extern SW_HIDDEN DevState g_dev[64];   // sw_api.hip

// A launch table: every instantiation beside the index the planner gives it, checked at compile time to sit at that index.
template <typename K> struct Indexed { int index; K k; };
template <typename K, size_t N> constexpr bool at_their_indices(const Indexed<K> (&t)[N]) {
    for (size_t i = 0; i < N; ++i)
        if (t[i].index != (int)i) return false;
    return true;
}

// The occupancy of every instantiation of a launch table at 256 threads (workgroups per CU), asked once per context: the plans' columns
// per lane and grids depend on it.  once() is the one way in; the jobs and device_facts read it like the plain array it stands for.
template <size_t N> class Occupancy {
    int per_cu[N] = {};
    bool known = false;
public:
    template <typename K> int once(const Indexed<K> (&tab)[N]) {
        if (known) return SW_OK;
        for (size_t k = 0; k < N; ++k) HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu[k], tab[k].k, 256, 0));
        known = true;
        return SW_OK;
    }
    int operator[](size_t k) const { return per_cu[k]; }
    const int* begin() const { return per_cu; }
    const int* end() const { return per_cu + N; }
};

// A device buffer of the context, freed with it; reads like the pointer it holds.  grow: to `need` elements of Elem bytes (+ `slack`
// bytes) -- waits for the stream (launches in flight may still read the old one), frees it and allocates afresh; `fresh` says whether
// the last grow did: the caller wipes what must start zeroed.  once: a buffer of fixed size, allocated at its first use.
template <typename T, size_t Elem = sizeof(T)> struct Workspace {
    T* p = nullptr;
    size_t cap = 0;      // elements
    bool fresh = false;
    Workspace() = default;
    Workspace(const Workspace&) = delete;
    Workspace& operator=(const Workspace&) = delete;
    ~Workspace() { if (p) (void)hipFree(p); }
    operator T*() const { return p; }
    T* operator->() const { return p; }
    int grow(size_t need, hipStream_t stream, size_t slack = 0) {
        fresh = false;
        if (need <= cap) return SW_OK;
        HIP_TRY(hipStreamSynchronize(stream));
        if (p) HIP_TRY(hipFree(p));
        p = nullptr; cap = 0;
        const size_t bytes = need * Elem + slack;
        if (hipMalloc((void**)&p, bytes) != hipSuccess) { set_err("workspace allocation of %zu bytes failed", bytes); return SW_ENOMEM; }
        cap = need; fresh = true;
        return SW_OK;
    }
    int once(size_t bytes) { if (!p) HIP_TRY(hipMalloc((void**)&p, bytes)); return SW_OK; }
};

// A device buffer and the pinned host copy it is uploaded from, grown together to `need` elements (the caller has waited for the last
// upload from the pinned copy); `who` names the call in the text of a failed allocation.  once: the pair at a fixed size.
template <typename T> struct Staged {
    T* d = nullptr;
    T* h = nullptr;
    size_t cap = 0;
    Staged() = default;
    Staged(const Staged&) = delete;
    Staged& operator=(const Staged&) = delete;
    ~Staged() { if (d) (void)hipFree(d); if (h) (void)hipHostFree(h); }
    int grow(size_t need, hipStream_t stream, const char* who) {
        if (need <= cap) return SW_OK;
        HIP_TRY(hipStreamSynchronize(stream));
        if (d) HIP_TRY(hipFree(d));
        if (h) HIP_TRY(hipHostFree(h));
        d = nullptr; h = nullptr; cap = 0;
        if (hipMalloc((void**)&d, need * sizeof(T)) != hipSuccess || hipHostMalloc((void**)&h, need * sizeof(T), 0) != hipSuccess) {
            set_err("%s: workspace allocation failed", who);
            return SW_ENOMEM;
        }
        cap = need;
        return SW_OK;
    }
    int once() {
        if (!d) HIP_TRY(hipMalloc((void**)&d, sizeof(T)));
        if (!h) HIP_TRY(hipHostMalloc((void**)&h, sizeof(T), 0));
        return SW_OK;
    }
};

struct SW_HIDDEN sw_ctx {
    int device = 0;
    int num_cus = 256;
    bool xcd_round_robin = false;       // sw_xcc_probe saw workgroup i on XCD i % 8 (8 XCDs of 32 CUs)
    Workspace<unsigned char> d_alpha;     // [64..323] letter code table + letter count; [512..1535] XCD of every workgroup of the running launch (sw_systolic2, xcd_mode)
    Workspace<unsigned int> d_part;       // sw_prep_scan: one 256-bit presence map of byte values per block (up to 2048 blocks)
    int64_t opt_dbg_ptr = 0;
    swp::PlanOptions opt;               // the options the planners read (sw_set_option; include/swhip.h)
    // ---- fills (sw_api_fill.hip)
    unsigned epoch = 0;                 // 12-bit launch tag, see FillParams::tag_base
    Workspace<unsigned long long> d_edge;   // (granules)
    Workspace<unsigned long long> d_key; // [0] = arg-max key, [1] low word = abort flag
    Workspace<unsigned char, 4> d_cb;   // systolic engine: padded copies of b (bytes, 16-bit, letter codes; sw_pad_b): 4 bytes per element
    Workspace<unsigned int> d_edge4;    // perm producer: lane-63 columns as self-tagged 4-byte values
    unsigned epoch8 = 0;                // 8-bit launch tag of those values
    Workspace<unsigned int> d_sync;       // one-launch fills (sw_systolic2's prologue / epilogue): barrier and exit counters, presence map; zero between launches
    Workspace<unsigned char> d_priv;      // ... and every workgroup's own padded copy of b + letter codes
    bool key_dirty = false;             // d_key was left non-zero by a launch that does not re-arm it (everything but the one-launch fill)
    bool last_fused = false;            // the last launch_fill reports by itself (no sw_finalize behind it)
    swp::FillPlan last_plan;            // the plan of the last fill (sw_get_option "last_*")
    int64_t last_grid = 0;              // ... and the grid of its one-column kernel after the occupancy cap
    int s2_per_cu = 0;                  // occupancy of sw_systolic2 at 768 threads (queried at the first fill)
    struct { int threads, per_cu; } sys_occ[8][2] = {};   // occupancy of every sw_systolic instantiation (kSystolic x int32 / int64 H) at the workgroup size last asked about
    int64_t opt_xcd_order = 0;          // systolic: 1 = neighbouring strip groups on one XCD
    int64_t opt_pace_ps = 0;            // systolic: pacing of strip 0 (ps per row; 0 = off)
    int64_t opt_band_wait_ms = 20000;   // band-resident launch: patience of the top-halo poll
    // ---- batches (sw_api_fill.hip)
    Workspace<unsigned long long> d_keys;      // the fall-back: one key per pair
    Workspace<unsigned char> d_bcodes;         // batch kernel: padded letter codes of every pair's b
    Workspace<int> d_bnd;                      // batch kernel: boundary columns between strips (ints)
    int64_t opt_batch_lds = 0;          // batch kernel: dynamic LDS bytes per workgroup (caps the waves per CU; experiments)
    int64_t last_batch_kernel = 0;      // 1: the last sw_batch_device call ran on sw_batch_wave (one pair per wave)
    // ---- the search family (sw_api_search.hip).  Shared by its three calls: profile of the query, per-wave boundary columns, the schedule
    // and the substitution matrix (each on the device + a pinned host copy it is uploaded from), the work counter.  sitems_ev is recorded
    // behind the uploads of a call; the next call waits for it before it overwrites the pinned copies (stage_search_call).
    Workspace<signed char> d_sprof;
    Workspace<int> d_sbnd;
    Staged<swk::SearchItem> sitems;
    Staged<sw_submat> submat;
    hipEvent_t sitems_ev = nullptr;
    Workspace<unsigned int> d_sctr;
    int64_t last_search_grid = 0;       // workgroups of the last search launch
    int64_t last_search_kernel = 0;     // its kernel: index in kSearch (swp::search_kernel_index)
    Occupancy<swp::kSearchKernels> search_per_cu;  // of every sw_search_wave instantiation, queried at the first search
    int64_t last_search_affine_grid = 0;    // workgroups of the last affine search launch
    int64_t last_search_affine_kernel = 0;  // its kernel: index in kSearchAffine (swp::search_affine_kernel_index)
    Occupancy<swp::kSearchAffineKernels> search_affine_per_cu;  // of every sw_search_affine_wave instantiation, queried at the first affine search
    // alignment of hits (sw_align_affine_device): one direction matrix per wave at work
    Workspace<unsigned char> d_adir;
    int64_t opt_align_workspace_mib = 1024;
    int64_t last_align_affine_kernel = 0, last_align_affine_slots = 0;
    Occupancy<swp::kAlignAffineKernels> align_affine_per_cu;    // of every sw_align_affine_wave instantiation, queried at the first call
    // checkpointed alignment (sw_align_ckpt.hip) of both alignment calls: 0 whole matrices, 1 always, 2 where 0 would refuse for size
    int64_t opt_align_checkpoint = 0, opt_align_checkpoint_rows = 0;
    int64_t last_align_affine_checkpointed = 0, last_align_affine_band_rows = 0, last_align_affine_slot_bytes = 0;
    int64_t last_align_hits_checkpointed = 0, last_align_hits_band_rows = 0;
    Occupancy<swp::kAlignAffineKernels> align_ckpt_per_cu;      // of every sw_align_ckpt_wave instantiation, queried at the first checkpointed call
    Occupancy<swp::kAlignHitsKernels> align_hits_ckpt_per_cu;   // likewise sw_align_hits_ckpt_wave
    // alignment of the hits of many queries (sw_db_align_affine_hits): the item list of a group and the control words of its lists; the
    // profiles, the boundary columns, the query table and the direction workspace are those of the calls above
    Workspace<swk::AlignHitItem> d_ahitems;
    Workspace<swk::AlignHitsCtl> d_ahctl;
    Workspace<unsigned int> d_ahfilled;  // lists of the last call that received items, counted by the binning ("last_align_hits_lists")
    int64_t last_align_hits_launches = 0, last_align_hits_tiers = 0, last_align_hits_slots = 0;
    Occupancy<swp::kAlignHitsKernels> align_hits_per_cu;        // of every sw_align_hits_wave instantiation, queried at the first call
    // many queries against a prepared database (sw_db_search_affine): the call's query table on the device + the pinned copy it is uploaded
    // from (the protocol of sitems_ev covers it), the budget of a group's profiles
    Staged<swk::MultiQuery> mq;
    int64_t opt_search_profile_mib = 256;
    int64_t last_search_multi_groups = 0, last_search_multi_launches = 0, last_search_multi_grid = 0;   // of the last call; the grid of its last launch
    Occupancy<swp::kSearchMultiKernels> search_multi_per_cu;    // of every sw_search_affine_multi_wave instantiation, queried at the first call
    // the same search on packed 16-bit lanes (sw_search_multi16.hip): "search_lanes" (32 / 16), the packed launches of the last call
    int64_t opt_search_lanes = 32;
    int64_t last_search_multi_packed_launches = 0;
    Occupancy<swp::kSearchMultiKernels> search_multi_packed_per_cu;   // of every sw_search_multi_pk_wave instantiation, queried at the first call
    // a pair list against a prepared database (sw_db_search_affine_pairs): the items of a chunk and the control words of a (chunk, group);
    // the profiles, the boundary columns and the query table are those of the calls above (the table carries entry_of behind its entries)
    Workspace<swk::SearchPairItem, 1> d_spitems;                // (grown in bytes)
    Workspace<swk::SearchPairsCtl> d_spctl;
    int64_t opt_search_pairs_chunk = swp::kSearchPairsChunk;
    int64_t last_search_pairs_groups = 0, last_search_pairs_chunks = 0, last_search_pairs_launches = 0;
    Occupancy<swp::kSearchPairsKernels> search_pairs_per_cu;    // of every sw_search_affine_pairs_wave instantiation, queried at the first call
    // the same call on packed 16-bit lanes (sw_search_pairs16.hip): "search_pairs_lanes" (32 / 16), the cell workspace of a (chunk, group)
    // -- control words, then count, cursor and base of every cell --, the two-pair items the device built in the last call, its packed launches
    int64_t opt_search_pairs_lanes = 32;
    Workspace<unsigned char> d_spcells;
    Workspace<unsigned long long> d_sptotal;                    // "last_search_pairs_packed_items"
    int64_t last_search_pairs_packed_launches = 0;
    Occupancy<swp::kSearchPairsKernels> search_pairs_packed_per_cu;   // of every sw_search_pairs_pk_wave instantiation, queried at the first call
    // the ungapped pre-filter (sw_db_prefilter_ungapped): its control words, "prefilter_lanes", what the last call did
    Workspace<swk::PrefilterCtl> d_pfctl;
    int64_t opt_prefilter_lanes = 0;
    int64_t last_prefilter_groups = 0, last_prefilter_launches = 0, last_prefilter_packed_launches = 0;
    Occupancy<swp::kPrefilterKernels> prefilter_per_cu;         // of every sw_prefilter_wave / _wave16 instantiation, queried at the first call
    // the best targets per query (sw_top_hits_device, sw_db_search_affine_top): the result rows of a chunk, the histograms and the
    // per-row states of the radix select
    Workspace<sw_result> d_tres;
    Workspace<unsigned int> d_thist;
    Workspace<swk::TopState> d_tstate;
    int64_t opt_search_results_mib = 1024;
    int64_t last_search_top_chunks = 0, last_search_top_kernel = 0;
    int top_hist_per_cu = 0;                                    // occupancy of sw_top_hist at 256 threads, queried at the first call
    // the best entries per query of a pair list (sw_top_hits_pairs_device): the segments' keys and positions, the per-query counts and
    // offsets; sw_db_search_affine_top_prefiltered keeps its list and the list's results (16 + 24 bytes per entry) in d_tplist
    Workspace<unsigned long long> d_tpkeys;
    Workspace<unsigned int> d_tppos;
    Workspace<unsigned int> d_tpseg;
    Workspace<unsigned char, sizeof(sw_pair) + sizeof(sw_result)> d_tplist;   // (grown in entries)
    int64_t last_top_pairs_launches = 0, last_top_pairs_kernel = 0;
    // the next PSSM from aligned hits (sw_db_pssm_from_hits): the call's table -- S, the code table, the query offsets -- on the device +
    // TWO pinned copies it is uploaded from in turn: phtab_ev[i] is recorded behind the upload from copy i, and a call waits for the event
    // of the copy it is about to overwrite -- the upload of the call before the last one --, so a loop can be enqueued one call ahead
    Workspace<unsigned char> d_phtab; unsigned char* h_phtab[2] = {nullptr, nullptr};   // (released by sw_destroy beside their events)
    hipEvent_t phtab_ev[2] = {nullptr, nullptr};
    int phtab_turn = 0;
    int64_t last_pssm_hits_launches = 0;
    // the weights of aligned hits (sw_db_pssm_hit_weights): the entries' accumulators; its small table -- the code table, the query
    // offsets -- goes through d_phtab and the two pinned copies above, in the same turns
    Workspace<unsigned long long> d_pwacc;
    int64_t last_pssm_weights_launches = 0, last_pssm_weights_tiles = 0;   // ... and the tiles of its longest query
    // the alignment rows of aligned hits (sw_db_msa_from_hits): the sums, then offsets, of its scan chunks; the query offsets go through
    // d_phtab and the two pinned copies above, in the same turns
    Workspace<long long> d_msasum;
    int64_t last_msa_hits_launches = 0;
    // the filter of the column rows (sw_msa_filter_device): the bit planes of a chunk of queries, at most "msa_filter_workspace_mib"; the
    // query offsets go through d_phtab and the two pinned copies above, in the same turns
    Workspace<unsigned long long> d_msafilt;
    int64_t opt_msa_filter_workspace_mib = 256;
    int64_t last_msa_filter_launches = 0, last_msa_filter_chunks = 0;
    // the score histogram (sw_score_hist_device, the _top_stats searches) and the thresholds of a hit table: no workspace; the LDS
    // copies per workgroup ("score_hist_copies": 0 = the planner's choice) and what the last call did
    int64_t opt_score_hist_copies = 0;
    int64_t last_score_hist_launches = 0, last_score_hist_slices = 0;
    int score_hist_lds_set = 0;         // the dynamic-LDS limit the kernel has been given (bytes)
    // the low-complexity mask (sw_db_mask_low_complexity): the three bit arrays, the summaries and the carries of swp::plan_mask
    Workspace<unsigned char> d_mask;
    int64_t last_mask_launches = 0, last_mask_tiles = 0;
    // ---- placement of the output matrices (sw_place.hip)
    int64_t opt_place_hold_gib = 0;     // sw_alloc_outputs: GiB a pair of small matrices may hold beside itself where no plain candidate is good (0: none)
    int64_t opt_place_budget_ms = 1500; // sw_alloc_outputs: time the search for a P in another class of the HBM may take
    int place_spacer_gib = 0;           // ... the spacer that led to one last time
    int64_t last_place_held_gib = 0;
    float last_place_ratio = 0.f;       // ... two-stream / one-stream time of the pair handed out last (~1.3-1.45: different classes, ~2: one class)
    std::map<void*, void*> out_base;    // sw_alloc_outputs: pointer handed out -> allocation to free
    std::map<void*, float> pair_ratio;  // ... P handed out -> the store probe's ratio of its pair (~1.4: two classes of the HBM, ~2: one)
};

// A prepared database (sw_db_create): the caller's device bytes, borrowed, the search schedule of its targets on the device -- what
// every search of it needs and no query changes -- and the offsets themselves: the schedule is ordered by length, and the alignment of
// a hit table (sw_db_align_affine_hits) has to get from a target INDEX to that target's bytes.
struct SW_HIDDEN sw_db {
    int device = 0;
    const char* d_db = nullptr;
    int64_t ntargets = 0, nonempty = 0, longest = 0, letters = 0, first = 0;   // first: offsets[0]
    swk::SearchItem* d_items = nullptr;  // the nonempty targets, longest first (swp::search_schedule)
    int64_t* d_offsets = nullptr;        // the ntargets + 1 offsets, the caller's order
};

constexpr sw_scores kDefaultScores = {3, -3, -2};  // serial_smithW.c:59-61

// gr, gc: extent (rows, cols) of the WHOLE matrix the values may come from (== rows, cols unless this is a tile or a
// band whose halo carries scores accumulated outside it)
static inline int check_dims(int64_t cols, int64_t rows, const sw_scores* sc, int64_t gc = -1, int64_t gr = -1) {
    if (gc < cols) gc = cols;
    if (gr < rows) gr = rows;
    if (cols < 0 || rows < 0 || cols > swk::SW_MAX_DIM || rows > swk::SW_MAX_DIM || gc > swk::SW_MAX_DIM || gr > swk::SW_MAX_DIM) {
        set_err("dimensions out of range: cols=%lld rows=%lld (max %lld)", (long long)cols, (long long)rows,
                (long long)swk::SW_MAX_DIM);
        return SW_EINVAL;
    }
    if (sc->gap > 0) { set_err("gap score must be <= 0 (got %d)", sc->gap); return SW_EINVAL; }
    if (sc->match < 0) { set_err("match score must be >= 0 (got %d)", sc->match); return SW_EINVAL; }
    if (sc->mismatch > sc->match) { set_err("mismatch score must not exceed the match score"); return SW_EINVAL; }
    const int64_t lo = std::min(gc, gr);
    // largest G-space magnitude: H <= match*min(dims) plus -gap*(row+col); the per-step constants ride on top
    const int64_t gmax = (int64_t)sc->match * lo + (int64_t)(-sc->gap) * (rows + cols + 2);
    const int64_t step = std::max<int64_t>(std::llabs((int64_t)sc->mismatch), (int64_t)sc->match) + 2 * (int64_t)(-sc->gap);
    if (gmax + step >= (1ll << 31) || step >= (1ll << 24) || (int64_t)sc->match * lo >= (1ll << 24)) {
        set_err("scores too large for this problem size (32-bit cell / 24-bit arg-max key)");
        return SW_EINVAL;
    }
    return SW_OK;
}

static inline swp::DeviceFacts device_facts(const sw_ctx* c) {
    swp::DeviceFacts dev;
    dev.num_cus = c->num_cus; dev.xcd_round_robin = c->xcd_round_robin; dev.s2_per_cu = c->s2_per_cu;
    std::copy(std::begin(c->search_per_cu), std::end(c->search_per_cu), dev.search_per_cu);
    return dev;
}

// called with g_dev[device].mu held: make `stream` wait for the fill enqueued last on another stream of this device.  The
// event is recorded on a fill's OWN stream when the fill has been enqueued (DevOrder's destructor), never on the previous
// stream later on: that stream may have been destroyed by then.
static inline int order_after_previous_fill(DevState& d, hipStream_t stream, bool allow_concurrent) {
    if (d.any && d.last_stream != stream && !allow_concurrent && d.ev) HIP_TRY(hipStreamWaitEvent(stream, d.ev, 0));
    return SW_OK;
}

struct DevOrder {   // RAII: device lock + stream ordering for one fill call
    std::unique_lock<std::mutex> lk;
    DevState& d;
    hipStream_t stream;
    int rc;
    DevOrder(sw_ctx* c, hipStream_t st, bool concurrent) : lk(g_dev[c->device & 63].mu), d(g_dev[c->device & 63]), stream(st) {
        rc = order_after_previous_fill(d, stream, concurrent);
    }
    ~DevOrder() {
        if (!d.ev && hipEventCreateWithFlags(&d.ev, hipEventDisableTiming) != hipSuccess) { d.ev = nullptr; (void)hipGetLastError(); }
        if (d.ev && hipEventRecord(d.ev, stream) == hipSuccess) { d.any = true; d.last_stream = stream; }
        else { (void)hipGetLastError(); d.any = false; }
    }
};
