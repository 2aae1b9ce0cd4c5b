// sw_api.hip -- C-ABI entry points that drive the HIP kernels (see include/swhip.h).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "sw_kernels.h"
#include "sw_plan.h"

namespace swh {
void set_err(const char* fmt, ...);
int check_search_affine(const char* who, int64_t qlen, const int64_t* offsets, int64_t ntargets, const sw_affine* sc, int64_t* maxlen_out,
                        int64_t* nonempty_out);   // sw_host.cpp
int check_align_affine(const char* who, const int64_t* offsets, int64_t ntargets, const int64_t* hits, int64_t nhits, const void* aln, const void* ops,
                       int64_t ops_cap, int64_t* maxhit_out);   // sw_host.cpp
}
extern "C" int sw_place_pair_ratio(void* d_X, size_t xbytes, void* d_Y, size_t ybytes, float* ratio, float* ms_together);   // sw_place.hip
using swh::set_err;

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
static DevState g_dev[64];

struct sw_ctx {
    int device = 0;
    int num_cus = 256;
    unsigned epoch = 0;                 // 12-bit launch tag, see FillParams::tag_base
    unsigned long long* d_edge = nullptr;
    size_t edge_cap = 0;                // granules
    unsigned long long* d_key = nullptr; // [0] = arg-max key, [1] low word = abort flag
    unsigned long long* d_keys = nullptr; size_t keys_cap = 0;  // batch: one key per pair
    unsigned char* d_cb = nullptr;      // systolic engine: padded copies of b (bytes, 16-bit, letter codes; sw_pad_b)
    size_t cb_cap = 0;
    unsigned int* d_edge4 = nullptr;    // perm producer: lane-63 columns as self-tagged 4-byte values
    size_t edge4_cap = 0;               // elements
    unsigned epoch8 = 0;                // 8-bit launch tag of those values
    unsigned char* d_alpha = nullptr;   // [64..323] letter code table + letter count; [512..1535] XCD of every workgroup of the running launch (sw_systolic2, xcd_mode)
    unsigned int* d_part = nullptr;     // sw_prep_scan: one 256-bit presence map of byte values per block (up to 2048 blocks)
    unsigned int* d_sync = nullptr;     // one-launch fills (sw_systolic2's prologue / epilogue): barrier and exit counters, presence map; zero between launches
    unsigned char* d_priv = nullptr; size_t priv_cap = 0;   // ... and every workgroup's own padded copy of b + letter codes
    int64_t opt_place_hold_gib = 0;     // sw_alloc_outputs: GiB a pair of small matrices may hold beside itself where no plain candidate is good (0: none)
    int64_t opt_place_budget_ms = 1500; // sw_alloc_outputs: time the search for a P in another class of the HBM may take
    int place_spacer_gib = 0;           // ... the spacer that led to one last time
    int64_t last_place_held_gib = 0;
    float last_place_ratio = 0.f;       // ... two-stream / one-stream time of the pair handed out last (~1.3-1.45: different classes, ~2: one class)
    bool key_dirty = false;             // d_key was left non-zero by a launch that does not re-arm it (everything but the one-launch fill)
    bool last_fused = false;            // the last launch_fill reports by itself (no sw_finalize behind it)
    swp::PlanOptions opt;               // the options the fill planner reads (sw_set_option; include/swhip.h)
    swp::FillPlan last_plan;            // the plan of the last fill (sw_get_option "last_*")
    int64_t last_grid = 0;              // ... and the grid of its one-column kernel after the occupancy cap
    int s2_per_cu = 0;                  // occupancy of sw_systolic2 at 768 threads (queried at the first fill)
    struct { int threads, per_cu; } sys_occ[8][2] = {};   // occupancy of every sw_systolic instantiation (kSystolic x int32 / int64 H) at the workgroup size last asked about
    int64_t opt_xcd_order = 0;          // systolic: 1 = neighbouring strip groups on one XCD
    int64_t opt_pace_ps = 0;            // systolic: pacing of strip 0 (ps per row; 0 = off)
    int64_t opt_dbg_ptr = 0;
    int64_t opt_band_wait_ms = 20000;   // band-resident launch: patience of the top-halo poll
    unsigned char* d_bcodes = nullptr; size_t bcodes_cap = 0;   // batch kernel: padded letter codes of every pair's b
    int* d_bnd = nullptr; size_t bnd_cap = 0;                   // batch kernel: boundary columns between strips (ints)
    int64_t opt_batch_lds = 0;          // batch kernel: dynamic LDS bytes per workgroup (caps the waves per CU; experiments)
    int64_t last_batch_kernel = 0;      // 1: the last sw_batch_device call ran on sw_batch_wave (one pair per wave)
    // database search (sw_search_device): profile of the query, per-wave boundary columns, the schedule (device + a pinned host copy
    // whose upload the next call waits for before it overwrites it), the work counter
    signed char* d_sprof = nullptr; size_t sprof_cap = 0;
    int* d_sbnd = nullptr; size_t sbnd_cap = 0;
    swk::SearchItem* d_sitems = nullptr; swk::SearchItem* h_sitems = nullptr; size_t sitems_cap = 0;
    hipEvent_t sitems_ev = nullptr;
    unsigned int* d_sctr = nullptr;
    int64_t last_search_grid = 0;       // workgroups of the last search launch
    int64_t last_search_kernel = 0;     // its kernel: index in kSearch (swp::search_kernel_index)
    int search_per_cu[swp::kSearchKernels] = {};   // occupancy of every sw_search_wave instantiation at 256 threads ...
    bool search_per_cu_known = false;              // ... queried at the first search
    // affine search (sw_search_affine_device): it shares the workspaces above; its own are the substitution matrix (device + a pinned
    // host copy under the schedule's event: both uploads of a call are behind sitems_ev when it is recorded)
    signed char* d_submat = nullptr; signed char* h_submat = nullptr;
    int64_t last_search_affine_grid = 0;    // workgroups of the last affine search launch
    int64_t last_search_affine_kernel = 0;  // its kernel: index in kSearchAffine (swp::search_affine_kernel_index)
    int search_affine_per_cu[swp::kSearchAffineKernels] = {};   // occupancy of every sw_search_affine_wave instantiation at 256 threads ...
    bool search_affine_per_cu_known = false;                    // ... queried at the first affine search
    // alignment of hits (sw_align_affine_device): the search's workspaces plus one direction matrix per wave at work
    unsigned char* d_adir = nullptr; size_t adir_cap = 0;
    int64_t opt_align_workspace_mib = 1024;
    int64_t last_align_affine_kernel = 0, last_align_affine_slots = 0;
    int align_affine_per_cu[swp::kAlignAffineKernels] = {};     // occupancy of every sw_align_affine_wave instantiation at 256 threads ...
    bool align_affine_per_cu_known = false;                     // ... queried at the first call
    bool xcd_round_robin = false;       // sw_xcc_probe saw workgroup i on XCD i % 8 (8 XCDs of 32 CUs)
    std::map<void*, void*> out_base;    // sw_alloc_outputs: pointer handed out -> allocation to free
    std::map<void*, float> pair_ratio;  // ... P handed out -> the store probe's ratio of its pair (~1.4: two classes of the HBM, ~2: one)
};

// A launch table: every instantiation beside the index the planner gives it, checked at compile time to sit at that index.
template <typename K> struct Indexed { int index; K k; };
template <typename K, size_t N> constexpr bool at_their_indices(const Indexed<K> (&t)[N]) {
    for (size_t i = 0; i < N; ++i)
        if (t[i].index != (int)i) return false;
    return true;
}

extern "C" {

int sw_create(int device, sw_ctx** out) {
    if (!out) { set_err("sw_create: out is NULL"); return SW_EINVAL; }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { set_err("sw_create: no HIP device"); return SW_ENODEV; }
    if (device < 0 || device >= n) { set_err("sw_create: device %d out of range (%d)", device, n); return SW_EINVAL; }
    HIP_TRY(hipSetDevice(device));
    sw_ctx* c = new sw_ctx();
    c->device = device;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    c->num_cus = prop.multiProcessorCount;
    HIP_TRY(hipMalloc((void**)&c->d_key, 64));
    HIP_TRY(hipMemset(c->d_key, 0, 64));
    HIP_TRY(hipMalloc((void**)&c->d_alpha, 2048));
    HIP_TRY(hipMemset(c->d_alpha, 0, 2048));
    HIP_TRY(hipMalloc((void**)&c->d_part, 2048 * 32));
    HIP_TRY(hipMalloc((void**)&c->d_sync, 256));
    HIP_TRY(hipMemset(c->d_sync, 0, 256));
    // Are the workgroups of a launch dealt round-robin to 8 XCDs of 32 CUs (workgroup i on XCD i % 8)?  The two-column kernel then
    // places every scout on the XCD of the workgroups that read its edge column (sw_systolic2.inc).
    if (c->num_cus == 256) {
        unsigned int h[256];
        hipLaunchKernelGGL(swk::sw_xcc_probe, dim3(256), dim3(768), 0, nullptr, c->d_part);
        if (hipMemcpy(h, c->d_part, sizeof h, hipMemcpyDeviceToHost) == hipSuccess) {
            c->xcd_round_robin = true;
            for (int i = 0; i < 256; ++i) c->xcd_round_robin = c->xcd_round_robin && h[i] == (unsigned)(i & 7);
        } else {
            (void)hipGetLastError();
        }
    }
    *out = c;
    return SW_OK;
}

void sw_destroy(sw_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->d_edge) (void)hipFree(c->d_edge);
    if (c->d_key) (void)hipFree(c->d_key);
    if (c->d_cb) (void)hipFree(c->d_cb);
    if (c->d_edge4) (void)hipFree(c->d_edge4);
    if (c->d_alpha) (void)hipFree(c->d_alpha);
    if (c->d_part) (void)hipFree(c->d_part);
    if (c->d_sync) (void)hipFree(c->d_sync);
    if (c->d_priv) (void)hipFree(c->d_priv);
    if (c->d_keys) (void)hipFree(c->d_keys);
    if (c->d_bcodes) (void)hipFree(c->d_bcodes);
    if (c->d_bnd) (void)hipFree(c->d_bnd);
    if (c->sitems_ev) { (void)hipEventSynchronize(c->sitems_ev); (void)hipEventDestroy(c->sitems_ev); }
    if (c->d_sprof) (void)hipFree(c->d_sprof);
    if (c->d_sbnd) (void)hipFree(c->d_sbnd);
    if (c->d_sitems) (void)hipFree(c->d_sitems);
    if (c->h_sitems) (void)hipHostFree(c->h_sitems);
    if (c->d_sctr) (void)hipFree(c->d_sctr);
    if (c->d_submat) (void)hipFree(c->d_submat);
    if (c->h_submat) (void)hipHostFree(c->h_submat);
    if (c->d_adir) (void)hipFree(c->d_adir);
    delete c;
}

int sw_set_option(sw_ctx* c, const char* name, int64_t v) {
    if (!c || !name) { set_err("sw_set_option: bad argument"); return SW_EINVAL; }
    if (!strcmp(name, "waves_per_block")) {
        if (v != 0 && v != 1 && v != 2 && v != 4 && v != 8) { set_err("waves_per_block must be 1,2,4,8"); return SW_EINVAL; }
        c->opt.waves_per_block = v ? v : 4;
        return SW_OK;
    }
    if (!strcmp(name, "max_blocks")) { c->opt.max_blocks = v < 0 ? 0 : v; return SW_OK; }
    if (!strcmp(name, "strips_per_group")) { c->opt.strips_per_group = v; return SW_OK; }
    if (!strcmp(name, "consumers")) { c->opt.consumers = v; return SW_OK; }
    if (!strcmp(name, "debug_flags")) { c->opt.debug_flags = v; return SW_OK; }
    if (!strcmp(name, "xcd_chain")) { c->opt.xcd_chain = v; return SW_OK; }
    if (!strcmp(name, "filler_hop_ps")) { c->opt.filler_hop_ps = v < 0 ? 0 : v; return SW_OK; }
    if (!strcmp(name, "filler_tau_ps")) { c->opt.filler_tau_ps = v < 1000 ? 1000 : v; return SW_OK; }
    if (!strcmp(name, "filler_bw_gbs")) { c->opt.filler_bw_gbs = v < 100 ? 100 : v; return SW_OK; }
    if (!strcmp(name, "pace_ps")) { c->opt_pace_ps = v; return SW_OK; }
    if (!strcmp(name, "store_policy")) { if (v < 0 || v > 2) return SW_EINVAL; c->opt.store_policy = v; return SW_OK; }
    if (!strcmp(name, "xcd_order")) { c->opt_xcd_order = v ? 1 : 0; return SW_OK; }
    if (!strcmp(name, "importers")) { if (v < 0 || v > 8) return SW_EINVAL; c->opt.importers = v; return SW_OK; }
    if (!strcmp(name, "debug_buf")) { c->opt_dbg_ptr = v; return SW_OK; }
    if (!strcmp(name, "batch_lds")) { c->opt_batch_lds = v < 0 ? 0 : v; return SW_OK; }
    if (!strcmp(name, "band_wait_ms")) { c->opt_band_wait_ms = v > 0 ? v : 20000; return SW_OK; }
    if (!strcmp(name, "align_workspace_mib")) {
        if (v < 1 || v > (1ll << 20)) { set_err("align_workspace_mib must be 1..2^20"); return SW_EINVAL; }
        c->opt_align_workspace_mib = v;
        return SW_OK;
    }
    if (!strcmp(name, "placement_budget_ms")) { c->opt_place_budget_ms = v > 0 ? v : 1500; return SW_OK; }
    if (!strcmp(name, "placement_hold_gib")) { c->opt_place_hold_gib = v < 0 ? 0 : (v > 128 ? 128 : v); return SW_OK; }
    if (!strcmp(name, "probe_foreign_pairs")) { c->opt.probe_foreign_pairs = v ? 1 : 0; return SW_OK; }
    if (!strcmp(name, "s2w")) { if (v != 0 && v != 126 && v != 110) return SW_EINVAL; c->opt.s2w = v; return SW_OK; }
    if (!strcmp(name, "split_blk")) { c->opt.split_blk = v > 0 ? v : 0; return SW_OK; }
    if (!strcmp(name, "split_from")) { c->opt.split_from = v > 0 ? v : 0; return SW_OK; }
    if (!strcmp(name, "debug_epoch8")) { c->epoch8 = (unsigned)(v & 255); return SW_OK; }   // development aid: next launch tag = v + 1
    if (!strcmp(name, "engine")) {
        if (v != 0 && v != 1) { set_err("engine must be 0 (systolic) or 1 (strip_scan)"); return SW_EINVAL; }
        c->opt.engine = v;
        return SW_OK;
    }
    set_err("sw_set_option: unknown option '%s'", name);
    return SW_EINVAL;
}

int64_t sw_get_option(sw_ctx* c, const char* name) {
    if (!c || !name) return -1;
    if (!strcmp(name, "waves_per_block")) return c->opt.waves_per_block;
    if (!strcmp(name, "max_blocks")) return c->opt.max_blocks;
    if (!strcmp(name, "engine")) return c->opt.engine;
    if (!strcmp(name, "strips_per_group")) return c->opt.strips_per_group;
    if (!strcmp(name, "consumers")) return c->opt.consumers;
    if (!strcmp(name, "store_policy")) return c->opt.store_policy;
    if (!strcmp(name, "xcd_order")) return c->opt_xcd_order;
    if (!strcmp(name, "importers")) return c->opt.importers;
    if (!strcmp(name, "pace_ps")) return c->opt_pace_ps;
    if (!strcmp(name, "band_wait_ms")) return c->opt_band_wait_ms;
    if (!strcmp(name, "num_cus")) return c->num_cus;
    if (!strcmp(name, "debug_edge4_ptr")) return (int64_t)(uintptr_t)c->d_edge4;
    if (!strcmp(name, "debug_edge4_cap")) return (int64_t)c->edge4_cap;
    if (!strcmp(name, "last_grid")) return c->last_grid;
    const swp::TilePlan& last_tile = c->last_plan.tile[c->last_plan.ntile - 1];   // (all zero where the two-column kernel did not run)
    if (!strcmp(name, "last_strips")) return c->last_plan.S;
    if (!strcmp(name, "last_strips2")) return last_tile.strips;
    if (!strcmp(name, "last_perm")) return c->last_plan.perm ? 1 : 0;
    if (!strcmp(name, "last_scouts")) return last_tile.nscout;
    if (!strcmp(name, "last_xcd_mode")) return last_tile.xcd_mode;
    if (!strcmp(name, "last_tiles")) return c->last_plan.ntile;
    if (!strcmp(name, "last_split_from")) return last_tile.split_blk ? last_tile.split_from : 0;
    if (!strcmp(name, "last_scan_all")) return last_tile.scan_all;
    if (!strcmp(name, "xcd_round_robin")) return c->xcd_round_robin ? 1 : 0;
    if (!strcmp(name, "last_batch_kernel")) return c->last_batch_kernel;
    if (!strcmp(name, "last_search_grid")) return c->last_search_grid;
    if (!strcmp(name, "last_search_kernel")) return c->last_search_kernel;
    if (!strcmp(name, "last_search_affine_grid")) return c->last_search_affine_grid;
    if (!strcmp(name, "last_search_affine_kernel")) return c->last_search_affine_kernel;
    if (!strcmp(name, "last_align_affine_kernel")) return c->last_align_affine_kernel;
    if (!strcmp(name, "last_align_affine_slots")) return c->last_align_affine_slots;
    if (!strcmp(name, "align_workspace_mib")) return c->opt_align_workspace_mib;
    if (!strcmp(name, "placement_budget_ms")) return c->opt_place_budget_ms;
    if (!strcmp(name, "placement_hold_gib")) return c->opt_place_hold_gib;
    if (!strcmp(name, "probe_foreign_pairs")) return c->opt.probe_foreign_pairs;
    if (!strcmp(name, "last_placement_held_gib")) return c->last_place_held_gib;
    if (!strcmp(name, "last_placement_ratio_x1000")) return (int64_t)(c->last_place_ratio * 1000.f);
    return -1;
}

// gr, gc: extent (rows, cols) of the WHOLE matrix the values may come from (== rows, cols unless this is a tile or a
// band whose halo carries scores accumulated outside it)
static int check_dims(int64_t cols, int64_t rows, const sw_scores* sc, int64_t gc = -1, int64_t gr = -1) {
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

// One launch of the fill: a whole matrix, a tile of a bigger matrix (row stride, halo row/column) or a
// batch of independent problems.
struct FillJob {
    const char* d_a; int64_t cols; const char* d_b; int64_t rows;
    void* d_H; int h_elem_bytes; void* d_P; int64_t stride;     // d_H / d_P may be NULL: that matrix is not written
    const int32_t* d_top; const int32_t* d_left; int32_t* d_right;
    int64_t npairs; int64_t a_pstride, b_pstride, hp_pstride;
    unsigned long long* d_keys;   // npairs packed arg-max keys (device)
    int p_elem_bytes = 4;         // 4: int32 P (reference layout); 1: compact int8 P
    // band-resident launch (sw_fill_band_device)
    const unsigned long long* d_top_gran = nullptr; unsigned long long* d_bot_gran = nullptr; unsigned int* d_bot_done = nullptr;
    unsigned int top_tag = 0, bot_tag = 0;
    int reserve_cus = 0;          // CUs left free for other kernels (halo transfers)
    bool concurrent = false;      // do not order this launch behind fills on other streams (the caller partitions the CUs)
    int64_t total_rows = 0;       // band: rows of the whole matrix (bounds the scores a halo can carry)
    bool zero_key = false;        // the preparation kernel also zeroes d_keys[0..1] (fill_one leaves that to it)
    sw_result* d_result = nullptr;   // fill_one: where the result goes (a one-launch fill writes it by itself)
    bool keep_row0 = false;       // a tile under a neighbour (sw_fill_tile_device with d_top): row 0 of H and P is the neighbour's, not written
};

// called with g_dev[device].mu held: make `stream` wait for the fill enqueued last on another stream of this device.  The
// event is recorded on a fill's OWN stream when the fill has been enqueued (DevOrder's destructor), never on the previous
// stream later on: that stream may have been destroyed by then.
static int order_after_previous_fill(DevState& d, hipStream_t stream, bool allow_concurrent) {
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

// Grows a workspace of the context to `need` elements of `elem` bytes (+ `slack` bytes): waits for the stream (launches in flight may
// still read the old one), frees it and allocates afresh.  `fresh` says whether it did: the caller wipes what must start zeroed.
static int grow_workspace(void** buf, size_t& cap, size_t need, size_t elem, size_t slack, hipStream_t stream, bool& fresh) {
    fresh = false;
    if (need <= cap) return SW_OK;
    HIP_TRY(hipStreamSynchronize(stream));
    if (*buf) HIP_TRY(hipFree(*buf));
    *buf = nullptr; cap = 0;
    const size_t bytes = need * elem + slack;
    if (hipMalloc(buf, bytes) != hipSuccess) { set_err("workspace allocation of %zu bytes failed", bytes); return SW_ENOMEM; }
    cap = need; fresh = true;
    return SW_OK;
}

static int ensure_workspaces(sw_ctx* c, const swp::FillPlan& f, hipStream_t stream) {
    bool fresh = false;
    if (int rc = grow_workspace((void**)&c->d_edge, c->edge_cap, f.edge_need, 8, 0, stream, fresh)) return rc;
    if (fresh) { HIP_TRY(hipMemsetAsync(c->d_edge, 0, c->edge_cap * 8, stream)); c->epoch = 0; }
    if (int rc = grow_workspace((void**)&c->d_cb, c->cb_cap, f.cb_need, 4, 64, stream, fresh)) return rc;
    if (int rc = grow_workspace((void**)&c->d_edge4, c->edge4_cap, f.edge4_need, 4, 0, stream, fresh)) return rc;
    if (fresh) c->epoch8 = 255;   // fresh memory: the next tag wraps and wipes it
    return grow_workspace((void**)&c->d_priv, c->priv_cap, f.priv_need, 1, 0, stream, fresh);
}

// Advances the 8-bit launch tag of the perm producer's self-tagged edge values and returns the G bias that carries it.  A wrapped tag
// could match stale values: they are wiped.
static unsigned next_gbias(sw_ctx* c, hipStream_t stream) {
    if (++c->epoch8 >= (unsigned)((c->opt.debug_flags & swk::DBG_EPOCH8_WRAP_EARLY) ? 4 : 256)) {
        const unsigned nb = (unsigned)std::max<size_t>(1, std::min<size_t>((c->edge4_cap + 255) / 256, 2048));
        hipLaunchKernelGGL(swk::sw_wipe_u32, dim3(nb), dim3(256), 0, stream, c->d_edge4, c->edge4_cap);
        c->epoch8 = 1;
    }
    return (c->epoch8 << 24) | 0x10000u;
}

static swp::DeviceFacts device_facts(const sw_ctx* c) {
    swp::DeviceFacts dev;
    dev.num_cus = c->num_cus; dev.xcd_round_robin = c->xcd_round_robin; dev.s2_per_cu = c->s2_per_cu;
    std::copy(std::begin(c->search_per_cu), std::end(c->search_per_cu), dev.search_per_cu);
    return dev;
}

static int plan_for(sw_ctx* c, const swp::PlanJob& pj, swp::FillPlan& plan) {
    if (c->opt.engine == 0 && c->s2_per_cu < 1)
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&c->s2_per_cu, swk::sw_systolic2<6, false>, 768, 0));
    plan = swp::plan_fill(pj, device_facts(c), c->opt);
    return SW_OK;
}

// the instantiations of the two kernels (sw_systolic.hip, sw_systolic2.inc)
using SystolicKernel = void (*)(const unsigned char*, const unsigned char*, const unsigned char*, swk::FillParams);
static const struct { int ns, nc; SystolicKernel h32, h64; } kSystolic[] = {
    {2, 2, swk::sw_systolic<int32_t, 2, 2>, swk::sw_systolic<int64_t, 2, 2>}, {2, 3, swk::sw_systolic<int32_t, 2, 3>, swk::sw_systolic<int64_t, 2, 3>},
    {2, 4, swk::sw_systolic<int32_t, 2, 4>, swk::sw_systolic<int64_t, 2, 4>}, {1, 2, swk::sw_systolic<int32_t, 1, 2>, swk::sw_systolic<int64_t, 1, 2>},
    {1, 3, swk::sw_systolic<int32_t, 1, 3>, swk::sw_systolic<int64_t, 1, 3>}, {1, 4, swk::sw_systolic<int32_t, 1, 4>, swk::sw_systolic<int64_t, 1, 4>},
    {1, 6, swk::sw_systolic<int32_t, 1, 6>, swk::sw_systolic<int64_t, 1, 6>}, {1, 7, swk::sw_systolic<int32_t, 1, 7>, swk::sw_systolic<int64_t, 1, 7>},
};
using Systolic2Kernel = void (*)(const unsigned char*, const unsigned char*, swk::FillParams);
static const Systolic2Kernel kSystolic2[4][2] = {   // [consumers - 4][overlapping strips]
    {swk::sw_systolic2<4, false>, swk::sw_systolic2<4, true>}, {swk::sw_systolic2<5, false>, swk::sw_systolic2<5, true>},
    {swk::sw_systolic2<6, false>, swk::sw_systolic2<6, true>}, {swk::sw_systolic2<7, false>, swk::sw_systolic2<7, true>},
};

static swp::PlanJob plan_job(const FillJob& j, const sw_scores* sc) {
    swp::PlanJob pj;
    pj.cols = j.cols; pj.rows = j.rows; pj.npairs = j.npairs; pj.full_stride = j.stride == j.cols + 1;
    pj.h_elem_bytes = j.h_elem_bytes; pj.p_elem_bytes = j.p_elem_bytes; pj.has_H = j.d_H; pj.has_P = j.d_P;
    pj.has_top = j.d_top; pj.has_left = j.d_left; pj.has_right = j.d_right; pj.has_top_gran = j.d_top_gran; pj.has_bot_gran = j.d_bot_gran;
    pj.has_result = j.d_result; pj.total_rows = j.total_rows; pj.reserve_cus = j.reserve_cus;
    pj.h_aligned = ((uintptr_t)j.d_H & (j.h_elem_bytes == 8 ? 15u : 7u)) == 0; pj.p_aligned = ((uintptr_t)j.d_P & 7u) == 0;
    pj.match = sc->match; pj.mismatch = sc->mismatch; pj.gap = sc->gap;
    return pj;
}

// Carries out the plan of one fill (sw_plan.cpp): workspaces, launch tags, parameters, launches.
static int launch_fill(sw_ctx* c, const sw_scores* sc, const FillJob& j, hipStream_t stream) {
    const int64_t cols = j.cols, rows = j.rows;
    const bool systolic = (c->opt.engine == 0);
    c->last_fused = false;
    const bool tile_features = j.d_left || j.d_right || j.stride != cols + 1 || j.npairs != 1 || !j.d_H || !j.d_P || j.d_top_gran || j.d_bot_gran;
    if (!systolic && tile_features) { set_err("tiles / batches / bands / matrix-less fills need the systolic engine (engine 0)"); return SW_EINVAL; }
    if (j.p_elem_bytes == 1 && !systolic) { set_err("compact (int8) P needs the systolic engine"); return SW_EINVAL; }
    if (j.keep_row0 && !systolic) { set_err("a tile with a top halo needs the systolic engine (engine 0)"); return SW_EINVAL; }
    if (((uintptr_t)j.d_b & 15) != 0 || (j.b_pstride & 15) != 0) { set_err("d_b (and the batch stride of b) must be 16-byte aligned"); return SW_EINVAL; }
    // (the caller holds the device lock and has ordered `stream` behind earlier fills: DevOrder)
    swp::PlanJob pj = plan_job(j, sc);
    auto known = j.d_P ? c->pair_ratio.find(j.d_P) : c->pair_ratio.end();
    if (known != c->pair_ratio.end()) pj.pair_ratio = known->second;
    swp::FillPlan plan;
    if (int rc = plan_for(c, pj, plan)) return rc;
    if (plan.probe_pair_class) {
        // option "probe_foreign_pairs": a pair the library did not allocate is probed once, at its first fill -- the probe WRITES both
        // buffers (this fill overwrites them anyway) and synchronises the stream (~0.3 ms); remembered by the address of P (at most 64)
        float r = 0.f, ms = 0.f;
        if (c->pair_ratio.size() >= 64) c->pair_ratio.clear();
        if (hipStreamSynchronize(stream) == hipSuccess && sw_place_pair_ratio(j.d_H, plan.h_bytes, j.d_P, plan.p_bytes, &r, &ms) == SW_OK) {
            c->pair_ratio[j.d_P] = pj.pair_ratio = r;
            if (int rc = plan_for(c, pj, plan)) return rc;
        }
    }
    const auto* one_col = systolic ? std::find_if(std::begin(kSystolic), std::end(kSystolic), [&](const auto& k) { return k.ns == plan.NS && k.nc == plan.NC; })
                                   : std::end(kSystolic);
    if (systolic && one_col == std::end(kSystolic)) { set_err("unsupported strips_per_group/consumers combination %d/%d", plan.NS, plan.NC); return SW_EINVAL; }
    if (int rc = ensure_workspaces(c, plan, stream)) return rc;
    if (++c->epoch >= 4096) {  // 12-bit tag wrapped: stale tags could match again, wipe them
        HIP_TRY(hipMemsetAsync(c->d_edge, 0, c->edge_cap * 8, stream));
        c->epoch = 1;
    }
    c->last_plan = plan;
    const int64_t S = plan.S;
    swk::FillParams p;
    memset(&p, 0, sizeof p);
    p.cols = cols; p.rows = rows; p.M = j.stride;
    p.H = j.d_H; p.P = (int32_t*)j.d_P; p.top = j.d_top; p.left = j.d_left; p.right = j.d_right;
    p.top_gran = j.d_top_gran; p.bot_gran = j.d_bot_gran; p.bot_done = j.d_bot_done; p.top_tag = j.top_tag; p.bot_tag = j.bot_tag;
    p.top_wait_ticks = (unsigned)std::min<int64_t>(0x7fffffff, c->opt_band_wait_ms * 100000 >> 10);
    p.mm = sc->match - 2 * sc->gap; p.xm = sc->mismatch - 2 * sc->gap; p.ngap = -sc->gap;
    p.edge = c->d_edge; p.tag_base = c->epoch << 20;
    p.result_key = j.d_keys; p.abort_flag = (unsigned int*)(c->d_key + 1);
    p.nstrips = (int)S;
    p.debug_flags = (int)c->opt.debug_flags;
    p.pace_ps = (int)c->opt_pace_ps;
    p.store_nt = plan.store_nt;
    p.xcd_order = (int)c->opt_xcd_order;
    p.dbg = (unsigned long long*)(uintptr_t)c->opt_dbg_ptr;
    p.npairs = (int)j.npairs; p.store_hp = (j.d_H || j.d_P) ? 1 : 0;
    p.p_bytes = j.p_elem_bytes;
    p.skip_row0 = j.keep_row0 ? 2 : 0;   // (2: not even the halo values are stored into row 0 of H)
    p.a_pstride = j.a_pstride; p.b_pstride = j.b_pstride; p.hp_pstride = j.hp_pstride;
    p.edge_pstride = S * (rows + 1);
    const unsigned char* ua = (const unsigned char*)j.d_a;
    const unsigned char* ub = (const unsigned char*)j.d_b;
    if (!systolic) {
        c->key_dirty = true;
        c->last_grid = plan.grid;
        if (j.h_elem_bytes == 4)
            hipLaunchKernelGGL((swk::sw_strip_scan<int32_t, 16>), dim3(plan.grid), dim3(plan.threads), 0, stream, ua, ub, p);
        else
            hipLaunchKernelGGL((swk::sw_strip_scan<int64_t, 16>), dim3(plan.grid), dim3(plan.threads), 0, stream, ua, ub, p);
        HIP_TRY(hipGetLastError());
        return SW_OK;
    }
    const size_t cb16 = ((c->cb_cap + 15) / 16) * 16;
    unsigned short* d_cb16 = (unsigned short*)(c->d_cb + cb16);
    unsigned char* d_cbc = c->d_cb + cb16 + ((2 * c->cb_cap + 15) / 16) * 16;
    if (plan.perm) {
        p.edge4 = c->d_edge4; p.e4stride = plan.e4stride; p.edge4_pstride = S * plan.e4stride;
        p.gbias = next_gbias(c, stream);
    }
    p.bcode = d_cbc;
    p.atab = c->d_alpha + 64;
    p.phi_base = plan.fast ? (int)S - 1 : -1;
    p.bfront = (int)plan.bfront;
    p.bpad16 = d_cb16;
    p.bpad8 = c->d_cb;
    p.bpad_pstride = plan.per;
    if (plan.two_cols) {
        // one launch per tile: the kernel's prologue prepares (letter codes, every workgroup's padded copy of b, zeros in row 0 /
        // column 0 -- except a band's halo row: its H comes from the row above, written by the kernel; its P belongs to the band
        // above), its last workgroup out reports and re-arms key / abort flag / sync words -- which therefore are zero here, unless
        // another kind of launch has used the key since
        if (c->key_dirty) { HIP_TRY(hipMemsetAsync(c->d_key, 0, 16, stream)); c->key_dirty = false; }
        for (int64_t tile = 0; tile < plan.ntile; ++tile) {
            const swp::TilePlan& t = plan.tile[tile];
            swk::FillParams p2 = p;
            p2.nstrips = (int)t.strips; p2.cols = t.cols; p2.h_bytes = j.h_elem_bytes; p2.s2w = plan.W2; p2.store_nt = t.store_nt;
            p2.alpha_a = ua; p2.alpha_cols = cols;
            p2.idx_off = t.c0; p2.final_launch = tile + 1 == plan.ntile ? 1 : 0;
            if (plan.ntile > 1) {   // a tile's left halo is the previous tile's last column, read from H itself
                p2.H = (char*)j.d_H + t.c0 * 4; p2.P = (int32_t*)((char*)j.d_P + t.c0 * 4);
                p2.tile_left = tile ? (const int32_t*)j.d_H + t.c0 : nullptr;
                if (tile) p2.gbias = next_gbias(c, stream);   // (the edge values are self-tagged: every tile launch has its own tag)
            }
            p2.nscout = t.nscout; p2.scout_double = t.scout_double; p2.xcd_mode = t.xcd_mode;
            p2.split_blk = t.split_blk; p2.split_from = t.split_from; p2.split_extra = t.split_extra;
            p2.filler_end_steps = t.filler_end_steps; p2.filler_full_steps = t.filler_full_steps;
            p2.filler_hop_ps = t.filler_hop_ps; p2.filler_tau_ps = t.filler_tau_ps; p2.filler_bw_gbs = t.filler_bw_gbs;
            p2.sync = c->d_sync; p2.priv = c->d_priv; p2.priv_stride = plan.priv_stride;
            p2.bpad16_w = d_cb16; p2.bpad8_w = c->d_cb; p2.bcode_w = d_cbc; p2.atab_w = c->d_alpha + 64;
            p2.result = j.d_result; p2.skip_row0 = j.keep_row0 ? 2 : (j.d_top || j.d_top_gran) ? 1 : 0;
            p2.scan_all = t.scan_all;
            hipLaunchKernelGGL(kSystolic2[t.consumers - 4][plan.W2 == 110], dim3(t.grid), dim3(768), 0, stream, ua + t.c0, ub, p2);
        }
        // the fall-back (an alphabet of more than 7 letters, known on the device only): enqueued behind, leaves at once otherwise;
        // it fills the whole matrix by itself, whatever the tiling
        p.skip_if_perm = 1;
        p.sync = c->d_sync; p.atab_w = c->d_alpha + 64; p.result = j.d_result; p.final_launch = 1;
        c->last_fused = true;
    } else {
        // input preparation, two dispatches (sw_systolic.hip): presence maps of the letters, then codes / padded copies of b
        const int64_t total = (cols + rows) * j.npairs;
        const unsigned nscan = (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 1023) / 1024, 2048));
        hipLaunchKernelGGL(swk::sw_prep_scan, dim3(nscan), dim3(256), 0, stream, ua, cols, j.a_pstride, ub, rows, j.b_pstride, j.npairs, c->d_part);
        const unsigned npad = (unsigned)((plan.per + 255) / 256);
        hipLaunchKernelGGL(swk::sw_prep_code, dim3(npad, (unsigned)j.npairs), dim3(256), 0, stream, ub, rows, plan.bfront, j.b_pstride, c->d_cb, d_cb16,
                           d_cbc, (const unsigned int*)c->d_part, (int)nscan, c->d_alpha + 64, plan.per, (int)npad, (void*)nullptr, j.h_elem_bytes,
                           (void*)nullptr, j.p_elem_bytes, cols + 1, rows + 1, 0, j.zero_key ? j.d_keys : nullptr);
        c->key_dirty = true;
    }
    const SystolicKernel kern = j.h_elem_bytes == 4 ? one_col->h32 : one_col->h64;
    // (asked once per context, kernel and workgroup size, not on every fill)
    static_assert(sizeof(kSystolic) / sizeof(kSystolic[0]) == 8, "sw_ctx::sys_occ has one row per instantiation");
    auto& occ = c->sys_occ[one_col - std::begin(kSystolic)][j.h_elem_bytes == 4 ? 0 : 1];
    if (occ.threads != plan.threads) {
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ.per_cu, kern, plan.threads, 0));
        occ.threads = plan.threads;
    }
    const int per_cu = occ.per_cu;
    if (per_cu < 1) { set_err("the fill kernel does not fit a CU on this device"); return SW_EDEVICE; }
    c->last_grid = std::min<int64_t>(plan.grid, (int64_t)per_cu * c->num_cus);
    hipLaunchKernelGGL(kern, dim3((unsigned)c->last_grid), dim3(plan.threads), 0, stream, ua, ub, (const unsigned char*)c->d_cb, p);
    HIP_TRY(hipGetLastError());
    return SW_OK;
}

static const sw_scores kDefaultScores = {3, -3, -2};  // serial_smithW.c:59-61

// one matrix / tile / band: validation, empty shapes, launch, finalize
static int fill_one(sw_ctx* c, const sw_scores* scores, FillJob j, int64_t gcols, int64_t grows, sw_result* d_result, void* stream_,
                    const char* who) {
    const sw_scores* sc = scores ? scores : &kDefaultScores;
    const int64_t cols = j.cols, rows = j.rows;
    if (!c || !d_result || (j.h_elem_bytes != 4 && j.h_elem_bytes != 8) || (j.p_elem_bytes != 4 && j.p_elem_bytes != 1) ||
        j.stride < cols + 1) {
        set_err("%s: bad argument", who);
        return SW_EINVAL;
    }
    if (int rc = check_dims(cols, rows, sc, gcols, grows)) return rc;
    if ((cols > 0 && !j.d_a) || (rows > 0 && !j.d_b)) { set_err("%s: NULL sequence", who); return SW_EINVAL; }
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    DevOrder order(c, stream, j.concurrent);
    if (order.rc) return order.rc;
    j.d_keys = c->d_key;
    j.d_result = d_result;
    j.zero_key = c->opt.engine == 0 && cols > 0 && rows > 0;   // (the systolic engine's preparation zeroes the key and the abort flag -- or finds them zero)
    if (!j.zero_key) { HIP_TRY(hipMemsetAsync(c->d_key, 0, 16, stream)); c->key_dirty = true; }
    c->last_fused = false;
    if (cols == 0 || rows == 0) {
        // no interior cell: H (= halo row / zero column) and P are all boundary
        if (j.stride != cols + 1 || j.d_left || j.d_right || j.d_top_gran || j.d_bot_gran) { set_err("%s: empty tiles / bands are not supported", who); return SW_EINVAL; }
        const int64_t M = cols + 1;
        if (j.d_H) HIP_TRY(hipMemsetAsync(j.d_H, 0, (size_t)(M * (rows + 1)) * j.h_elem_bytes, stream));
        if (j.d_P) HIP_TRY(hipMemsetAsync(j.d_P, 0, (size_t)(M * (rows + 1)) * j.p_elem_bytes, stream));
        if (j.d_H && j.d_top && j.h_elem_bytes == 4) HIP_TRY(hipMemcpyAsync(j.d_H, j.d_top, (size_t)M * 4, hipMemcpyDeviceToDevice, stream));
        if (j.d_H && j.d_top && j.h_elem_bytes == 8) { set_err("top halo with an empty int64 band is unsupported"); return SW_EINVAL; }
    } else {
        if (int rc = launch_fill(c, sc, j, stream)) return rc;
    }
    // (a one-launch fill has written the result by itself: sw_systolic2.inc)
    if (!c->last_fused) hipLaunchKernelGGL(swk::sw_finalize, dim3(1), dim3(64), 0, stream, c->d_key, (const unsigned int*)(c->d_key + 1), d_result, 1);
    HIP_TRY(hipGetLastError());
    return SW_OK;
}

static FillJob make_job(const char* d_a, int64_t cols, const char* d_b, int64_t rows, void* d_H, int h_elem_bytes, void* d_P, int p_elem_bytes,
                        int64_t row_stride, const int32_t* d_top, const int32_t* d_left, int32_t* d_right) {
    FillJob j = {d_a, cols, d_b, rows, d_H, h_elem_bytes, d_P, row_stride, d_top, d_left, d_right, 1, 0, 0, 0, nullptr};
    j.p_elem_bytes = p_elem_bytes;
    return j;
}

int sw_fill_tile_device(sw_ctx* c, const char* d_a, int64_t cols, const char* d_b, int64_t rows, const sw_scores* scores,
                        void* d_H, int h_elem_bytes, int32_t* d_P, int64_t row_stride, const int32_t* d_top,
                        const int32_t* d_left, int32_t* d_right, sw_result* d_result, void* stream_) {
    if (!d_H || !d_P) { set_err("sw_fill_tile_device: bad argument"); return SW_EINVAL; }
    FillJob j = make_job(d_a, cols, d_b, rows, d_H, h_elem_bytes, d_P, 4, row_stride, d_top, d_left, d_right);
    j.keep_row0 = d_top != nullptr;
    return fill_one(c, scores, j, -1, -1, d_result, stream_, "sw_fill_tile_device");
}

int sw_fill_device(sw_ctx* c, const char* d_a, int64_t cols, const char* d_b, int64_t rows, const sw_scores* scores,
                   void* d_H, int h_elem_bytes, int32_t* d_P, const int32_t* d_top, sw_result* d_result, void* stream_) {
    if (!d_H || !d_P) { set_err("sw_fill_device: bad argument"); return SW_EINVAL; }
    return fill_one(c, scores, make_job(d_a, cols, d_b, rows, d_H, h_elem_bytes, d_P, 4, cols + 1, d_top, nullptr, nullptr), -1, -1, d_result,
                    stream_, "sw_fill_device");
}

// compact P (one byte per predecessor code, same values 0..3, -1..-3 after the traceback) and matrix-less fills
// (d_H and/or d_P NULL: that matrix is not written; arg-max stays exact), SURVEY.md 8f-2
int sw_fill_device_ex(sw_ctx* c, const char* d_a, int64_t cols, const char* d_b, int64_t rows, const sw_scores* scores,
                      void* d_H, int h_elem_bytes, void* d_P, int p_elem_bytes, const int32_t* d_top, sw_result* d_result,
                      void* stream_) {
    return fill_one(c, scores, make_job(d_a, cols, d_b, rows, d_H, h_elem_bytes, d_P, p_elem_bytes, cols + 1, d_top, nullptr, nullptr), -1, -1,
                    d_result, stream_, "sw_fill_device_ex");
}

// One row band of a (total_rows+1) x (cols+1) matrix as ONE persistent launch (multi-GPU): the halo row
// arrives and leaves as {tag, H} granules while the kernel runs.
int sw_fill_band_device(sw_ctx* c, const char* d_a, int64_t cols, const char* d_b, int64_t rows, int64_t total_rows,
                        const sw_scores* scores, void* d_H, int h_elem_bytes, void* d_P, int p_elem_bytes,
                        const uint64_t* d_top_gran, uint32_t top_tag, uint64_t* d_bot_gran, uint32_t bot_tag, uint32_t* d_bot_done,
                        int reserve_cus, int concurrent, sw_result* d_result, void* stream_) {
    if ((d_top_gran && top_tag == 0) || (d_bot_gran && bot_tag == 0) || (d_bot_done && !d_bot_gran) || reserve_cus < 0 || total_rows < rows) {
        set_err("sw_fill_band_device: bad argument");
        return SW_EINVAL;
    }
    if (c && c->opt.engine != 0) { set_err("sw_fill_band_device needs the systolic engine"); return SW_EINVAL; }
    FillJob j = make_job(d_a, cols, d_b, rows, d_H, h_elem_bytes, d_P, p_elem_bytes, cols + 1, nullptr, nullptr, nullptr);
    j.d_top_gran = (const unsigned long long*)d_top_gran; j.d_bot_gran = (unsigned long long*)d_bot_gran; j.d_bot_done = d_bot_done;
    j.top_tag = top_tag; j.bot_tag = bot_tag; j.reserve_cus = reserve_cus; j.concurrent = concurrent != 0; j.total_rows = total_rows;
    return fill_one(c, scores, j, cols, total_rows, d_result, stream_, "sw_fill_band_device");
}

// the instantiations of the batch kernels (sw_batch.hip), picked by swp::batch_kernel
using BatchKernel = void (*)(swk::BatchParams);
static constexpr Indexed<BatchKernel> kBatch[] = {
    {swp::batch_wave_index(4, 0), swk::sw_batch_wave<4, 0>}, {swp::batch_wave_index(4, 1), swk::sw_batch_wave<4, 1>},
    {swp::batch_wave_index(4, 4), swk::sw_batch_wave<4, 4>}, {swp::batch_wave_index(8, 0), swk::sw_batch_wave<8, 0>},
    {swp::batch_wave_index(8, 1), swk::sw_batch_wave<8, 1>}, {swp::batch_wave_index(8, 4), swk::sw_batch_wave<8, 4>},
    {swp::batch_wave_index(16, 0), swk::sw_batch_wave<16, 0>}, {swp::batch_wave_index(16, 1), swk::sw_batch_wave<16, 1>},
    {swp::batch_wave_index(16, 4), swk::sw_batch_wave<16, 4>},
    {swp::batch_wave16_index(false, false, false), swk::sw_batch_wave16<false, false, false>},
    {swp::batch_wave16_index(false, false, true), swk::sw_batch_wave16<false, false, true>},
    {swp::batch_wave16_index(false, true, false), swk::sw_batch_wave16<false, true, false>},
    {swp::batch_wave16_index(false, true, true), swk::sw_batch_wave16<false, true, true>},
    {swp::batch_wave16_index(true, false, false), swk::sw_batch_wave16<true, false, false>},
    {swp::batch_wave16_index(true, false, true), swk::sw_batch_wave16<true, false, true>},
    {swp::batch_wave16_index(true, true, false), swk::sw_batch_wave16<true, true, false>},
    {swp::batch_wave16_index(true, true, true), swk::sw_batch_wave16<true, true, true>},
};
static_assert(std::size(kBatch) == swp::kBatchKernels && at_their_indices(kBatch));

// The batch kernel proper (csrc/sw_batch.hip): one pair per wave, no inter-workgroup traffic.  Carries out a plan whose `wave` is set;
// returns 1 when the batch has more than 8 distinct letters after all (found on the device: the caller then runs it on the single-pair
// machinery).
static int batch_one_pair_per_wave(sw_ctx* c, const swp::BatchPlan& plan, const char* d_a, int64_t a_stride, int64_t cols, const char* d_b,
                                   int64_t b_stride, int64_t rows, int64_t npairs, const sw_scores* sc, int32_t* d_H, void* d_P, int p_elem_bytes,
                                   sw_result* d_results, hipStream_t stream) {
    bool fresh = false;
    if (int rc = grow_workspace((void**)&c->d_bcodes, c->bcodes_cap, plan.bcodes_need, 1, 64, stream, fresh)) return rc;
    if (int rc = grow_workspace((void**)&c->d_bnd, c->bnd_cap, plan.bnd_need, 4, 0, stream, fresh)) return rc;
    const unsigned char* ua = (const unsigned char*)d_a;
    const unsigned char* ub = (const unsigned char*)d_b;
    // alphabet of the whole batch -> letter codes; the count decides whether the profile look-up applies
    hipLaunchKernelGGL(swk::sw_prep_scan, dim3((unsigned)plan.scan_blocks), dim3(256), 0, stream, ua, cols, a_stride, ub, rows, b_stride, npairs, c->d_part);
    // (one map for the half million blocks of sw_batch_codes: every one of them ORing all the maps by itself cost 29 ms per 100 000 pairs)
    hipLaunchKernelGGL(swk::sw_prep_reduce, dim3(1), dim3(256), 0, stream, c->d_part, plan.scan_blocks);
    // lane 0 of a later strip also reads boundary entries below the matrix that no strip of THIS call writes: they must not hold
    // an earlier call's scores (a cell outside the matrix may never exceed the cells of the matrix, see the arg-max in sw_batch.hip)
    if (plan.bnd_need) HIP_TRY(hipMemsetAsync(c->d_bnd, 0, plan.bnd_need * 4, stream));
    const int64_t cells = (cols + 1) * (rows + 1);
    const int pb = d_P ? p_elem_bytes : 0;
    unsigned int nletters = 0;
    for (int64_t k0 = 0; k0 < npairs; k0 += plan.chunk) {
        const int64_t n = std::min(plan.chunk, npairs - k0);
        hipLaunchKernelGGL(swk::sw_batch_codes, dim3((unsigned)plan.codes_blocks, (unsigned)std::min<int64_t>(n, 65535)), dim3(256), 0, stream,
                           ub + k0 * b_stride, rows, b_stride, c->d_bcodes, plan.per, plan.front, (const unsigned int*)c->d_part, 1, c->d_alpha + 64, n);
        HIP_TRY(hipGetLastError());
        if (k0 == 0) {   // the letter count (4 bytes) decides the path: the one host round trip of a batch call
            HIP_TRY(hipMemcpyAsync(&nletters, c->d_alpha + 64 + 256, 4, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        }
        const int k = swp::batch_kernel(plan, nletters, n, pb);
        if (k < 0) return 1;
        swk::BatchParams bp;
        memset(&bp, 0, sizeof bp);
        bp.a = ua + k0 * a_stride; bp.a_pstride = a_stride; bp.cols = cols;
        bp.bcode = c->d_bcodes; bp.bcode_pstride = plan.per; bp.bfront = plan.front;
        bp.rows = rows; bp.npairs = n; bp.atab = c->d_alpha + 64;
        bp.H = d_H ? d_H + k0 * cells : nullptr;
        bp.P = d_P ? (void*)((char*)d_P + k0 * cells * p_elem_bytes) : nullptr;
        bp.hp_pstride = cells;
        bp.match = sc->match; bp.mismatch = sc->mismatch; bp.ngap = -sc->gap;
        bp.bnd = c->d_bnd; bp.bnd_pstride = plan.bnd_per;
        bp.results = d_results + k0;
        bp.debug = (int)(c->opt.debug_flags & swk::DBG_BATCH_MASK);
        const bool two = k >= swp::kBatchWave16;   // two pairs per wave (sw_batch_wave16)
        const int64_t per_block = two ? 8 : 4;     // 4 waves per workgroup
        hipLaunchKernelGGL(kBatch[k].k, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(256), two ? 0 : (size_t)c->opt_batch_lds, stream, bp);
        HIP_TRY(hipGetLastError());
        if (two) c->last_batch_kernel = 2;
    }
    if (c->last_batch_kernel != 2) c->last_batch_kernel = 1;
    c->last_grid = plan.grid; c->last_plan.S = plan.nstrips;   // (sw_get_option "last_grid", "last_strips")
    return SW_OK;
}

// (library-internal) Sizes ctx's workspaces for band-resident launches of this shape without launching anything.  sw_multi_create
// calls it for every band: a launch that has to allocate synchronises its stream, and with several persistent band kernels on
// one GPU that stream can share a hardware queue with a kernel that is still polling for its halo -- which only arrives once the
// host is past the launches (seen with 8 bands on one GPU: band 1 gave up after "band_wait_ms" and the relay stalled).
int sw_fill_band_reserve(sw_ctx* c, int64_t cols, int64_t rows, int64_t total_rows, const sw_scores* scores, int h_elem_bytes, int p_elem_bytes, int want_h,
                         void* stream_) {
    const sw_scores* sc = scores ? scores : &kDefaultScores;
    if (!c || cols <= 0 || rows <= 0) { set_err("sw_fill_band_reserve: bad argument"); return SW_EINVAL; }
    if (c->opt.engine != 0) { set_err("sw_fill_band_reserve needs the systolic engine"); return SW_EINVAL; }
    if (int rc = check_dims(cols, rows, sc, cols, total_rows)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    swp::PlanJob pj;   // (a band: halo row in and last row out as granules, a result of its own)
    pj.cols = cols; pj.rows = rows; pj.total_rows = total_rows; pj.h_elem_bytes = h_elem_bytes; pj.p_elem_bytes = p_elem_bytes; pj.has_H = want_h != 0;
    pj.has_top_gran = pj.has_bot_gran = true;
    pj.match = sc->match; pj.mismatch = sc->mismatch; pj.gap = sc->gap;
    swp::FillPlan plan;
    if (int rc = plan_for(c, pj, plan)) return rc;
    std::unique_lock<std::mutex> lk(g_dev[c->device & 63].mu);
    if (int rc = ensure_workspaces(c, plan, (hipStream_t)stream_)) return rc;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream_));   // (every workspace exists now, and is wiped where fresh)
    return SW_OK;
}

// BASELINE config 5: npairs independent cols x rows problems; pair k reads a at d_a + k*a_stride, b at d_b + k*b_stride.
// d_H and/or d_P may be NULL (that matrix is not written); the arg-max is exact in every mode.
int sw_batch_device_ex(sw_ctx* c, const char* d_a, int64_t a_stride, int64_t cols, const char* d_b, int64_t b_stride, int64_t rows,
                       int64_t npairs, const sw_scores* scores, int32_t* d_H, void* d_P, int p_elem_bytes, sw_result* d_results,
                       void* stream_) {
    const sw_scores* sc = scores ? scores : &kDefaultScores;
    if (!c || !d_a || !d_b || !d_results || npairs <= 0 || cols <= 0 || rows <= 0 || a_stride < cols || b_stride < rows ||
        (p_elem_bytes != 4 && p_elem_bytes != 1)) {
        set_err("sw_batch_device: bad argument");
        return SW_EINVAL;
    }
    if (c->opt.engine != 0) { set_err("sw_batch_device needs the systolic engine"); return SW_EINVAL; }
    if (int rc = check_dims(cols, rows, sc)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    DevOrder order(c, stream, false);
    if (order.rc) return order.rc;
    swp::BatchJob bj;
    bj.cols = cols; bj.rows = rows; bj.npairs = npairs; bj.has_H = d_H; bj.has_P = d_P; bj.p_elem_bytes = p_elem_bytes;
    bj.match = sc->match; bj.mismatch = sc->mismatch; bj.gap = sc->gap;
    const swp::BatchPlan plan = swp::plan_batch(bj, c->opt);
    c->last_batch_kernel = 0;
    if (plan.wave) {
        int rc = batch_one_pair_per_wave(c, plan, d_a, a_stride, cols, d_b, b_stride, rows, npairs, sc, d_H, d_P, p_elem_bytes, d_results, stream);
        if (rc != 1) return rc;      // 1: not eligible after all (an alphabet of more than 8 letters)
    }
    // the fall-back: the single-pair machinery, plan.single_chunk pairs per launch
    bool fresh = false;
    if (int rc = grow_workspace((void**)&c->d_keys, c->keys_cap, (size_t)plan.single_chunk, 8, 0, stream, fresh)) return rc;
    HIP_TRY(hipMemsetAsync(c->d_key, 0, 16, stream));
    c->key_dirty = true;
    const int64_t cells = (cols + 1) * (rows + 1);
    for (int64_t k0 = 0; k0 < npairs; k0 += plan.single_chunk) {
        const int64_t n = std::min(plan.single_chunk, npairs - k0);
        HIP_TRY(hipMemsetAsync(c->d_keys, 0, (size_t)n * 8, stream));
        FillJob j = {d_a + k0 * a_stride, cols, d_b + k0 * b_stride, rows, d_H ? (void*)(d_H + k0 * cells) : nullptr, 4,
                     d_P ? (void*)((char*)d_P + k0 * cells * p_elem_bytes) : nullptr, cols + 1, nullptr, nullptr, nullptr, n, a_stride, b_stride,
                     cells, c->d_keys};
        j.p_elem_bytes = p_elem_bytes;
        if (int rc = launch_fill(c, sc, j, stream)) return rc;
        hipLaunchKernelGGL(swk::sw_finalize, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, c->d_keys,
                           (const unsigned int*)(c->d_key + 1), d_results + k0, (int)n);
        HIP_TRY(hipGetLastError());
    }
    return SW_OK;
}
int sw_batch_device(sw_ctx* c, const char* d_a, int64_t a_stride, int64_t cols, const char* d_b, int64_t b_stride, int64_t rows,
                    int64_t npairs, const sw_scores* scores, int32_t* d_H, int32_t* d_P, sw_result* d_results, void* stream_) {
    return sw_batch_device_ex(c, d_a, a_stride, cols, d_b, b_stride, rows, npairs, scores, d_H, d_P, 4, d_results, stream_);
}

// the instantiations of the search kernel (sw_search.hip), picked by swp::plan_search
using SearchKernel = void (*)(swk::SearchParams);
static constexpr Indexed<SearchKernel> kSearch[] = {
    {swp::search_kernel_index(4, false), swk::sw_search_wave<4, false>}, {swp::search_kernel_index(4, true), swk::sw_search_wave<4, true>},
    {swp::search_kernel_index(8, false), swk::sw_search_wave<8, false>}, {swp::search_kernel_index(8, true), swk::sw_search_wave<8, true>},
    {swp::search_kernel_index(16, false), swk::sw_search_wave<16, false>}, {swp::search_kernel_index(16, true), swk::sw_search_wave<16, true>},
};
static_assert(std::size(kSearch) == swp::kSearchKernels && at_their_indices(kSearch));

// The search schedule's device buffer and the pinned copy it is uploaded from, grown together to `need` items (the caller has waited
// for the last upload from the pinned copy).
static int grow_schedule(sw_ctx* c, size_t need, hipStream_t stream) {
    if (need <= c->sitems_cap) return SW_OK;
    HIP_TRY(hipStreamSynchronize(stream));
    if (c->d_sitems) HIP_TRY(hipFree(c->d_sitems));
    if (c->h_sitems) HIP_TRY(hipHostFree(c->h_sitems));
    c->d_sitems = nullptr; c->h_sitems = nullptr; c->sitems_cap = 0;
    if (hipMalloc((void**)&c->d_sitems, need * sizeof(swk::SearchItem)) != hipSuccess ||
        hipHostMalloc((void**)&c->h_sitems, need * sizeof(swk::SearchItem), 0) != hipSuccess) {
        set_err("sw_search_device: workspace allocation failed");
        return SW_ENOMEM;
    }
    c->sitems_cap = need;
    return SW_OK;
}

// Database search (csrc/sw_search.hip): for every target k the reference fill of query x target k, score and arg-max only.  No host
// round trip: the lengths come from the host offsets, the profile is built on the device from the query.
int sw_search_device(sw_ctx* c, const char* d_query, int64_t qlen, const char* d_db, const int64_t* offsets, int64_t ntargets,
                     const sw_scores* scores, sw_result* d_results, void* stream_) {
    const sw_scores* sc = scores ? scores : &kDefaultScores;
    if (!c || !d_query || !d_db || !offsets || !d_results || ntargets < 0) { set_err("sw_search_device: NULL pointer or negative target count"); return SW_EINVAL; }
    if (qlen < 1 || qlen > swk::SW_MAX_DIM) { set_err("sw_search_device: query length %lld out of range 1..%lld", (long long)qlen, (long long)swk::SW_MAX_DIM); return SW_EINVAL; }
    if (offsets[0] < 0) { set_err("sw_search_device: offsets[0] = %lld is negative", (long long)offsets[0]); return SW_EINVAL; }
    int64_t maxlen = 0, nonempty = 0;
    for (int64_t k = 0; k < ntargets; ++k) {
        const int64_t len = offsets[k + 1] - offsets[k];
        if (len < 0) { set_err("sw_search_device: offsets decrease at target %lld", (long long)k); return SW_EINVAL; }
        if (len > swk::SW_MAX_DIM) { set_err("sw_search_device: target %lld has length %lld (max %lld)", (long long)k, (long long)len, (long long)swk::SW_MAX_DIM); return SW_EINVAL; }
        maxlen = std::max(maxlen, len);
        nonempty += len > 0;
    }
    if (int rc = check_dims(qlen, maxlen, sc)) return rc;
    if (ntargets == 0) return SW_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    DevOrder order(c, stream, false);
    if (order.rc) return order.rc;
    // empty targets keep the zeros: {0, 0, 0}
    HIP_TRY(hipMemsetAsync(d_results, 0, (size_t)ntargets * sizeof(sw_result), stream));
    if (nonempty == 0) return SW_OK;
    // occupancy of every instantiation, once per context: the grid depends on the one the plan picks
    if (!c->search_per_cu_known) {
        for (int k = 0; k < swp::kSearchKernels; ++k) HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&c->search_per_cu[k], kSearch[k].k, 256, 0));
        c->search_per_cu_known = true;
    }
    swp::SearchJob sj;
    sj.qlen = qlen; sj.maxlen = maxlen; sj.ntargets = nonempty; sj.match = sc->match; sj.mismatch = sc->mismatch; sj.gap = sc->gap;
    const swp::SearchPlan plan = swp::plan_search(sj, device_facts(c));
    if (c->search_per_cu[plan.kernel] < 1) { set_err("the search kernel does not fit a CU on this device"); return SW_EDEVICE; }
    // the schedule is uploaded from a pinned copy: the previous upload has to have left it
    if (c->sitems_ev) HIP_TRY(hipEventSynchronize(c->sitems_ev));
    else HIP_TRY(hipEventCreateWithFlags(&c->sitems_ev, hipEventDisableTiming));
    bool fresh = false;
    if (int rc = grow_schedule(c, (size_t)nonempty, stream)) return rc;
    if (int rc = grow_workspace((void**)&c->d_sprof, c->sprof_cap, plan.prof_need, 1, 0, stream, fresh)) return rc;
    if (int rc = grow_workspace((void**)&c->d_sbnd, c->sbnd_cap, plan.bnd_need, 4, 0, stream, fresh)) return rc;
    if (!c->d_sctr) HIP_TRY(hipMalloc((void**)&c->d_sctr, 64));
    swp::search_schedule(offsets, ntargets, c->h_sitems);
    HIP_TRY(hipMemcpyAsync(c->d_sitems, c->h_sitems, (size_t)nonempty * sizeof(swk::SearchItem), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(c->sitems_ev, stream));
    hipLaunchKernelGGL(swk::sw_search_profile, dim3((unsigned)plan.prof_blocks), dim3(256), 0, stream, (const unsigned char*)d_query, qlen, plan.qpad,
                       c->d_sprof, sc->match, sc->mismatch, plan.wide ? 1 : 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(c->d_sctr, 0, 4, stream));
    swk::SearchParams sp;
    memset(&sp, 0, sizeof sp);
    sp.db = (const unsigned char*)d_db;
    sp.items = c->d_sitems; sp.nitems = nonempty;
    sp.prof = c->d_sprof; sp.qpad = plan.qpad; sp.qlen = qlen;
    sp.match = sc->match; sp.mismatch = sc->mismatch; sp.ngap = -sc->gap;
    sp.bnd = plan.bnd_per ? c->d_sbnd : nullptr; sp.bnd_per = plan.bnd_per;
    sp.counter = c->d_sctr;
    sp.results = d_results;
    hipLaunchKernelGGL(kSearch[plan.kernel].k, dim3((unsigned)plan.grid), dim3(256), 0, stream, sp);
    HIP_TRY(hipGetLastError());
    c->last_search_grid = plan.grid; c->last_search_kernel = plan.kernel;
    return SW_OK;
}

// the instantiations of the affine search kernel (sw_search_affine.hip), picked by swp::plan_search_affine
using SearchAffineKernel = void (*)(swk::SearchAffineParams);
static constexpr Indexed<SearchAffineKernel> kSearchAffine[] = {
    {swp::search_affine_kernel_index(4), swk::sw_search_affine_wave<4>},
    {swp::search_affine_kernel_index(8), swk::sw_search_affine_wave<8>},
    {swp::search_affine_kernel_index(16), swk::sw_search_affine_wave<16>},
};
static_assert(std::size(kSearchAffine) == swp::kSearchAffineKernels && at_their_indices(kSearchAffine));

// Database search with a substitution matrix and affine gaps (csrc/sw_search_affine.hip).  The shape of sw_search_device: no host
// round trip, the schedule and the 64 KiB table are uploaded from pinned copies, the profile is built on the device.
int sw_search_affine_device(sw_ctx* c, const char* d_query, int64_t qlen, const char* d_db, const int64_t* offsets, int64_t ntargets,
                            const sw_affine* scoring, sw_result* d_results, void* stream_) {
    if (!c || !d_query || !d_db || !offsets || !d_results || !scoring || ntargets < 0) {
        set_err("sw_search_affine_device: NULL pointer or negative target count");
        return SW_EINVAL;
    }
    int64_t maxlen = 0, nonempty = 0;
    if (int rc = swh::check_search_affine("sw_search_affine_device", qlen, offsets, ntargets, scoring, &maxlen, &nonempty)) return rc;
    if (ntargets == 0) return SW_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    DevOrder order(c, stream, false);
    if (order.rc) return order.rc;
    // empty targets keep the zeros: {0, 0, 0}
    HIP_TRY(hipMemsetAsync(d_results, 0, (size_t)ntargets * sizeof(sw_result), stream));
    if (nonempty == 0) return SW_OK;
    // occupancy of every instantiation, once per context: the columns per lane and the grid depend on it
    if (!c->search_affine_per_cu_known) {
        for (int k = 0; k < swp::kSearchAffineKernels; ++k)
            HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&c->search_affine_per_cu[k], kSearchAffine[k].k, 256, 0));
        c->search_affine_per_cu_known = true;
    }
    swp::SearchAffineJob sj;
    sj.qlen = qlen; sj.maxlen = maxlen; sj.ntargets = nonempty; sj.num_cus = c->num_cus;
    std::copy(std::begin(c->search_affine_per_cu), std::end(c->search_affine_per_cu), sj.per_cu);
    const swp::SearchAffinePlan plan = swp::plan_search_affine(sj);
    if (c->search_affine_per_cu[plan.kernel] < 1) { set_err("the affine search kernel does not fit a CU on this device"); return SW_EDEVICE; }
    // the schedule and the table are uploaded from pinned copies: the previous uploads have to have left them
    if (c->sitems_ev) HIP_TRY(hipEventSynchronize(c->sitems_ev));
    else HIP_TRY(hipEventCreateWithFlags(&c->sitems_ev, hipEventDisableTiming));
    bool fresh = false;
    if (int rc = grow_schedule(c, (size_t)nonempty, stream)) return rc;
    if (int rc = grow_workspace((void**)&c->d_sprof, c->sprof_cap, plan.prof_need, 1, 0, stream, fresh)) return rc;
    if (int rc = grow_workspace((void**)&c->d_sbnd, c->sbnd_cap, plan.bnd_need, 4, 0, stream, fresh)) return rc;
    if (!c->d_sctr) HIP_TRY(hipMalloc((void**)&c->d_sctr, 64));
    if (!c->d_submat) HIP_TRY(hipMalloc((void**)&c->d_submat, sizeof(sw_submat)));
    if (!c->h_submat) HIP_TRY(hipHostMalloc((void**)&c->h_submat, sizeof(sw_submat), 0));
    swp::search_schedule(offsets, ntargets, c->h_sitems);
    memcpy(c->h_submat, scoring->sub, sizeof(sw_submat));
    HIP_TRY(hipMemcpyAsync(c->d_sitems, c->h_sitems, (size_t)nonempty * sizeof(swk::SearchItem), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(c->d_submat, c->h_submat, sizeof(sw_submat), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(c->sitems_ev, stream));
    hipLaunchKernelGGL(swk::sw_search_profile_submat, dim3((unsigned)plan.prof_blocks), dim3(256), 0, stream, (const unsigned char*)d_query, qlen,
                       plan.qpad, c->d_sprof, (const signed char*)c->d_submat);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(c->d_sctr, 0, 4, stream));
    swk::SearchAffineParams sp;
    memset(&sp, 0, sizeof sp);
    sp.db = (const unsigned char*)d_db;
    sp.items = c->d_sitems; sp.nitems = nonempty;
    sp.prof = c->d_sprof; sp.qpad = plan.qpad; sp.qlen = qlen;
    sp.ge = scoring->gap_extend; sp.goe = scoring->gap_open + scoring->gap_extend;
    sp.bnd = plan.bnd_per ? c->d_sbnd : nullptr; sp.bnd_per = plan.bnd_per;
    sp.counter = c->d_sctr;
    sp.results = d_results;
    hipLaunchKernelGGL(kSearchAffine[plan.kernel].k, dim3((unsigned)plan.grid), dim3(256), 0, stream, sp);
    HIP_TRY(hipGetLastError());
    c->last_search_affine_grid = plan.grid; c->last_search_affine_kernel = plan.kernel;
    return SW_OK;
}

// the instantiations of the alignment kernel (sw_align_affine.hip), picked by swp::plan_align_affine
using AlignAffineKernel = void (*)(swk::AlignAffineParams);
static constexpr Indexed<AlignAffineKernel> kAlignAffine[] = {
    {swp::align_affine_kernel_index(4), swk::sw_align_affine_wave<4>},
    {swp::align_affine_kernel_index(8), swk::sw_align_affine_wave<8>},
    {swp::align_affine_kernel_index(16), swk::sw_align_affine_wave<16>},
};
static_assert(std::size(kAlignAffine) == swp::kAlignAffineKernels && at_their_indices(kAlignAffine));

// The alignment of chosen hits under affine scoring (csrc/sw_align_affine.hip).  The shape of sw_search_affine_device: no host round
// trip, the order of the hits and the table are uploaded from pinned copies, the profile is built on the device; the plan decides.
int sw_align_affine_device(sw_ctx* c, const char* d_query, int64_t qlen, const char* d_db, const int64_t* offsets, int64_t ntargets,
                           const int64_t* hits, int64_t nhits, const sw_affine* scoring, sw_alignment* d_aln, char* d_ops, int64_t ops_cap,
                           void* stream_) {
    if (!c || !d_query || !d_db || !offsets || !scoring || ntargets < 0) {
        set_err("sw_align_affine_device: NULL pointer or negative target count");
        return SW_EINVAL;
    }
    int64_t maxlen = 0, nonempty = 0, maxhit = 0;
    if (int rc = swh::check_search_affine("sw_align_affine_device", qlen, offsets, ntargets, scoring, &maxlen, &nonempty)) return rc;
    if (int rc = swh::check_align_affine("sw_align_affine_device", offsets, ntargets, hits, nhits, d_aln, d_ops, ops_cap, &maxhit)) return rc;
    if (nhits == 0) return SW_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    DevOrder order(c, stream, false);
    if (order.rc) return order.rc;
    if (!c->align_affine_per_cu_known) {
        for (int k = 0; k < swp::kAlignAffineKernels; ++k)
            HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&c->align_affine_per_cu[k], kAlignAffine[k].k, 256, 0));
        c->align_affine_per_cu_known = true;
    }
    swp::AlignAffineJob aj;
    aj.qlen = qlen; aj.maxhit = maxhit; aj.nhits = nhits; aj.num_cus = c->num_cus; aj.budget_bytes = c->opt_align_workspace_mib << 20;
    std::copy(std::begin(c->align_affine_per_cu), std::end(c->align_affine_per_cu), aj.per_cu);
    const swp::AlignAffinePlan plan = swp::plan_align_affine(aj);
    if (!plan.fits) {
        set_err("sw_align_affine_device: the direction matrix of the longest hit (%lld rows x %lld bytes = %lld bytes) does not fit align_workspace_mib = %lld "
                "(or the 2 GiB a slot may take)", (long long)maxhit, (long long)plan.qpad, (long long)plan.slot_bytes, (long long)c->opt_align_workspace_mib);
        return SW_EINVAL;
    }
    if (c->align_affine_per_cu[plan.kernel] < 1) { set_err("the alignment kernel does not fit a CU on this device"); return SW_EDEVICE; }
    // the order of the hits and the table are uploaded from pinned copies: the previous uploads have to have left them
    if (c->sitems_ev) HIP_TRY(hipEventSynchronize(c->sitems_ev));
    else HIP_TRY(hipEventCreateWithFlags(&c->sitems_ev, hipEventDisableTiming));
    bool fresh = false;
    if (int rc = grow_schedule(c, (size_t)nhits, stream)) return rc;
    if (int rc = grow_workspace((void**)&c->d_sprof, c->sprof_cap, plan.prof_need, 1, 0, stream, fresh)) return rc;
    if (int rc = grow_workspace((void**)&c->d_sbnd, c->sbnd_cap, plan.bnd_need, 4, 0, stream, fresh)) return rc;
    if (int rc = grow_workspace((void**)&c->d_adir, c->adir_cap, plan.dir_need, 1, 0, stream, fresh)) return rc;
    if (!c->d_sctr) HIP_TRY(hipMalloc((void**)&c->d_sctr, 64));
    if (!c->d_submat) HIP_TRY(hipMalloc((void**)&c->d_submat, sizeof(sw_submat)));
    if (!c->h_submat) HIP_TRY(hipHostMalloc((void**)&c->h_submat, sizeof(sw_submat), 0));
    swp::align_schedule(offsets, hits, nhits, c->h_sitems);
    memcpy(c->h_submat, scoring->sub, sizeof(sw_submat));
    HIP_TRY(hipMemcpyAsync(c->d_sitems, c->h_sitems, (size_t)nhits * sizeof(swk::SearchItem), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(c->d_submat, c->h_submat, sizeof(sw_submat), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(c->sitems_ev, stream));
    hipLaunchKernelGGL(swk::sw_search_profile_submat, dim3((unsigned)plan.prof_blocks), dim3(256), 0, stream, (const unsigned char*)d_query, qlen,
                       plan.qpad, c->d_sprof, (const signed char*)c->d_submat);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(c->d_sctr, 0, 4, stream));
    swk::AlignAffineParams ap;
    memset(&ap, 0, sizeof ap);
    ap.db = (const unsigned char*)d_db;
    ap.items = c->d_sitems; ap.nitems = nhits;
    ap.prof = c->d_sprof; ap.qpad = plan.qpad; ap.qlen = qlen;
    ap.ge = scoring->gap_extend; ap.goe = scoring->gap_open + scoring->gap_extend;
    ap.bnd = plan.bnd_per ? c->d_sbnd : nullptr; ap.bnd_per = plan.bnd_per;
    ap.counter = c->d_sctr;
    ap.dir = c->d_adir; ap.slot_bytes = plan.slot_bytes; ap.nslots = plan.slots;
    ap.aln = d_aln; ap.ops = d_ops; ap.ops_cap = ops_cap;
    ap.stamps = (unsigned long long*)(uintptr_t)c->opt_dbg_ptr;
    hipLaunchKernelGGL(kAlignAffine[plan.kernel].k, dim3((unsigned)plan.grid), dim3(256), 0, stream, ap);
    HIP_TRY(hipGetLastError());
    c->last_align_affine_kernel = plan.kernel; c->last_align_affine_slots = plan.slots;
    return SW_OK;
}

// backtrack() of every pair of a batch (serial_smithW.c:262-277 per pair): one lane per pair walks its P from
// d_results[k].max_pos, negates the path and sets d_results[k].path_len; d_paths (optional) receives the visited
// pair-local indices, path_cap per pair.
int sw_batch_traceback_device(sw_ctx* c, void* d_P, int p_elem_bytes, int64_t cols, int64_t rows, int64_t npairs, int64_t* d_paths,
                              int64_t path_cap, sw_result* d_results, void* stream_) {
    if (!c || !d_P || !d_results || cols < 0 || rows < 0 || npairs <= 0 || (p_elem_bytes != 4 && p_elem_bytes != 1) || (d_paths && path_cap <= 0)) {
        set_err("sw_batch_traceback_device: bad argument");
        return SW_EINVAL;
    }
    HIP_TRY(hipSetDevice(c->device));
    const int64_t cells = (cols + 1) * (rows + 1);
    const dim3 grid((unsigned)npairs), block(64);   // one wave per pair (csrc/sw_traceback.hip)
    if (p_elem_bytes == 4)
        hipLaunchKernelGGL(swk::sw_traceback_wave<int32_t>, grid, block, 0, (hipStream_t)stream_, (int32_t*)d_P, cols + 1, rows + 1, cells, (int64_t)-1, d_paths,
                           d_paths ? path_cap : 0, d_results, (int64_t*)nullptr, (unsigned int*)nullptr);
    else
        hipLaunchKernelGGL(swk::sw_traceback_wave<signed char>, grid, block, 0, (hipStream_t)stream_, (signed char*)d_P, cols + 1, rows + 1, cells, (int64_t)-1,
                           d_paths, d_paths ? path_cap : 0, d_results, (int64_t*)nullptr, (unsigned int*)nullptr);
    HIP_TRY(hipGetLastError());
    return SW_OK;
}

int sw_fill_host(sw_ctx* c, const char* a, int64_t cols, const char* b, int64_t rows, const sw_scores* scores,
                 int32_t* H, int32_t* P, sw_result* result) {
    if (!c || !result || cols < 0 || rows < 0 || (cols > 0 && !a) || (rows > 0 && !b)) { set_err("sw_fill_host: bad argument"); return SW_EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    const size_t cells = (size_t)(cols + 1) * (size_t)(rows + 1);
    char *d_a = nullptr, *d_b = nullptr; void *d_H = nullptr, *d_P = nullptr; sw_result* d_r = nullptr;
    int rc = SW_OK;
    auto cleanup = [&]() { (void)hipFree(d_a); (void)hipFree(d_b); if (d_H || d_P) (void)sw_free_outputs(c, d_H, d_P); (void)hipFree(d_r); };
    if (hipMalloc((void**)&d_a, (size_t)cols + 16) != hipSuccess || hipMalloc((void**)&d_b, (size_t)rows + 16) != hipSuccess ||
        hipMalloc((void**)&d_r, sizeof(sw_result)) != hipSuccess) {
        cleanup(); set_err("sw_fill_host: device allocation failed"); return SW_ENOMEM;
    }
    // (H and P from the placement-aware allocator: different classes of the HBM, classified by its store probe -- no trial fills)
    if ((rc = sw_alloc_outputs(c, nullptr, cols, nullptr, rows, scores, 4, 4, 0, &d_H, &d_P, nullptr)) != SW_OK) { cleanup(); return rc; }
    auto copy = [&](void* dst, const void* src, size_t n, hipMemcpyKind kind, const char* what) {
        if (rc != SW_OK || n == 0) return;
        const hipError_t e = hipMemcpy(dst, src, n, kind);
        if (e != hipSuccess) { set_err("sw_fill_host: copying %s failed: %s", what, hipGetErrorString(e)); rc = SW_EDEVICE; }
    };
    copy(d_a, a, (size_t)cols, hipMemcpyHostToDevice, "a");
    copy(d_b, b, (size_t)rows, hipMemcpyHostToDevice, "b");
    if (rc == SW_OK) rc = sw_fill_device(c, d_a, cols, d_b, rows, scores, d_H, 4, (int32_t*)d_P, nullptr, d_r, nullptr);
    if (rc == SW_OK) {
        hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess) { set_err("fill kernel failed: %s", hipGetErrorString(e)); rc = SW_EDEVICE; }
    }
    copy(result, d_r, sizeof(sw_result), hipMemcpyDeviceToHost, "the result");
    if (rc == SW_OK && result->path_len < 0) { set_err("fill kernel: hand-off wait timed out"); rc = SW_ETIMEOUT; }
    // The copy-out is what a host-buffer caller pays: 2 x 4 B per cell over PCIe (16384^2: 2.1 GB, ~40 ms at 55 GB/s against a 0.8 ms
    // fill).  A pageable destination goes through the runtime's staging buffers at a fraction of that: pin the caller's matrices for the
    // duration of the copies where the platform allows it, and run the two copies on two streams.
    if (rc == SW_OK && (H || P)) {
        // Matrices fresh from calloc (what the reference's main hands over, serial_smithW.c:96-103) have no pages yet: whoever writes them first
        // pays 2.1 GB of page faults at 16384^2 -- one thread ~80 ms.  Every byte is about to be overwritten, so the pages are touched first,
        // by several threads (one write per 4 KiB page).
        if (cells * 4 >= (64u << 20)) {
            const unsigned nt = std::max(1u, std::min(std::min(16u, std::thread::hardware_concurrency()), (unsigned)(cells * 4 / (128u << 20))));
            std::vector<std::thread> th;
            for (unsigned t = 0; t < nt; ++t)
                th.emplace_back([=]() {
                    const size_t n = cells * 4, lo = n / nt * t, hi = t + 1 == nt ? n : n / nt * (t + 1);
                    for (int32_t* M : {H, P})
                        if (M) for (size_t o = (lo + 4095) & ~(size_t)4095; o < hi; o += 4096) ((volatile char*)M)[o] = 0;
                });
            for (auto& x : th) x.join();
        }
        const bool pinH = H && cells * 4 >= (64u << 20) && hipHostRegister(H, cells * 4, hipHostRegisterDefault) == hipSuccess;
        const bool pinP = P && cells * 4 >= (64u << 20) && hipHostRegister(P, cells * 4, hipHostRegisterDefault) == hipSuccess;
        (void)hipGetLastError();
        hipStream_t s2 = nullptr;
        if (pinH && pinP && hipStreamCreateWithFlags(&s2, hipStreamNonBlocking) != hipSuccess) { s2 = nullptr; (void)hipGetLastError(); }
        hipError_t e = hipSuccess;
        if (H) e = pinH ? hipMemcpyAsync(H, d_H, cells * 4, hipMemcpyDeviceToHost, nullptr) : hipMemcpy(H, d_H, cells * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess && P) e = pinP ? hipMemcpyAsync(P, d_P, cells * 4, hipMemcpyDeviceToHost, s2) : hipMemcpy(P, d_P, cells * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (s2) (void)hipStreamDestroy(s2);
        if (pinH) (void)hipHostUnregister(H);
        if (pinP) (void)hipHostUnregister(P);
        if (e != hipSuccess) { set_err("sw_fill_host: copying the matrices back failed: %s", hipGetErrorString(e)); rc = SW_EDEVICE; }
    }
    cleanup();
    return rc;
}

// Adaptive dispatch in the spirit of omp_smithW-v7-adaptive.cpp:304-396 (serial / OpenMP / offload chosen per diagonal by
// its length): here the whole problem is sized once.  Below `SW_AUTO_CPU_CELLS` cells the host fill (sw_fill_cpu) wins
// against launch + transfer latency; everything else goes to the GPU of `ctx`.  (Several GPUs: sw_multi_*, the caller
// decides -- a single pair only scales once it is HBM-bound, about 65536^2 and up.)  path_len is set by the traceback.
int sw_align_auto(sw_ctx* c, const char* a, int64_t cols, const char* b, int64_t rows, const sw_scores* scores, int32_t* H, int32_t* P,
                  sw_result* result, int* used_gpu) {
    if (!result || !H || !P) { set_err("sw_align_auto: bad argument"); return SW_EINVAL; }
    const bool gpu = c && (double)cols * (double)rows >= 2.0e5;   // measured: a 512 x 512 host fill takes ~1.3 ms, launch + copies ~0.3 ms
    if (used_gpu) *used_gpu = gpu ? 1 : 0;
    int rc = gpu ? sw_fill_host(c, a, cols, b, rows, scores, H, P, result) : sw_fill_cpu(a, cols, b, rows, scores, H, P, result);
    if (rc != SW_OK) return rc;
    int64_t n = 0;
    rc = sw_traceback_host(P, cols, rows, result->max_pos, nullptr, 0, &n);
    result->path_len = n;
    return rc;
}

static int traceback_launch(sw_ctx* c, void* d_P, int p_elem_bytes, int64_t cols, int64_t rows, int64_t max_pos, int64_t* d_path, int64_t path_cap,
                            sw_result* d_result, int64_t* d_stop, hipStream_t stream, unsigned int* d_pathbits = nullptr) {
    // a big matrix is in no cache when the walk starts: a second wave reads ahead of the walking one (csrc/sw_traceback.hip)
    // (p_elem_bytes 0: a 2-bit matrix, four cells per byte)
    const dim3 block((double)(cols + 1) * (double)(rows + 1) * (p_elem_bytes ? (double)p_elem_bytes : 0.25) > 64.0e6 ? 128 : 64);
    if (p_elem_bytes == 0)
        hipLaunchKernelGGL(swk::sw_traceback_wave<swk::P2Cells>, dim3(1), block, 0, stream, (swk::P2Cells*)d_P, cols + 1, rows + 1, (int64_t)0, max_pos, d_path,
                           d_path ? path_cap : 0, d_result, d_stop, d_pathbits);
    else if (p_elem_bytes == 4)
        hipLaunchKernelGGL(swk::sw_traceback_wave<int32_t>, dim3(1), block, 0, stream, (int32_t*)d_P, cols + 1, rows + 1, (int64_t)0, max_pos, d_path,
                           d_path ? path_cap : 0, d_result, d_stop, (unsigned int*)nullptr);
    else
        hipLaunchKernelGGL(swk::sw_traceback_wave<signed char>, dim3(1), block, 0, stream, (signed char*)d_P, cols + 1, rows + 1, (int64_t)0, max_pos, d_path,
                           d_path ? path_cap : 0, d_result, d_stop, (unsigned int*)nullptr);
    HIP_TRY(hipGetLastError());
    return SW_OK;
}
// (library-internal: the traceback that also reports where the walk stopped -- sw_multi_traceback hops bands with it)
int sw_traceback_stop_device(sw_ctx* c, void* d_P, int p_elem_bytes, int64_t cols, int64_t rows, int64_t max_pos, sw_result* d_result, int64_t* d_stop,
                             void* stream_) {
    if (!c || !d_P || !d_result || !d_stop || max_pos < 0 || max_pos >= (cols + 1) * (rows + 1)) { set_err("sw_traceback_stop_device: bad argument"); return SW_EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    return traceback_launch(c, d_P, p_elem_bytes, cols, rows, max_pos, nullptr, 0, d_result, d_stop, (hipStream_t)stream_);
}

int sw_traceback_device_ex(sw_ctx* c, void* d_P, int p_elem_bytes, int64_t cols, int64_t rows, int64_t max_pos, int64_t* d_path,
                           int64_t path_cap, sw_result* d_result, void* stream_) {
    if (!c || !d_P || !d_result || cols < 0 || rows < 0 || max_pos < 0 || max_pos >= (cols + 1) * (rows + 1) ||
        (p_elem_bytes != 4 && p_elem_bytes != 1)) {
        set_err("sw_traceback_device: bad argument");
        return SW_EINVAL;
    }
    HIP_TRY(hipSetDevice(c->device));
    return traceback_launch(c, d_P, p_elem_bytes, cols, rows, max_pos, d_path, path_cap, d_result, nullptr, (hipStream_t)stream_);
}
int sw_traceback_device(sw_ctx* c, int32_t* d_P, int64_t cols, int64_t rows, int64_t max_pos, int64_t* d_path,
                        int64_t path_cap, sw_result* d_result, void* stream_) {
    return sw_traceback_device_ex(c, d_P, 4, cols, rows, max_pos, d_path, path_cap, d_result, stream_);
}

// Output matrices placed for speed.  Physical HBM falls into a few coarse classes (regions of tens of GiB), and two store streams into
// the SAME class run ~1.4x slower than into different ones; a fill stores H[r][c] and P[r][c] together, so a 16384^2 fill takes 0.79 ms
// with H and P in different classes and 1.05 ms with both in one (profiles/r04_placement_classes_probe.log).  Two
// back-to-back hipMallocs land in one class.  trials <= 0 (the default): candidates for P -- from the second one on behind a temporary
// spacer allocation, so that they come from elsewhere in the HBM -- are CLASSIFIED against H with the two-stream store probe of
// csrc/sw_place.hip (~0.3 ms per candidate, no fill of the caller's problem), the first one in another class is kept.  trials == 1: a plain
// pair.  trials > 1: round 3's search with trial fills of the caller's problem (kept for A/B runs).

static int alloc_outputs_probed(sw_ctx* c, size_t hbytes, size_t pbytes, void** d_H, void** d_P, float* trial_ms, int ntrial_ms) {
    const size_t phase = 4u << 20;
    void* H = nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    auto elapsed_ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    if (hipMalloc(&H, hbytes ? hbytes : 1) != hipSuccess) { (void)hipGetLastError(); set_err("sw_alloc_outputs: %zu bytes do not fit", hbytes); return SW_ENOMEM; }
    // what a spacer can cost: 0.3 ms flat on fresh memory, 30-50 ms per GiB where the driver first wipes memory that was in use before (seen:
    // 32 GiB in 0.2 ms, the next 64 GiB in 3.3 s) -- nothing tells beforehand, so a spacer is only tried while its worst case fits the budget
    double ms_per_gib = 40.0;
    struct Cand { void* base; void* P; float ratio; };
    std::vector<Cand> cands;
    // Candidates for P: three plain ones (a class boundary may be right here), then behind temporary spacer allocations (taken only while
    // 8 GiB of head room remain, released as soon as the candidate behind them exists: the next spacer, of another size, then lands
    // elsewhere).  The classes are regions of 16 .. 120 GiB in the order the driver hands memory out.  What a spacer costs depends on the
    // box: memory that was in use before (by this or an earlier process) is wiped by the driver at ~30 GiB/s when it changes hands, fresh
    // memory costs 0.3 ms per allocation -- so the search runs against a time budget (option "placement_budget_ms", default 1500 ms; a
    // caller that fills many times into the pair raises it) and settles for the best candidate seen when that is spent; a spacer whose
    // allocation alone could overrun the budget (at the wipe rate) is not tried: the default admits spacers up to 37 GiB.  The spacer that worked is
    // remembered per context and tried first next time.
    static const int kSpacerGiB[14] = {0, 0, 0, 32, 64, 16, 96, 48, 128, 24, 80, 8, 160, 112};
    const bool debug = getenv("SW_PLACE_DEBUG") != nullptr;
    // (a matrix of many GiB spans several classes itself: more sample windows, and the best of a few candidates rather than the first good one)
    const bool big = std::max(hbytes, pbytes) > (6ull << 30);
    const float accept = big ? 1.40f : 1.5f;   // another class: ~1.3-1.45; the same class: ~2.0
    int best = -1, rc = SW_OK;
    for (int i = 0; i < 14; ++i) {
        int gib = kSpacerGiB[i];
        if (i == 3 && c->place_spacer_gib > 0) gib = c->place_spacer_gib;                 // what worked last time, first
        else if (i > 3 && gib == c->place_spacer_gib) continue;
        size_t sp = (size_t)gib << 30;
        if (sp && elapsed_ms() > (double)c->opt_place_budget_ms) break;
        if (sp && elapsed_ms() + ms_per_gib * (double)gib > (double)c->opt_place_budget_ms) continue;   // (this spacer alone would overrun the budget: a smaller one may not)
        if (sp) {
            size_t fr = 0, tot = 0;
            if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < sp + pbytes + (8ull << 30)) continue;   // not enough head room for this one
        }
        void* spacer = nullptr;
        const double ts = elapsed_ms();
        if (sp && hipMalloc(&spacer, sp) != hipSuccess) { (void)hipGetLastError(); spacer = nullptr; continue; }
        const double ts1 = elapsed_ms();
        Cand k = {nullptr, nullptr, 0.f};
        const hipError_t e = hipMalloc(&k.base, pbytes + phase);
        const double ts2 = elapsed_ms();
        if (spacer) (void)hipFree(spacer);   // (it only steered where P landed)
        if (sp) ms_per_gib = std::max(ms_per_gib, (elapsed_ms() - ts) / (double)gib);
        if (debug) fprintf(stderr, "sw_alloc_outputs: spacer %d GiB: malloc %.1f ms, candidate malloc %.1f ms, free %.1f ms\n", gib, ts1 - ts, ts2 - ts1, elapsed_ms() - ts2);
        if (e != hipSuccess) { (void)hipGetLastError(); break; }
        // P two MiB out of phase with H modulo 4 MiB (round 1: neighbouring 2 MiB pages of the two streams)
        const uintptr_t want = ((uintptr_t)H + (2u << 20)) % phase;
        k.P = (char*)k.base + (want + phase - ((uintptr_t)k.base % phase)) % phase;
        float ms = 0.f;
        rc = sw_place_pair_ratio(H, hbytes, k.P, pbytes, &k.ratio, &ms);
        cands.push_back(k);
        if (rc != SW_OK) break;
        if (debug) fprintf(stderr, "sw_alloc_outputs: candidate %d (spacer %d GiB): H %p P %p ratio %.3f (%.3f ms), %.1f ms so far\n", i, gib, H, k.P, k.ratio, ms, elapsed_ms());
        if (trial_ms && (int)cands.size() <= ntrial_ms) trial_ms[cands.size() - 1] = ms;
        const int prev_best = best;
        if (best < 0 || k.ratio < cands[best].ratio) best = (int)cands.size() - 1;
        if (big) {   // candidates of tens of GiB: only the best so far stays allocated
            const int loser = best == (int)cands.size() - 1 ? prev_best : (int)cands.size() - 1;
            if (loser >= 0 && cands[loser].base) { (void)hipFree(cands[loser].base); cands[loser].base = nullptr; }
        }
        if (k.ratio < accept) { if (gib) c->place_spacer_gib = gib; break; }
        if (big && cands.size() >= 5) break;   // (... and the best of five)
    }
    // The slide.  Where no candidate is good -- matrices of many GiB span classes themselves, and so does every candidate; on a box whose
    // memory was in use before, the driver hands out the little clean memory it has, all of one class, whatever the spacers (seen: twelve
    // candidates in a row at ratio 2.0) -- P is allocated with slack and SLID inside its own allocation in steps of 4 GiB: one allocation is
    // backed by whatever memory there is, dirty regions of the other classes included, and the classes are regions of 8 .. 120 GiB, so the
    // slide changes which parts of H and P meet.  The best offset is kept; the slack stays allocated while the pair lives.  Many-GiB pairs
    // take up to 32 GiB of slack by themselves (a few per cent of a 288 GB part for fills that are ~25 % faster); smaller pairs only what
    // option "placement_hold_gib" allows (default 0: bench.py, which fills thousands of times into the pair, allows 48).  Only while the
    // budget covers the worst case of that allocation.
    c->last_place_held_gib = 0;
    const size_t hold_max = big ? (32ull << 30) : ((size_t)c->opt_place_hold_gib << 30);
    const bool force_slide = getenv("SW_PLACE_FORCE_SLIDE") != nullptr;   // (tests: take the slide whatever the candidates were)
    if (hold_max >= (8ull << 30) && rc == SW_OK && best >= 0 && (cands[best].ratio >= accept || force_slide)) {
        size_t fr = 0, tot = 0;
        size_t slack = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess && fr > pbytes + (24ull << 30)) slack = std::min<size_t>(hold_max, (fr - pbytes - (16ull << 30)) & ~((4ull << 30) - 1));
        const double worst_ms = 40.0 * (double)((pbytes + slack) >> 30);
        if (slack >= (8ull << 30) && elapsed_ms() + worst_ms <= (double)c->opt_place_budget_ms) {
            void* blk = nullptr;
            if (hipMalloc(&blk, pbytes + slack + phase) == hipSuccess) {
                float bratio = cands[best].ratio; void* bP = nullptr;
                for (size_t off = 0; off <= slack && rc == SW_OK; off += (4ull << 30)) {
                    char* q = (char*)blk + off;
                    const uintptr_t want = ((uintptr_t)H + (2u << 20)) % phase;
                    q += (want + phase - ((uintptr_t)q % phase)) % phase;
                    float r = 0.f, ms = 0.f;
                    rc = sw_place_pair_ratio(H, hbytes, q, pbytes, &r, &ms);
                    if (debug) fprintf(stderr, "sw_alloc_outputs: slide %zu GiB: ratio %.3f, %.1f ms so far\n", off >> 30, r, elapsed_ms());
                    if (rc == SW_OK && (r < bratio || (force_slide && !bP))) { bratio = r; bP = q; }
                    if (r < accept && !force_slide) break;
                }
                if (rc == SW_OK && bP) {
                    Cand k = {blk, bP, bratio};
                    cands.push_back(k);
                    best = (int)cands.size() - 1;
                    c->last_place_held_gib = (int64_t)(slack >> 30);
                } else {
                    (void)hipFree(blk);
                }
            } else {
                (void)hipGetLastError();
            }
        }
    }
    for (int i = 0; i < (int)cands.size(); ++i)
        if ((i != best || rc != SW_OK) && cands[i].base) (void)hipFree(cands[i].base);
    if (rc != SW_OK || best < 0) {
        (void)hipFree(H);
        if (rc == SW_OK) { set_err("sw_alloc_outputs: %zu + %zu bytes do not fit", hbytes, pbytes); rc = SW_ENOMEM; }
        return rc;
    }
    c->last_place_ratio = cands[best].ratio;
    c->pair_ratio[cands[best].P] = cands[best].ratio;
    *d_H = H; *d_P = cands[best].P;
    c->out_base[cands[best].P] = cands[best].base;
    return SW_OK;
}

int sw_alloc_outputs(sw_ctx* c, const char* d_a, int64_t cols, const char* d_b, int64_t rows, const sw_scores* scores, int h_elem_bytes,
                     int p_elem_bytes, int trials, void** d_H, void** d_P, float* trial_ms) {
    if (!c || !d_H || !d_P || cols < 0 || rows < 0 || (h_elem_bytes != 4 && h_elem_bytes != 8) || (p_elem_bytes != 4 && p_elem_bytes != 1) ||
        (trials > 1 && (!d_a || !d_b))) {
        set_err("sw_alloc_outputs: bad argument");
        return SW_EINVAL;
    }
    HIP_TRY(hipSetDevice(c->device));
    const size_t cells = (size_t)(cols + 1) * (size_t)(rows + 1);
    const size_t hbytes = cells * (size_t)h_elem_bytes, pbytes = cells * (size_t)p_elem_bytes;
    // (below half a GiB of output the strip chain bounds a fill, not the stores: a plain pair)
    if (trials <= 0) {
        if (hbytes + pbytes >= (512ull << 20)) {
            for (int i = 0; i < 16 && trial_ms; ++i) trial_ms[i] = 0.f;
            return alloc_outputs_probed(c, hbytes, pbytes, d_H, d_P, trial_ms, 16);
        }
        trials = 1;
    }
    const size_t phase = 4u << 20;
    struct Cand { void* H; void* Pbase; void* P; void* spacer; float ms; };
    std::vector<Cand> cands;
    std::vector<void*> Hs;
    sw_result* d_res = nullptr;
    if (hipMalloc((void**)&d_res, sizeof(sw_result)) != hipSuccess) { set_err("sw_alloc_outputs: allocation failed"); return SW_ENOMEM; }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    int best = -1, rc = SW_OK;
    for (int i = 0; i < trials; ++i) {
        Cand k = {nullptr, nullptr, nullptr, nullptr, 0.f};
        // H stays where it is and the candidates differ in where P lands; half way through a second H is tried as well
        if (i == 0 || (i == trials / 2 && trials >= 6 && hbytes < (8ull << 30))) {
            void* h = nullptr;
            if (hipMalloc(&h, hbytes ? hbytes : 1) != hipSuccess) { (void)hipGetLastError(); if (i == 0) break; }
            else Hs.push_back(h);
        }
        if (Hs.empty()) break;
        k.H = Hs.back();
        // Measured (scripts/ab_arena.py, profiles/r02_placement_arena.log): inside one 96 GiB allocation a 16384^2 fill takes
        // 1.12 ms when H and P lie on different sides of the 64 GiB mark and 1.38-1.47 ms when they share a side, whatever
        // their distance.  So from the second candidate on a spacer of 64 GiB (then 32, 96, 48, 80) is allocated between
        // H and P -- and released again when the search ends: no memory stays held.
        // (a box where five of the first six candidates were slow has been seen: the search goes on to sixteen before it settles for a slow one)
        static const int kSpacerGiB[16] = {0, 64, 96, 32, 128, 48, 160, 80, 16, 112, 144, 24, 176, 72, 104, 56};
        size_t sp = (i > 0 && hbytes < (8ull << 30)) ? (size_t)kSpacerGiB[i % 16] << 30 : 0;
        if (sp) {
            size_t fr = 0, tot = 0;
            if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < sp + pbytes + (8ull << 30)) sp = 0;   // not enough head room: plain candidate
        }
        if (!sp || hipMalloc(&k.spacer, sp) != hipSuccess) { (void)hipGetLastError(); k.spacer = nullptr; }
        if (hipMalloc(&k.Pbase, pbytes + phase) != hipSuccess) { (void)hipGetLastError(); if (k.spacer) (void)hipFree(k.spacer); break; }
        // P two MiB out of phase with H modulo 4 MiB
        const uintptr_t want = ((uintptr_t)k.H + (2u << 20)) % phase;
        const uintptr_t off = (want + phase - ((uintptr_t)k.Pbase % phase)) % phase;
        k.P = (char*)k.Pbase + off;
        if (trials > 1) {
            for (int f = 0; f < 4 && rc == SW_OK; ++f) {
                if (f == 1) (void)hipEventRecord(e0, nullptr);
                rc = sw_fill_device_ex(c, d_a, cols, d_b, rows, scores, k.H, h_elem_bytes, k.P, p_elem_bytes, nullptr, d_res, nullptr);
            }
            (void)hipEventRecord(e1, nullptr);
            if (rc == SW_OK && hipEventSynchronize(e1) != hipSuccess) { set_err("sw_alloc_outputs: trial fill failed"); rc = SW_EDEVICE; }
            if (rc == SW_OK) { (void)hipEventElapsedTime(&k.ms, e0, e1); k.ms /= 3.f; }
        }
        // the spacer only steers where P lands: release it before the next candidate is placed
        if (k.spacer) { (void)hipFree(k.spacer); k.spacer = nullptr; }
        cands.push_back(k);
        if (rc != SW_OK) break;
        if (trial_ms) trial_ms[i] = k.ms;
        if (best < 0 || k.ms < cands[best].ms) best = (int)cands.size() - 1;
        if ((int)cands.size() >= std::min(trials, 6)) {   // several placements seen (there are half-good ones) and clearly in the fast mode: stop looking
            float worst = 0.f;   // (the first candidate also pays the one-time costs of the first launches: not a placement signal)
            for (size_t x = 1; x < cands.size(); ++x) worst = std::max(worst, cands[x].ms);
            if (cands[best].ms < 0.80f * worst) {   // (fast and slow mode are 20-25 % apart; the two-column kernel also has a half-good one in between)
                for (int j = i + 1; j < trials && trial_ms; ++j) trial_ms[j] = 0.f; break; }
        }
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(d_res);
    for (int i = 0; i < (int)cands.size(); ++i) {
        if (cands[i].spacer) (void)hipFree(cands[i].spacer);
        if (i != best || rc != SW_OK) (void)hipFree(cands[i].Pbase);
    }
    for (void* h : Hs)
        if (best < 0 || rc != SW_OK || h != cands[best].H) (void)hipFree(h);
    if (rc != SW_OK) return rc;
    if (best < 0) { set_err("sw_alloc_outputs: %zu + %zu bytes do not fit", hbytes, pbytes); return SW_ENOMEM; }
    *d_H = cands[best].H; *d_P = cands[best].P;
    c->out_base[cands[best].P] = cands[best].Pbase;
    if (hbytes + pbytes >= (512ull << 20)) {   // (which kind of pair it is decides the strip geometry of fills into it: launch_fill)
        float r = 0.f, ms = 0.f;
        if (sw_place_pair_ratio(*d_H, hbytes, *d_P, pbytes, &r, &ms) == SW_OK) { c->pair_ratio[*d_P] = r; c->last_place_ratio = r; }
    }
    return SW_OK;
}

int sw_free_outputs(sw_ctx* c, void* d_H, void* d_P) {
    if (!c) { set_err("sw_free_outputs: bad argument"); return SW_EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    if (d_H) HIP_TRY(hipFree(d_H));
    if (d_P) {
        auto it = c->out_base.find(d_P);
        void* base = (it != c->out_base.end()) ? it->second : d_P;
        if (it != c->out_base.end()) c->out_base.erase(it);
        c->pair_ratio.erase(d_P);
        HIP_TRY(hipFree(base));
    }
    return SW_OK;
}

int sw_device_malloc(sw_ctx* c, size_t bytes, void** d_ptr) {
    if (!c || !d_ptr) { set_err("sw_device_malloc: bad argument"); return SW_EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    if (hipMalloc(d_ptr, bytes ? bytes : 1) != hipSuccess) { set_err("sw_device_malloc: %zu bytes failed", bytes); return SW_ENOMEM; }
    return SW_OK;
}
int sw_device_free(sw_ctx* c, void* d_ptr) {
    if (!c) { set_err("sw_device_free: bad argument"); return SW_EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    if (d_ptr) HIP_TRY(hipFree(d_ptr));
    return SW_OK;
}
int sw_memcpy_h2d(sw_ctx* c, void* d_dst, const void* src, size_t bytes) {
    if (!c || (bytes && (!d_dst || !src))) { set_err("sw_memcpy_h2d: bad argument"); return SW_EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    if (bytes) HIP_TRY(hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice));
    return SW_OK;
}
int sw_memcpy_d2h(sw_ctx* c, void* dst, const void* d_src, size_t bytes) {
    if (!c || (bytes && (!dst || !d_src))) { set_err("sw_memcpy_d2h: bad argument"); return SW_EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    if (bytes) HIP_TRY(hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
    return SW_OK;
}
int sw_synchronize(sw_ctx* c, void* stream_) {
    if (!c) { set_err("sw_synchronize: bad argument"); return SW_EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream_));
    return SW_OK;
}

int sw_p8_to_p32_device(sw_ctx* c, const void* d_P8, int32_t* d_P32, int64_t count, void* stream_) {
    if (!c || count < 0 || (count > 0 && (!d_P8 || !d_P32))) { set_err("sw_p8_to_p32_device: bad argument"); return SW_EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    if (count == 0) return SW_OK;
    const unsigned nb = (unsigned)std::min<int64_t>((count + 256 * 16 - 1) / (256 * 16), 8192);
    hipLaunchKernelGGL(swk::sw_widen_p8, dim3(nb), dim3(256), 0, (hipStream_t)stream_, (const signed char*)d_P8, d_P32, (size_t)count);
    HIP_TRY(hipGetLastError());
    return SW_OK;
}

// ---- 2-bit predecessor matrix: 4 codes per byte + a path bitmap; csrc/sw_kernels.hip, csrc/sw_traceback.hip
int sw_p_to_p2_device(sw_ctx* c, const void* d_P, int p_elem_bytes, void* d_P2, uint32_t* d_pathbits, int64_t count, void* stream_) {
    if (!c || count < 0 || (count > 0 && (!d_P || !d_P2)) || (p_elem_bytes != 1 && p_elem_bytes != 4)) { set_err("sw_p_to_p2_device: bad argument"); return SW_EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    if (count == 0) return SW_OK;
    const unsigned nb = (unsigned)std::min<int64_t>(((count + 31) / 32 + 255) / 256, 16384);
    if (p_elem_bytes == 1) hipLaunchKernelGGL(swk::sw_pack_p2<signed char>, dim3(nb), dim3(256), 0, (hipStream_t)stream_, (const signed char*)d_P, (unsigned char*)d_P2, d_pathbits, (size_t)count);
    else hipLaunchKernelGGL(swk::sw_pack_p2<int32_t>, dim3(nb), dim3(256), 0, (hipStream_t)stream_, (const int32_t*)d_P, (unsigned char*)d_P2, d_pathbits, (size_t)count);
    HIP_TRY(hipGetLastError());
    return SW_OK;
}
int sw_p2_to_p32_device(sw_ctx* c, const void* d_P2, const uint32_t* d_pathbits, int32_t* d_P32, int64_t count, void* stream_) {
    if (!c || count < 0 || (count > 0 && (!d_P2 || !d_P32))) { set_err("sw_p2_to_p32_device: bad argument"); return SW_EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    if (count == 0) return SW_OK;
    const unsigned nb = (unsigned)std::min<int64_t>(((count + 3) / 4 + 255) / 256, 16384);
    hipLaunchKernelGGL(swk::sw_unpack_p2, dim3(nb), dim3(256), 0, (hipStream_t)stream_, (const unsigned char*)d_P2, d_pathbits, d_P32, (size_t)count);
    HIP_TRY(hipGetLastError());
    return SW_OK;
}
int sw_traceback_p2_device(sw_ctx* c, const void* d_P2, int64_t cols, int64_t rows, int64_t max_pos, uint32_t* d_pathbits, int64_t* d_path,
                           int64_t path_cap, sw_result* d_result, void* stream_) {
    if (!c || !d_P2 || !d_result || cols < 0 || rows < 0 || max_pos < 0 || max_pos >= (cols + 1) * (rows + 1)) {
        set_err("sw_traceback_p2_device: bad argument");
        return SW_EINVAL;
    }
    HIP_TRY(hipSetDevice(c->device));
    return traceback_launch(c, const_cast<void*>(d_P2), 0, cols, rows, max_pos, d_path, path_cap, d_result, nullptr, (hipStream_t)stream_, d_pathbits);
}

int sw_row_checksums_device(sw_ctx* c, const void* d_X, int elem_bytes, int64_t rows1, int64_t m, uint64_t* d_cs,
                            void* stream_) {
    if (!c || !d_X || !d_cs || rows1 <= 0 || m <= 0 || (elem_bytes != 4 && elem_bytes != 8 && elem_bytes != 1) || rows1 > 0x7fffffff) {
        set_err("sw_row_checksums_device: bad argument");
        return SW_EINVAL;
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = (hipStream_t)stream_;
    if (elem_bytes == 4)
        hipLaunchKernelGGL((swk::sw_row_checksums<int32_t>), dim3((unsigned)rows1), dim3(256), 0, stream,
                           (const int32_t*)d_X, m, (unsigned long long*)d_cs);
    else if (elem_bytes == 1)
        hipLaunchKernelGGL((swk::sw_row_checksums<signed char>), dim3((unsigned)rows1), dim3(256), 0, stream,
                           (const signed char*)d_X, m, (unsigned long long*)d_cs);
    else
        hipLaunchKernelGGL((swk::sw_row_checksums<int64_t>), dim3((unsigned)rows1), dim3(256), 0, stream,
                           (const int64_t*)d_X, m, (unsigned long long*)d_cs);
    HIP_TRY(hipGetLastError());
    return SW_OK;
}

}  // extern "C"
