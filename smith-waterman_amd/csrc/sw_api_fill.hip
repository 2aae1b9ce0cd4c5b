// sw_api_fill.hip -- the fills of the C-ABI (see include/swhip.h): one matrix, tile or band, batches of pairs, the host-buffer calls.
// launch_fill carries a plan of sw_plan.cpp out; a batch falls back onto it.
#include <cstring>
#include <thread>
#include <vector>
#include "sw_ctx.h"

extern "C" {

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

static int ensure_workspaces(sw_ctx* c, const swp::FillPlan& f, hipStream_t stream) {
    if (int rc = c->d_edge.grow(f.edge_need, stream)) return rc;
    if (c->d_edge.fresh) { HIP_TRY(hipMemsetAsync(c->d_edge, 0, c->d_edge.cap * 8, stream)); c->epoch = 0; }
    if (int rc = c->d_cb.grow(f.cb_need, stream, 64)) return rc;
    if (int rc = c->d_edge4.grow(f.edge4_need, stream)) return rc;
    if (c->d_edge4.fresh) c->epoch8 = 255;   // fresh memory: the next tag wraps and wipes it
    return c->d_priv.grow(f.priv_need, stream);
}

// Advances the 8-bit launch tag of the perm producer's self-tagged edge values and returns the G bias that carries it.  A wrapped tag
// could match stale values: they are wiped.
static unsigned next_gbias(sw_ctx* c, hipStream_t stream) {
    if (++c->epoch8 >= (unsigned)((c->opt.debug_flags & swk::DBG_EPOCH8_WRAP_EARLY) ? 4 : 256)) {
        const unsigned nb = (unsigned)std::max<size_t>(1, std::min<size_t>((c->d_edge4.cap + 255) / 256, 2048));
        hipLaunchKernelGGL(swk::sw_wipe_u32, dim3(nb), dim3(256), 0, stream, c->d_edge4, c->d_edge4.cap);
        c->epoch8 = 1;
    }
    return (c->epoch8 << 24) | 0x10000u;
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
        HIP_TRY(hipMemsetAsync(c->d_edge, 0, c->d_edge.cap * 8, stream));
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
    const size_t cb16 = ((c->d_cb.cap + 15) / 16) * 16;
    unsigned short* d_cb16 = (unsigned short*)(c->d_cb + cb16);
    unsigned char* d_cbc = c->d_cb + cb16 + ((2 * c->d_cb.cap + 15) / 16) * 16;
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
    if (int rc = c->d_bcodes.grow(plan.bcodes_need, stream, 64)) return rc;
    if (int rc = c->d_bnd.grow(plan.bnd_need, stream)) return rc;
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
    if (int rc = c->d_keys.grow((size_t)plan.single_chunk, stream)) return rc;
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

}  // extern "C"
