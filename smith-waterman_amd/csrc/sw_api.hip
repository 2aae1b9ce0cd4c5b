// sw_api.hip -- C-ABI entry points (see include/swhip.h): the context and its options, device memory helpers, conversions of P,
// the traceback launches.  Fills and batches: sw_api_fill.hip; the search family: sw_api_search.hip; the output allocator: sw_place.hip.
#include <cstring>
#include "sw_ctx.h"

DevState g_dev[64];

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
    if (int rc = c->d_key.once(64)) return rc;
    HIP_TRY(hipMemset(c->d_key, 0, 64));
    if (int rc = c->d_alpha.once(2048)) return rc;
    HIP_TRY(hipMemset(c->d_alpha, 0, 2048));
    if (int rc = c->d_part.once(2048 * 32)) return rc;
    if (int rc = c->d_sync.once(256)) return rc;
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
    // the uploads from the pinned copies have to have left them; every Workspace and Staged member is released with the context
    if (c->sitems_ev) { (void)hipEventSynchronize(c->sitems_ev); (void)hipEventDestroy(c->sitems_ev); }
    for (int i = 0; i < 2; ++i) {
        if (c->phtab_ev[i]) { (void)hipEventSynchronize(c->phtab_ev[i]); (void)hipEventDestroy(c->phtab_ev[i]); }
        if (c->h_phtab[i]) (void)hipHostFree(c->h_phtab[i]);
    }
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
    if (!strcmp(name, "align_checkpoint")) {
        if (v < 0 || v > 2) { set_err("align_checkpoint must be 0 (whole direction matrices), 1 (checkpointed) or 2 (checkpointed where 0 would refuse)"); return SW_EINVAL; }
        c->opt_align_checkpoint = v;
        return SW_OK;
    }
    if (!strcmp(name, "align_checkpoint_rows")) {
        if (v != 0 && (v < swp::kAlignCkptMinRows || v > swp::kAlignCkptMaxRows || (v & (v - 1)) != 0)) {
            set_err("align_checkpoint_rows must be 0 (the planner's choice) or a power of two in 64..2^20");
            return SW_EINVAL;
        }
        c->opt_align_checkpoint_rows = v;
        return SW_OK;
    }
    if (!strcmp(name, "search_profile_mib")) {
        if (v < 1 || v > (1ll << 20)) { set_err("search_profile_mib must be 1..2^20"); return SW_EINVAL; }
        c->opt_search_profile_mib = v;
        return SW_OK;
    }
    if (!strcmp(name, "search_results_mib")) {
        if (v < 1 || v > (1ll << 20)) { set_err("search_results_mib must be 1..2^20"); return SW_EINVAL; }
        c->opt_search_results_mib = v;
        return SW_OK;
    }
    if (!strcmp(name, "msa_filter_workspace_mib")) {
        if (v < swp::kMsaFilterMinMib || v > (1ll << 20)) { set_err("msa_filter_workspace_mib must be %lld (one query of top 4096) .. 2^20", (long long)swp::kMsaFilterMinMib); return SW_EINVAL; }
        c->opt_msa_filter_workspace_mib = v;
        return SW_OK;
    }
    if (!strcmp(name, "score_hist_copies")) {
        if (v != 0 && v != 1 && v != 2 && v != 4) { set_err("score_hist_copies must be 0 (the planner's choice), 1, 2 or 4"); return SW_EINVAL; }
        c->opt_score_hist_copies = v;
        return SW_OK;
    }
    if (!strcmp(name, "search_pairs_chunk")) {
        if (v < 1 || v > swp::kSearchPairsChunkMax) { set_err("search_pairs_chunk must be 1..2^31 - 1"); return SW_EINVAL; }
        c->opt_search_pairs_chunk = v;
        return SW_OK;
    }
    if (!strcmp(name, "search_pairs_lanes")) {
        if (v != 32 && v != 16) { set_err("search_pairs_lanes must be 32 (one pair per wave) or 16 (two pairs of a query per wave on packed lanes where the query is eligible)"); return SW_EINVAL; }
        c->opt_search_pairs_lanes = v;
        return SW_OK;
    }
    if (!strcmp(name, "prefilter_lanes")) {
        if (v != 0 && v != 32) { set_err("prefilter_lanes must be 0 (the planner decides) or 32 (never the packed kernel)"); return SW_EINVAL; }
        c->opt_prefilter_lanes = v;
        return SW_OK;
    }
    if (!strcmp(name, "search_lanes")) {
        if (v != 32 && v != 16) { set_err("search_lanes must be 32 (one target per wave) or 16 (two targets per wave on packed lanes where a query is eligible)"); return SW_EINVAL; }
        c->opt_search_lanes = v;
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
    if (!strcmp(name, "debug_edge4_ptr")) return (int64_t)(uintptr_t)c->d_edge4.p;
    if (!strcmp(name, "debug_edge4_cap")) return (int64_t)c->d_edge4.cap;
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
    if (!strcmp(name, "last_align_hits_launches")) return c->last_align_hits_launches;
    if (!strcmp(name, "last_align_hits_tiers")) return c->last_align_hits_tiers;
    if (!strcmp(name, "last_align_hits_slots")) return c->last_align_hits_slots;
    if (!strcmp(name, "last_align_hits_lists")) {   // counted on the device: waits for it, then reads the one word back
        unsigned int n = 0;
        if (!c->d_ahfilled || c->last_align_hits_tiers == 0) return 0;
        if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(&n, c->d_ahfilled, sizeof n, hipMemcpyDeviceToHost) != hipSuccess) return -1;
        return n;
    }
    if (!strcmp(name, "align_workspace_mib")) return c->opt_align_workspace_mib;
    if (!strcmp(name, "align_checkpoint")) return c->opt_align_checkpoint;
    if (!strcmp(name, "align_checkpoint_rows")) return c->opt_align_checkpoint_rows;
    if (!strcmp(name, "last_align_affine_checkpointed")) return c->last_align_affine_checkpointed;
    if (!strcmp(name, "last_align_affine_band_rows")) return c->last_align_affine_band_rows;
    if (!strcmp(name, "last_align_affine_slot_bytes")) return c->last_align_affine_slot_bytes;
    if (!strcmp(name, "last_align_hits_checkpointed")) return c->last_align_hits_checkpointed;
    if (!strcmp(name, "last_align_hits_band_rows")) return c->last_align_hits_band_rows;
    if (!strcmp(name, "search_profile_mib")) return c->opt_search_profile_mib;
    if (!strcmp(name, "last_search_multi_groups")) return c->last_search_multi_groups;
    if (!strcmp(name, "last_search_multi_launches")) return c->last_search_multi_launches;
    if (!strcmp(name, "last_search_multi_grid")) return c->last_search_multi_grid;
    if (!strcmp(name, "search_lanes")) return c->opt_search_lanes;
    if (!strcmp(name, "last_search_multi_packed_launches")) return c->last_search_multi_packed_launches;
    if (!strcmp(name, "search_results_mib")) return c->opt_search_results_mib;
    if (!strcmp(name, "last_search_top_chunks")) return c->last_search_top_chunks;
    if (!strcmp(name, "last_search_top_kernel")) return c->last_search_top_kernel;
    if (!strcmp(name, "last_top_pairs_launches")) return c->last_top_pairs_launches;
    if (!strcmp(name, "last_top_pairs_kernel")) return c->last_top_pairs_kernel;
    if (!strcmp(name, "last_pssm_hits_launches")) return c->last_pssm_hits_launches;
    if (!strcmp(name, "last_msa_hits_launches")) return c->last_msa_hits_launches;
    if (!strcmp(name, "msa_filter_workspace_mib")) return c->opt_msa_filter_workspace_mib;
    if (!strcmp(name, "last_msa_filter_launches")) return c->last_msa_filter_launches;
    if (!strcmp(name, "last_msa_filter_chunks")) return c->last_msa_filter_chunks;
    if (!strcmp(name, "score_hist_copies")) return c->opt_score_hist_copies;
    if (!strcmp(name, "last_score_hist_launches")) return c->last_score_hist_launches;
    if (!strcmp(name, "last_score_hist_slices")) return c->last_score_hist_slices;
    if (!strcmp(name, "last_mask_launches")) return c->last_mask_launches;
    if (!strcmp(name, "last_mask_tiles")) return c->last_mask_tiles;
    if (!strcmp(name, "mask_tile")) return swp::kMaskTile;
    if (!strcmp(name, "last_pssm_weights_launches")) return c->last_pssm_weights_launches;
    if (!strcmp(name, "last_pssm_weights_tiles")) return c->last_pssm_weights_tiles;
    if (!strcmp(name, "search_pairs_chunk")) return c->opt_search_pairs_chunk;
    if (!strcmp(name, "last_search_pairs_groups")) return c->last_search_pairs_groups;
    if (!strcmp(name, "last_search_pairs_chunks")) return c->last_search_pairs_chunks;
    if (!strcmp(name, "last_search_pairs_launches")) return c->last_search_pairs_launches;
    if (!strcmp(name, "search_pairs_lanes")) return c->opt_search_pairs_lanes;
    if (!strcmp(name, "last_search_pairs_packed_launches")) return c->last_search_pairs_packed_launches;
    if (!strcmp(name, "last_search_pairs_packed_items")) {   // counted on the device: waits for it, then reads the one word back
        unsigned long long n = 0;
        if (!c->d_sptotal || c->last_search_pairs_packed_launches == 0) return 0;
        if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(&n, c->d_sptotal, sizeof n, hipMemcpyDeviceToHost) != hipSuccess) return -1;
        return (int64_t)n;
    }
    if (!strcmp(name, "prefilter_lanes")) return c->opt_prefilter_lanes;
    if (!strcmp(name, "last_prefilter_groups")) return c->last_prefilter_groups;
    if (!strcmp(name, "last_prefilter_launches")) return c->last_prefilter_launches;
    if (!strcmp(name, "last_prefilter_packed_launches")) return c->last_prefilter_packed_launches;
    if (!strcmp(name, "debug_search_pairs_items_ptr")) return (int64_t)(uintptr_t)c->d_spitems.p;
    if (!strcmp(name, "placement_budget_ms")) return c->opt_place_budget_ms;
    if (!strcmp(name, "placement_hold_gib")) return c->opt_place_hold_gib;
    if (!strcmp(name, "probe_foreign_pairs")) return c->opt.probe_foreign_pairs;
    if (!strcmp(name, "last_placement_held_gib")) return c->last_place_held_gib;
    if (!strcmp(name, "last_placement_ratio_x1000")) return (int64_t)(c->last_place_ratio * 1000.f);
    return -1;
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

int sw_traceback_p2_device(sw_ctx* c, const void* d_P2, int64_t cols, int64_t rows, int64_t max_pos, uint32_t* d_pathbits, int64_t* d_path,
                           int64_t path_cap, sw_result* d_result, void* stream_) {
    if (!c || !d_P2 || !d_result || cols < 0 || rows < 0 || max_pos < 0 || max_pos >= (cols + 1) * (rows + 1)) {
        set_err("sw_traceback_p2_device: bad argument");
        return SW_EINVAL;
    }
    HIP_TRY(hipSetDevice(c->device));
    return traceback_launch(c, const_cast<void*>(d_P2), 0, cols, rows, max_pos, d_path, path_cap, d_result, nullptr, (hipStream_t)stream_, d_pathbits);
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

}  // extern "C"
