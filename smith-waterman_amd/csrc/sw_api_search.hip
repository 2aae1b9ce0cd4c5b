// sw_api_search.hip -- the search family of the C-ABI (see include/swhip.h): database search, affine search, alignment of hits, and the
// prepared database with its many-query search.  The calls share the workspaces of the context and one protocol around them; each reads
// validate, plan, stage, upload, launch.
#include <cstdint>
#include <cstring>
#include <vector>
#include "sw_ctx.h"

// the instantiations of the search kernel (sw_search.hip), picked by swp::plan_search
using SearchKernel = void (*)(swk::SearchParams);
static constexpr Indexed<SearchKernel> kSearch[] = {
    {swp::search_kernel_index(4, false), swk::sw_search_wave<4, false>}, {swp::search_kernel_index(4, true), swk::sw_search_wave<4, true>},
    {swp::search_kernel_index(8, false), swk::sw_search_wave<8, false>}, {swp::search_kernel_index(8, true), swk::sw_search_wave<8, true>},
    {swp::search_kernel_index(16, false), swk::sw_search_wave<16, false>}, {swp::search_kernel_index(16, true), swk::sw_search_wave<16, true>},
};
static_assert(std::size(kSearch) == swp::kSearchKernels && at_their_indices(kSearch));

// the instantiations of the affine search kernel (sw_search_affine.hip), picked by swp::plan_search_affine
using SearchAffineKernel = void (*)(swk::SearchAffineParams);
static constexpr Indexed<SearchAffineKernel> kSearchAffine[] = {
    {swp::search_affine_kernel_index(4), swk::sw_search_affine_wave<4>},
    {swp::search_affine_kernel_index(8), swk::sw_search_affine_wave<8>},
    {swp::search_affine_kernel_index(16), swk::sw_search_affine_wave<16>},
};
static_assert(std::size(kSearchAffine) == swp::kSearchAffineKernels && at_their_indices(kSearchAffine));

// the instantiations of the alignment kernel (sw_align_affine.hip), picked by swp::plan_align_affine
using AlignAffineKernel = void (*)(swk::AlignAffineParams);
static constexpr Indexed<AlignAffineKernel> kAlignAffine[] = {
    {swp::align_affine_kernel_index(4), swk::sw_align_affine_wave<4>},
    {swp::align_affine_kernel_index(8), swk::sw_align_affine_wave<8>},
    {swp::align_affine_kernel_index(16), swk::sw_align_affine_wave<16>},
};
static_assert(std::size(kAlignAffine) == swp::kAlignAffineKernels && at_their_indices(kAlignAffine));

// the instantiations of the many-query kernel (sw_search_multi.hip), picked by swp::plan_search_multi
using SearchMultiKernel = void (*)(swk::SearchMultiParams);
static constexpr Indexed<SearchMultiKernel> kSearchMulti[] = {
    {swp::search_multi_kernel_index(4), swk::sw_search_affine_multi_wave<4>},
    {swp::search_multi_kernel_index(8), swk::sw_search_affine_multi_wave<8>},
    {swp::search_multi_kernel_index(16), swk::sw_search_affine_multi_wave<16>},
};
static_assert(std::size(kSearchMulti) == swp::kSearchMultiKernels && at_their_indices(kSearchMulti));

// the instantiations of its packed form (sw_search_multi16.hip: two targets per wave), picked by swp::plan_search_multi_lanes
using SearchMultiPackedKernel = void (*)(swk::SearchMultiPackedParams);
static constexpr Indexed<SearchMultiPackedKernel> kSearchMultiPacked[] = {
    {swp::search_multi_kernel_index(4), swk::sw_search_multi_pk_wave<4>},
    {swp::search_multi_kernel_index(8), swk::sw_search_multi_pk_wave<8>},
    {swp::search_multi_kernel_index(16), swk::sw_search_multi_pk_wave<16>},
};
static_assert(std::size(kSearchMultiPacked) == swp::kSearchMultiKernels && at_their_indices(kSearchMultiPacked));

// the instantiations of the hit-table alignment kernel (sw_align_hits.hip), picked by swp::plan_align_hits
using AlignHitsKernel = void (*)(swk::AlignHitsParams);
static constexpr Indexed<AlignHitsKernel> kAlignHits[] = {
    {swp::align_hits_kernel_index(4), swk::sw_align_hits_wave<4>},
    {swp::align_hits_kernel_index(8), swk::sw_align_hits_wave<8>},
    {swp::align_hits_kernel_index(16), swk::sw_align_hits_wave<16>},
};
static_assert(std::size(kAlignHits) == swp::kAlignHitsKernels && at_their_indices(kAlignHits));

// the instantiations of the checkpointed alignment kernels (sw_align_ckpt.hip), picked by swp::plan_align_ckpt / plan_align_hits_ckpt
using AlignCkptKernel = void (*)(swk::AlignCkptParams);
static constexpr Indexed<AlignCkptKernel> kAlignCkpt[] = {
    {swp::align_affine_kernel_index(4), swk::sw_align_ckpt_wave<4>},
    {swp::align_affine_kernel_index(8), swk::sw_align_ckpt_wave<8>},
    {swp::align_affine_kernel_index(16), swk::sw_align_ckpt_wave<16>},
};
static_assert(std::size(kAlignCkpt) == swp::kAlignAffineKernels && at_their_indices(kAlignCkpt));
using AlignHitsCkptKernel = void (*)(swk::AlignHitsCkptParams);
static constexpr Indexed<AlignHitsCkptKernel> kAlignHitsCkpt[] = {
    {swp::align_hits_kernel_index(4), swk::sw_align_hits_ckpt_wave<4>},
    {swp::align_hits_kernel_index(8), swk::sw_align_hits_ckpt_wave<8>},
    {swp::align_hits_kernel_index(16), swk::sw_align_hits_ckpt_wave<16>},
};
static_assert(std::size(kAlignHitsCkpt) == swp::kAlignHitsKernels && at_their_indices(kAlignHitsCkpt));

// the instantiations of the pair-list kernel (sw_search_pairs.hip), picked by swp::plan_search_pairs
using SearchPairsKernel = void (*)(swk::SearchPairsParams);
static constexpr Indexed<SearchPairsKernel> kSearchPairs[] = {
    {swp::search_pairs_kernel_index(4), swk::sw_search_affine_pairs_wave<4>},
    {swp::search_pairs_kernel_index(8), swk::sw_search_affine_pairs_wave<8>},
    {swp::search_pairs_kernel_index(16), swk::sw_search_affine_pairs_wave<16>},
};
static_assert(std::size(kSearchPairs) == swp::kSearchPairsKernels && at_their_indices(kSearchPairs));

// the instantiations of its packed form (sw_search_pairs16.hip: two pairs of a query per wave), picked by swp::plan_search_pairs_lanes
using SearchPairsPackedKernel = void (*)(swk::SearchPairsPackedParams);
static constexpr Indexed<SearchPairsPackedKernel> kSearchPairsPacked[] = {
    {swp::search_pairs_kernel_index(4), swk::sw_search_pairs_pk_wave<4>},
    {swp::search_pairs_kernel_index(8), swk::sw_search_pairs_pk_wave<8>},
    {swp::search_pairs_kernel_index(16), swk::sw_search_pairs_pk_wave<16>},
};
static_assert(std::size(kSearchPairsPacked) == swp::kSearchPairsKernels && at_their_indices(kSearchPairsPacked));

// the instantiations of the pre-filter kernels (sw_prefilter.hip), picked by swp::plan_prefilter
using PrefilterKernel = void (*)(swk::PrefilterParams);
static constexpr Indexed<PrefilterKernel> kPrefilter[] = {
    {swp::prefilter_kernel_index(4, false), swk::sw_prefilter_wave<4>}, {swp::prefilter_kernel_index(4, true), swk::sw_prefilter_wave16<4>},
    {swp::prefilter_kernel_index(8, false), swk::sw_prefilter_wave<8>}, {swp::prefilter_kernel_index(8, true), swk::sw_prefilter_wave16<8>},
    {swp::prefilter_kernel_index(16, false), swk::sw_prefilter_wave<16>}, {swp::prefilter_kernel_index(16, true), swk::sw_prefilter_wave16<16>},
};
static_assert(std::size(kPrefilter) == swp::kPrefilterKernels && at_their_indices(kPrefilter));

// the instantiations of the pair-list selection's sort (sw_top_pairs.hip), picked by swp::plan_top_pairs
using TopPairsSortKernel = void (*)(swk::TopPairsParams);
static constexpr Indexed<TopPairsSortKernel> kTopPairsSort[] = {
    {swp::top_pairs_kernel_index(swp::kTopMax, false), swk::sw_top_pairs_sort<(int)swp::kTopMax, false>},
    {swp::top_pairs_kernel_index(swp::kTopMax, true), swk::sw_top_pairs_sort<(int)swp::kTopMax, true>},
    {swp::top_pairs_kernel_index(2 * swp::kTopMax, true), swk::sw_top_pairs_sort<2 * (int)swp::kTopMax, true>},
};
static_assert(std::size(kTopPairsSort) == swp::kTopPairsKernels && at_their_indices(kTopPairsSort));

// The schedule and the table are uploaded from pinned copies, which a call overwrites: first the previous call's uploads have to have left
// them (sitems_ev, recorded by upload_search_call).  Then the workspaces the three kernels share grow to what this call's plan needs; the
// counter and (for a call with a `table`) the table's two copies are allocated at their first use.  On return c->sitems.h is free to write.
static int stage_search_call(sw_ctx* c, hipStream_t stream, size_t nitems, size_t prof_need, size_t bnd_need, bool table) {
    if (c->sitems_ev) HIP_TRY(hipEventSynchronize(c->sitems_ev));
    else HIP_TRY(hipEventCreateWithFlags(&c->sitems_ev, hipEventDisableTiming));
    if (int rc = c->sitems.grow(nitems, stream, "sw_search_device")) return rc;
    if (int rc = c->d_sprof.grow(prof_need, stream)) return rc;
    if (int rc = c->d_sbnd.grow(bnd_need, stream)) return rc;
    if (int rc = c->d_sctr.once(64)) return rc;
    return table ? c->submat.once() : SW_OK;
}

// Uploads the schedule the caller has written to c->sitems.h, and the table through its pinned copy.  The event is recorded once, behind
// BOTH uploads: whoever has waited for it may overwrite either pinned copy.  The work counter starts every launch at zero.
static int upload_search_call(sw_ctx* c, hipStream_t stream, size_t nitems, const sw_submat* table) {
    if (table) memcpy(c->submat.h, table, sizeof(sw_submat));
    HIP_TRY(hipMemcpyAsync(c->sitems.d, c->sitems.h, nitems * sizeof(swk::SearchItem), hipMemcpyHostToDevice, stream));
    if (table) HIP_TRY(hipMemcpyAsync(c->submat.d, c->submat.h, sizeof(sw_submat), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(c->sitems_ev, stream));
    HIP_TRY(hipMemsetAsync(c->d_sctr, 0, 4, stream));
    return SW_OK;
}

// What the parameters of the three kernels have in common (sw_kernels.h); the rest is zero for the entry point to set.
template <typename Params, typename Plan>
static Params search_params(const sw_ctx* c, const char* d_db, int64_t nitems, int64_t qlen, const Plan& plan) {
    Params p;
    memset(&p, 0, sizeof p);
    p.db = (const unsigned char*)d_db;
    p.items = c->sitems.d; p.nitems = nitems;
    p.prof = c->d_sprof; p.qpad = plan.qpad; p.qlen = qlen;
    p.bnd = plan.bnd_per ? c->d_sbnd : nullptr; p.bnd_per = plan.bnd_per;
    p.counter = c->d_sctr;
    return p;
}

// What every call on a prepared database checks first: the two handles and the pointers it cannot do without (`pointers`: all of them
// are there), and that both handles live on one device.
static int check_db_call(const char* who, const sw_ctx* c, const sw_db* db, bool pointers) {
    if (!c || !db || !pointers) { set_err("%s: NULL pointer", who); return SW_EINVAL; }
    if (db->device != c->device) { set_err("%s: the handle was created on device %d, the context runs on device %d", who, db->device, c->device); return SW_EINVAL; }
    return SW_OK;
}


// The lengths of a call's queries, as the planners of the many-query calls take them.
static std::vector<int64_t> query_lengths(const int64_t* qoffsets, int64_t nqueries) {
    std::vector<int64_t> qlens((size_t)nqueries);
    for (int64_t q = 0; q < nqueries; ++q) qlens[(size_t)q] = qoffsets[q + 1] - qoffsets[q];
    return qlens;
}

// Where the profiles of a many-query call come from.  Everything behind the profile -- the sweeps, the selection, the alignments --
// reads 257 x qpad bytes per query and the two gap costs, whichever source built them:
//   * the queries' letters on the device and a 256 x 256 table on the host (the sw_*_affine_* calls), or
//   * a position-specific scoring matrix on the device (the sw_*_pssm_* calls): one column of `nletters` bytes per query column, and
//     the host's 256-byte code table from a target byte to its place in a column (swh::check_search_pssm builds it).
// A call builds one from its checked arguments; upload_query_table and launch_group_profiles are the only two places that look inside.
struct QuerySource {
    const char* d_queries = nullptr; const sw_submat* sub = nullptr;                                          // letters through a table
    const signed char* d_pssm = nullptr; int nletters = 0, other = 0, smax = 0; unsigned char code[256] = {};   // a PSSM
    int gap_open = 0, gap_extend = 0;
    bool pssm() const { return d_pssm != nullptr; }
    // what bounds a profile byte from above: the table's largest entry; a PSSM's smax (entries are clamped to it, other <= smax)
    int max_entry() const {
        if (pssm()) return smax;
        int m = -128;
        for (int x = 0; x < 256; ++x)
            for (int y = 0; y < 256; ++y) m = std::max<int>(m, sub->s[x][y]);
        return m;
    }
    static QuerySource sequences(const char* d_queries, const sw_affine* sc) {
        QuerySource s;
        s.d_queries = d_queries; s.sub = sc->sub; s.gap_open = sc->gap_open; s.gap_extend = sc->gap_extend;
        return s;
    }
    static QuerySource matrix(const int8_t* d_pssm, const sw_pssm_scoring* sc, const unsigned char (&code)[256]) {
        QuerySource s;
        s.d_pssm = (const signed char*)d_pssm; s.nletters = sc->nletters; s.other = sc->other; s.smax = sc->smax;
        memcpy(s.code, code, sizeof s.code);
        s.gap_open = sc->gap_open; s.gap_extend = sc->gap_extend;
        return s;
    }
};

// The start of a many-query call, behind stage_search_call (which has waited for the last uploads from the pinned copies): the plan's
// table, every entry's qstart taken from the caller's offsets, and behind its entries an optional tail (the pair list's entry_of) go
// through one pinned copy to c->mq.d in one upload; the scoring table follows through its own.  The event is recorded once, behind BOTH
// uploads: whoever has waited for it may overwrite either pinned copy.
static int upload_query_table(sw_ctx* c, hipStream_t stream, const std::vector<swk::MultiQuery>& table, const int64_t* qoffsets, const QuerySource& src,
                              const void* tail = nullptr, size_t tail_bytes = 0) {
    const size_t nq = table.size(), slots = nq + (tail_bytes + sizeof(swk::MultiQuery) - 1) / sizeof(swk::MultiQuery);
    if (int rc = c->mq.grow(slots, stream, "sw_db_search_affine")) return rc;
    for (size_t t = 0; t < nq; ++t) {
        c->mq.h[t] = table[t];
        c->mq.h[t].qstart = qoffsets[table[t].row];
    }
    if (tail_bytes) memcpy(c->mq.h + nq, tail, tail_bytes);
    // a PSSM's code table takes the place of the scoring table in the same two copies: its first 256 bytes
    const size_t table_bytes = src.pssm() ? sizeof src.code : sizeof(sw_submat);
    memcpy(c->submat.h, src.pssm() ? (const void*)src.code : (const void*)src.sub, table_bytes);
    HIP_TRY(hipMemcpyAsync(c->mq.d, c->mq.h, slots * sizeof(swk::MultiQuery), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(c->submat.d, c->submat.h, table_bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(c->sitems_ev, stream));
    return SW_OK;
}

// The profiles of a group's queries (the table entries grp.q0 .. grp.q0 + grp.nq - 1) in one launch: every query's profile in shares of
// about 16 KiB, over at most 4096 workgroups; from the letters and the table, or from the PSSM (csrc/sw_pssm.hip: shares of whole tiles).
template <typename Group>
static int launch_group_profiles(sw_ctx* c, hipStream_t stream, const QuerySource& src, const Group& grp) {
    const int parts = (int)std::clamp<int64_t>(grp.prof_bytes / grp.nq / 16384, 1, 4096);
    const unsigned blocks = (unsigned)std::min<int64_t>(grp.nq * parts, 4096);
    if (src.pssm())
        hipLaunchKernelGGL(swk::sw_search_profile_pssm_multi, dim3(blocks), dim3(256), swk::sw_pssm_profile_lds_bytes(src.nletters), stream, src.d_pssm,
                           c->mq.d + grp.q0, grp.nq, parts, c->d_sprof, (const unsigned char*)c->submat.d, src.nletters, src.other, src.smax);
    else
        hipLaunchKernelGGL(swk::sw_search_profile_submat_multi, dim3(blocks), dim3(256), 0, stream, (const unsigned char*)src.d_queries, c->mq.d + grp.q0,
                           grp.nq, parts, c->d_sprof, (const signed char*)c->submat.d);
    HIP_TRY(hipGetLastError());
    return SW_OK;
}

// The twins of a launch -- the 32-bit kernel's parameters and those of its packed or checkpointed form (sw_kernels.h) -- are filled by
// one template each: the fields the twins share; the rest is zero, and what only one of them has is set where it is launched.
//
// A launch cut by target ranks (SearchMultiParams, SearchMultiPackedParams, the head of PrefilterParams): its part of the handle's
// schedule and of the query table.
template <typename Params, typename Launch>
static Params rank_launch_params(const sw_ctx* c, const sw_db* db, const Launch& l) {
    Params p;
    memset(&p, 0, sizeof p);
    p.db = (const unsigned char*)db->d_db;
    p.items = db->d_items; p.rank0 = l.rank0;
    p.queries = c->mq.d + l.q0; p.nq = (unsigned)l.nq; p.nitems = l.items;
    p.prof = c->d_sprof; p.ntargets = db->ntargets;
    p.bnd = l.bnd_per ? c->d_sbnd : nullptr; p.bnd_per = l.bnd_per;
    return p;
}
template <typename Params>
static Params search_multi_params(const sw_ctx* c, const sw_db* db, const QuerySource& src, const swp::MultiLanesLaunch& l, sw_result* d_results) {
    Params p = rank_launch_params<Params>(c, db, l);
    p.ge = src.gap_extend; p.goe = src.gap_open + src.gap_extend;
    p.counter = c->d_sctr;
    p.results = d_results;
    return p;
}
// The score launch of a class of a pair list (SearchPairsParams, SearchPairsPackedParams); items, list and counter are the caller's.
template <typename Params>
static Params search_pairs_params(const sw_ctx* c, const sw_db* db, const sw_affine* scoring, const swp::PairsLanesLaunch& l, sw_result* d_results) {
    Params p;
    memset(&p, 0, sizeof p);
    p.db = (const unsigned char*)db->d_db;
    p.queries = c->mq.d; p.prof = c->d_sprof;
    p.ge = scoring->gap_extend; p.goe = scoring->gap_open + scoring->gap_extend;
    p.bnd = l.bnd_per ? c->d_sbnd : nullptr; p.bnd_per = l.bnd_per;
    p.results = d_results;
    return p;
}
// A tier's launch of the hit-table alignment (AlignHitsParams, AlignHitsCkptParams); log_band is the caller's.
template <typename Params>
static Params align_hits_params(sw_ctx* c, const sw_db* db, const QuerySource& src, const swp::AlignHitsGroup& grp, const swp::AlignHitsLaunch& l,
                                sw_alignment* d_aln, char* d_ops, int64_t ops_cap) {
    Params p;
    memset(&p, 0, sizeof p);
    p.db = (const unsigned char*)db->d_db;
    p.items = c->d_ahitems + grp.cls[l.kernel].item0;
    p.counts = c->d_ahctl->count[l.kernel]; p.tier = l.tier;
    p.queries = c->mq.d + grp.q0; p.prof = c->d_sprof;
    p.ge = src.gap_extend; p.goe = src.gap_open + src.gap_extend;
    p.bnd = l.bnd_per ? c->d_sbnd : nullptr; p.bnd_per = l.bnd_per;
    p.counter = &c->d_ahctl->work[l.kernel][l.tier];
    p.dir = c->d_adir; p.slot_bytes = l.slot_bytes; p.nslots = l.slots;
    p.aln = d_aln; p.ops = d_ops; p.ops_cap = ops_cap;
    return p;
}
// The alignment of one query's hits (AlignAffineParams, AlignCkptParams), on search_params; log_band is the caller's.
template <typename Params>
static Params align_affine_params(const sw_ctx* c, const char* d_db, int64_t nhits, int64_t qlen, const swp::AlignAffinePlan& plan, const sw_affine* scoring,
                                  sw_alignment* d_aln, char* d_ops, int64_t ops_cap) {
    Params p = search_params<Params>(c, d_db, nhits, qlen, plan);
    p.ge = scoring->gap_extend; p.goe = scoring->gap_open + scoring->gap_extend;
    p.dir = c->d_adir; p.slot_bytes = plan.slot_bytes; p.nslots = plan.slots;
    p.aln = d_aln; p.ops = d_ops; p.ops_cap = ops_cap;
    p.stamps = (unsigned long long*)(uintptr_t)c->opt_dbg_ptr;
    return p;
}

// The many-query search of checked arguments into `d_results` (nqueries x ntargets, nqueries > 0, ntargets > 0): what sw_db_search_affine
// and sw_db_search_pssm do for a whole call and their _top forms for every chunk of one.  The caller holds the device's launch order
// (DevOrder).
static int run_search_multi(sw_ctx* c, const sw_db* db, const QuerySource& src, const int64_t* qoffsets, int64_t nqueries, sw_result* d_results,
                            hipStream_t stream) {
    // empty targets keep the zeros: {0, 0, 0}
    HIP_TRY(hipMemsetAsync(d_results, 0, (size_t)nqueries * (size_t)db->ntargets * sizeof(sw_result), stream));
    c->last_search_multi_packed_launches = 0;   // (a call that launches no kernel reports none)
    if (db->nonempty == 0) return SW_OK;
    if (int rc = c->search_multi_per_cu.once(kSearchMulti)) return rc;
    const bool lanes16 = c->opt_search_lanes == 16;
    if (lanes16)
        if (int rc = c->search_multi_packed_per_cu.once(kSearchMultiPacked)) return rc;
    const std::vector<int64_t> qlens = query_lengths(qoffsets, nqueries);
    swp::SearchMultiLanesJob mj;
    mj.qlens = qlens.data(); mj.nqueries = nqueries; mj.longest = db->longest; mj.nonempty = db->nonempty; mj.num_cus = c->num_cus;
    mj.budget_bytes = c->opt_search_profile_mib << 20;
    std::copy(std::begin(c->search_multi_per_cu), std::end(c->search_multi_per_cu), mj.per_cu);
    mj.lanes = (int)c->opt_search_lanes; mj.gap_open = src.gap_open; mj.gap_extend = src.gap_extend;
    if (lanes16) {   // (the 32-bit plan asks for neither)
        std::copy(std::begin(c->search_multi_packed_per_cu), std::end(c->search_multi_packed_per_cu), mj.packed_per_cu);
        mj.max_entry = src.max_entry();
    }
    const swp::SearchMultiLanesPlan plan = swp::plan_search_multi_lanes(mj);
    for (const swp::MultiLanesLaunch& l : plan.launch)
        if ((l.packed ? c->search_multi_packed_per_cu : c->search_multi_per_cu)[l.kernel] < 1) { set_err("the many-query search kernel does not fit a CU on this device"); return SW_EDEVICE; }
    if (int rc = stage_search_call(c, stream, 0, plan.prof_need, plan.bnd_need, true)) return rc;
    if (int rc = upload_query_table(c, stream, plan.table, qoffsets, src)) return rc;
    size_t li = 0;
    for (size_t g = 0; g < plan.group.size(); ++g) {
        const swp::MultiGroup& grp = plan.group[g];
        if (int rc = launch_group_profiles(c, stream, src, grp)) return rc;
        for (; li < plan.launch.size() && plan.launch[li].group == (int)g; ++li) {
            const swp::MultiLanesLaunch& l = plan.launch[li];
            HIP_TRY(hipMemsetAsync(c->d_sctr, 0, 4, stream));   // the work counter starts every launch at zero
            if (l.packed) {   // two targets per wave: the ranks rank0 .. rank0 + nranks - 1 in pairs
                swk::SearchMultiPackedParams kp = search_multi_params<swk::SearchMultiPackedParams>(c, db, src, l, d_results);
                kp.nranks = l.nranks;
                hipLaunchKernelGGL(kSearchMultiPacked[l.kernel].k, dim3((unsigned)l.grid), dim3(256), 0, stream, kp);
            } else {
                const swk::SearchMultiParams sp = search_multi_params<swk::SearchMultiParams>(c, db, src, l, d_results);
                hipLaunchKernelGGL(kSearchMulti[l.kernel].k, dim3((unsigned)l.grid), dim3(256), 0, stream, sp);
            }
            HIP_TRY(hipGetLastError());
            c->last_search_multi_grid = l.grid;
        }
    }
    c->last_search_multi_groups = (int64_t)plan.group.size(); c->last_search_multi_launches = (int64_t)plan.launch.size();
    c->last_search_multi_packed_launches = plan.packed_launches;
    return SW_OK;
}

// The selection of one chunk (sw_search_top.hip): rows [0, nq) of `d_table` into d_hits / d_nhits, by the plan's kernel.  Everything
// follows the stream; the histograms are wiped first, and every scan leaves them wiped for the next pass.
static int select_top(sw_ctx* c, const swp::SearchTopPlan& plan, const sw_result* d_table, int64_t nq, int64_t ntargets, int64_t top, int64_t min_score,
                      sw_hit* d_hits, int64_t* d_nhits, hipStream_t stream) {
    swk::TopParams tp;
    memset(&tp, 0, sizeof tp);
    tp.results = d_table; tp.ntargets = ntargets; tp.nq = (unsigned)nq;
    tp.wgs_row = (unsigned)plan.wgs_row; tp.slice = plan.slice; tp.tbits = plan.tbits;
    tp.top = top; tp.min_score = min_score;
    tp.hist = c->d_thist; tp.state = c->d_tstate;
    tp.hits = d_hits; tp.nhits = d_nhits;
    if (plan.kernel == 1) {
        const unsigned row_grid = (unsigned)(nq * plan.wgs_row);
        HIP_TRY(hipMemsetAsync(c->d_thist, 0, ((size_t)nq << swp::kTopDigitBits) * sizeof(unsigned int), stream));
        for (int ps = 0; ps < plan.npasses; ++ps) {
            tp.shift = plan.pass[ps].shift; tp.bits = plan.pass[ps].bits; tp.first = ps == 0;
            hipLaunchKernelGGL(swk::sw_top_hist, dim3(row_grid), dim3(256), 0, stream, tp);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(swk::sw_top_scan, dim3((unsigned)nq), dim3(256), 0, stream, tp);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(swk::sw_top_compact, dim3(row_grid), dim3(256), 0, stream, tp);
        HIP_TRY(hipGetLastError());
        tp.selected = 1;
    }
    hipLaunchKernelGGL(swk::sw_top_sort, dim3((unsigned)nq), dim3(256), 0, stream, tp);
    HIP_TRY(hipGetLastError());
    return SW_OK;
}

// The score histogram of rows [0, nq) of `d_table` (sw_score_hist.hip) into d_hist, nq x 40 x 256 counters: zeroed on the stream, then
// one launch as swp::plan_score_hist cuts it.  The caller has checked the arguments and holds the device's launch order.
static int launch_score_hist(sw_ctx* c, const sw_db* db, const sw_result* d_table, int64_t nq, int shift, uint32_t* d_hist, hipStream_t stream) {
    HIP_TRY(hipMemsetAsync(d_hist, 0, (size_t)nq * swp::kScoreHistCells * sizeof(uint32_t), stream));
    swp::ScoreHistJob hj;
    hj.nqueries = nq; hj.ntargets = db->ntargets; hj.num_cus = c->num_cus; hj.copies = (int)c->opt_score_hist_copies;
    const swp::ScoreHistPlan plan = swp::plan_score_hist(hj);
    if (plan.grid == 0) return SW_OK;
    if (plan.lds_bytes > c->score_hist_lds_set) {   // (beyond 64 KiB a kernel asks for its dynamic LDS)
        HIP_TRY(hipFuncSetAttribute((const void*)swk::sw_score_hist, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes));
        c->score_hist_lds_set = (int)plan.lds_bytes;
    }
    swk::ScoreHistParams kp;
    memset(&kp, 0, sizeof kp);
    kp.results = d_table; kp.offsets = db->d_offsets; kp.ntargets = db->ntargets; kp.nq = nq;
    kp.slices_per_query = plan.slices_per_query; kp.slice = plan.slice; kp.items = plan.items;
    kp.shift = shift; kp.copies = plan.copies; kp.hist = d_hist;
    hipLaunchKernelGGL(swk::sw_score_hist, dim3((unsigned)plan.grid), dim3(256), (size_t)plan.lds_bytes, stream, kp);
    HIP_TRY(hipGetLastError());
    c->last_score_hist_launches += plan.launches; c->last_score_hist_slices = plan.slices_per_query;
    return SW_OK;
}

// What the two selecting calls check alike, the plan of the call and the workspaces of the radix select.
static int plan_top_call(sw_ctx* c, const char* who, int64_t nqueries, int64_t ntargets, int64_t top, const void* d_hits, const void* d_nhits,
                         int64_t budget_bytes, swp::SearchTopPlan& plan) {
    static_assert(SW_TOP_MAX == swp::kTopMax);
    if (top < 1 || top > SW_TOP_MAX) { set_err("%s: top = %lld is out of range 1..%d", who, (long long)top, SW_TOP_MAX); return SW_EINVAL; }
    if (!d_hits || !d_nhits) { set_err("%s: NULL d_hits or d_nhits", who); return SW_EINVAL; }
    if (ntargets >= (1ll << 31)) { set_err("%s: %lld targets, the selection takes fewer than 2^31", who, (long long)ntargets); return SW_EINVAL; }
    if (nqueries == 0) return SW_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (c->top_hist_per_cu == 0) HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&c->top_hist_per_cu, swk::sw_top_hist, 256, 0));
    swp::SearchTopJob tj;
    tj.nqueries = nqueries; tj.ntargets = ntargets; tj.top = top; tj.budget_bytes = budget_bytes; tj.num_cus = c->num_cus; tj.per_cu = c->top_hist_per_cu;
    plan = swp::plan_search_top(tj);
    return SW_OK;
}

// ... grown under the device's launch order; `rows`: the call keeps the result rows of a chunk in the context's workspace
static int grow_top_workspaces(sw_ctx* c, const swp::SearchTopPlan& plan, bool rows, hipStream_t stream) {
    if (int rc = c->d_thist.grow(plan.hist_need, stream)) return rc;
    if (int rc = c->d_tstate.grow(plan.state_need, stream)) return rc;
    if (rows)
        if (int rc = c->d_tres.grow(plan.results_need, stream)) return rc;
    return SW_OK;
}

// What sw_top_hits_pairs_device and sw_db_search_affine_top_prefiltered check alike, and the plan of the selection.
static int plan_top_pairs_call(sw_ctx* c, const char* who, int64_t npairs, int64_t nqueries, int64_t ntargets, int64_t top, const void* d_hits,
                               const void* d_nhits, swp::TopPairsPlan& plan) {
    static_assert(SW_TOP_MAX == swp::kTopMax);
    if (!d_hits || !d_nhits) { set_err("%s: NULL d_hits or d_nhits", who); return SW_EINVAL; }
    swp::TopPairsJob tj;
    tj.npairs = npairs; tj.nqueries = nqueries; tj.ntargets = ntargets; tj.top = top; tj.num_cus = c->num_cus;
    plan = swp::plan_top_pairs(tj);
    if (plan.refused) {
        set_err("%s: %s (npairs = %lld, nqueries = %lld, ntargets = %lld, top = %lld, SW_TOP_MAX = %d)", who, plan.refused, (long long)npairs,
                (long long)nqueries, (long long)ntargets, (long long)top, SW_TOP_MAX);
        return SW_EINVAL;
    }
    return SW_OK;
}

// ... grown under the device's launch order
static int grow_top_pairs_workspaces(sw_ctx* c, const swp::TopPairsPlan& plan, hipStream_t stream) {
    if (int rc = c->d_tpkeys.grow(plan.keys_need, stream)) return rc;
    if (int rc = c->d_tppos.grow(plan.pos_need, stream)) return rc;
    if (int rc = c->d_tpseg.grow(plan.seg_need, stream)) return rc;
    return SW_OK;
}

extern "C" {

// Database search (csrc/sw_search.hip): for every target k the reference fill of query x target k, score and arg-max only.  No host
// round trip: the lengths come from the host offsets, the profile is built on the device from the query.
int sw_search_device(sw_ctx* c, const char* d_query, int64_t qlen, const char* d_db, const int64_t* offsets, int64_t ntargets,
                     const sw_scores* scores, sw_result* d_results, void* stream_) {
    const sw_scores* sc = scores ? scores : &kDefaultScores;
    if (!c || !d_query || !d_db || !offsets || !d_results || ntargets < 0) { set_err("sw_search_device: NULL pointer or negative target count"); return SW_EINVAL; }
    int64_t maxlen = 0, nonempty = 0;
    if (int rc = swh::check_targets("sw_search_device", qlen, offsets, ntargets, &maxlen, &nonempty)) return rc;
    if (int rc = check_dims(qlen, maxlen, sc)) return rc;
    if (ntargets == 0) return SW_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    DevOrder order(c, stream, false);
    if (order.rc) return order.rc;
    // empty targets keep the zeros: {0, 0, 0}
    HIP_TRY(hipMemsetAsync(d_results, 0, (size_t)ntargets * sizeof(sw_result), stream));
    if (nonempty == 0) return SW_OK;
    if (int rc = c->search_per_cu.once(kSearch)) return rc;
    swp::SearchJob sj;
    sj.qlen = qlen; sj.maxlen = maxlen; sj.ntargets = nonempty; sj.match = sc->match; sj.mismatch = sc->mismatch; sj.gap = sc->gap;
    const swp::SearchPlan plan = swp::plan_search(sj, device_facts(c));
    if (c->search_per_cu[plan.kernel] < 1) { set_err("the search kernel does not fit a CU on this device"); return SW_EDEVICE; }
    if (int rc = stage_search_call(c, stream, (size_t)nonempty, plan.prof_need, plan.bnd_need, false)) return rc;
    swp::search_schedule(offsets, ntargets, c->sitems.h);
    if (int rc = upload_search_call(c, stream, (size_t)nonempty, nullptr)) return rc;
    hipLaunchKernelGGL(swk::sw_search_profile, dim3((unsigned)plan.prof_blocks), dim3(256), 0, stream, (const unsigned char*)d_query, qlen, plan.qpad,
                       c->d_sprof, sc->match, sc->mismatch, plan.wide ? 1 : 0);
    HIP_TRY(hipGetLastError());
    swk::SearchParams sp = search_params<swk::SearchParams>(c, d_db, nonempty, qlen, plan);
    sp.match = sc->match; sp.mismatch = sc->mismatch; sp.ngap = -sc->gap;
    sp.results = d_results;
    hipLaunchKernelGGL(kSearch[plan.kernel].k, dim3((unsigned)plan.grid), dim3(256), 0, stream, sp);
    HIP_TRY(hipGetLastError());
    c->last_search_grid = plan.grid; c->last_search_kernel = plan.kernel;
    return SW_OK;
}

// Database search with a substitution matrix and affine gaps (csrc/sw_search_affine.hip).  The shape of sw_search_device: no host
// round trip, the schedule and the 64 KiB table are uploaded from pinned copies, the profile is built on the device.
int sw_search_affine_device(sw_ctx* c, const char* d_query, int64_t qlen, const char* d_db, const int64_t* offsets, int64_t ntargets,
                            const sw_affine* scoring, sw_result* d_results, void* stream_) {
    if (!c || !d_query || !d_db || !offsets || !d_results || !scoring || ntargets < 0) { set_err("sw_search_affine_device: NULL pointer or negative target count"); return SW_EINVAL; }
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
    if (int rc = c->search_affine_per_cu.once(kSearchAffine)) return rc;
    swp::SearchAffineJob sj;
    sj.qlen = qlen; sj.maxlen = maxlen; sj.ntargets = nonempty; sj.num_cus = c->num_cus;
    std::copy(std::begin(c->search_affine_per_cu), std::end(c->search_affine_per_cu), sj.per_cu);
    const swp::SearchAffinePlan plan = swp::plan_search_affine(sj);
    if (c->search_affine_per_cu[plan.kernel] < 1) { set_err("the affine search kernel does not fit a CU on this device"); return SW_EDEVICE; }
    if (int rc = stage_search_call(c, stream, (size_t)nonempty, plan.prof_need, plan.bnd_need, true)) return rc;
    swp::search_schedule(offsets, ntargets, c->sitems.h);
    if (int rc = upload_search_call(c, stream, (size_t)nonempty, scoring->sub)) return rc;
    hipLaunchKernelGGL(swk::sw_search_profile_submat, dim3((unsigned)plan.prof_blocks), dim3(256), 0, stream, (const unsigned char*)d_query, qlen,
                       plan.qpad, c->d_sprof, (const signed char*)c->submat.d);
    HIP_TRY(hipGetLastError());
    swk::SearchAffineParams sp = search_params<swk::SearchAffineParams>(c, d_db, nonempty, qlen, plan);
    sp.ge = scoring->gap_extend; sp.goe = scoring->gap_open + scoring->gap_extend;
    sp.results = d_results;
    hipLaunchKernelGGL(kSearchAffine[plan.kernel].k, dim3((unsigned)plan.grid), dim3(256), 0, stream, sp);
    HIP_TRY(hipGetLastError());
    c->last_search_affine_grid = plan.grid; c->last_search_affine_kernel = plan.kernel;
    return SW_OK;
}

// The alignment of chosen hits under affine scoring (csrc/sw_align_affine.hip; checkpointed: csrc/sw_align_ckpt.hip).  The shape of
// sw_search_affine_device: no host round trip, the order of the hits and the table are uploaded from pinned copies, the profile is built
// on the device; the plan decides.  "align_checkpoint" decides once, here, before any launch, whether the call runs on whole direction
// matrices or checkpointed.
int sw_align_affine_device(sw_ctx* c, const char* d_query, int64_t qlen, const char* d_db, const int64_t* offsets, int64_t ntargets,
                           const int64_t* hits, int64_t nhits, const sw_affine* scoring, sw_alignment* d_aln, char* d_ops, int64_t ops_cap,
                           void* stream_) {
    if (!c || !d_query || !d_db || !offsets || !scoring || ntargets < 0) { set_err("sw_align_affine_device: NULL pointer or negative target count"); return SW_EINVAL; }
    int64_t maxlen = 0, nonempty = 0, maxhit = 0;
    if (int rc = swh::check_search_affine("sw_align_affine_device", qlen, offsets, ntargets, scoring, &maxlen, &nonempty)) return rc;
    if (int rc = swh::check_align_affine("sw_align_affine_device", offsets, ntargets, hits, nhits, d_aln, d_ops, ops_cap, &maxhit)) return rc;
    if (nhits == 0) return SW_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    DevOrder order(c, stream, false);
    if (order.rc) return order.rc;
    if (int rc = c->align_affine_per_cu.once(kAlignAffine)) return rc;
    swp::AlignCkptJob aj;
    aj.qlen = qlen; aj.maxhit = maxhit; aj.nhits = nhits; aj.num_cus = c->num_cus; aj.budget_bytes = c->opt_align_workspace_mib << 20;
    aj.band_rows = c->opt_align_checkpoint_rows;
    std::copy(std::begin(c->align_affine_per_cu), std::end(c->align_affine_per_cu), aj.per_cu);
    swp::AlignCkptPlan plan;   // (band_rows and log_band stay 0 on whole matrices)
    static_cast<swp::AlignAffinePlan&>(plan) = swp::plan_align_affine(aj);
    c->last_align_affine_checkpointed = c->last_align_affine_band_rows = 0;
    const bool ckpt = swp::align_use_ckpt(c->opt_align_checkpoint, plan.fits);
    if (ckpt) {
        if (int rc = c->align_ckpt_per_cu.once(kAlignCkpt)) return rc;
        std::copy(std::begin(c->align_ckpt_per_cu), std::end(c->align_ckpt_per_cu), aj.per_cu);
        plan = swp::plan_align_ckpt(aj);
    }
    if (!plan.fits && ckpt) {
        set_err("sw_align_affine_device: the checkpointed slot of the longest hit (%lld rows against %lld padded columns in bands of %lld rows = %lld bytes) "
                "does not fit align_workspace_mib = %lld (or the 2 GiB a slot may take)", (long long)maxhit, (long long)plan.qpad, (long long)plan.band_rows,
                (long long)plan.slot_bytes, (long long)c->opt_align_workspace_mib);
        return SW_EINVAL;
    }
    if (!plan.fits) {
        set_err("sw_align_affine_device: the direction matrix of the longest hit (%lld rows x %lld bytes = %lld bytes) does not fit align_workspace_mib = %lld "
                "(or the 2 GiB a slot may take)", (long long)maxhit, (long long)plan.qpad, (long long)plan.slot_bytes, (long long)c->opt_align_workspace_mib);
        return SW_EINVAL;
    }
    if ((ckpt ? c->align_ckpt_per_cu : c->align_affine_per_cu)[plan.kernel] < 1) {
        set_err("%s", ckpt ? "the checkpointed alignment kernel does not fit a CU on this device" : "the alignment kernel does not fit a CU on this device");
        return SW_EDEVICE;
    }
    if (int rc = stage_search_call(c, stream, (size_t)nhits, plan.prof_need, plan.bnd_need, true)) return rc;
    // the direction workspace: per slot one direction matrix, or a band and its checkpoint rows
    if (int rc = c->d_adir.grow(plan.dir_need, stream)) return rc;
    swp::align_schedule(offsets, hits, nhits, c->sitems.h);
    if (int rc = upload_search_call(c, stream, (size_t)nhits, scoring->sub)) return rc;
    hipLaunchKernelGGL(swk::sw_search_profile_submat, dim3((unsigned)plan.prof_blocks), dim3(256), 0, stream, (const unsigned char*)d_query, qlen,
                       plan.qpad, c->d_sprof, (const signed char*)c->submat.d);
    HIP_TRY(hipGetLastError());
    if (ckpt) {
        swk::AlignCkptParams ap = align_affine_params<swk::AlignCkptParams>(c, d_db, nhits, qlen, plan, scoring, d_aln, d_ops, ops_cap);
        ap.log_band = plan.log_band;
        hipLaunchKernelGGL(kAlignCkpt[plan.kernel].k, dim3((unsigned)plan.grid), dim3(256), 0, stream, ap);
    } else {
        const swk::AlignAffineParams ap = align_affine_params<swk::AlignAffineParams>(c, d_db, nhits, qlen, plan, scoring, d_aln, d_ops, ops_cap);
        hipLaunchKernelGGL(kAlignAffine[plan.kernel].k, dim3((unsigned)plan.grid), dim3(256), 0, stream, ap);
    }
    HIP_TRY(hipGetLastError());
    c->last_align_affine_kernel = plan.kernel; c->last_align_affine_slots = plan.slots; c->last_align_affine_slot_bytes = plan.slot_bytes;
    c->last_align_affine_checkpointed = ckpt ? 1 : 0; c->last_align_affine_band_rows = plan.band_rows;
    return SW_OK;
}

// ---- a prepared database and the search of many queries against it (csrc/sw_search_multi.hip)

// Everything a search needs to know about the database and no query changes: the checks of the offsets and the schedule (the stable
// sort of the lengths), done once.  Synchronous; the pinned staging copy of the schedule is gone when it returns.
int sw_db_create(sw_ctx* c, const char* d_db, const int64_t* offsets, int64_t ntargets, sw_db** out) {
    if (!c || !d_db || !offsets || !out || ntargets < 0) { set_err("sw_db_create: NULL pointer or negative target count"); return SW_EINVAL; }
    *out = nullptr;
    int64_t maxlen = 0, nonempty = 0;
    if (int rc = swh::check_targets("sw_db_create", 1, offsets, ntargets, &maxlen, &nonempty)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    sw_db* db = new sw_db;
    db->device = c->device; db->d_db = d_db;
    db->ntargets = ntargets; db->nonempty = nonempty; db->longest = maxlen; db->letters = offsets[ntargets] - offsets[0]; db->first = offsets[0];
    {   // the offsets, for the calls that get from a target index to its bytes on the device (8 bytes per target)
        const size_t bytes = (size_t)(ntargets + 1) * sizeof(int64_t);
        hipError_t e = hipMalloc((void**)&db->d_offsets, bytes);
        if (e == hipSuccess) e = hipMemcpy(db->d_offsets, offsets, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            set_err("sw_db_create: the offsets of %lld targets could not be placed on the device: %s", (long long)ntargets, hipGetErrorString(e));
            if (db->d_offsets) (void)hipFree(db->d_offsets);
            delete db;
            return e == hipErrorOutOfMemory ? SW_ENOMEM : SW_EDEVICE;
        }
    }
    if (nonempty > 0) {
        swk::SearchItem* h_items = nullptr;
        const size_t bytes = (size_t)nonempty * sizeof(swk::SearchItem);
        hipError_t e = hipHostMalloc((void**)&h_items, bytes, 0);
        if (e == hipSuccess) e = hipMalloc((void**)&db->d_items, bytes);
        if (e == hipSuccess) {
            swp::search_schedule(offsets, ntargets, h_items);
            e = hipMemcpy(db->d_items, h_items, bytes, hipMemcpyHostToDevice);
        }
        if (h_items) (void)hipHostFree(h_items);
        if (e != hipSuccess) {
            set_err("sw_db_create: the schedule of %lld targets could not be placed on the device: %s", (long long)nonempty, hipGetErrorString(e));
            if (db->d_items) (void)hipFree(db->d_items);
            (void)hipFree(db->d_offsets);
            delete db;
            return e == hipErrorOutOfMemory ? SW_ENOMEM : SW_EDEVICE;
        }
    }
    *out = db;
    return SW_OK;
}

void sw_db_free(sw_db* db) {
    if (!db) return;
    (void)hipSetDevice(db->device);
    if (db->d_items) (void)hipFree(db->d_items);
    if (db->d_offsets) (void)hipFree(db->d_offsets);
    delete db;
}

int sw_db_info(const sw_db* db, int64_t* ntargets, int64_t* nonempty, int64_t* longest, int64_t* letters) {
    if (!db) { set_err("sw_db_info: NULL handle"); return SW_EINVAL; }
    if (ntargets) *ntargets = db->ntargets;
    if (nonempty) *nonempty = db->nonempty;
    if (longest) *longest = db->longest;
    if (letters) *letters = db->letters;
    return SW_OK;
}

// sw_db_search_affine / sw_db_search_pssm behind their checks: the stream's turn on the device and the search.
static int db_search_call(sw_ctx* c, const sw_db* db, const QuerySource& src, const int64_t* qoffsets, int64_t nqueries, sw_result* d_results, void* stream_) {
    c->last_search_multi_packed_launches = 0;   // (a call that launches no kernel reports none)
    if (nqueries == 0 || db->ntargets == 0) return SW_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    DevOrder order(c, stream, false);
    if (order.rc) return order.rc;
    return run_search_multi(c, db, src, qoffsets, nqueries, d_results, stream);
}

// Every query against every target of the handle.  Per call the host checks and plans the QUERIES (O(nqueries)), uploads their table
// and the scoring table from pinned copies, and enqueues per group one profile launch and one launch per class of queries; the targets'
// offsets are not looked at again and nothing is sorted.
int sw_db_search_affine(sw_ctx* c, const sw_db* db, const char* d_queries, const int64_t* qoffsets, int64_t nqueries, const sw_affine* scoring,
                        sw_result* d_results, void* stream_) {
    if (int rc = check_db_call("sw_db_search_affine", c, db, d_queries && qoffsets && scoring && d_results)) return rc;
    int64_t maxq = 0;
    if (int rc = swh::check_search_multi("sw_db_search_affine", qoffsets, nqueries, db->longest, scoring, &maxq)) return rc;
    return db_search_call(c, db, QuerySource::sequences(d_queries, scoring), qoffsets, nqueries, d_results, stream_);
}

// The same search with a position-specific scoring matrix in place of letters and a table: only the source of the profiles differs.
int sw_db_search_pssm(sw_ctx* c, const sw_db* db, const int8_t* d_pssm, const int64_t* qoffsets, int64_t nqueries, const sw_pssm_scoring* scoring,
                      sw_result* d_results, void* stream_) {
    if (int rc = check_db_call("sw_db_search_pssm", c, db, d_pssm && qoffsets && scoring && d_results)) return rc;
    int64_t maxq = 0;
    unsigned char code[256];
    if (int rc = swh::check_search_pssm("sw_db_search_pssm", qoffsets, nqueries, db->longest, scoring, &maxq, code)) return rc;
    return db_search_call(c, db, QuerySource::matrix(d_pssm, scoring, code), qoffsets, nqueries, d_results, stream_);
}

// The selection alone over a table the caller holds: the plan's chunks only bound the histograms here (no budget on the rows).
int sw_top_hits_device(sw_ctx* c, const sw_result* d_results, int64_t nqueries, int64_t ntargets, int64_t top, int64_t min_score, sw_hit* d_hits,
                       int64_t* d_nhits, void* stream_) {
    if (!c || !d_results || nqueries < 0 || ntargets < 0) { set_err("sw_top_hits_device: NULL pointer or negative count"); return SW_EINVAL; }
    hipStream_t stream = (hipStream_t)stream_;
    swp::SearchTopPlan plan;
    if (int rc = plan_top_call(c, "sw_top_hits_device", nqueries, ntargets, top, d_hits, d_nhits, INT64_MAX, plan)) return rc;
    if (nqueries == 0) return SW_OK;
    DevOrder order(c, stream, false);
    if (order.rc) return order.rc;
    if (int rc = grow_top_workspaces(c, plan, false, stream)) return rc;
    for (const swp::TopChunk& ch : plan.chunk)
        if (int rc = select_top(c, plan, d_results + ch.q0 * ntargets, ch.nq, ntargets, top, min_score, d_hits + ch.q0 * top, d_nhits + ch.q0, stream)) return rc;
    c->last_search_top_chunks = (int64_t)plan.chunk.size(); c->last_search_top_kernel = plan.kernel;
    return SW_OK;
}

// Search and selection with bounded result memory: chunk after chunk of queries through run_search_multi into the result workspace,
// then that chunk's rows of d_hits.  The stream orders the chunks, which share the workspace.  (`who`'s search arguments are checked.)
// With d_hist (the _top_stats calls) the score histogram of a chunk is taken between the two, while its rows are in the workspace.
static int db_search_top_call(const char* who, sw_ctx* c, const sw_db* db, const QuerySource& src, const int64_t* qoffsets, int64_t nqueries, int64_t top,
                              int64_t min_score, sw_hit* d_hits, int64_t* d_nhits, int shift, uint32_t* d_hist, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    swp::SearchTopPlan plan;
    if (int rc = plan_top_call(c, who, nqueries, db->ntargets, top, d_hits, d_nhits, c->opt_search_results_mib << 20, plan)) return rc;
    c->last_search_multi_packed_launches = 0;   // (a call that launches no kernel reports none)
    if (d_hist) c->last_score_hist_launches = c->last_score_hist_slices = 0;
    if (nqueries == 0) return SW_OK;
    DevOrder order(c, stream, false);
    if (order.rc) return order.rc;
    if (int rc = grow_top_workspaces(c, plan, true, stream)) return rc;
    for (const swp::TopChunk& ch : plan.chunk) {
        if (db->ntargets > 0)
            if (int rc = run_search_multi(c, db, src, qoffsets + ch.q0, ch.nq, c->d_tres, stream)) return rc;
        if (d_hist)
            if (int rc = launch_score_hist(c, db, c->d_tres, ch.nq, shift, d_hist + ch.q0 * swp::kScoreHistCells, stream)) return rc;
        if (int rc = select_top(c, plan, c->d_tres, ch.nq, db->ntargets, top, min_score, d_hits + ch.q0 * top, d_nhits + ch.q0, stream)) return rc;
    }
    c->last_search_top_chunks = (int64_t)plan.chunk.size(); c->last_search_top_kernel = plan.kernel;
    return SW_OK;
}

// The sequence form behind its checks: d_hist == NULL is the plain call, `stats` says which of the two was asked for.
static int db_search_affine_top(const char* who, bool stats, sw_ctx* c, const sw_db* db, const char* d_queries, const int64_t* qoffsets, int64_t nqueries,
                                const sw_affine* scoring, int64_t top, int64_t min_score, sw_hit* d_hits, int64_t* d_nhits, int shift, uint32_t* d_hist,
                                void* stream_) {
    if (int rc = check_db_call(who, c, db, d_queries && qoffsets && scoring && (d_hist || !stats))) return rc;
    if (stats && (shift < 0 || shift > SW_HIST_SHIFT_MAX)) { set_err("%s: shift = %d is out of range 0..%d", who, shift, SW_HIST_SHIFT_MAX); return SW_EINVAL; }
    int64_t maxq = 0;
    if (int rc = swh::check_search_multi(who, qoffsets, nqueries, db->longest, scoring, &maxq)) return rc;
    return db_search_top_call(who, c, db, QuerySource::sequences(d_queries, scoring), qoffsets, nqueries, top, min_score, d_hits, d_nhits, shift, d_hist, stream_);
}

// ... and the matrix form.
static int db_search_pssm_top(const char* who, bool stats, sw_ctx* c, const sw_db* db, const int8_t* d_pssm, const int64_t* qoffsets, int64_t nqueries,
                              const sw_pssm_scoring* scoring, int64_t top, int64_t min_score, sw_hit* d_hits, int64_t* d_nhits, int shift, uint32_t* d_hist,
                              void* stream_) {
    if (int rc = check_db_call(who, c, db, d_pssm && qoffsets && scoring && (d_hist || !stats))) return rc;
    if (stats && (shift < 0 || shift > SW_HIST_SHIFT_MAX)) { set_err("%s: shift = %d is out of range 0..%d", who, shift, SW_HIST_SHIFT_MAX); return SW_EINVAL; }
    int64_t maxq = 0;
    unsigned char code[256];
    if (int rc = swh::check_search_pssm(who, qoffsets, nqueries, db->longest, scoring, &maxq, code)) return rc;
    return db_search_top_call(who, c, db, QuerySource::matrix(d_pssm, scoring, code), qoffsets, nqueries, top, min_score, d_hits, d_nhits, shift, d_hist, stream_);
}

int sw_db_search_affine_top(sw_ctx* c, const sw_db* db, const char* d_queries, const int64_t* qoffsets, int64_t nqueries, const sw_affine* scoring,
                            int64_t top, int64_t min_score, sw_hit* d_hits, int64_t* d_nhits, void* stream_) {
    return db_search_affine_top("sw_db_search_affine_top", false, c, db, d_queries, qoffsets, nqueries, scoring, top, min_score, d_hits, d_nhits, 0, nullptr, stream_);
}

int sw_db_search_pssm_top(sw_ctx* c, const sw_db* db, const int8_t* d_pssm, const int64_t* qoffsets, int64_t nqueries, const sw_pssm_scoring* scoring,
                          int64_t top, int64_t min_score, sw_hit* d_hits, int64_t* d_nhits, void* stream_) {
    return db_search_pssm_top("sw_db_search_pssm_top", false, c, db, d_pssm, qoffsets, nqueries, scoring, top, min_score, d_hits, d_nhits, 0, nullptr, stream_);
}

// The same searches with the score histogram of every query (include/swhip.h: the statistics of a many-query search).
int sw_db_search_affine_top_stats(sw_ctx* c, const sw_db* db, const char* d_queries, const int64_t* qoffsets, int64_t nqueries, const sw_affine* scoring,
                                  int64_t top, int64_t min_score, sw_hit* d_hits, int64_t* d_nhits, int shift, uint32_t* d_hist, void* stream_) {
    return db_search_affine_top("sw_db_search_affine_top_stats", true, c, db, d_queries, qoffsets, nqueries, scoring, top, min_score, d_hits, d_nhits, shift, d_hist,
                                stream_);
}

int sw_db_search_pssm_top_stats(sw_ctx* c, const sw_db* db, const int8_t* d_pssm, const int64_t* qoffsets, int64_t nqueries, const sw_pssm_scoring* scoring,
                                int64_t top, int64_t min_score, sw_hit* d_hits, int64_t* d_nhits, int shift, uint32_t* d_hist, void* stream_) {
    return db_search_pssm_top("sw_db_search_pssm_top_stats", true, c, db, d_pssm, qoffsets, nqueries, scoring, top, min_score, d_hits, d_nhits, shift, d_hist,
                              stream_);
}

// The score histogram of a table the caller holds.
int sw_score_hist_device(sw_ctx* c, const sw_db* db, const sw_result* d_results, int64_t nqueries, int shift, uint32_t* d_hist, void* stream_) {
    const char* who = "sw_score_hist_device";
    if (int rc = check_db_call(who, c, db, true)) return rc;
    if (int rc = swh::check_score_hist(who, d_results, nqueries, db->ntargets, shift, d_hist)) return rc;
    c->last_score_hist_launches = c->last_score_hist_slices = 0;   // (a call that launches no kernel reports none)
    if (nqueries == 0) return SW_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    DevOrder order(c, stream, false);
    if (order.rc) return order.rc;
    return launch_score_hist(c, db, d_results, nqueries, shift, d_hist, stream);
}

// The thresholds of sw_score_thresholds on a hit table (sw_score_hist.hip): one launch, one workgroup per query.
int sw_hits_threshold_device(sw_ctx* c, const sw_db* db, const int64_t* d_thresholds, int64_t nqueries, int64_t top, const sw_hit* d_hits, const int64_t* d_nhits,
                             sw_hit* d_hits_out, int32_t* d_keep, int64_t* d_nkept, void* stream_) {
    const char* who = "sw_hits_threshold_device";
    if (int rc = check_db_call(who, c, db, true)) return rc;
    if (int rc = swh::check_hits_threshold(who, d_thresholds, nqueries, db->ntargets, top, d_hits, d_hits_out, d_keep)) return rc;
    const swp::HitsThresholdPlan plan = swp::plan_hits_threshold(nqueries);
    if (plan.grid == 0) return SW_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    DevOrder order(c, stream, false);
    if (order.rc) return order.rc;
    swk::HitsThresholdParams kp;
    memset(&kp, 0, sizeof kp);
    kp.offsets = db->d_offsets; kp.ntargets = db->ntargets; kp.thresholds = d_thresholds; kp.nq = nqueries; kp.top = top;
    kp.hits = d_hits; kp.nhits = d_nhits; kp.hits_out = d_hits_out; kp.keep = d_keep; kp.nkept = d_nkept;
    hipLaunchKernelGGL(swk::sw_hits_threshold, dim3((unsigned)plan.grid), dim3(256), 0, stream, kp);
    HIP_TRY(hipGetLastError());
    return SW_OK;
}

// The alignments of a device hit table (csrc/sw_align_hits.hip).  Per call the host checks and plans the QUERIES (O(nqueries)) against
// the handle's longest target; the table, the counts and the targets' offsets are read on the device only.  Per group: one profile
// launch, two binning launches, one alignment launch per (class, tier) whose grid the plan fixed for the longest list it could get.
// (`who`'s search arguments are checked)
static int db_align_hits_call(const char* who, sw_ctx* c, const sw_db* db, const QuerySource& src, const int64_t* qoffsets, int64_t nqueries,
                              const sw_hit* d_hits, const int64_t* d_nhits, int64_t top, sw_alignment* d_aln, char* d_ops, int64_t ops_cap, void* stream_) {
    if (int rc = swh::check_align_hits(who, top, d_hits, d_aln, d_ops, ops_cap)) return rc;
    c->last_align_hits_launches = c->last_align_hits_tiers = c->last_align_hits_slots = 0;   // (a call that launches no alignment reports none)
    c->last_align_hits_checkpointed = c->last_align_hits_band_rows = 0;
    if (nqueries == 0) return SW_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = c->align_hits_per_cu.once(kAlignHits)) return rc;
    const std::vector<int64_t> qlens = query_lengths(qoffsets, nqueries);
    swp::AlignHitsJob aj;
    aj.qlens = qlens.data(); aj.nqueries = nqueries; aj.top = top; aj.longest = db->longest; aj.num_cus = c->num_cus;
    aj.profile_budget_bytes = c->opt_search_profile_mib << 20; aj.budget_bytes = c->opt_align_workspace_mib << 20;
    std::copy(std::begin(c->align_hits_per_cu), std::end(c->align_hits_per_cu), aj.per_cu);
    swp::AlignHitsPlan plan = swp::plan_align_hits(aj);
    // "align_checkpoint": decided once, from host data alone, before any launch
    const bool ckpt = swp::align_use_ckpt(c->opt_align_checkpoint, plan.fits);
    if (ckpt) {
        if (int rc = c->align_hits_ckpt_per_cu.once(kAlignHitsCkpt)) return rc;
        swp::AlignHitsCkptJob cj;
        static_cast<swp::AlignHitsJob&>(cj) = aj;
        std::copy(std::begin(c->align_hits_ckpt_per_cu), std::end(c->align_hits_ckpt_per_cu), cj.per_cu);
        cj.band_rows = c->opt_align_checkpoint_rows;
        plan = swp::plan_align_hits_ckpt(cj);
        if (!plan.fits) {
            set_err("%s: the checkpointed slot of the handle's longest target against the longest query (%lld rows against %lld padded "
                    "columns = %lld bytes) does not fit align_workspace_mib = %lld (or the 2 GiB a slot may take)", who, (long long)std::max<int64_t>(1, db->longest),
                    (long long)plan.worst_qpad, (long long)plan.worst_bytes, (long long)c->opt_align_workspace_mib);
            return SW_EINVAL;
        }
    } else if (!plan.fits) {   // decided from host data alone, whatever the table names
        set_err("%s: the direction matrix of the handle's longest target against the longest query (%lld rows x %lld bytes = %lld bytes) "
                "does not fit align_workspace_mib = %lld (or the 2 GiB a slot may take)", who, (long long)std::max<int64_t>(1, db->longest), (long long)plan.worst_qpad,
                (long long)plan.worst_bytes, (long long)c->opt_align_workspace_mib);
        return SW_EINVAL;
    }
    DevOrder order(c, stream, false);
    if (order.rc) return order.rc;
    if (db->ntargets == 0) {   // no index is inside an empty database: every entry is the zero alignment
        HIP_TRY(hipMemsetAsync(d_aln, 0, (size_t)nqueries * (size_t)top * sizeof(sw_alignment), stream));
        return SW_OK;
    }
    for (const swp::AlignHitsLaunch& l : plan.launch)
        if ((ckpt ? c->align_hits_ckpt_per_cu : c->align_hits_per_cu)[l.kernel] < 1) { set_err("the hit-table alignment kernel does not fit a CU on this device"); return SW_EDEVICE; }
    if (int rc = stage_search_call(c, stream, 0, plan.prof_need, plan.bnd_need, true)) return rc;
    if (int rc = c->d_adir.grow(plan.dir_need, stream)) return rc;
    if (int rc = c->d_ahitems.grow(plan.items_need, stream)) return rc;
    if (int rc = c->d_ahctl.once(sizeof(swk::AlignHitsCtl))) return rc;
    if (int rc = c->d_ahfilled.once(64)) return rc;
    HIP_TRY(hipMemsetAsync(c->d_ahfilled, 0, 4, stream));
    if (int rc = upload_query_table(c, stream, plan.table, qoffsets, src)) return rc;
    size_t li = 0;
    for (size_t g = 0; g < plan.group.size(); ++g) {
        const swp::AlignHitsGroup& grp = plan.group[g];
        if (int rc = launch_group_profiles(c, stream, src, grp)) return rc;
        // the lists of the group: counts, cursors and work counters start at zero
        HIP_TRY(hipMemsetAsync(c->d_ahctl, 0, sizeof(swk::AlignHitsCtl), stream));
        swk::AlignHitsBinParams bp;
        memset(&bp, 0, sizeof bp);
        bp.hits = d_hits; bp.nhits = d_nhits; bp.top = top;
        bp.offsets = db->d_offsets; bp.ntargets = db->ntargets;
        bp.queries = c->mq.d + grp.q0; bp.nq = grp.nq;
        for (int k = 0; k < swp::kAlignHitsKernels; ++k) {
            bp.cls_q0[k] = grp.cls[k].q0 - grp.q0;
            bp.ntiers[k] = grp.cls[k].ntiers;
            bp.log_band[k] = grp.cls[k].log_band;
            std::copy(std::begin(grp.cls[k].bound), std::end(grp.cls[k].bound), bp.bound[k]);
        }
        bp.cls_q0[swp::kAlignHitsKernels] = grp.nq;
        bp.ctl = c->d_ahctl; bp.items = c->d_ahitems; bp.aln = d_aln; bp.filled = c->d_ahfilled;
        const unsigned bin_blocks = (unsigned)std::clamp<int64_t>((grp.nq * top + 255) / 256, 1, 4096);
        hipLaunchKernelGGL(swk::sw_align_hits_bin<false>, dim3(bin_blocks), dim3(256), 0, stream, bp);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(swk::sw_align_hits_bin<true>, dim3(bin_blocks), dim3(256), 0, stream, bp);
        HIP_TRY(hipGetLastError());
        for (; li < plan.launch.size() && plan.launch[li].group == (int)g; ++li) {
            const swp::AlignHitsLaunch& l = plan.launch[li];
            if (ckpt) {
                swk::AlignHitsCkptParams kp = align_hits_params<swk::AlignHitsCkptParams>(c, db, src, grp, l, d_aln, d_ops, ops_cap);
                kp.log_band = l.log_band;
                hipLaunchKernelGGL(kAlignHitsCkpt[l.kernel].k, dim3((unsigned)l.grid), dim3(256), 0, stream, kp);
            } else {
                const swk::AlignHitsParams ap = align_hits_params<swk::AlignHitsParams>(c, db, src, grp, l, d_aln, d_ops, ops_cap);
                hipLaunchKernelGGL(kAlignHits[l.kernel].k, dim3((unsigned)l.grid), dim3(256), 0, stream, ap);
            }
            HIP_TRY(hipGetLastError());
            if (ckpt) c->last_align_hits_band_rows = std::max<int64_t>(c->last_align_hits_band_rows, 1ll << l.log_band);
        }
    }
    c->last_align_hits_launches = (int64_t)(3 * plan.group.size() + plan.launch.size()); c->last_align_hits_tiers = plan.tiers; c->last_align_hits_slots = plan.slots;
    c->last_align_hits_checkpointed = ckpt ? 1 : 0;
    return SW_OK;
}

int sw_db_align_affine_hits(sw_ctx* c, const sw_db* db, const char* d_queries, const int64_t* qoffsets, int64_t nqueries, const sw_affine* scoring,
                            const sw_hit* d_hits, const int64_t* d_nhits, int64_t top, sw_alignment* d_aln, char* d_ops, int64_t ops_cap, void* stream_) {
    if (int rc = check_db_call("sw_db_align_affine_hits", c, db, d_queries && qoffsets && scoring)) return rc;
    int64_t maxq = 0;
    if (int rc = swh::check_search_multi("sw_db_align_affine_hits", qoffsets, nqueries, db->longest, scoring, &maxq)) return rc;
    return db_align_hits_call("sw_db_align_affine_hits", c, db, QuerySource::sequences(d_queries, scoring), qoffsets, nqueries, d_hits, d_nhits, top, d_aln, d_ops,
                              ops_cap, stream_);
}

int sw_db_align_pssm_hits(sw_ctx* c, const sw_db* db, const int8_t* d_pssm, const int64_t* qoffsets, int64_t nqueries, const sw_pssm_scoring* scoring,
                          const sw_hit* d_hits, const int64_t* d_nhits, int64_t top, sw_alignment* d_aln, char* d_ops, int64_t ops_cap, void* stream_) {
    if (int rc = check_db_call("sw_db_align_pssm_hits", c, db, d_pssm && qoffsets && scoring)) return rc;
    int64_t maxq = 0;
    unsigned char code[256];
    if (int rc = swh::check_search_pssm("sw_db_align_pssm_hits", qoffsets, nqueries, db->longest, scoring, &maxq, code)) return rc;
    return db_align_hits_call("sw_db_align_pssm_hits", c, db, QuerySource::matrix(d_pssm, scoring, code), qoffsets, nqueries, d_hits, d_nhits, top, d_aln, d_ops,
                              ops_cap, stream_);
}

// The small table of sw_db_pssm_from_hits and sw_db_pssm_hit_weights: one device copy (d_phtab), at least `need` bytes after this, and
// the pinned copy h_phtab[*turn_out] the caller fills and uploads, recording phtab_ev[*turn_out] behind the upload.
static int pssm_table_turn(const char* who, sw_ctx* c, hipStream_t stream, size_t need, int* turn_out) {
    // two pinned copies in turn: this call overwrites the copy of the call before the last one, and waits (on the host) for THAT upload only
    const int turn = c->phtab_turn;
    *turn_out = turn;
    c->phtab_turn ^= 1;
    if (c->phtab_ev[turn]) HIP_TRY(hipEventSynchronize(c->phtab_ev[turn]));
    else HIP_TRY(hipEventCreateWithFlags(&c->phtab_ev[turn], hipEventDisableTiming));
    if (need > c->d_phtab.cap) {
        HIP_TRY(hipStreamSynchronize(stream));                   // launches in flight may still read the old table
        if (c->phtab_ev[turn ^ 1]) HIP_TRY(hipEventSynchronize(c->phtab_ev[turn ^ 1]));   // ... and an upload the other copy
        if (c->d_phtab) HIP_TRY(hipFree(c->d_phtab));
        c->d_phtab.p = nullptr; c->d_phtab.cap = 0;
        for (int i = 0; i < 2; ++i) {
            if (c->h_phtab[i]) HIP_TRY(hipHostFree(c->h_phtab[i]));
            c->h_phtab[i] = nullptr;
        }
        if (hipMalloc((void**)&c->d_phtab.p, need) != hipSuccess || hipHostMalloc((void**)&c->h_phtab[0], need, 0) != hipSuccess ||
            hipHostMalloc((void**)&c->h_phtab[1], need, 0) != hipSuccess) {
            set_err("%s: workspace allocation of %zu bytes failed", who, need);
            return SW_ENOMEM;
        }
        c->d_phtab.cap = need;
    }
    return SW_OK;
}

// The small table of a call that reads a hit table's alignments, on the device: S (with `sub`; nletters x nletters, padded to 256
// bytes), the 256-byte code table (with `code`), the nqueries + 1 offsets -- in this order, so every device address keeps its alignment.
// Filled into the pinned copy of the call's turn, one upload, phtab_ev[turn] recorded behind it.
struct HitsCallTable { const signed char* S; const unsigned char* code; const int64_t* qoffs; };
static int upload_hits_call_table(const char* who, sw_ctx* c, hipStream_t stream, const sw_submat* sub, const char* letters, int nletters,
                                  const unsigned char* code, const int64_t* qoffsets, int64_t nqueries, HitsCallTable* tab) {
    const size_t s_bytes = sub ? ((size_t)nletters * nletters + 255) & ~(size_t)255 : 0, code_bytes = code ? 256 : 0;
    const size_t off_bytes = (size_t)(nqueries + 1) * sizeof(int64_t), need = s_bytes + code_bytes + off_bytes;
    int turn = 0;
    if (int rc = pssm_table_turn(who, c, stream, need, &turn)) return rc;
    unsigned char* h_tab = c->h_phtab[turn];
    if (sub) swh::pssm_update_table(sub, letters, nletters, (int8_t*)h_tab);
    if (code) memcpy(h_tab + s_bytes, code, 256);
    memcpy(h_tab + s_bytes + code_bytes, qoffsets, off_bytes);
    HIP_TRY(hipMemcpyAsync(c->d_phtab, h_tab, need, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(c->phtab_ev[turn], stream));
    tab->S = (const signed char*)c->d_phtab.p; tab->code = c->d_phtab + s_bytes; tab->qoffs = (const int64_t*)(c->d_phtab + s_bytes + code_bytes);
    return SW_OK;
}

// The tables those calls' kernels read: the handle's targets, the uploaded offsets and the caller's device tables.
static swk::HitTables hit_tables(const sw_db* db, const int64_t* d_qoffs, int64_t nqueries, const sw_hit* d_hits, const int64_t* d_nhits, int64_t top,
                                 const sw_alignment* d_aln, const char* d_ops, int64_t ops_cap, int64_t include_min) {
    swk::HitTables t;
    t.qoffs = d_qoffs; t.nqueries = nqueries;
    t.db = (const unsigned char*)db->d_db; t.offsets = db->d_offsets; t.ntargets = db->ntargets;
    t.hits = d_hits; t.nhits = d_nhits; t.top = top;
    t.aln = d_aln; t.ops = d_ops; t.ops_cap = ops_cap;
    t.include_min = include_min;
    return t;
}

// The next iteration's PSSM from a device hit table, its alignments and their ops (csrc/sw_pssm_hits.hip).  The host checks the
// arguments, cuts the tiles (swp::plan_pssm_hits) and uploads one small table through two pinned copies of its own, used in turn -- S
// (nletters x nletters), the 256-byte code table, the nqueries + 1 offsets --; the hit table, the alignments, the ops, the weights and the targets'
// offsets are read on the device only.  One launch; a handle without targets takes the same launch (no entry is used).
int sw_db_pssm_from_hits(sw_ctx* c, const sw_db* db, const int8_t* d_prior, const int64_t* qoffsets, int64_t nqueries, const sw_pssm_scoring* scoring,
                         const sw_pssm_update* upd, const sw_hit* d_hits, const int64_t* d_nhits, int64_t top, const sw_alignment* d_aln, const char* d_ops,
                         int64_t ops_cap, const int32_t* d_weights, int8_t* d_pssm_out, int32_t* d_counts, void* stream_) {
    const char* who = "sw_db_pssm_from_hits";
    if (int rc = check_db_call(who, c, db, d_prior && qoffsets && scoring)) return rc;
    int64_t maxq = 0;
    unsigned char code[256];
    if (int rc = swh::check_search_pssm(who, qoffsets, nqueries, db->longest, scoring, &maxq, code)) return rc;
    if (int rc = swh::check_pssm_update(who, upd, top, d_hits, d_aln, d_ops, ops_cap, d_pssm_out, d_counts)) return rc;
    c->last_pssm_hits_launches = 0;   // (a call that launches no kernel reports none)
    if (nqueries == 0) return SW_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    const std::vector<int64_t> qlens = query_lengths(qoffsets, nqueries);
    swp::PssmHitsJob pj;
    pj.qlens = qlens.data(); pj.nqueries = nqueries; pj.nletters = scoring->nletters; pj.num_cus = c->num_cus;
    const swp::PssmHitsPlan plan = swp::plan_pssm_hits(pj);
    DevOrder order(c, stream, false);
    if (order.rc) return order.rc;
    const int n = scoring->nletters;
    HitsCallTable tab;
    if (int rc = upload_hits_call_table(who, c, stream, upd->sub, scoring->letters, n, code, qoffsets, nqueries, &tab)) return rc;
    swk::PssmHitsParams kp;
    memset(&kp, 0, sizeof kp);
    kp.t = hit_tables(db, tab.qoffs, nqueries, d_hits, d_nhits, top, d_aln, d_ops, ops_cap, upd->include_min_score);
    kp.prior = (const signed char*)d_prior; kp.out = (signed char*)d_pssm_out; kp.counts = d_counts;
    kp.S = tab.S; kp.code = tab.code; kp.weights = d_weights;
    kp.tiles_per_query = plan.tiles_per_query; kp.col0 = qoffsets[0];
    kp.nletters = n; kp.stride = plan.stride; kp.tile_cols = plan.tile_cols; kp.smax = scoring->smax; kp.prior_weight = upd->prior_weight;
    hipLaunchKernelGGL(swk::sw_pssm_from_hits, dim3((unsigned)plan.grid), dim3(256), plan.lds_bytes, stream, kp);
    HIP_TRY(hipGetLastError());
    c->last_pssm_hits_launches = plan.launches;
    return SW_OK;
}

// The weights of a device hit table's entries (csrc/sw_pssm_weights.hip): the d_weights of the call above.  The host checks the
// arguments, plans (swp::plan_pssm_weights) and uploads the code table and the offsets through the small table of the call above; one
// memset zeroes the entries' accumulators, then the tile launch and the finish launch.  A handle without targets takes the same
// launches (no entry is used: every weight is 0).
int sw_db_pssm_hit_weights(sw_ctx* c, const sw_db* db, const int64_t* qoffsets, int64_t nqueries, const sw_pssm_scoring* scoring,
                           const sw_pssm_weighting* weighting, const sw_hit* d_hits, const int64_t* d_nhits, int64_t top, const sw_alignment* d_aln,
                           const char* d_ops, int64_t ops_cap, int32_t* d_weights, void* stream_) {
    const char* who = "sw_db_pssm_hit_weights";
    if (int rc = check_db_call(who, c, db, qoffsets && scoring)) return rc;
    int64_t maxq = 0;
    unsigned char code[256];
    if (int rc = swh::check_search_pssm(who, qoffsets, nqueries, db->longest, scoring, &maxq, code)) return rc;
    if (int rc = swh::check_pssm_weighting(who, weighting, top, d_hits, d_aln, d_ops, ops_cap, d_weights)) return rc;
    c->last_pssm_weights_launches = c->last_pssm_weights_tiles = 0;   // (a call that launches no kernel reports none)
    if (nqueries == 0) return SW_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    const std::vector<int64_t> qlens = query_lengths(qoffsets, nqueries);
    swp::PssmWeightsJob pj;
    pj.queries.qlens = qlens.data(); pj.queries.nqueries = nqueries; pj.queries.nletters = scoring->nletters; pj.queries.num_cus = c->num_cus;
    pj.top = top;
    const swp::PssmWeightsPlan plan = swp::plan_pssm_weights(pj);
    DevOrder order(c, stream, false);
    if (order.rc) return order.rc;
    if (int rc = c->d_pwacc.grow((size_t)plan.acc_entries, stream)) return rc;
    HitsCallTable tab;
    if (int rc = upload_hits_call_table(who, c, stream, nullptr, nullptr, 0, code, qoffsets, nqueries, &tab)) return rc;
    HIP_TRY(hipMemsetAsync(c->d_pwacc, 0, (size_t)plan.acc_bytes, stream));
    swk::PssmWeightsParams kp;
    memset(&kp, 0, sizeof kp);
    kp.t = hit_tables(db, tab.qoffs, nqueries, d_hits, d_nhits, top, d_aln, d_ops, ops_cap, weighting->include_min_score);
    kp.code = tab.code; kp.acc = c->d_pwacc; kp.weights = d_weights;
    kp.tiles_per_query = plan.tiles.tiles_per_query;
    kp.nletters = scoring->nletters; kp.stride = plan.tiles.stride; kp.tile_cols = plan.tiles.tile_cols; kp.per_hit = weighting->per_hit;
    hipLaunchKernelGGL(swk::sw_pssm_weights_tile, dim3((unsigned)plan.tiles.grid), dim3(256), plan.tiles.lds_bytes, stream, kp);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(swk::sw_pssm_weights_finish, dim3((unsigned)plan.finish_grid), dim3(256), 0, stream, kp);
    HIP_TRY(hipGetLastError());
    c->last_pssm_weights_launches = plan.launches; c->last_pssm_weights_tiles = plan.tiles.tiles_per_query;
    return SW_OK;
}

// The query-anchored alignment of a device hit table's entries (csrc/sw_msa_hits.hip).  The host checks the arguments, plans
// (swp::plan_msa_hits) and uploads the offsets through the small table of the calls above; the hit table, the alignments, the ops and
// the targets' offsets are read on the device only.  Launch A always; with d_rows the two scan launches and the row launch.  A handle
// without targets takes the same launches (no entry is used).
int sw_db_msa_from_hits(sw_ctx* c, const sw_db* db, const char* d_queries, const int64_t* qoffsets, int64_t nqueries, int64_t include_min_score,
                        const sw_hit* d_hits, const int64_t* d_nhits, int64_t top, const sw_alignment* d_aln, const char* d_ops, int64_t ops_cap, char* d_cols,
                        sw_msa_row* d_rows, char* d_a3m, int64_t a3m_cap, int64_t* d_a3m_bytes, void* stream_) {
    const char* who = "sw_db_msa_from_hits";
    if (int rc = check_db_call(who, c, db, qoffsets != nullptr)) return rc;
    if (int rc = swh::check_msa(who, qoffsets, nqueries, top, d_hits, d_aln, d_ops, ops_cap, d_cols, d_rows, d_a3m, a3m_cap, d_a3m_bytes)) return rc;
    c->last_msa_hits_launches = 0;   // (a call that launches no kernel reports none)
    if (nqueries == 0) return SW_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    swp::MsaHitsJob mj;
    mj.nqueries = nqueries; mj.top = top; mj.num_cus = c->num_cus; mj.rows = d_rows != nullptr;
    const swp::MsaHitsPlan plan = swp::plan_msa_hits(mj);
    DevOrder order(c, stream, false);
    if (order.rc) return order.rc;
    if (int rc = c->d_msasum.grow((size_t)plan.scan_chunks, stream)) return rc;
    HitsCallTable tab;
    if (int rc = upload_hits_call_table(who, c, stream, nullptr, nullptr, 0, nullptr, qoffsets, nqueries, &tab)) return rc;
    swk::MsaHitsParams kp;
    memset(&kp, 0, sizeof kp);
    kp.t = hit_tables(db, tab.qoffs, nqueries, d_hits, d_nhits, top, d_aln, d_ops, ops_cap, include_min_score);
    kp.queries = (const unsigned char*)d_queries;
    kp.cols = (unsigned char*)d_cols; kp.rows = d_rows; kp.a3m = (unsigned char*)d_a3m; kp.a3m_cap = a3m_cap; kp.a3m_bytes = d_a3m_bytes;
    kp.chunk_off = (int64_t*)c->d_msasum.p;
    kp.entries = plan.entries; kp.chunks = plan.scan_chunks;
    kp.slices_per_query = plan.slices_per_query; kp.slice_entries = plan.slice_entries; kp.col0 = qoffsets[0];
    hipLaunchKernelGGL(swk::sw_msa_cols, dim3((unsigned)plan.cols_grid), dim3(256), 0, stream, kp);
    HIP_TRY(hipGetLastError());
    if (d_rows) {
        hipLaunchKernelGGL(swk::sw_msa_scan_chunks, dim3((unsigned)plan.scan_grid), dim3(256), 0, stream, kp);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(swk::sw_msa_scan_top, dim3(1), dim3(256), 0, stream, kp);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(swk::sw_msa_rows, dim3((unsigned)plan.rows_grid), dim3(256), 0, stream, kp);
        HIP_TRY(hipGetLastError());
    }
    c->last_msa_hits_launches = plan.launches;
    return SW_OK;
}

// The filter of the column rows of the call above (csrc/sw_msa_filter.hip).  The host checks the arguments, plans (swp::plan_msa_filter)
// and uploads the offsets through the small table of the calls above; per chunk of queries the pair launch fills the bit planes of the
// workspace and the greedy launch turns them into the outputs.  Needs no handle: the column rows hold the targets' letters.
int sw_msa_filter_device(sw_ctx* c, const char* d_cols, const char* d_queries, const int64_t* qoffsets, int64_t nqueries, int64_t top,
                         const sw_msa_filter* filter, const sw_hit* d_hits, sw_hit* d_hits_out, int32_t* d_keep, int64_t* d_nkept, void* stream_) {
    const char* who = "sw_msa_filter_device";
    if (!c) { set_err("%s: NULL pointer", who); return SW_EINVAL; }
    if (int rc = swh::check_msa_filter(who, qoffsets, nqueries, top, d_cols, filter, d_hits, d_hits_out, d_keep)) return rc;
    c->last_msa_filter_launches = c->last_msa_filter_chunks = 0;   // (a call that launches no kernel reports none)
    if (nqueries == 0) return SW_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    swp::MsaFilterJob fj;
    fj.nqueries = nqueries; fj.top = top; fj.budget_bytes = c->opt_msa_filter_workspace_mib << 20;
    const swp::MsaFilterPlan plan = swp::plan_msa_filter(fj);
    DevOrder order(c, stream, false);
    if (order.rc) return order.rc;
    if (int rc = c->d_msafilt.grow((size_t)(plan.queries_per_chunk * plan.query_words), stream)) return rc;
    HitsCallTable tab;
    if (int rc = upload_hits_call_table(who, c, stream, nullptr, nullptr, 0, nullptr, qoffsets, nqueries, &tab)) return rc;
    swk::MsaFilterParams kp;
    memset(&kp, 0, sizeof kp);
    kp.cols = (const unsigned char*)d_cols; kp.queries = (const unsigned char*)d_queries; kp.qoffs = tab.qoffs; kp.col0 = qoffsets[0];
    kp.top = top; kp.blocks = plan.blocks; kp.tiles_per_query = plan.tiles_per_query; kp.query_words = plan.query_words;
    kp.ws = c->d_msafilt;
    kp.max_ident_pct = filter->max_ident_pct; kp.min_cover_pct = filter->min_cover_pct;
    kp.hits = d_hits; kp.hits_out = d_hits_out; kp.keep = d_keep; kp.nkept = d_nkept;
    for (int64_t ch = 0; ch < plan.chunks; ++ch) {
        const bool last = ch == plan.chunks - 1;
        kp.q0 = ch * plan.queries_per_chunk; kp.nq = last ? plan.last_queries : plan.queries_per_chunk;
        hipLaunchKernelGGL(swk::sw_msa_filter_pairs, dim3((unsigned)(last ? plan.last_pair_grid : plan.pair_grid)), dim3(256), 0, stream, kp);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(swk::sw_msa_filter_greedy, dim3((unsigned)(last ? plan.last_greedy_grid : plan.greedy_grid)), dim3(256), 0, stream, kp);
        HIP_TRY(hipGetLastError());
    }
    c->last_msa_filter_launches = plan.launches; c->last_msa_filter_chunks = plan.chunks;
    return SW_OK;
}

// The low-complexity mask of a handle's bytes (csrc/sw_mask.hip).  The host checks the rule, turns the two bounds into integers
// (swh::check_mask_params), plans from the handle's counts (swp::plan_mask) and launches; the lengths are read on the device only.
int sw_db_mask_low_complexity(sw_ctx* c, const sw_db* db, const sw_mask_params* params, char* d_out, int64_t* d_nmasked, void* stream_) {
    const char* who = "sw_db_mask_low_complexity";
    if (int rc = check_db_call(who, c, db, params && d_out)) return rc;
    if (d_out == db->d_db) { set_err("%s: in place (d_out == the handle's bytes) is refused", who); return SW_EINVAL; }
    int32_t bound1, bound2;
    unsigned char cls[256];
    if (int rc = swh::check_mask_params(who, params, &bound1, &bound2, cls)) return rc;
    c->last_mask_launches = c->last_mask_tiles = 0;   // (a call that launches no kernel reports none)
    swp::MaskJob mj;
    mj.letters = db->letters; mj.ntargets = db->ntargets; mj.window = params->window; mj.count = d_nmasked != nullptr;
    const swp::MaskPlan plan = swp::plan_mask(mj);
    if (plan.launches == 0) return SW_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    DevOrder order(c, stream, false);
    if (order.rc) return order.rc;
    if (int rc = c->d_mask.grow((size_t)plan.workspace_bytes, stream)) return rc;
    swk::MaskParams kp;
    memset(&kp, 0, sizeof kp);
    kp.in = (const unsigned char*)db->d_db; kp.out = (unsigned char*)d_out; kp.offs = db->d_offsets; kp.ntargets = db->ntargets;
    kp.base = db->first; kp.letters = db->letters; kp.tiles = plan.tiles;
    if (plan.tiles) {
        kp.low1 = (unsigned long long*)(c->d_mask + plan.low1_off); kp.low2 = (unsigned long long*)(c->d_mask + plan.low2_off);
        kp.mask = (unsigned long long*)(c->d_mask + plan.mask_off);
        kp.summary = (unsigned int*)(c->d_mask + plan.summary_off); kp.carry = (unsigned int*)(c->d_mask + plan.carry_off);
    }
    kp.window = params->window; kp.bound1 = bound1; kp.bound2 = bound2; kp.gw = swp::kMaskG[params->window];
    kp.nletters = params->nletters; memcpy(kp.letters_, params->letters, sizeof kp.letters_);
    kp.mask_byte = params->mask_byte; kp.nmasked = d_nmasked;
    if (plan.tiles) {
        hipLaunchKernelGGL(swk::sw_mask_windows, dim3((unsigned)plan.window_grid), dim3(256), 0, stream, kp);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(swk::sw_mask_carries, dim3((unsigned)plan.carry_grid), dim3(swp::kMaskCarryThreads), 0, stream, kp);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(swk::sw_mask_apply, dim3((unsigned)plan.apply_grid), dim3(256), 0, stream, kp);
        HIP_TRY(hipGetLastError());
    }
    if (plan.count_grid) {
        hipLaunchKernelGGL(swk::sw_mask_count, dim3((unsigned)plan.count_grid), dim3(256), 0, stream, kp);
        HIP_TRY(hipGetLastError());
    }
    c->last_mask_launches = plan.launches; c->last_mask_tiles = plan.tiles;
    return SW_OK;
}

// The scores of a device pair list (csrc/sw_search_pairs.hip).  Per call the host checks and plans the QUERIES (O(nqueries)) against the
// handle's longest target; the pairs and the targets' offsets are read on the device only.  One memset zeroes the call's results up
// front -- the pairs that never become an item keep it, the binning writes no result --, then per group one profile launch and per
// chunk of the list two binning launches and one score launch per class of the group, its grid planned for the most its list could hold.
// Under "search_pairs_lanes" = 16 a group that holds packed queries gets the three binning launches of csrc/sw_search_pairs16.hip instead,
// and a class a packed score launch ahead of the 32-bit one; under 32 the plan, and so every launch, is swp::plan_search_pairs's.
int sw_db_search_affine_pairs(sw_ctx* c, const sw_db* db, const char* d_queries, const int64_t* qoffsets, int64_t nqueries, const sw_affine* scoring,
                              const sw_pair* d_pairs, int64_t npairs, sw_result* d_results, void* stream_) {
    if (int rc = check_db_call("sw_db_search_affine_pairs", c, db, d_queries && qoffsets && scoring)) return rc;
    int64_t maxq = 0;
    if (int rc = swh::check_search_multi("sw_db_search_affine_pairs", qoffsets, nqueries, db->longest, scoring, &maxq)) return rc;
    if (npairs < 0) { set_err("sw_db_search_affine_pairs: negative pair count"); return SW_EINVAL; }
    if (npairs > 0 && (!d_pairs || !d_results)) { set_err("sw_db_search_affine_pairs: NULL d_pairs or d_results with %lld pairs", (long long)npairs); return SW_EINVAL; }
    c->last_search_pairs_groups = c->last_search_pairs_chunks = c->last_search_pairs_launches = 0;   // (a call that launches no kernel reports none)
    c->last_search_pairs_packed_launches = 0;
    if (npairs == 0) return SW_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    DevOrder order(c, stream, false);
    if (order.rc) return order.rc;
    // every entry that names no query, no target or an empty target keeps these zeros: {0, 0, 0}
    HIP_TRY(hipMemsetAsync(d_results, 0, (size_t)npairs * sizeof(sw_result), stream));
    if (nqueries == 0 || db->nonempty == 0) return SW_OK;
    if (int rc = c->search_pairs_per_cu.once(kSearchPairs)) return rc;
    const bool lanes16 = c->opt_search_pairs_lanes == 16;
    if (lanes16)
        if (int rc = c->search_pairs_packed_per_cu.once(kSearchPairsPacked)) return rc;
    const QuerySource src = QuerySource::sequences(d_queries, scoring);
    const std::vector<int64_t> qlens = query_lengths(qoffsets, nqueries);
    swp::SearchPairsLanesJob pj;
    pj.qlens = qlens.data(); pj.nqueries = nqueries; pj.npairs = npairs; pj.longest = db->longest; pj.num_cus = c->num_cus;
    pj.budget_bytes = c->opt_search_profile_mib << 20; pj.chunk = c->opt_search_pairs_chunk;
    std::copy(std::begin(c->search_pairs_per_cu), std::end(c->search_pairs_per_cu), pj.per_cu);
    pj.lanes = (int)c->opt_search_pairs_lanes; pj.gap_open = scoring->gap_open; pj.gap_extend = scoring->gap_extend;
    if (lanes16) {   // (the 32-bit plan asks for neither)
        std::copy(std::begin(c->search_pairs_packed_per_cu), std::end(c->search_pairs_packed_per_cu), pj.packed_per_cu);
        pj.max_entry = src.max_entry();
    }
    const swp::SearchPairsLanesPlan plan = swp::plan_search_pairs_lanes(pj);
    for (const swp::PairsLanesLaunch& l : plan.launch)
        if ((l.packed ? c->search_pairs_packed_per_cu : c->search_pairs_per_cu)[l.kernel] < 1) { set_err("the pair-list search kernel does not fit a CU on this device"); return SW_EDEVICE; }
    if (int rc = stage_search_call(c, stream, 0, plan.prof_need, plan.bnd_need, true)) return rc;
    if (int rc = c->d_spitems.grow(plan.items_need, stream)) return rc;
    if (int rc = c->d_spctl.once(sizeof(swk::SearchPairsCtl))) return rc;
    if (plan.cells_need) {   // the cells of the packed queries and the call's count of two-pair items, which starts at zero
        if (int rc = c->d_spcells.grow(plan.cells_need, stream)) return rc;
        if (int rc = c->d_sptotal.once(sizeof(unsigned long long))) return rc;
        HIP_TRY(hipMemsetAsync(c->d_sptotal, 0, sizeof(unsigned long long), stream));
    }
    // behind the table's nqueries entries: entry_of (4 bytes per query)
    if (int rc = upload_query_table(c, stream, plan.table, qoffsets, src, plan.entry_of.data(), (size_t)nqueries * sizeof(int32_t))) return rc;
    size_t l0 = 0;
    for (size_t g = 0; g < plan.group.size(); ++g) {
        const swp::PairsLanesGroup& grp = plan.group[g];
        if (int rc = launch_group_profiles(c, stream, src, grp)) return rc;
        size_t l1 = l0;
        while (l1 < plan.launch.size() && plan.launch[l1].group == (int)g) ++l1;
        for (int64_t ch = 0; ch < plan.nchunks; ++ch) {
            const int64_t np = plan.chunk_pairs(ch, npairs);
            // the lists of the (chunk, group): counts, cursors and work counters start at zero
            HIP_TRY(hipMemsetAsync(c->d_spctl, 0, sizeof(swk::SearchPairsCtl), stream));
            swk::SearchPairsBinParams bp;
            memset(&bp, 0, sizeof bp);
            bp.pairs = d_pairs; bp.p0 = plan.chunk_p0(ch); bp.np = np;
            bp.offsets = db->d_offsets; bp.ntargets = db->ntargets;
            bp.queries = c->mq.d; bp.entry_of = (const int32_t*)(c->mq.d + nqueries); bp.nqueries = nqueries;
            std::copy(std::begin(grp.cls_q0), std::end(grp.cls_q0), bp.cls_q0);
            bp.ctl = c->d_spctl; bp.items = c->d_spitems;
            const unsigned bin_blocks = (unsigned)std::clamp<int64_t>((np + 255) / 256, 1, 4096);
            if (grp.cells) {   // a group with packed queries: count, scan, scatter (sw_search_pairs16.hip)
                swk::SearchPairsPackedCtl* const pk = (swk::SearchPairsPackedCtl*)c->d_spcells.p;
                // its control words, counts and cursors start at zero; the scan writes every base
                HIP_TRY(hipMemsetAsync(c->d_spcells, 0, (size_t)(swp::kSearchPairsCellsHead + 8 * grp.cells), stream));
                swk::SearchPairsPackedBinParams kp;
                memset(&kp, 0, sizeof kp);
                kp.bin = bp;
                std::copy(std::begin(grp.pk_q1), std::end(grp.pk_q1), kp.pk_q1);
                kp.cells = grp.cells; kp.pk = pk; kp.total = c->d_sptotal;
                hipLaunchKernelGGL(swk::sw_search_pairs_pk_bin<false>, dim3(bin_blocks), dim3(256), 0, stream, kp);
                HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(swk::sw_search_pairs_pk_scan, dim3(1), dim3(256), 0, stream, kp);
                HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(swk::sw_search_pairs_pk_bin<true>, dim3(bin_blocks), dim3(256), 0, stream, kp);
                HIP_TRY(hipGetLastError());
            } else {
                hipLaunchKernelGGL(swk::sw_search_pairs_bin<false>, dim3(bin_blocks), dim3(256), 0, stream, bp);
                HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(swk::sw_search_pairs_bin<true>, dim3(bin_blocks), dim3(256), 0, stream, bp);
                HIP_TRY(hipGetLastError());
            }
            for (size_t li = l0; li < l1; ++li) {
                const swp::PairsLanesLaunch& l = plan.launch[li];
                const unsigned grid = (unsigned)swp::search_pairs_lanes_grid(l, np, grp.cells);
                if (l.packed) {   // two pairs of a query per wave: the class's two-pair items at the head of the item buffer
                    swk::SearchPairsPackedCtl* const pk = (swk::SearchPairsPackedCtl*)c->d_spcells.p;
                    swk::SearchPairsPackedParams kp = search_pairs_params<swk::SearchPairsPackedParams>(c, db, scoring, l, d_results);
                    kp.items = (const swk::SearchPairItem2*)c->d_spitems.p; kp.list = &pk->list[l.kernel];
                    kp.counter = &pk->work[l.kernel];
                    hipLaunchKernelGGL(kSearchPairsPacked[l.kernel].k, dim3(grid), dim3(256), 0, stream, kp);
                } else {
                    swk::SearchPairsParams sp = search_pairs_params<swk::SearchPairsParams>(c, db, scoring, l, d_results);
                    sp.items = c->d_spitems; sp.list = &c->d_spctl->list[l.kernel];
                    sp.counter = &c->d_spctl->work[l.kernel];
                    hipLaunchKernelGGL(kSearchPairs[l.kernel].k, dim3(grid), dim3(256), 0, stream, sp);
                }
                HIP_TRY(hipGetLastError());
            }
        }
        l0 = l1;
    }
    c->last_search_pairs_groups = (int64_t)plan.group.size(); c->last_search_pairs_chunks = plan.nchunks; c->last_search_pairs_launches = plan.launches;
    c->last_search_pairs_packed_launches = plan.packed_launches;
    return SW_OK;
}

// The ungapped pre-filter (csrc/sw_prefilter.hip).  Per call the host checks and plans the QUERIES (O(nqueries)) against the handle; one
// memset writes the {-1, -1} of the whole list up front, then per group one profile launch and per class the launches of its packed and
// of its other queries, a one-thread commit between them: it starts the work counter and the cursor of the next launch at zero and
// keeps the count.  Nothing is read back.
int sw_db_prefilter_ungapped(sw_ctx* c, const sw_db* db, const char* d_queries, const int64_t* qoffsets, int64_t nqueries, const sw_submat* sub,
                             int64_t min_score, sw_pair* d_pairs, int64_t pairs_cap, int64_t* d_npairs, int32_t* d_scores, void* stream_) {
    const char* who = "sw_db_prefilter_ungapped";
    if (int rc = check_db_call(who, c, db, d_queries && qoffsets && sub)) return rc;
    int64_t maxq = 0;
    const sw_affine scoring = {sub, 0, 0};
    if (int rc = swh::check_search_multi(who, qoffsets, nqueries, db->longest, &scoring, &maxq)) return rc;
    if (int rc = swh::check_prefilter(who, min_score, d_pairs, pairs_cap, d_npairs, d_scores)) return rc;
    c->last_prefilter_groups = c->last_prefilter_launches = c->last_prefilter_packed_launches = 0;   // (a call that launches no kernel reports none)
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    DevOrder order(c, stream, false);
    if (order.rc) return order.rc;
    // the entries behind the written ones keep these {-1, -1}; empty targets keep the zeros of the scores
    if (pairs_cap > 0) HIP_TRY(hipMemsetAsync(d_pairs, 0xFF, (size_t)pairs_cap * sizeof(sw_pair), stream));
    if (d_scores && nqueries > 0 && db->ntargets > 0) HIP_TRY(hipMemsetAsync(d_scores, 0, (size_t)nqueries * (size_t)db->ntargets * sizeof(int32_t), stream));
    if (nqueries == 0 || db->nonempty == 0) {
        if (d_npairs) HIP_TRY(hipMemsetAsync(d_npairs, 0, sizeof(int64_t), stream));
        return SW_OK;
    }
    if (int rc = c->prefilter_per_cu.once(kPrefilter)) return rc;
    const std::vector<int64_t> qlens = query_lengths(qoffsets, nqueries);
    swp::PrefilterJob pj;
    pj.qlens = qlens.data(); pj.nqueries = nqueries; pj.longest = db->longest; pj.nonempty = db->nonempty; pj.num_cus = c->num_cus;
    pj.budget_bytes = c->opt_search_profile_mib << 20; pj.lanes = (int)c->opt_prefilter_lanes;
    // (of a table without a positive entry max_entry() is that entry where this call used to plan with 0: swp::prefilter_packed clamps a
    // negative value to 0, so the plan is the same)
    const QuerySource src = QuerySource::sequences(d_queries, &scoring);
    pj.max_entry = src.max_entry();
    std::copy(std::begin(c->prefilter_per_cu), std::end(c->prefilter_per_cu), pj.per_cu);
    const swp::PrefilterPlan plan = swp::plan_prefilter(pj);
    for (const swp::PrefilterLaunch& l : plan.launch)
        if (c->prefilter_per_cu[l.kernel] < 1) { set_err("the pre-filter kernel does not fit a CU on this device"); return SW_EDEVICE; }
    if (int rc = stage_search_call(c, stream, 0, plan.prof_need, plan.bnd_need, true)) return rc;
    if (int rc = c->d_pfctl.once(sizeof(swk::PrefilterCtl))) return rc;
    if (int rc = upload_query_table(c, stream, plan.table, qoffsets, src)) return rc;
    hipLaunchKernelGGL(swk::sw_prefilter_commit, dim3(1), dim3(64), 0, stream, c->d_pfctl, d_npairs, 1);
    HIP_TRY(hipGetLastError());
    size_t li = 0;
    for (size_t g = 0; g < plan.group.size(); ++g) {
        if (int rc = launch_group_profiles(c, stream, src, plan.group[g])) return rc;
        for (; li < plan.launch.size() && plan.launch[li].group == (int)g; ++li) {
            const swp::PrefilterLaunch& l = plan.launch[li];
            swk::PrefilterParams pp = rank_launch_params<swk::PrefilterParams>(c, db, l);
            pp.nranks = l.nranks;
            pp.ctl = c->d_pfctl;
            pp.min_score = (int)std::min<int64_t>(min_score, INT32_MAX);
            pp.pairs = d_pairs; pp.pairs_cap = pairs_cap;
            pp.scores = d_scores;
            hipLaunchKernelGGL(kPrefilter[l.kernel].k, dim3((unsigned)l.grid), dim3(256), 0, stream, pp);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(swk::sw_prefilter_commit, dim3(1), dim3(64), 0, stream, c->d_pfctl, d_npairs, 0);
            HIP_TRY(hipGetLastError());
        }
    }
    c->last_prefilter_groups = (int64_t)plan.group.size(); c->last_prefilter_launches = (int64_t)plan.launch.size();
    c->last_prefilter_packed_launches = plan.packed_launches;
    return SW_OK;
}

// The selection over a scored pair list (csrc/sw_top_pairs.hip).  The host checks the counts and plans from them alone; it reads
// neither the list nor the results.  One memset zeroes the counts, then count, scan, scatter and sort follow each other in the stream;
// an empty list takes the sort alone, which writes the empty rows.
int sw_top_hits_pairs_device(sw_ctx* c, const sw_pair* d_pairs, const sw_result* d_results, int64_t npairs, int64_t nqueries, int64_t ntargets,
                             int64_t top, int64_t min_score, sw_hit* d_hits, int64_t* d_nhits, void* stream_) {
    const char* who = "sw_top_hits_pairs_device";
    if (!c) { set_err("%s: NULL context", who); return SW_EINVAL; }
    swp::TopPairsPlan plan;
    if (int rc = plan_top_pairs_call(c, who, npairs, nqueries, ntargets, top, d_hits, d_nhits, plan)) return rc;
    if (npairs > 0 && (!d_pairs || !d_results)) { set_err("%s: NULL d_pairs or d_results with %lld pairs", who, (long long)npairs); return SW_EINVAL; }
    c->last_top_pairs_launches = 0; c->last_top_pairs_kernel = plan.kernel;
    if (nqueries == 0) return SW_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    DevOrder order(c, stream, false);
    if (order.rc) return order.rc;
    if (int rc = grow_top_pairs_workspaces(c, plan, stream)) return rc;
    swk::TopPairsParams tp;
    memset(&tp, 0, sizeof tp);
    tp.pairs = d_pairs; tp.results = d_results; tp.npairs = npairs; tp.nqueries = nqueries; tp.ntargets = ntargets;
    tp.slice = plan.slice; tp.tbits = plan.tbits; tp.top = top; tp.min_score = min_score; tp.T = (unsigned)plan.T;
    tp.cnt = c->d_tpseg; tp.offs = c->d_tpseg + (nqueries + 1);
    tp.keys = c->d_tpkeys; tp.pos = c->d_tppos;
    tp.hits = d_hits; tp.nhits = d_nhits;
    if (npairs > 0) {
        HIP_TRY(hipMemsetAsync(tp.cnt, 0, (size_t)nqueries * sizeof(unsigned int), stream));
        const dim3 grid((unsigned)plan.grid);
        if (plan.lds) hipLaunchKernelGGL(swk::sw_top_pairs_count<true>, grid, dim3(256), 0, stream, tp);
        else hipLaunchKernelGGL(swk::sw_top_pairs_count<false>, grid, dim3(256), 0, stream, tp);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(swk::sw_top_pairs_scan, dim3(1), dim3(256), 0, stream, tp);
        HIP_TRY(hipGetLastError());
        if (plan.lds) hipLaunchKernelGGL(swk::sw_top_pairs_scatter<true>, grid, dim3(256), 0, stream, tp);
        else hipLaunchKernelGGL(swk::sw_top_pairs_scatter<false>, grid, dim3(256), 0, stream, tp);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(kTopPairsSort[plan.sort_kernel].k, dim3((unsigned)plan.sort_grid), dim3(1024), 0, stream, tp);
    HIP_TRY(hipGetLastError());
    c->last_top_pairs_launches = plan.launches;
    return SW_OK;
}

// Filter, rescoring and selection in one call.  Everything is checked and every workspace has its size before the first launch; the
// three stages then follow each other in the stream through their own entry points, the list and its results in the context's workspace.
int sw_db_search_affine_top_prefiltered(sw_ctx* c, const sw_db* db, const char* d_queries, const int64_t* qoffsets, int64_t nqueries, const sw_affine* scoring,
                                        int64_t prefilter_min_score, int64_t pairs_cap, int64_t top, int64_t min_score, sw_hit* d_hits, int64_t* d_nhits,
                                        int64_t* d_npairs, void* stream_) {
    const char* who = "sw_db_search_affine_top_prefiltered";
    if (int rc = check_db_call(who, c, db, d_queries && qoffsets && scoring)) return rc;
    int64_t maxq = 0;
    if (int rc = swh::check_search_multi(who, qoffsets, nqueries, db->longest, scoring, &maxq)) return rc;
    if (prefilter_min_score < 1) { set_err("%s: prefilter_min_score = %lld, a pair passes from 1 on", who, (long long)prefilter_min_score); return SW_EINVAL; }
    if (pairs_cap < 0) { set_err("%s: negative pairs_cap", who); return SW_EINVAL; }
    if (!d_npairs) { set_err("%s: NULL d_npairs", who); return SW_EINVAL; }
    swp::TopPairsPlan plan;
    if (int rc = plan_top_pairs_call(c, who, pairs_cap, nqueries, db->ntargets, top, d_hits, d_nhits, plan)) return rc;
    if (pairs_cap > swp::top_prefiltered_cap(c->opt_search_results_mib << 20)) {
        set_err("%s: pairs_cap = %lld entries of %lld bytes do not fit search_results_mib = %lld (at most %lld entries)", who, (long long)pairs_cap,
                (long long)swp::kTopPrefilteredEntryBytes, (long long)c->opt_search_results_mib, (long long)swp::top_prefiltered_cap(c->opt_search_results_mib << 20));
        return SW_EINVAL;
    }
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    {
        DevOrder order(c, stream, false);
        if (order.rc) return order.rc;
        if (int rc = c->d_tplist.grow((size_t)pairs_cap, stream)) return rc;
        if (nqueries > 0)
            if (int rc = grow_top_pairs_workspaces(c, plan, stream)) return rc;
    }
    sw_pair* d_pairs = pairs_cap > 0 ? (sw_pair*)c->d_tplist.p : nullptr;
    sw_result* d_results = pairs_cap > 0 ? (sw_result*)(c->d_tplist + (size_t)pairs_cap * sizeof(sw_pair)) : nullptr;
    if (int rc = sw_db_prefilter_ungapped(c, db, d_queries, qoffsets, nqueries, scoring->sub, prefilter_min_score, d_pairs, pairs_cap, d_npairs, nullptr, stream_)) return rc;
    if (int rc = sw_db_search_affine_pairs(c, db, d_queries, qoffsets, nqueries, scoring, d_pairs, pairs_cap, d_results, stream_)) return rc;
    return sw_top_hits_pairs_device(c, d_pairs, d_results, pairs_cap, nqueries, db->ntargets, top, min_score, d_hits, d_nhits, stream_);
}

}  // extern "C"
