// sw_plan.cpp -- the fill, batch and search planners (sw_plan.h).  No side effects, no allocation, no runtime calls -- except search_schedule,
// which writes the schedule to the caller's buffer and sorts through a vector of its own, and the many-query plans, which grow with the queries.
#include "sw_plan.h"
#include <algorithm>
#include <vector>

namespace swp {

// ---- measured constants (MI355X, 256 CUs).  Changing one is a change of policy: tests/test_fill_plan.py and tests/test_batch_plan.py have
// each threshold from both sides.
//
// Workgroup shape of the one-column kernel.  One strip + 8 consumers per workgroup gives every producer a SIMD of its own (measured on
// single pairs from 4096^2 to 32768^2: equal to 5 % faster than 2 + 2x4, equal at 65536^2) -- while the strips fit the CUs 4.5 times;
// batches that do not fit the CUs at once run two strips per workgroup, twice the work per CU (1024^2 pairs: 415 vs 194 GCUPS for
// 20000 pairs, 203 vs 143 for 64).
constexpr double kOneStripPerCu = 4.5;
// A chain-bound fill (one pair, up to ~3.5e8 cells: 16384^2) wants the hand-off found early -- 4 consumers + 5 importer waves: 240 vs
// 232 GCUPS at 16384^2, +7 % at 8192^2; bigger fills are bound by the stores and want 6 consumers + 3 importer waves (65536^2: 389 vs
// 340 GCUPS).
constexpr double kChainBoundCells = 3.5e8;
// Streaming stores pay off while the matrices are small next to what is in flight; measured cross-over between 16384^2 (nt 15-18 %
// faster) and 32768^2 (write-back 2-20 % faster).
constexpr double kStreamCells = 6.0e8;
// Where the two-column kernel pays: always for int32 H + P (8-byte stores of both matrices); in the other output formats while the
// strip chain (~3.1 us per 63-column strip) rather than the output volume (~3.2 TB/s) bounds the fill -- measured: 262144 x 32768
// with int8 P +18 %, 131072^2 with int8 P -3 %, 262144^2 P-only -21 % (two byte stores per row and the in-block arg-max).
constexpr double kChainSecPerStrip = 3.1e-6, kHbmBytesPerSec = 3.2e12;
// Scouts beside one filler per strip need 1.5 .. 2 workgroups per strip: up to ~170 strips (21 000 columns) on 256 CUs.
constexpr int64_t kScoutStrips = 170;
// A pair that lies in ONE class of the HBM (store probe ratio >= 1.7) and has at least 2e8 cells is slowed much less when its lines are
// streamed whole: 16384^2 307 against 232 GCUPS with 126-column strips -- 7 % behind a pair in two classes instead of 30 %.
constexpr double kOneClassCells = 2.0e8;
constexpr float kOneClassRatio = 1.7f;
// Column tiles of at most 160 strips.  Measured (one box, GCUPS tiled / untiled): 24576^2 314 / 277, 32768^2 376 / 330, 40000^2 328 /
// 394, 49152^2 308 / 406 -- a tile ramps up and drains its chain with the stores idle (3.0 TB/s on average where the untiled fill of a
// big matrix keeps 3.3), so tiles pay while the untiled fill is bound by its 7 us hand-offs, up to ~36 000 columns.  Estimates: a tile
// hands over every 2.4 us and takes 26 ns per row (+200 rows of ramp), the classic chain 7.6 us per hand-off and 35 ns per row;
// tiles are taken when they are estimated at least 2 % faster.
constexpr int64_t kTileStrips = 160;
constexpr double kTileHopSec = 2.4e-6, kTileRowSec = 26e-9, kTileBytesPerSec = 3.0e12;
constexpr double kClassicHopSec = 7.6e-6, kClassicRowSec = 35e-9, kClassicBytesPerSec = 3.3e12;
constexpr double kTileGain = 0.98;
// Roles dealt per XCD in the classic chain pay only where a workgroup runs several strips (same buffers, classic against dealt per XCD:
// 24576^2 -1 %, 32768^2 -0.4 %, 65536^2 int32 +0.3 %, int64 H +2.3 %, 262144 x 32768 with int8 P +4.4 %: the classic hand-off is not
// the trip through memory -- the polls of a filler queue behind its own H / P stores in the CU); with overlapping strips and streaming
// stores the dealing costs instead: 65536^2 int64 H 9.52 against 8.59 ms, int32 7.00 / 6.89, 24576^2 1.60 / 1.48.
constexpr int64_t kXcdChainStrips = 384;
// Split strips: a scout runs ~21.5 ns ahead of its consumers; fills of fewer rows are not split.
constexpr double kScoutLeadSec = 21.5e-9;
constexpr int64_t kSplitRows = 4096;

// One pair per wave (sw_batch.hip, sw_search.hip).  Columns per lane: 4 up to 256 columns, 8 up to 512, 16 beyond; a strip is 64 C
// columns, wider pairs (queries) go strip after strip through a boundary column of rows + 160 ints.
constexpr int64_t kC4Cols = 256, kC8Cols = 512;
constexpr int64_t kBndSlackRows = 160;
// The batch kernel: a pair whose matrix does not fit a 2 GiB buffer descriptor ((rows + 132) x (cols + 1) ints) runs on the single-pair
// machinery; so do scores beyond a signed byte and, found on the device, more than 8 distinct letters.
constexpr int64_t kWaveSlackRows = 132;
constexpr double kWaveMatrixBytes = 2147483648.0;
constexpr int kWaveScore = 127;
constexpr unsigned kWaveLetters = 8, kLE4Letters = 4;   // (up to four letters: half-size score profiles)
// padded letter codes of every pair's b: 64 in front, 80 + 72 behind (+40: the drain steps of the delayed int8 P stores read on)
constexpr int kCodesFront = 64;
constexpr int64_t kCodesTail = 80 + 72;
// pairs per launch: bounds the workspace (codes: ~1.2 KB per 1024-row pair), 1 GiB of codes and 1 GiB of boundary columns
constexpr int64_t kBatchWorkspaceBytes = 1ll << 30;
// alphabet of the whole batch: one sw_prep_scan block per 4096 letters, at most 2048 (sw_prep_reduce merges their maps); sw_batch_codes:
// at most 64 blocks per pair
constexpr int64_t kScanLetters = 4096, kScanBlocks = 2048, kCodesBlocks = 64;
// Score-only batches whose scores fit 15 bits run two pairs per wave on packed 16-bit lanes (sw_batch_wave16: 5 VALU per two cells
// instead of 8): match x min(cols, rows) and -gap below 32000, fewer than 65000 rows.  (debug bit 18: off, A/B runs)
constexpr int64_t kWave16Score = 32000, kWave16Rows = 65000;
// (scores of 12 bits: the arg-max runs on score * 16 + column keys)
constexpr int64_t kKeyedScore = 4096;
// the fall-back, pairs per launch: bounds the edge / padded-b workspace
constexpr int64_t kSingleChunk = 4096;
// Database search: persistent waves, as many workgroups (4 waves) as are resident, fewer where the targets are fewer or the boundary
// columns of a multi-strip query (one per wave, sized by the longest target) would pass 1 GiB.  The profile: at most 4096 blocks.
constexpr int64_t kSearchBndBytes = 1ll << 30;
constexpr int64_t kProfileBlocks = 4096;

namespace {

// Roles dealt per XCD (workgroup i on XCD i % 8, 32 CUs each): an eighth of the fillers on every XCD and the scouts that feed them,
// two strips to a scout where the XCD has no room for one each.  The last strip needs no scout (one fewer on XCD 0); split strips
// give it one (one more on XCD 7).
struct Deal { bool fits = true; int scouts = 0, doubles = 0; };
Deal deal_per_xcd(int64_t S2, bool last_strip_scout) {
    Deal r;
    for (int x = 0; x < 8 && r.fits; ++x) {
        const int nf = (int)(S2 / 8) + (x < (int)(S2 % 8) ? 1 : 0), ns = (x ? nf : nf - 1) + (last_strip_scout && x == 7 ? 1 : 0);
        const int ndx = std::max(0, ns - (32 - nf));
        r.fits = nf <= 31 && 2 * ndx <= ns;
        r.scouts += ns - ndx; r.doubles += ndx;
    }
    return r;
}

}  // namespace

FillPlan plan_fill(const PlanJob& j, const DeviceFacts& dev, const PlanOptions& o) {
    using namespace swk;
    FillPlan f;
    const int64_t cols = j.cols, rows = j.rows;
    const bool systolic = o.engine == 0;
    f.engine = systolic ? 0 : 1;
    const int64_t S = f.S = systolic ? (cols + 62) / 63 : (cols + 63) / 64;
    f.edge_need = (size_t)S * (size_t)(rows + 1) * (size_t)j.npairs;
    f.h_bytes = (size_t)(cols + 1) * (size_t)(rows + 1) * (size_t)j.h_elem_bytes;
    f.p_bytes = (size_t)(cols + 1) * (size_t)(rows + 1) * (size_t)j.p_elem_bytes;
    f.store_nt = o.store_policy == 2 || (o.store_policy == 0 && (double)cols * (double)rows * (double)j.npairs <= kStreamCells);
    if (!systolic) {
        const int wpb = (int)o.waves_per_block;
        const int64_t maxb = o.max_blocks > 0 ? o.max_blocks : 2ll * dev.num_cus;
        f.grid = (int)std::max<int64_t>(1, std::min<int64_t>((S + wpb - 1) / wpb, maxb));
        f.threads = 64 * wpb;
        return f;
    }
    int NS = (int)o.strips_per_group, NC = (int)o.consumers;
    if (NS == 0) NS = (j.npairs == 1 ? (double)S <= kOneStripPerCu * dev.num_cus : (double)S * (double)j.npairs <= (double)dev.num_cus) ? 1 : 2;
    // NS == 1: nine waves on the three SIMDs the producer leaves
    const bool chain_bound = NS == 1 && j.npairs == 1 && (double)cols * (double)rows <= kChainBoundCells;
    if (NC == 0) NC = (NS == 1) ? (chain_bound ? 4 : 6) : 4;
    f.importers = o.importers > 0 ? (int)o.importers : (chain_bound && NC <= 4 ? 4 : 2);
    if (NS == 1 && NC > 7) NC = 7;         // nine waves off the producer's SIMD: at most 7 consumers + exporter + importer
    if (NS == 1 && NC == 5) NC = 4;        // (the one-column kernel has no five-consumer form: option "consumers" = 5 is for the two-column kernel)
    f.NS = NS; f.NC = NC;
    // padded copies of b per problem: [front | b | tail]; front covers the fast producers' phi (< strips) + 63 lanes
    // (+ one 16-step block: the perm producer's first score window ends at step 0)
    f.bfront = ((S + 64 + 32 + 127) / 128) * 128;
    f.per = ((rows + f.bfront + 512 + 15) / 16) * 16;
    f.cb_need = (size_t)f.per * (size_t)j.npairs;
    // perm producer (alphabets of up to 7 letters): eligible when the scores fit a signed byte and every G value,
    // with the 2^16 bias, stays below 2^24 (the top byte carries the launch tag)
    const int64_t mm = j.match - 2 * j.gap, xm = j.mismatch - 2 * j.gap;
    const int64_t lo = std::min(cols, rows);
    const int64_t gmax = (int64_t)j.match * std::max<int64_t>(lo, std::min(cols, j.total_rows)) + (int64_t)(-j.gap) * (rows + cols + 2);
    const bool halo_unbounded = (j.has_top || j.has_left) && j.total_rows == 0;   // a tile whose halo magnitudes are unknown here
    f.perm = !halo_unbounded && mm <= 127 && mm >= -127 && xm <= 127 && xm >= -127 && gmax + 0x10000 + 1024 < (1ll << 24) &&
             !(o.debug_flags & DBG_NO_PERM);
    if (f.perm) {
        f.e4stride = ((rows + S + 160 + 31) / 32) * 32;   // (whole 128-byte lines: strips written on different XCDs share none)
        f.edge4_need = (size_t)S * (size_t)f.e4stride * (size_t)j.npairs;
    }
    f.fast = !j.has_top && !j.has_top_gran && j.mismatch <= 0 && !(o.debug_flags & DBG_GENERIC_PRODUCER);
    const int64_t ngroups = ((S + NS - 1) / NS) * j.npairs;
    const int64_t maxb = o.max_blocks > 0 ? o.max_blocks : std::max<int64_t>(8, (int64_t)dev.num_cus - j.reserve_cus);
    f.grid = (int)std::max<int64_t>(1, std::min<int64_t>(ngroups, maxb));
    if (NS == 1) {
        // wave 0 (the producer) owns SIMD 0: waves 4, 8, 12 idle; consumers, the exporter and the importers are the
        // K waves off SIMD 0 (wave id of ordinal k: k + 1 + k/3)
        const int K = std::min<int>(9, NC + 1 + std::max(1, f.importers));   // 12 waves: 3 per SIMD
        f.threads = 64 * (K + (K - 1) / 3 + 1);
    } else {
        f.threads = 64 * (NS * (1 + NC) + 2);
    }

    // Two matrix columns per lane (sw_systolic2.inc): half as many strips -- and row segments of 504 bytes per store -- for the
    // same work: 16384^2 +4 %, 8192^2 +11 %, 24576^2 +29 %, 32768^2 +32 %, 65536^2 +9 % over one column per lane.  Whole
    // matrix of one pair, int32 H and P both stored, rows a multiple of 16; the alphabet (found on the device) must allow the
    // perm path -- so both kernels are enqueued and each checks for itself which of them has to work.
    // Also: int8 P, either matrix left out, and band-resident launches (halo row in, last row out as granules).
    const bool base_mode = j.has_H && j.has_P && j.h_elem_bytes == 4 && j.p_elem_bytes == 4 && !j.has_top && !j.has_top_gran && !j.has_bot_gran;   // int32 H + P, whole matrix
    const double est_chain = (double)S * kChainSecPerStrip;
    const double est_hbm = (double)(cols + 1) * (double)(rows + 1) * ((j.has_H ? (double)j.h_elem_bytes : 0.0) + (j.has_P ? (double)j.p_elem_bytes : 0.0)) / kHbmBytesPerSec;
    // (... and int32 H + int8 P or H alone beyond the reach of the scouts: the H of overlapping strips goes out in streamed whole lines --
    //  65536^2 597 GCUPS against 429 on the one-column kernel and 494 with 126-column strips)
    const bool pays = (j.has_H && j.has_P && j.p_elem_bytes == 4) || (j.has_H && j.h_elem_bytes == 8) || est_chain >= (j.has_H ? 0.5 : 2.0) * est_hbm ||
                      (o.debug_flags & DBG_FORCE_TWO_COLUMNS) ||
                      (j.has_H && j.h_elem_bytes == 4 && (!j.has_P || j.p_elem_bytes == 1) && cols % 2 == 0 && cols > 126 * kScoutStrips);
    // The two-column kernel is ONE launch per fill: its prologue does what sw_prep_scan / sw_prep_code do for the other kernels (every
    // workgroup keeps its own padded copy of b and of its letter codes) and its last workgroup out writes the result (sw_systolic2.inc).
    // The strict one-launch path needs a result to write (a batch keeps its own keys and never comes here).
    f.two_cols = pays && f.perm && o.strips_per_group == 0 && (o.consumers == 0 || o.consumers >= 4) && j.npairs == 1 &&
                 !j.has_left && !j.has_right && j.full_stride && (rows % 16 == 0 || !j.has_bot_gran) && rows >= 1 && cols >= 1 &&   // (a band's last row leaves from a full block)
                 (base_mode || (cols % 2 == 0)) &&   // (an odd column count leaves one lane with a single column: only the base mode handles it)
                 !(o.debug_flags & (DBG_PRODUCER_ONLY | DBG_SKIP_STRIP1 | DBG_WAVE_PLACEMENT | DBG_BLOCK_STAMPS | DBG_EDGE_DUMP | DBG_NO_TWO_COLUMNS)) &&
                 dev.s2_per_cu >= 1 && j.has_result;
    f.priv_stride = ((2 * f.per + 255) / 256) * 256;
    if (!f.two_cols) return f;
    f.priv_need = (size_t)f.priv_stride * (size_t)dev.s2_per_cu * (size_t)dev.num_cus;

    // Strip geometry: every 126 columns (the strips tile the matrix), or every 110 with 16 columns of overlap -- whole-line stores
    // (sw_systolic2.inc); option "s2w" forces one of the two (tests, A/B runs).
    // Overlapping strips store whole 64-byte lines, and whole lines can be STREAMED (nt): together that is worth 1.2 - 1.5x wherever the strips
    // do not leave room for scouts (GCUPS, strips every 126 write-back / every 110 streaming, same buffers: int32 H 21760^2 278 (tiles) / 363,
    // 24576^2 314 (tiles) / 409, 32768^2 382 (tiles) / 481, 40000^2 385 / 540, 49152^2 403 / 595, 65536^2 436 / 624, 81920^2 474 / 559; int64 H
    // 20480^2 264 (scouts) / 330, 24576^2 238 / 369, 32768^2 265 / 409, 49152^2 282 / 403, 65536^2 382 / 451).  Streaming PARTIAL lines is what
    // round 2 measured as harmful; write-back whole lines are what the first version of the overlap did (+14 % for int64 H only).  Behind
    // scouts (up to 170 strips) the 126-column geometry stays: there the chain bounds the fill and 14 % more strips cost more than the
    // stores gain (int32 16384^2: 335 / 322) -- except for an int64 H whose 110-column strips no longer fit beside scouts (18 700 - 21 400
    // columns), which is faster as a plain chain of overlapping strips than behind scouts.
    const bool band_io = j.has_top || j.has_top_gran || j.has_bot_gran;
    const bool wl_fmt = !band_io && j.has_H && (!j.has_P || j.p_elem_bytes == 4 || (j.h_elem_bytes == 4 && cols % 2 == 0)) && (j.has_P || cols % 2 == 0) &&
                        j.full_stride && j.h_aligned && j.p_aligned;
    const int64_t S126 = cols <= 126 ? 1 : (cols - 126 + 125) / 126 + 1, S110 = cols <= 126 ? 1 : (cols - 126 + 109) / 110 + 1;
    // A pair in one class of the HBM: the allocator's probe knows (its search ran out of budget, or the caller asked for a plain pair).  Pairs
    // the library did not allocate are probed only with option "probe_foreign_pairs" -- the probe writes -- and keep 126 otherwise.
    bool one_class = false;
    if (j.has_P && (double)cols * (double)rows >= kOneClassCells) {
        f.probe_pair_class = j.pair_ratio == 0.f && o.probe_foreign_pairs && o.s2w == 0 && wl_fmt && S126 <= kScoutStrips;
        one_class = j.pair_ratio >= kOneClassRatio;
    }
    int64_t W2 = 126;
    if (o.s2w == 110 ? (!band_io && (cols % 2 == 0 || wl_fmt))
                     : (o.s2w == 0 && wl_fmt && (S126 > kScoutStrips || (j.h_elem_bytes == 8 && S110 > kScoutStrips) || one_class)))
        W2 = 110;
    f.W2 = (int)W2;
    const bool ov_auto = W2 == 110 && o.s2w == 0;   // (the library's own choice: one launch, streaming stores)
    auto strips_of = [&](int64_t ncols) { return ncols <= 126 ? (int64_t)1 : (ncols - 126 + W2 - 1) / W2 + 1; };
    const int64_t S2all = strips_of(cols);
    // Column tiles.  A matrix wider than the scouts reach used to run the classic chain, fillers handing over to fillers at 7 us per
    // strip (32768^2: 349 GCUPS).  Now it is cut into column tiles, ONE LAUNCH EACH, every one with scouts, roles per XCD and paced
    // fillers; a tile's left halo is the previous tile's last column, read from H itself (kernel boundary: no flags), the arg-max
    // accumulates in the key across the launches and the last one reports.  Taken where the estimate says it pays: not where the
    // stores bound the fill anyway (int64 H at 65536^2), not for bands (their halo row arrives while they run).
    f.tstrips = S2all;
    if (S2all > kScoutStrips && base_mode && j.full_stride && j.has_result && !ov_auto && !(o.debug_flags & DBG_NO_TILES)) {
        const int64_t nt = (S2all + kTileStrips - 1) / kTileStrips, st = (S2all + nt - 1) / nt;
        const double bytes = (double)(cols + 1) * (double)(rows + 1) * 8.0;
        const double t_tiles = (double)nt * std::max((double)st * kTileHopSec + (double)(rows + 200) * kTileRowSec, bytes / (double)nt / kTileBytesPerSec);
        const double t_classic = std::max((double)S2all * kClassicHopSec + (double)rows * kClassicRowSec, bytes / kClassicBytesPerSec);
        if (t_tiles < kTileGain * t_classic) { f.ntile = nt; f.tstrips = st; }
    }
    const int64_t per_cu = dev.s2_per_cu;
    for (int64_t tile = 0; tile < f.ntile; ++tile) {
        TilePlan& t = f.tile[tile];
        t.c0 = tile * f.tstrips * W2;
        t.cols = tile + 1 == f.ntile ? cols - t.c0 : f.tstrips * W2;   // (a tile owns tstrips * W2 columns; the last one the rest)
        const int64_t S2 = t.strips = strips_of(t.cols);
        t.store_nt = f.store_nt;
        if (f.ntile > 1) t.store_nt = o.store_policy == 2 || (o.store_policy == 0 && (double)t.cols * (double)rows <= kStreamCells);   // (per launch, as for a matrix of the tile's size)
        if (W2 == 110 && wl_fmt && o.store_policy == 0) t.store_nt = 1;   // (whole lines: streamed)
        t.grid = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(S2, maxb), per_cu * dev.num_cus));
        // Scouts (sw_systolic2.inc): while every strip has a workgroup of its own and half as many more fit the device, the chain
        // of strips runs in extra workgroups that keep nothing but the edge columns, and the workgroups that write the matrices
        // follow them instead of each other.  One scout strip per workgroup where the device has the workgroups for it (S2 fillers
        // + S2 scouts), two in as many scout workgroups as it takes to fit; at least 1.5 S2 workgroups in all.
        const int64_t avail = std::min<int64_t>(maxb, per_cu * dev.num_cus);
        const int64_t ndouble = std::max<int64_t>(0, 2 * S2 - 1 - avail);   // (the last strip needs no scout: nobody reads its edge)
        const int64_t nsc = S2 - 1 - ndouble;
        const bool scouts = S2 >= 4 && 2 * ndouble <= S2 - 1 && nsc >= 1 && !(o.debug_flags & DBG_NO_SCOUTS);
        t.nscout = scouts ? (int)nsc : 0;
        t.scout_double = scouts ? (int)ndouble : 0;
        if (scouts) t.grid = (int)(S2 + nsc);
        // Roles dealt per XCD (sw_systolic2.inc): an eighth of the fillers and the scouts that feed them on every XCD, so that an edge
        // column is read on the XCD that wrote it -- out of its L2, without the trip through the memory fabric.  Needs the whole device
        // (256 workgroups, one per CU, workgroup i on XCD i % 8).
        if (scouts && dev.xcd_round_robin && avail >= 256 && S2 >= 16 && !(o.debug_flags & DBG_NO_XCD_DEALING)) {
            const Deal d = deal_per_xcd(S2, false);
            if (d.fits) { t.xcd_mode = 1; t.nscout = d.scouts; t.scout_double = d.doubles; t.grid = 256; }
        }
        // Split strips (sw_systolic2.inc): from strip split_from on -- those that would end after everybody else -- the strip's scout
        // (a workgroup with rings and consumers then) writes the blocks from split_blk on and the filler only those before; the
        // last strip gets a scout for it (one more workgroup on XCD 7).  The split point equalises the two ends: the filler needs
        // tau_f per row, the scout kScoutLeadSec before its consumers start and tau_f after.  Needs the per-XCD dealing and pacing
        // (the common end every filler is paced to moves with it).
        if (t.xcd_mode == 1 && (rows >= kSplitRows || o.split_blk > 0) && !j.has_top && !j.has_top_gran && !j.has_bot_gran && o.filler_hop_ps > 0 &&
            !(o.debug_flags & (DBG_NO_PACING | DBG_NO_SPLIT))) {
            const Deal d = deal_per_xcd(S2, true);
            const double hop = (double)o.filler_hop_ps * 1e-12, tf = (double)o.filler_tau_ps * 1e-12, ts = kScoutLeadSec;
            const int64_t nblk = (rows + 15) / 16;
            const int64_t sblk = (int64_t)((double)nblk * tf / (2.0 * tf - std::min(ts, tf)));
            const bool forced = o.split_blk > 0;   // (tests: any split point, any first strip)
            if (d.fits && forced && o.split_blk < nblk) {
                t.split_blk = (int)o.split_blk; t.split_from = (int)std::max<int64_t>(1, o.split_from); t.split_extra = 1;
                t.filler_end_steps = (int)((o.split_blk * 16 + 126) / 64 * 64 + 64); t.filler_full_steps = (int)((nblk * 16 + 126) / 64 * 64 + 64);
                t.nscout = d.scouts; t.scout_double = d.doubles;
            } else if (d.fits && sblk >= 16 && sblk < nblk && rows >= kSplitRows) {
                const int64_t full_steps = (nblk * 16 + 126) / 64 * 64 + 64, end_steps = (sblk * 16 + 126) / 64 * 64 + 64;
                // strip s, unsplit, would end s hand-offs + a whole strip after the start; the split ones end (S2 - 1) hand-offs + end_steps
                const double lead = ((double)full_steps - (double)end_steps) * tf / hop;
                const int64_t from = std::max<int64_t>(1, (int64_t)((double)(S2 - 1) - lead) + 1);
                if (from < S2) {
                    t.split_blk = (int)sblk; t.split_from = (int)from; t.split_extra = 1;
                    t.filler_end_steps = (int)end_steps; t.filler_full_steps = (int)full_steps;
                    t.nscout = d.scouts; t.scout_double = d.doubles;
                }
            }
        }
        // The classic chain (no room for scouts), dealt per XCD the same way: neighbouring strips on one XCD, edge columns through
        // its L2.  (option "xcd_chain": 0 auto, 1 on, 2 off)
        const bool xcd_chain_pays = S2 >= kXcdChainStrips && W2 != 110;
        if (!scouts && dev.xcd_round_robin && t.grid >= 64 && !(o.debug_flags & DBG_NO_XCD_DEALING) &&
            (o.xcd_chain == 1 || (o.xcd_chain == 0 && xcd_chain_pays)))
            t.xcd_mode = 2;
        // pacing of the fillers behind scouts (sw_systolic2.inc): estimates on the low side, so that nobody is held back more
        // than the last filler's best case allows.  (options "filler_hop_ps" / "filler_tau_ps")
        t.filler_hop_ps = (scouts && !(o.debug_flags & DBG_NO_PACING)) ? (int)o.filler_hop_ps : 0;
        t.filler_tau_ps = (int)o.filler_tau_ps;
        t.filler_bw_gbs = (int)o.filler_bw_gbs;
        // consumer waves (+ 9 - consumers importers).  Behind scouts a filler is never the one a hand-off waits for: two importers do, and
        // seven consumers keep more stores in flight (16384^2 -1.5 %, 12288^2 -2.5 %, 20480^2 +-0 against five)
        // (overlapping strips, whose consumers are dearer: seven as well -- 32768^2 485 against 453-466 GCUPS, 65536^2 633 / 607, int64 H 502 / 495)
        t.consumers = o.consumers == 0 ? ((scouts || W2 == 110) ? 7 : (chain_bound ? 5 : 6)) : (int)std::min<int64_t>(7, o.consumers);
        // The alphabet scan of the prologue (sw_systolic2.inc).  Shared among the workgroups it costs eight agent-scope atomics and a
        // grid barrier over up to 256 workgroups before anybody's first step, whatever the size; done by every workgroup for itself it
        // costs cols + rows bytes read from the L2 with 16-byte loads, 12 KB per pass of a workgroup.  Decided by the WHOLE matrix'
        // columns and the launch's rows, so that every column tile decides alike.  (debug bits 28 / 29 force either)
        // Measured (us until every workgroup knows the alphabet, shared | private): 32 K letters 12.4 | 10.5, 48 K 12.2 | 12.0, 64 K 12.5 | 15.3,
        // 128 K 12.8 | 23.0 -- the crossover is at ~50 K letters (profiles/r05_prologue_stamps.log).
        t.scan_all = (cols + rows <= kScanAllLetters) ? 1 : 0;
        if (o.debug_flags & DBG_S2_BARRIER_SCAN) t.scan_all = 0;
        if (o.debug_flags & DBG_S2_SCAN_ALL) t.scan_all = 1;
    }
    return f;
}

namespace {
int lane_columns(int64_t cols) { return cols <= kC4Cols ? 4 : cols <= kC8Cols ? 8 : 16; }
int64_t boundary_ints(int64_t nstrips, int64_t rows) { return nstrips > 1 ? ((rows + kBndSlackRows + 3) / 4) * 4 : 0; }
}  // namespace

BatchPlan plan_batch(const BatchJob& j, const PlanOptions& o) {
    using namespace swk;
    BatchPlan b;
    const int64_t cols = j.cols, rows = j.rows;
    b.wave = !(o.debug_flags & DBG_BATCH_SINGLE_PAIR) && j.match <= kWaveScore && j.match >= -kWaveScore && j.mismatch <= kWaveScore &&
             j.mismatch >= -kWaveScore && (double)(rows + kWaveSlackRows) * (double)(cols + 1) * 4.0 < kWaveMatrixBytes;
    b.single_chunk = std::min(j.npairs, kSingleChunk);
    b.C = lane_columns(cols);
    b.nstrips = (cols + 64 * b.C - 1) / (64 * b.C);
    b.front = kCodesFront;
    b.per = ((rows + kCodesFront + kCodesTail + 15) / 16) * 16;
    b.bnd_per = boundary_ints(b.nstrips, rows);
    b.chunk = std::max<int64_t>(1, std::min<int64_t>(j.npairs, std::min<int64_t>(kBatchWorkspaceBytes / b.per,
                                                                                  b.bnd_per ? kBatchWorkspaceBytes / (b.bnd_per * 4) : j.npairs)));
    b.grid = (b.chunk + 3) / 4;   // (4 pairs, one per wave, per workgroup)
    b.scan_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(((cols + rows) * j.npairs + kScanLetters - 1) / kScanLetters, kScanBlocks));
    b.codes_blocks = (int)std::min<int64_t>((b.per + 255) / 256, kCodesBlocks);
    b.bcodes_need = (size_t)(b.chunk * b.per);
    b.bnd_need = (size_t)(b.chunk * b.bnd_per);
    const int64_t smax = (int64_t)j.match * std::min(cols, rows);
    b.fits16 = j.npairs >= 2 && b.C == 16 && smax < kWave16Score && -j.gap < kWave16Score && rows < kWave16Rows && !(o.debug_flags & DBG_BATCH_NO_WAVE16);
    b.k12 = smax < kKeyedScore;
    // ... and with an int8 P as the only matrix, P codes from packed arithmetic (debug bit 21: off)
    b.packed16 = b.fits16 && !j.has_H && (!j.has_P || (j.p_elem_bytes == 1 && !(o.debug_flags & DBG_BATCH_NO_PACKED_P)));
    return b;
}

int batch_kernel(const BatchPlan& b, unsigned nletters, int64_t n, int p_bytes) {
    if (nletters > kWaveLetters) return -1;
    if (b.packed16 && n >= 2)   // (an odd last pair runs in both halves of a wave)
        return batch_wave16_index(nletters <= kLE4Letters, b.k12, p_bytes != 0);
    return batch_wave_index(b.C, p_bytes);
}

SearchPlan plan_search(const SearchJob& j, const DeviceFacts& dev) {
    using swk::SW_SEARCH_ROWS;
    SearchPlan s;
    s.C = lane_columns(j.qlen);
    s.wide = j.match > kWaveScore || j.mismatch < -kWaveScore;   // (mismatch <= match: both fit a signed byte otherwise)
    s.kernel = search_kernel_index(s.C, s.wide);
    s.nstrips = (j.qlen + 64 * s.C - 1) / (64 * s.C);
    s.qpad = s.nstrips * 64 * s.C;
    s.bnd_per = boundary_ints(s.nstrips, j.maxlen);
    s.grid = std::min<int64_t>((int64_t)dev.search_per_cu[s.kernel] * dev.num_cus, (j.ntargets + 3) / 4);
    if (s.bnd_per) s.grid = std::max<int64_t>(1, std::min<int64_t>(s.grid, kSearchBndBytes / (s.bnd_per * 4 * 4)));
    s.prof_need = (size_t)(SW_SEARCH_ROWS * s.qpad);
    s.prof_blocks = (int)std::min<int64_t>((SW_SEARCH_ROWS * s.qpad + 255) / 256, kProfileBlocks);
    s.bnd_need = s.bnd_per ? (size_t)(s.grid * 4 * s.bnd_per) : 0;
    return s;
}

// The affine kernel keeps two values per cell (h, e) in registers where the linear one keeps one.  What the gfx950 code object reports
// (waves per SIMD of 512 VGPRs: 6 at 4 columns per lane, 5 at 8, 3 at 16 -- 77 / 94 / 134 VGPRs) leaves 16 columns per lane at three
// workgroups per CU: fewer waves, but each step's hand-over, arg-max and waits are spread over twice the cells and a query takes half
// the strips, and the loads are software-pipelined a group of rows ahead, so the kernel needs waves only to cover issue bubbles.  The
// linear thresholds are kept while 16 columns per lane still give two waves per SIMD (two workgroups per CU); below that 8 are taken.
// Measured: 3371 GCUPS on the kernel at 16 columns per lane and a query of 2048, 3017 at 8 columns and a query of 512.
constexpr int kAffineC16MinPerCu = 2;

namespace {

// Columns per lane of a query under affine gaps: lane_columns, but 16 only where the 16-column kernel (occupancy per_cu16) keeps
// kAffineC16MinPerCu workgroups on a CU.
int query_columns(int64_t qlen, int per_cu16) {
    const int C = lane_columns(qlen);
    return C == 16 && per_cu16 < kAffineC16MinPerCu ? 8 : C;
}
int64_t query_padded(int64_t qlen, int per_cu16) {
    const int64_t w = 64 * query_columns(qlen, per_cu16);
    return (qlen + w - 1) / w * w;
}

// Workgroups of four waves a launch may run: the resident ones, a quarter of its items (items < 0: not known here, the answer is the
// most any list can use), what the boundary columns leave of kSearchBndBytes; at least 1.
int64_t grid_cap(int per_cu, int num_cus, int64_t bnd_per, int64_t items = -1) {
    int64_t grid = (int64_t)per_cu * num_cus;
    if (items >= 0) grid = std::min(grid, (items + 3) / 4);
    if (bnd_per) grid = std::min(grid, kSearchBndBytes / (bnd_per * 4 * 4));
    return std::max<int64_t>(1, grid);
}

// Slots of an alignment launch, one per wave at work: the entries, the resident waves, the budget, the boundary columns; at least 1.
int64_t slot_cap(int64_t entries, int per_cu, int num_cus, int64_t budget_bytes, int64_t slot_bytes, int64_t bnd_per) {
    int64_t slots = std::min<int64_t>({entries, (int64_t)per_cu * num_cus * 4, budget_bytes / slot_bytes});
    if (bnd_per) slots = std::min(slots, kSearchBndBytes / (bnd_per * 4));
    return std::max<int64_t>(1, slots);
}

}  // namespace

SearchAffinePlan plan_search_affine(const SearchAffineJob& j) {
    using swk::SW_SEARCH_ROWS;
    SearchAffinePlan s;
    s.C = query_columns(j.qlen, j.per_cu[search_affine_kernel_index(16)]);
    s.kernel = search_affine_kernel_index(s.C);
    s.nstrips = (j.qlen + 64 * s.C - 1) / (64 * s.C);
    s.qpad = s.nstrips * 64 * s.C;
    s.bnd_row_ints = 2;
    s.bnd_per = s.bnd_row_ints * boundary_ints(s.nstrips, j.maxlen);
    s.grid = grid_cap(j.per_cu[s.kernel], j.num_cus, s.bnd_per, j.ntargets);
    s.prof_need = (size_t)(SW_SEARCH_ROWS * s.qpad);
    s.prof_blocks = (int)std::min<int64_t>((SW_SEARCH_ROWS * s.qpad + 255) / 256, kProfileBlocks);
    s.bnd_need = s.bnd_per ? (size_t)(s.grid * 4 * s.bnd_per) : 0;
    return s;
}

// ---- the shared parts of the many-query plans.  Every many-query kernel table has one instantiation per width, at index C / 8.
namespace {

constexpr int kQueryClasses = 3;
static_assert(kSearchMultiKernels == kQueryClasses && kSearchPairsKernels == kQueryClasses && kAlignHitsKernels == kQueryClasses &&
              kPrefilterKernels == 2 * kQueryClasses && search_multi_kernel_index(16) == kQueryClasses - 1);
constexpr int class_columns(int k) { return k == 0 ? 4 : 8 * k; }

// The layout of a call's queries.  Groups: consecutive queries while their profiles fit the budget and, where the caller bounds them,
// at most group_queries of them; at least one, so one query alone may exceed the budget.  The table of a group: by class, input order
// within a class; the profiles lie in table order.  Host work is O(nqueries); nothing here looks at a target.
struct QueryClass { int64_t q0 = 0, nq = 0, qpad = 0, nstrips = 0; };   // entries q0 .. q0 + nq - 1; the largest qpad and nstrips among them
struct QueryGroup {
    int64_t q0 = 0, nq = 0, prof_bytes = 0;
    QueryClass cls[kQueryClasses];
};
struct QueryLayout {
    std::vector<swk::MultiQuery> table;
    std::vector<QueryGroup> group;
    size_t prof_need = 0;
};

QueryLayout layout_queries(const int64_t* qlens, int64_t n, int per_cu16, int64_t budget_bytes, int64_t group_queries = INT64_MAX) {
    using swk::SW_SEARCH_ROWS;
    QueryLayout y;
    y.table.resize((size_t)n);
    for (int64_t g0 = 0; g0 < n;) {
        QueryGroup grp;
        int64_t g1 = g0, bytes = 0;
        while (g1 < n && (g1 == g0 || (g1 - g0 < group_queries && bytes + SW_SEARCH_ROWS * query_padded(qlens[g1], per_cu16) <= budget_bytes)))
            bytes += SW_SEARCH_ROWS * query_padded(qlens[g1++], per_cu16);
        grp.q0 = g0; grp.nq = g1 - g0; grp.prof_bytes = bytes;
        y.prof_need = std::max(y.prof_need, (size_t)bytes);
        int64_t at[kQueryClasses + 1] = {};
        for (int64_t q = g0; q < g1; ++q) ++at[query_columns(qlens[q], per_cu16) / 8 + 1];
        for (int k = 0; k < kQueryClasses; ++k) {
            at[k + 1] += at[k];
            grp.cls[k].q0 = g0 + at[k]; grp.cls[k].nq = at[k + 1] - at[k];
        }
        for (int64_t q = g0; q < g1; ++q) {
            const int C = query_columns(qlens[q], per_cu16);
            const int64_t qpad = query_padded(qlens[q], per_cu16);
            QueryClass& c = grp.cls[C / 8];
            y.table[(size_t)(g0 + at[C / 8]++)] = swk::MultiQuery{0, 0, q, (int32_t)qlens[q], (int32_t)qpad, (int32_t)(qpad / (64 * C)), 0};
            c.qpad = std::max(c.qpad, qpad);
            c.nstrips = std::max(c.nstrips, qpad / (64 * C));
        }
        int64_t off = 0;
        for (int64_t t = g0; t < g1; ++t) { y.table[(size_t)t].prof_off = off; off += SW_SEARCH_ROWS * y.table[(size_t)t].qpad; }
        y.group.push_back(grp);
        g0 = g1;
    }
    return y;
}

// The entries [a, b) of a class with those that run packed moved to the front, input order within either part (every entry keeps its
// profile's place); returns where the others begin.
template <typename Packed>
int64_t packed_first(std::vector<swk::MultiQuery>& table, int64_t a, int64_t b, Packed packed) {
    return std::stable_partition(table.begin() + a, table.begin() + b, packed) - table.begin();
}
// (the packed kernel of 16 columns per lane is taken where it keeps the workgroups on a CU that the 32-bit one needs)
bool packed_kernel_fits(const int* packed_per_cu, int k) { return packed_per_cu[k] >= (class_columns(k) == 16 ? kAffineC16MinPerCu : 1); }

// The launches of the entries [s0, s1) of a class, all packed or all not, against every target rank: cut by target ranks (and by queries,
// should the part alone pass the limit) so that no launch has more than max_items items.  A packed launch takes the ranks in pairs and
// counts rank pairs.  The boundary columns are sized by the strips of the launch's own queries.  Returns the launches it added.
struct Ranks { int num_cus; int64_t nonempty, longest, max_items; };
template <typename Job>
Ranks ranks_of(const Job& j) { return Ranks{j.num_cus, j.nonempty, j.longest, std::max<int64_t>(1, std::min(j.max_items, kMultiMaxItems))}; }

template <typename Launch>
int64_t cut_rank_launches(std::vector<Launch>& out, size_t& bnd_need, const std::vector<swk::MultiQuery>& table, const Ranks& r, int group, int C, int kernel,
                          int per_cu, bool packed, int64_t s0, int64_t s1) {
    const size_t before = out.size();
    for (int64_t qa = s0; qa < s1 && r.nonempty > 0;) {
        const int64_t nq = std::min(s1 - qa, r.max_items), ranks_per = (packed ? 2 : 1) * (r.max_items / nq);
        int64_t strips = 1;
        for (int64_t t = qa; t < qa + nq; ++t) strips = std::max<int64_t>(strips, table[(size_t)t].nstrips);
        for (int64_t r0 = 0; r0 < r.nonempty; r0 += ranks_per) {
            Launch l;
            l.group = group; l.C = C; l.kernel = kernel;
            if constexpr (requires { l.packed; }) l.packed = packed;
            l.q0 = qa; l.nq = nq;
            l.rank0 = r0; l.nranks = std::min(ranks_per, r.nonempty - r0);
            l.items = l.nq * (packed ? (l.nranks + 1) / 2 : l.nranks);
            l.bnd_per = 2 * boundary_ints(strips, r.longest);
            l.grid = grid_cap(per_cu, r.num_cus, l.bnd_per, l.items);
            bnd_need = std::max(bnd_need, (size_t)(l.grid * 4 * l.bnd_per));
            out.push_back(l);
        }
        qa += nq;
    }
    return (int64_t)(out.size() - before);
}

// What the three plans of rank launches hand over of a layout.
template <typename Plan>
void take_layout(Plan& p, QueryLayout& y) {
    p.table = std::move(y.table);
    p.prof_need = y.prof_need;
    for (const QueryGroup& g : y.group) p.group.push_back(MultiGroup{g.q0, g.nq, g.prof_bytes});
}

}  // namespace

// Many queries against a prepared database: per (group, class) the launches of cut_rank_launches.
SearchMultiPlan plan_search_multi(const SearchMultiJob& j) {
    SearchMultiPlan m;
    QueryLayout y = layout_queries(j.qlens, j.nqueries, j.per_cu[search_multi_kernel_index(16)], j.budget_bytes);
    const Ranks r = ranks_of(j);
    for (size_t g = 0; g < y.group.size(); ++g)
        for (int k = 0; k < kQueryClasses; ++k) {
            const QueryClass& c = y.group[g].cls[k];
            cut_rank_launches(m.launch, m.bnd_need, y.table, r, (int)g, class_columns(k), k, j.per_cu[k], false, c.q0, c.q0 + c.nq);
        }
    take_layout(m, y);
    return m;
}

// A pair list against a prepared database.  O(nqueries): nothing here looks at a pair or a target, and the chunks are arithmetic.  One
// score launch per class present in a group; its boundary columns are sized by the whole class.
SearchPairsPlan plan_search_pairs(const SearchPairsJob& j) {
    SearchPairsPlan s;
    QueryLayout y = layout_queries(j.qlens, j.nqueries, j.per_cu[search_pairs_kernel_index(16)], j.budget_bytes);
    s.table = std::move(y.table);
    s.prof_need = y.prof_need;
    s.entry_of.resize((size_t)j.nqueries);
    for (int64_t t = 0; t < j.nqueries; ++t) s.entry_of[(size_t)s.table[(size_t)t].row] = (int32_t)t;
    s.chunk = std::clamp<int64_t>(j.chunk, 1, kSearchPairsChunkMax);
    const int64_t npairs = std::max<int64_t>(0, j.npairs), most = std::min(npairs, s.chunk);   // pairs of the largest chunk
    s.nchunks = (npairs + s.chunk - 1) / s.chunk;
    s.items_need = (size_t)(24 * most);
    for (size_t g = 0; g < y.group.size(); ++g) {
        PairsGroup grp;
        grp.q0 = y.group[g].q0; grp.nq = y.group[g].nq; grp.prof_bytes = y.group[g].prof_bytes;
        for (int k = 0; k < kQueryClasses; ++k) grp.cls_q0[k] = y.group[g].cls[k].q0;
        grp.cls_q0[kQueryClasses] = grp.q0 + grp.nq;
        s.group.push_back(grp);
        for (int k = 0; k < kQueryClasses; ++k) {
            const QueryClass& c = y.group[g].cls[k];
            if (c.nq == 0) continue;
            PairsLaunch l;
            l.group = (int)g; l.C = class_columns(k); l.kernel = k;
            l.q0 = c.q0; l.nq = c.nq;
            l.bnd_per = 2 * boundary_ints(c.nstrips, j.longest);
            l.max_grid = grid_cap(j.per_cu[k], j.num_cus, l.bnd_per);
            s.bnd_need = std::max(s.bnd_need, (size_t)(search_pairs_grid(l, most) * 4 * l.bnd_per));
            s.launch.push_back(l);
        }
    }
    s.launches = (int64_t)s.group.size() + s.nchunks * (2 * (int64_t)s.group.size() + (int64_t)s.launch.size());
    return s;
}

// The ungapped pre-filter: per (group, class) the packed queries move to the front and either part gets its rank launches.  The classes
// take 16 columns per lane where both kernels of that width keep two workgroups on a CU.
PrefilterPlan plan_prefilter(const PrefilterJob& j) {
    PrefilterPlan f;
    QueryLayout y = layout_queries(j.qlens, j.nqueries, std::min(j.per_cu[prefilter_kernel_index(16, false)], j.per_cu[prefilter_kernel_index(16, true)]),
                                   j.budget_bytes);
    const Ranks r = ranks_of(j);
    auto packed = [&](const swk::MultiQuery& d) { return prefilter_packed(j.max_entry, d.qlen, j.longest, j.lanes); };
    for (size_t g = 0; g < y.group.size(); ++g)
        for (int k = 0; k < kQueryClasses; ++k) {
            const QueryClass& c = y.group[g].cls[k];
            const int C = class_columns(k), pk = prefilter_kernel_index(C, true), w32 = prefilter_kernel_index(C, false);
            const int64_t mid = packed_first(y.table, c.q0, c.q0 + c.nq, packed);
            f.packed_launches += cut_rank_launches(f.launch, f.bnd_need, y.table, r, (int)g, C, pk, j.per_cu[pk], true, c.q0, mid);
            cut_rank_launches(f.launch, f.bnd_need, y.table, r, (int)g, C, w32, j.per_cu[w32], false, mid, c.q0 + c.nq);
        }
    take_layout(f, y);
    return f;
}

// The many-query search with a choice of lanes: plan_prefilter's shape with search_multi_packed's rule.  The classes come from the
// 32-bit kernels' occupancy, so they do not depend on the lanes; with no packed query every class is one part and the launches are
// plan_search_multi's.
SearchMultiLanesPlan plan_search_multi_lanes(const SearchMultiLanesJob& j) {
    SearchMultiLanesPlan f;
    QueryLayout y = layout_queries(j.qlens, j.nqueries, j.per_cu[search_multi_kernel_index(16)], j.budget_bytes);
    const Ranks r = ranks_of(j);
    for (size_t g = 0; g < y.group.size(); ++g)
        for (int k = 0; k < kQueryClasses; ++k) {
            const QueryClass& c = y.group[g].cls[k];
            const bool fits = packed_kernel_fits(j.packed_per_cu, k);
            auto packed = [&](const swk::MultiQuery& d) { return fits && search_multi_packed(j.max_entry, d.qlen, j.longest, j.gap_open, j.gap_extend, j.lanes); };
            const int64_t mid = packed_first(y.table, c.q0, c.q0 + c.nq, packed);
            f.packed_launches += cut_rank_launches(f.launch, f.bnd_need, y.table, r, (int)g, class_columns(k), k, j.packed_per_cu[k], true, c.q0, mid);
            cut_rank_launches(f.launch, f.bnd_need, y.table, r, (int)g, class_columns(k), k, j.per_cu[k], false, mid, c.q0 + c.nq);
        }
    take_layout(f, y);
    return f;
}

// The pair list with a choice of lanes.  Everything but the order inside a class and the launches is plan_search_pairs's own answer: per
// (group, class) the packed queries move to the front, every entry keeping its profile's place, and a class with both kinds gets two
// score launches.  With no packed query nothing moves and nothing is added.  O(nqueries), as there.
SearchPairsLanesPlan plan_search_pairs_lanes(const SearchPairsLanesJob& j) {
    SearchPairsLanesPlan f;
    SearchPairsPlan s = plan_search_pairs(j);
    f.table = std::move(s.table);
    f.chunk = s.chunk; f.nchunks = s.nchunks;
    f.prof_need = s.prof_need; f.bnd_need = s.bnd_need; f.items_need = s.items_need;
    const int64_t most = std::min(std::max<int64_t>(0, j.npairs), f.chunk);   // pairs of the largest chunk
    int64_t binning = 0;                     // binning launches of one chunk
    size_t li = 0;
    for (size_t g = 0; g < s.group.size(); ++g) {
        PairsLanesGroup grp;
        static_cast<PairsGroup&>(grp) = s.group[g];
        int64_t npacked = 0;
        for (int k = 0; k < kSearchPairsKernels; ++k) {
            const bool fits = packed_kernel_fits(j.packed_per_cu, k);
            auto packed = [&](const swk::MultiQuery& d) { return fits && search_multi_packed(j.max_entry, d.qlen, j.longest, j.gap_open, j.gap_extend, j.lanes); };
            grp.pk_q1[k] = packed_first(f.table, grp.cls_q0[k], grp.cls_q0[k + 1], packed);
            npacked += grp.pk_q1[k] - grp.cls_q0[k];
        }
        grp.cells = kSearchPairsBuckets * npacked;
        binning += npacked ? 3 : 2;
        if (npacked) {
            f.items_need = std::max(f.items_need, (size_t)search_pairs_lanes_item_bytes(most, grp.cells));
            f.cells_need = std::max(f.cells_need, (size_t)(kSearchPairsCellsHead + 12 * grp.cells));
        }
        for (; li < s.launch.size() && s.launch[li].group == (int)g; ++li) {
            const int k = s.launch[li].kernel;
            for (int side = 0; side < 2; ++side) {
                const bool pk = side == 0;
                PairsLanesLaunch l;
                static_cast<PairsLaunch&>(l) = s.launch[li];
                l.packed = pk;
                l.q0 = pk ? grp.cls_q0[k] : grp.pk_q1[k];
                l.nq = (pk ? grp.pk_q1[k] : grp.cls_q0[k + 1]) - l.q0;
                if (l.nq == 0) continue;
                if (pk) {   // the waves the packed kernel keeps resident, under the class's boundary column
                    l.max_grid = grid_cap(j.packed_per_cu[k], j.num_cus, l.bnd_per);
                    f.bnd_need = std::max(f.bnd_need, (size_t)(search_pairs_lanes_grid(l, most, grp.cells) * 4 * l.bnd_per));
                    ++f.packed_launches;
                }
                f.launch.push_back(l);
            }
        }
        f.group.push_back(grp);
    }
    f.entry_of.resize((size_t)j.nqueries);
    for (int64_t t = 0; t < j.nqueries; ++t) f.entry_of[(size_t)f.table[(size_t)t].row] = (int32_t)t;
    f.packed_launches *= f.nchunks;
    f.launches = (int64_t)f.group.size() + f.nchunks * (binning + (int64_t)f.launch.size());
    return f;
}

// The best `top` of every row.  Every row has the same length, so the chunks are uniform and the geometry of a row is decided once.
// The passes take kTopDigitBits bits each from the top of the key down; the last one takes what is left.
SearchTopPlan plan_search_top(const SearchTopJob& j) {
    SearchTopPlan t;
    const int64_t nt = std::max<int64_t>(0, j.ntargets);
    while (t.tbits < 62 && (1ll << t.tbits) < nt) ++t.tbits;
    t.nbits = 24 + t.tbits;
    t.kernel = nt > kTopMax ? 1 : 0;
    const int64_t row_bytes = nt * 24;
    int64_t per = nt > 0 ? j.budget_bytes / row_bytes : kTopChunkQueries;
    per = std::clamp<int64_t>(per, 1, kTopChunkQueries);
    for (int64_t q = 0; q < j.nqueries; q += per) t.chunk.push_back(TopChunk{q, std::min(per, j.nqueries - q)});
    t.chunk_queries = std::min(per, std::max<int64_t>(0, j.nqueries));
    t.results_need = (size_t)(t.chunk_queries * nt);
    if (t.kernel == 0 || t.chunk_queries == 0) return t;
    for (int hi = t.nbits; hi > 0 && t.npasses < kTopMaxPasses; ++t.npasses) {
        const int bits = std::min(hi, kTopDigitBits);
        t.pass[t.npasses] = TopPass{hi - bits, bits};
        hi -= bits;
    }
    // enough workgroups to fill the device with the largest chunk, none with less than kTopMinSlice targets; slices in whole 256s
    const int64_t want = ((int64_t)std::max(1, j.per_cu) * j.num_cus + t.chunk_queries - 1) / t.chunk_queries;
    const int64_t wgs = std::clamp<int64_t>(want, 1, (nt + kTopMinSlice - 1) / kTopMinSlice);
    t.slice = ((nt + wgs - 1) / wgs + 255) / 256 * 256;
    t.wgs_row = (nt + t.slice - 1) / t.slice;
    t.hist_need = (size_t)t.chunk_queries << kTopDigitBits;
    t.state_need = (size_t)t.chunk_queries;
    return t;
}

TopPairsPlan plan_top_pairs(const TopPairsJob& j) {
    TopPairsPlan t;
    if (j.npairs < 0 || j.npairs >= (1ll << 31)) { t.refused = "npairs is negative or not below 2^31"; return t; }
    if (j.nqueries < 0) { t.refused = "nqueries is negative"; return t; }
    if (j.ntargets < 0 || j.ntargets >= (1ll << 31)) { t.refused = "ntargets is negative or not below 2^31"; return t; }
    if (j.top < 1 || j.top > kTopMax) { t.refused = "top is out of range 1..SW_TOP_MAX"; return t; }
    while ((1ll << t.tbits) < j.ntargets) ++t.tbits;
    t.lds = j.nqueries <= kTopPairsLdsQueries;
    // enough workgroups to fill the device four times over, none with less than kTopPairsMinSlice entries; slices in whole 256s
    if (j.npairs > 0) {
        const int64_t wgs = std::clamp<int64_t>((j.npairs + kTopPairsMinSlice - 1) / kTopPairsMinSlice, 1, 4ll * std::max(1, j.num_cus));
        t.slice = ((j.npairs + wgs - 1) / wgs + 255) / 256 * 256;
        t.grid = (j.npairs + t.slice - 1) / t.slice;
    }
    while (t.T < j.top) t.T <<= 1;
    t.kernel = j.npairs > kTopMax ? 1 : 0;
    t.items = t.kernel ? std::max<int64_t>(kTopMax, 2 * t.T) : kTopMax;
    t.sort_kernel = top_pairs_kernel_index(t.items, t.kernel == 1);
    t.sort_grid = std::min(j.nqueries, kTopPairsSortGrid);
    t.launches = j.nqueries == 0 ? 0 : (j.npairs > 0 ? 4 : 1);   // an empty list: the sort alone writes the empty rows
    t.keys_need = t.pos_need = (size_t)j.npairs;
    t.seg_need = 2 * ((size_t)j.nqueries + 1);
    t.segment_bytes = 12 * j.npairs;
    return t;
}

// The direction fill carries the search kernel's state plus the packed bytes of a row; the thresholds of the search hold for the same
// reasons (plan_search_affine).  A slot is a whole direction matrix of the longest hit, so that any hit runs in any slot; the waves
// take hits from a counter, longest first, and a call with more hits than slots simply keeps its waves busy longer.

AlignCkptBand align_ckpt_band(int64_t len, int64_t qpad, int64_t forced_rows, int64_t budget_bytes) {
    AlignCkptBand best;
    for (int64_t B = forced_rows ? forced_rows : kAlignCkptFloorRows; B <= (forced_rows ? forced_rows : kAlignCkptMaxRows); B *= 2) {
        const int64_t bytes = align_ckpt_slot_bytes(len, qpad, B);
        if (best.rows == 0 || bytes <= best.slot_bytes) { best.rows = B; best.slot_bytes = bytes; }
    }
    while ((1ll << best.log_rows) < best.rows) ++best.log_rows;
    best.fits = best.slot_bytes <= budget_bytes && best.slot_bytes <= kAlignSlotLimit;
    return best;
}

// One query's hits.  ckpt: the slot is align_ckpt_band's and a boundary column is one band's (plan_align_ckpt).
static AlignCkptPlan plan_align_one(const AlignAffineJob& j, bool ckpt, int64_t band_rows) {
    using swk::SW_SEARCH_ROWS;
    AlignCkptPlan a;
    a.C = query_columns(j.qlen, j.per_cu[align_affine_kernel_index(16)]);
    a.kernel = align_affine_kernel_index(a.C);
    a.nstrips = (j.qlen + 64 * a.C - 1) / (64 * a.C);
    a.qpad = a.nstrips * 64 * a.C;
    const int64_t rows = std::max<int64_t>(1, j.maxhit);
    if (ckpt) {
        const AlignCkptBand band = align_ckpt_band(j.maxhit, a.qpad, band_rows, j.budget_bytes);
        a.band_rows = band.rows; a.log_band = band.log_rows;
        a.bnd_per = 2 * boundary_ints(a.nstrips, std::min(band.rows, rows));
        a.slot_bytes = band.slot_bytes;
        a.fits = band.fits;
    } else {
        a.bnd_per = 2 * boundary_ints(a.nstrips, j.maxhit);
        a.slot_bytes = rows * a.qpad;
        a.fits = a.slot_bytes <= j.budget_bytes && a.slot_bytes <= kAlignSlotLimit;
    }
    a.prof_need = (size_t)(SW_SEARCH_ROWS * a.qpad);
    a.prof_blocks = (int)std::min<int64_t>((SW_SEARCH_ROWS * a.qpad + 255) / 256, kProfileBlocks);
    if (!a.fits) return a;
    a.slots = slot_cap(j.nhits, j.per_cu[a.kernel], j.num_cus, j.budget_bytes, a.slot_bytes, a.bnd_per);
    a.grid = (a.slots + 3) / 4;
    a.bnd_need = (size_t)(a.slots * a.bnd_per);
    a.dir_need = (size_t)(a.slots * a.slot_bytes);
    return a;
}

AlignAffinePlan plan_align_affine(const AlignAffineJob& j) { return plan_align_one(j, false, 0); }
AlignCkptPlan plan_align_ckpt(const AlignCkptJob& j) { return plan_align_one(j, true, j.band_rows); }

// The hits of many queries from a device table.  Host work is O(nqueries): layout_queries with the entry bound as a second reason to
// close a group, and per group a constant number of tiers and launches.  Nothing here depends on which targets the table names; the
// counts of items are products of int64 counts, never sums over items.
// ckpt: the sizes are align_ckpt_slot_bytes at the class's band height instead of len x qpad (plan_align_hits_ckpt).
static AlignHitsPlan plan_align_hits_sized(const AlignHitsJob& j, bool ckpt, int64_t band_rows) {
    AlignHitsPlan a;
    const int64_t n = j.nqueries, top = std::max<int64_t>(1, j.top), rows = std::max<int64_t>(1, j.longest);
    const int per_cu16 = j.per_cu[align_hits_kernel_index(16)];
    for (int64_t q = 0; q < n; ++q) a.worst_qpad = std::max(a.worst_qpad, query_padded(j.qlens[q], per_cu16));
    if (ckpt) {   // (a slot grows with qpad at every band height: the widest query's smallest slot is the call's worst)
        const AlignCkptBand worst = align_ckpt_band(rows, a.worst_qpad, band_rows, j.budget_bytes);
        a.worst_bytes = worst.slot_bytes;
        a.fits = worst.fits;
    } else {
        a.worst_bytes = rows * a.worst_qpad;
        a.fits = a.worst_bytes <= j.budget_bytes && a.worst_bytes <= kAlignSlotLimit;
    }
    if (!a.fits) return a;
    QueryLayout y = layout_queries(j.qlens, n, per_cu16, j.profile_budget_bytes, std::max<int64_t>(1, std::max<int64_t>(1, j.max_items) / top));
    a.table = std::move(y.table);
    a.prof_need = y.prof_need;
    for (const QueryGroup& yg : y.group) {
        AlignHitsGroup grp;
        grp.q0 = yg.q0; grp.nq = yg.nq; grp.prof_bytes = yg.prof_bytes;
        a.items_need = std::max(a.items_need, (size_t)(grp.nq * top));
        // the tiers of every class and their launches, largest first
        for (int k = 0; k < kAlignHitsKernels; ++k) {
            AlignHitsClass& c = grp.cls[k];
            c.q0 = yg.cls[k].q0; c.nq = yg.cls[k].nq; c.qpad = yg.cls[k].qpad; c.nstrips = yg.cls[k].nstrips;
            c.item0 = (c.q0 - grp.q0) * top; c.entries = c.nq * top;
            if (c.nq == 0) continue;
            const int C = class_columns(k);
            int64_t down[kAlignHitsTiers];
            const AlignCkptBand band = ckpt ? align_ckpt_band(rows, c.qpad, band_rows, j.budget_bytes) : AlignCkptBand{};
            c.log_band = band.log_rows;
            down[0] = ckpt ? band.slot_bytes : rows * c.qpad;
            for (c.ntiers = 1; c.ntiers < kAlignHitsTiers && down[c.ntiers - 1] / kAlignHitsTierRatio >= kAlignHitsTierFloor; ++c.ntiers)
                down[c.ntiers] = down[c.ntiers - 1] / kAlignHitsTierRatio;
            for (int t = 0; t < c.ntiers; ++t) c.bound[t] = down[c.ntiers - 1 - t];
            for (int t = c.ntiers - 1; t >= 0; --t) {
                AlignHitsLaunch l;
                l.group = (int)a.group.size(); l.C = C; l.kernel = k; l.tier = t;
                l.slot_bytes = c.bound[t];
                l.log_band = c.log_band;
                // a query of several strips is at least two strips wide: that bounds the rows of a tier's items that cross a boundary
                // (ckpt: a boundary column is one band's)
                l.bnd_per = 2 * boundary_ints(c.nstrips, ckpt ? std::min(rows, band.rows) : std::min(rows, c.bound[t] / (2 * 64 * C)));
                l.slots = slot_cap(c.entries, j.per_cu[k], j.num_cus, j.budget_bytes, l.slot_bytes, l.bnd_per);
                l.grid = (l.slots + 3) / 4;
                a.bnd_need = std::max(a.bnd_need, (size_t)(l.slots * l.bnd_per));
                a.dir_need = std::max(a.dir_need, (size_t)(l.slots * l.slot_bytes));
                a.slots += l.slots;
                a.launch.push_back(l);
            }
        }
        a.group.push_back(grp);
    }
    a.tiers = (int64_t)a.launch.size();
    return a;
}

AlignHitsPlan plan_align_hits(const AlignHitsJob& j) { return plan_align_hits_sized(j, false, 0); }
AlignHitsPlan plan_align_hits_ckpt(const AlignHitsCkptJob& j) { return plan_align_hits_sized(j, true, j.band_rows); }

PssmHitsPlan plan_pssm_hits(const PssmHitsJob& j) {
    PssmHitsPlan p;
    const int nl = std::clamp(j.nletters, 1, 256);
    p.stride = (nl + 1) | 1;
    p.max_cols = (kPssmHitsLdsBytes - kPssmHitsCodeBytes) / (4 * (int64_t)p.stride);
    int64_t total = 0, maxq = 0;
    for (int64_t q = 0; q < j.nqueries; ++q) {
        total += j.qlens[q];
        maxq = std::max(maxq, j.qlens[q]);
    }
    const int64_t share = (total + 2 * std::max(1, j.num_cus) - 1) / (2 * std::max(1, j.num_cus));   // columns per workgroup at two per CU
    int64_t tile = std::max<int64_t>(64, (share + 63) / 64 * 64);
    tile = std::min(tile, std::max<int64_t>(1, maxq));
    p.tile_cols = (int)std::min(tile, p.max_cols);
    p.lds_bytes = (unsigned)(kPssmHitsCodeBytes + 4 * (int64_t)p.tile_cols * p.stride);
    if (j.nqueries < 1) return p;
    p.tiles_per_query = (maxq + p.tile_cols - 1) / p.tile_cols;
    // (nqueries x tiles stays far inside 63 bits: query lengths are at most 2^20 - 1)
    p.grid = std::min(j.nqueries * p.tiles_per_query, kPssmHitsGridMax);
    p.launches = 1;
    return p;
}

PssmWeightsPlan plan_pssm_weights(const PssmWeightsJob& j) {
    PssmWeightsPlan p;
    p.tiles = plan_pssm_hits(j.queries);
    if (j.queries.nqueries < 1) return p;
    p.finish_grid = std::min(j.queries.nqueries, kPssmHitsGridMax);
    // (nqueries x top x 8 stays inside 63 bits for every nqueries a caller's memory could hold offsets for)
    p.acc_entries = j.queries.nqueries * std::clamp<int64_t>(j.top, 1, 4096);
    p.acc_bytes = p.acc_entries * kPssmWeightsAccBytes;
    p.launches = p.tiles.launches + 1;
    return p;
}

MsaHitsPlan plan_msa_hits(const MsaHitsJob& j) {
    MsaHitsPlan p;
    if (j.nqueries < 1) return p;
    const int64_t top = std::clamp<int64_t>(j.top, 1, 4096);
    // (nqueries x top stays inside 63 bits for every nqueries a caller's memory could hold offsets for)
    p.entries = j.nqueries * top;
    const int64_t wgs = kMsaHitsWgsPerCu * std::max(1, j.num_cus);
    const int64_t share = (p.entries + wgs - 1) / wgs;               // entries per workgroup at kMsaHitsWgsPerCu per CU
    p.slice_entries = std::min((share + 3) / 4 * 4, (top + 3) / 4 * 4);
    p.slices_per_query = (top + p.slice_entries - 1) / p.slice_entries;
    p.cols_grid = std::min(j.nqueries * p.slices_per_query, kPssmHitsGridMax);
    p.launches = 1;
    if (!j.rows) return p;
    p.scan_chunks = (p.entries + kMsaScanChunk - 1) / kMsaScanChunk;
    p.scan_grid = std::min(p.scan_chunks, kPssmHitsGridMax);
    p.top_rounds = (p.scan_chunks + kMsaScanChunk - 1) / kMsaScanChunk;
    p.scan_levels = p.scan_chunks > 1 ? 2 : 1;
    p.rows_grid = std::min((p.entries + 3) / 4, kPssmHitsGridMax);
    p.sums_bytes = 8 * p.scan_chunks;
    p.launches = 4;
    return p;
}

MsaFilterPlan plan_msa_filter(const MsaFilterJob& j) {
    MsaFilterPlan p;
    const int64_t top = std::clamp<int64_t>(j.top, 1, 4096);
    p.blocks = (top + kMsaFilterTile - 1) / kMsaFilterTile;
    p.tiles_per_query = p.blocks * (p.blocks + 1) / 2;
    p.chunk_cols = (int)kMsaFilterChunkCols;
    p.query_words = msa_filter_query_words(top);
    p.query_bytes = 8 * p.query_words;
    if (j.nqueries < 1) return p;
    p.queries_per_chunk = std::clamp<int64_t>(j.budget_bytes / p.query_bytes, 1, j.nqueries);
    p.chunks = (j.nqueries + p.queries_per_chunk - 1) / p.queries_per_chunk;
    p.workspace_bytes = p.queries_per_chunk * p.query_bytes;
    // (queries x tiles stays inside 63 bits: at most 2080 tiles)
    p.pair_grid = std::min(p.queries_per_chunk * p.tiles_per_query, kPssmHitsGridMax);
    p.greedy_grid = std::min(p.queries_per_chunk, kPssmHitsGridMax);
    p.last_queries = j.nqueries - (p.chunks - 1) * p.queries_per_chunk;
    p.last_pair_grid = std::min(p.last_queries * p.tiles_per_query, kPssmHitsGridMax);
    p.last_greedy_grid = std::min(p.last_queries, kPssmHitsGridMax);
    p.launches = (int)std::min<int64_t>(2 * p.chunks, INT32_MAX);
    return p;
}

ScoreHistPlan plan_score_hist(const ScoreHistJob& j) {
    ScoreHistPlan p;
    // one copy by default: the adds of a wave into one address are serialised inside its own instruction whichever copy they go to, and
    // one copy leaves room for four workgroups per CU (DESIGN 9y has the measurement)
    p.copies = j.copies == 2 || j.copies == 4 ? j.copies : 1;
    p.lds_bytes = p.copies * kScoreHistCells * 4;
    if (j.nqueries < 1 || j.ntargets < 1) return p;
    const int64_t want = std::max<int64_t>(1, (int64_t)std::max(j.num_cus, 1) * kScoreHistWgsPerCu / j.nqueries);
    const int64_t most = std::max<int64_t>(1, j.ntargets / kScoreHistMinSlice);
    p.slices_per_query = std::min({want, most, kScoreHistMaxSlices});
    p.slice = (j.ntargets + p.slices_per_query - 1) / p.slices_per_query;
    p.slices_per_query = (j.ntargets + p.slice - 1) / p.slice;   // (no empty slice)
    p.items = j.nqueries * p.slices_per_query;
    p.grid = std::min(p.items, kPssmHitsGridMax);
    p.launches = 1;
    return p;
}

HitsThresholdPlan plan_hits_threshold(int64_t nqueries) {
    HitsThresholdPlan p;
    if (nqueries < 1) return p;
    p.grid = std::min(nqueries, kPssmHitsGridMax);
    p.launches = 1;
    return p;
}

MaskPlan plan_mask(const MaskJob& j) {
    MaskPlan p;
    p.halo = std::clamp(j.window, 2, 64) - 1;
    if (j.count && j.ntargets >= 1) {        // (without letters the count launch still writes its zeroes)
        p.count_grid = std::min((j.ntargets + kMaskCountTargets - 1) / kMaskCountTargets, kPssmHitsGridMax);
        p.launches = 1;
    }
    if (j.letters < 1) return p;
    p.tiles = (j.letters + kMaskTile - 1) / kMaskTile;
    p.words = p.tiles * kMaskTileWords;
    p.low1_off = 0; p.low2_off = 8 * p.words; p.mask_off = 16 * p.words;
    p.summary_off = 24 * p.words; p.carry_off = p.summary_off + 4 * p.tiles;
    p.workspace_bytes = p.carry_off + 4 * p.tiles;
    p.window_grid = p.apply_grid = std::min(p.tiles, kPssmHitsGridMax);
    p.carry_grid = 1;
    p.launches += 3;
    return p;
}

void align_schedule(const int64_t* offsets, const int64_t* hits, int64_t nhits, swk::SearchItem* items) {
    std::vector<int64_t> order((size_t)nhits);
    for (int64_t h = 0; h < nhits; ++h) order[(size_t)h] = h;
    auto len = [&](int64_t h) { return offsets[hits[h] + 1] - offsets[hits[h]]; };
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return len(x) > len(y); });
    for (size_t i = 0; i < order.size(); ++i) items[i] = swk::SearchItem{offsets[hits[order[i]]], order[i], len(order[i])};
}

void search_schedule(const int64_t* offsets, int64_t ntargets, swk::SearchItem* items) {
    std::vector<int64_t> order;
    order.reserve((size_t)ntargets);
    for (int64_t k = 0; k < ntargets; ++k)
        if (offsets[k + 1] > offsets[k]) order.push_back(k);
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return offsets[x + 1] - offsets[x] > offsets[y + 1] - offsets[y]; });
    for (size_t i = 0; i < order.size(); ++i) {
        const int64_t k = order[i];
        items[i] = swk::SearchItem{offsets[k], k, offsets[k + 1] - offsets[k]};
    }
}

}  // namespace swp
