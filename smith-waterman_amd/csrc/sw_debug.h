// sw_debug.h -- the bits of option "debug_flags" (FillParams::debug_flags).  Development aids: A/B runs, timing experiments and
// tests of rare paths.  No HIP include: the fill planner (sw_plan.cpp) and the kernels share it.  The values are part of the
// interface (bench.py --debug-flags, the tests and scripts/ pass numbers): never renumber a bit.
#pragma once

namespace swk {

enum DebugFlag : int {
    DBG_NO_STORES = 1 << 0,            // drop the H / P stores (timing experiments; batch kernel too)
    DBG_PRODUCER_ONLY = 1 << 1,        // one-column kernel: consumers idle, the producer runs alone; no two-column kernel
    DBG_GENERIC_PRODUCER = 1 << 2,     // one-column kernel: generic producers, not the fast ones
    DBG_SKIP_STRIP1 = 1 << 3,          // one-column kernel: strip 1 never runs (tests the abort path); no two-column kernel
    DBG_NO_PERM = 1 << 4,              // no perm producer (and so no two-column kernel)
    DBG_NO_POLL_BACKOFF = 1 << 5,      // perm producer: poll without the back-off of 64
    DBG_WAVE_PLACEMENT = 1 << 6,       // one-column kernel: record where the hardware put the waves (debug_buf); no two-column kernel
    DBG_BLOCK_STAMPS = 1 << 7,         // one-column kernel: per-block completion stamps (debug_buf), no looped consumer; no two-column kernel
    DBG_NO_CONSUMER_LOOP = 1 << 8,     // one-column kernel: no looped consumer (the one-asm-statement form)
    DBG_EDGE_DUMP = 1 << 9,            // one-column kernel: dump exported edge values (debug_buf); no two-column kernel
    DBG_EPOCH8_WRAP_EARLY = 1 << 10,   // the 8-bit launch tag of the perm producer wraps after 3 launches (tests the wipe)
    DBG_POISON_HALO = 1 << 11,         // round-1 producers: poison the halo ring (a slot consumed before it was written shows)
    DBG_ONE_IMPORTER = 1 << 12,        // one-column kernel with a left halo: a single importer wave
    DBG_PROGRESS_FORM = 1 << 13,       // perm producer: the progress form everywhere
    DBG_NO_TWO_COLUMNS = 1 << 14,      // one column per lane: no two-column kernel
    DBG_FORCE_TWO_COLUMNS = 1 << 15,   // the two-column kernel wherever it is possible, whether or not it pays
    DBG_BATCH_SINGLE_PAIR = 1 << 16,   // batches on the single-pair machinery, not the one-pair-per-wave kernel
    DBG_NO_SCOUTS = 1 << 17,           // two-column kernel: no scout workgroups
    DBG_BATCH_NO_WAVE16 = 1 << 18,     // batch kernel: no two pairs per wave on 16-bit lanes
    DBG_NO_TILES = 1 << 19,            // two-column kernel: no column tiles
    DBG_NO_SPLIT = 1 << 20,            // two-column kernel: no split strips
    // Bit 21 means two different things to two different kernels: two names, one value.
    DBG_BATCH_NO_PACKED_P = 1 << 21,   // batch kernel: int8 P codes not from packed arithmetic
    DBG_S2_SCOUTS_NO_EXPORT = 1 << 21, // two-column kernel: scouts do not export their edge columns (timing experiments)
    DBG_S2_SYNTH_HALO = 1 << 22,       // two-column kernel: every importer invents its halo like strip 0 (timing experiments)
    DBG_NO_XCD_DEALING = 1 << 23,      // two-column kernel: roles not dealt per XCD (neither behind scouts nor in the chain)
    DBG_S2_IMPORTERS = 3 << 24,        // bits 24-25, a count: two-column kernel, that many importer waves on SIMD 2 only
    DBG_NO_PACING = 1 << 27,           // two-column kernel: fillers behind scouts unpaced (and so no split strips)
    DBG_S2_BARRIER_SCAN = 1 << 28,     // two-column kernel: the prologue's alphabet scan is shared and ends in a grid barrier, whatever the size
    DBG_S2_SCAN_ALL = 1 << 29,         // two-column kernel: every workgroup scans all letters itself (no grid barrier), whatever the size
};
constexpr int DBG_S2_IMPORTERS_SHIFT = 24;
constexpr int DBG_BATCH_MASK = DBG_NO_STORES | DBG_PRODUCER_ONLY | DBG_GENERIC_PRODUCER;   // handed on to BatchParams::debug (its kernels read bit 0)

}  // namespace swk
