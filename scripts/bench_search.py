#!/usr/bin/env python3
"""Database search throughput (sw_search_device) on one GPU; prints ONE JSON line.
  (a) query 512, protein alphabet, 200 000 targets, lengths log-normal (median 300, cut at 35 000)
  (b) the same total cells as equal-length targets
  (c) 4-letter equal-length 1024^2 database, search against sw_batch_device (score-only) on the same data
  (d) the (b) data through sw_batch_device, which takes the single-pair path for more than 8 letters
  (a) and (b) also through sw_search_affine_device (random symmetric 24-letter matrix, gap_open -11, gap_extend -1): *_affine_* beside
  the linear figures of the same database in the same process, and their ratio
  (a) then aligns the top 100 and the top 1000 hits of the affine search (sw_align_affine_device): a_align<K>_ms per call, the
  re-filled cells per second, the walk's share of the waves' time (the kernel's own tick stamps, option "debug_buf") beside the
  affine search call's time; --only-a stops after (a)
  --multi: data set (a) only, through a prepared database (sw_db_create / sw_db_search_affine): 1, 8 and 64 queries of --qlen in ONE call
  beside the same number of sw_search_affine_device calls in the same process (multi<N>_ms / single<N>_ms, and both per query), 64
  queries of log-normal length (median 300) likewise, and 64 queries of 32 letters against the first 2000 targets -- the case where a
  launch per query leaves most of the device idle
  --top: data set (a) only, 64 queries of --qlen, the best 100 targets of each onto the host by two paths in the same process, wall
  clock, medians and ranges of --reps after --warmup: (1) sw_db_search_affine into the full table, synchronize, the table to the host,
  top_hits of every row; (2) sw_db_search_affine_top until the hits are on the host, at the default "search_results_mib" and at 64 (five
  chunks).  The hits are compared one by one; the device memory of the results is computed from the sizes, not measured
  --align-hits: data set (a) only, 64 queries of --qlen, the alignments of their best 10 and best 100 targets onto the host by two paths in the
  same process, wall clock, medians and ranges of --reps after --warmup, from the device hit table of sw_db_search_affine_top: (1) the
  hits to the host, then one sw_align_affine_device call per query; (2) one sw_db_align_affine_hits call on the device table.  Both
  write one output buffer and copy the coordinates and the ops up to the longest alignment to the host in two copies; the alignments are compared entry by entry; the search call's time in
  the same process stands beside them
  --align-hits --checkpoint: data set (a) only, checkpointed alignment (option "align_checkpoint" = 1, the planner's band height) beside
  the whole-matrix path (0) in the same process, torch events, medians and ranges of --reps after --warmup: the sw_db_align_affine_hits
  call on the top 10 / top 100 hits of 64 queries of --qlen, and the sw_align_affine_device call on the top 100 / 1000 hits of one
  query with the waves' tick stamps (mode 0: fill, walk; mode 1: sweep, walk, re-fill).  The outputs of the two modes are compared on
  the device before anything is timed
  --pairs: data set (a) only, 64 queries of --qlen through one handle, three legs in one process, torch events around the whole call,
  medians and ranges of --reps after --warmup: (i) sw_db_search_affine over the full cross product, the baseline; (ii)
  sw_db_search_affine_pairs over a uniform random 1 % of the cross product (fixed seed); (iii) sw_db_search_affine_pairs over the full
  cross product as an explicit list in random order.  The results of (ii) and (iii) are compared on the device with the table of (i)
  --prefilter: data set (a) only, 64 queries of --qlen through one handle, three legs in one process, torch events around whole calls,
  medians and ranges of --reps after --warmup: (i) sw_db_search_affine over the full cross product, the baseline; (ii)
  sw_db_prefilter_ungapped alone, on 32-bit lanes ("prefilter_lanes" = 32) and packed (0), at the ungapped score about 1 % of the pairs
  reach (the quantile of a d_scores run, printed); (iii) the filter and sw_db_search_affine_pairs over its whole list, no count read in
  between.  Checked on the device: every result of (iii) for a passing pair is the table entry of (i), U <= max_score for ALL pairs, the
  two kernels give the same scores; the run fails if a check fails or if (ii) is not faster than (i)
  --prefiltered-top: the data set and the threshold rule of --prefilter, top = 10, six legs in one process on the same buffers, torch events
  around whole calls, medians and ranges of --reps after --warmup: (i) sw_db_search_affine_top, the baseline; (ii) sw_db_prefilter_ungapped,
  sw_db_search_affine_pairs and sw_top_hits_pairs_device chained by hand; (iii) sw_db_search_affine_top_prefiltered, the one call; (iv)
  the selection alone over the list of (ii); (v) the dense sw_top_hits_device over the full table, for scale; (vi) (i) and (iii) each
  followed by sw_db_align_affine_hits.  The selection alone again over the list of a threshold that 10 % of the pairs reach: segments of
  about 20 000 entries, the streaming sort.  Checked on the device: the tables of (ii) and (iii) are equal, both equal the top 10 of
  the full table masked by U >= S (torch, from a d_scores run), the count is at most the cap; the run fails if a check fails or if
  (iii) is not faster than (i).  The recall -- the share of (i)'s hits that (iii) found -- is recorded, not gated
  --pssm: data set (a) only, 64 queries of --qlen through one handle: sw_db_search_pssm on the matrices sw_pssm_from_queries derives from
  the queries beside sw_db_search_affine on the queries, in one process, ALTERNATING, at least five repeats each, torch events around
  whole calls, medians and ranges; the results are compared on the device.  The margin is the range of the sw_db_search_affine repeats
  (pssm_within_margin is recorded, not gated).  *_profile_call_ms: the same two calls against a handle of ONE one-letter target -- the
  uploads, the profile launch of all 64 queries and a sweep of 64 cells: what the two calls do NOT share, measured without the sweeps
  --lanes: data set (a) only, 64 queries of --qlen through one handle and the same buffers in one process: sw_db_search_affine under
  "search_lanes" = 32 and = 16, ALTERNATING, and a second pair of legs for sw_db_search_affine_top with top 10, torch events around whole
  calls, medians and ranges of --reps after --warmup, the ratio 16 / 32 of either pair.  lanes_identical is a byte comparison of the full
  result tables and of the hit tables of the two modes at the timed size; the run fails if it is false
  --pairs-lanes: data set (a) only, 64 queries of --qlen through one handle and the same buffers in one process: sw_db_search_affine_pairs
  under "search_pairs_lanes" = 32 and = 16, ALTERNATING, at three list sizes -- every pair of the cross product in shuffled order (the
  list of --pairs), a random 10 % and a random 1 % (the list of --pairs) -- and then sw_db_search_affine_top_prefiltered (top 10, threshold
  60) under both; torch events around whole calls, medians and ranges of 7 calls after a warm-up, the ratio 16 / 32 of every pair of legs.
  pairs_lanes_identical is a byte comparison of the result arrays (and of the hit tables) of the two modes at the timed size; the run
  fails if it is false.  pairs_lanes_*_packed_items is "last_search_pairs_packed_items" of the call under 16
  --pssm-iterate: data set (a) only, 64 PSSM queries of --qlen (sw_pssm_from_queries) through one handle, top 10, 100 and 4096, 7 calls
  each after a warm-up, torch events (device legs) or wall clock around a synchronised leg (legs with host work), ALTERNATING in one
  process.  (a) pssm_from_hits_device alone against what a caller had to do without it: D2H of d_aln, d_ops and d_hits (and the counts),
  pssm_from_hits_host, H2D of the matrix -- the matrices compared byte for byte (the run fails if they differ).  (b) one whole iteration,
  align_pssm_hits_device + pssm_from_hits_device + search_pssm_top_device, against search_pssm_top_device alone.  ops_cap is 4 x qlen, not
  qlen + the longest target: an entry whose alignment is longer counts as unused on both sides alike (*_over_cap says how many there are)
  --pssm-weights: data set (a) only, the queries, tables and ops_cap of --pssm-iterate, top 10, 100 and 4096, 7 calls each after a warm-up,
  wall clock around a synchronised leg, ALTERNATING in one process.  (a) pssm_hit_weights_device alone against what a caller had to do
  without it: D2H of d_hits, d_nhits, d_aln and d_ops, pssm_hit_weights_host, H2D of the weights -- the weights compared byte for byte (the
  run fails if they differ).  (b) one weighted iteration, align_pssm_hits_device + pssm_hit_weights_device + pssm_from_hits_device (with the
  weights; prior_weight x per_hit) + search_pssm_top_device, against the unweighted one of --pssm-iterate; *_update_alone_ms is
  pssm_from_hits_device without weights, the kernel the expectation "about twice" refers to
  --msa: data set (a) only, 64 sequence queries of --qlen through one handle, top 10, 100 and 4096: search_affine_top_device and
  align_affine_hits_device fill the device tables once (ops_cap 4 x qlen, as for --pssm-iterate); then msa_from_hits_device alone -- the
  column rows, the row table and the A3M rows into buffers sized by one sizing call beforehand -- against what a caller had to do
  without it: D2H of d_hits, d_nhits, d_aln and d_ops, then msa_from_hits_host.  7 calls each after a warm-up, wall clock around a
  synchronised leg, ALTERNATING in one process; the three outputs compared byte for byte (the run fails if they differ).  *_bytes_written
  is what the device call stores (column rows + 24 bytes per entry + A3M rows), *_write_gbs that over the device call's time
  --msa-filter: data set (a) only, the 64 queries, tables and top 10 / 100 / 4096 of --pssm-weights plus the column rows of
  msa_from_hits_device; the filter is (max_ident_pct 90, min_cover_pct 0), hhfilter's defaults.  (a) msa_filter_device alone -- keep,
  the counts and the filtered hit table -- against what a caller has to do without it: D2H of the column rows and the hit table,
  msa_filter_host, H2D of the filtered table; the three outputs compared byte for byte (the run fails if they differ).  7 calls each
  after a warm-up, ALTERNATING; a leg whose warm-up call takes more than 20 s is timed by that call alone (*_calls says how many calls
  stand behind a median).  (b) a weighted iteration (--pssm-weights (b)) beside one with msa_from_hits_device (column rows) and
  msa_filter_device in front of the weights, which with the update then read the filtered table
  --mask: data set (a) only.  (1) mask_low_complexity_device (SEG's window and bounds over the 20 letters) with and without the counts,
  beside torch.clone and copy_ of the same bytes and beside the path a caller had before -- D2H, mask_low_complexity_host, H2D (3 calls);
  7 calls each, alternating, medians; the outputs compared byte for byte (the run fails if they differ).  (2) the iteration by E-value
  of --score-stats on the plain handle and on a handle over the masked copy
  --score-stats: data set (a) only, 64 queries, top 100.  (1) search_affine_top_stats_device beside search_affine_top_device, 7 calls
  each after a warm-up, wall clock around a synchronised call, ALTERNATING; hits, counts and -- against score_hist_device over the full
  table -- histograms compared byte for byte (the run fails if they differ).  (2) score_hist_device alone over the full 64 x 200 000
  table (torch events, median of 20) in GB/s of the table's 24 bytes per entry, beside torch.sum over the same tensor, for the
  search's own scores and for a table with every score in ONE cell, under "score_hist_copies" 1, 2 and 4.  (3) what a round of
  --include-evalue adds: D2H of the histograms, score_fit, score_thresholds, H2D of the thresholds, hits_threshold_device.  (4) an
  iteration (align, update, search) with the inclusion by E-value beside one by raw score, at an E-value no hit misses, so that both
  build the same matrix and the searches that follow cost the same.  (5) the path a caller had before: D2H of
  the full table and score_hist_host
GCUPS = query letters x target letters / time of the call (torch events, median of --reps after --warmup)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
swamd = importlib.import_module("smith-waterman_amd")
import torch  # noqa: E402

PROTEIN = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
DNA = np.frombuffer(b"ACGT", np.uint8)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=200_000)
    ap.add_argument("--qlen", type=int, default=512)
    ap.add_argument("--pairs-c", type=int, default=20_000)
    ap.add_argument("--pairs-d", type=int, default=4096, help="pairs of the (b) data sent through sw_batch_device (its slow path)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-a", action="store_true", help="data set (a) only: linear search, affine search, alignment of its top hits")
    ap.add_argument("--multi", action="store_true", help="data set (a) only: many queries through a prepared database against one call per query")
    ap.add_argument("--align-hits", action="store_true", help="data set (a) only: the alignments of the top 10 / 100 hits of 64 queries, per query and in one call")
    ap.add_argument("--checkpoint", action="store_true", help="with --align-hits: checkpointed alignment beside the whole-matrix path, hit table and one query")
    ap.add_argument("--pairs", action="store_true", help="data set (a) only: a pair list of 1 %% and of all of the cross product of 64 queries beside the full search")
    ap.add_argument("--prefilter", action="store_true", help="data set (a) only: the ungapped pre-filter of 64 queries, alone and chained into the pair-list search, beside the full search")
    ap.add_argument("--prefiltered-top", action="store_true", help="data set (a) only: the top 10 of 64 queries by the full search and by pre-filter, rescoring and selection from the pair list")
    ap.add_argument("--pssm", action="store_true", help="data set (a) only: 64 PSSM queries derived from 64 sequence queries beside those, alternating")
    ap.add_argument("--pssm-iterate", action="store_true", help="data set (a) only: the PSSM update on the device against the host round trip, and a whole iteration against the search alone")
    ap.add_argument("--pssm-weights", action="store_true", help="data set (a) only: the hit weights on the device against the host round trip, and a weighted iteration against the unweighted one")
    ap.add_argument("--msa", action="store_true", help="data set (a) only: the query-anchored alignment of the top 10 / 100 / 4096 hits of 64 queries on the device against the host round trip")
    ap.add_argument("--msa-filter", action="store_true", help="data set (a) only: the filter of the column rows of the top 10 / 100 / 4096 hits of 64 queries on the device against the host round trip, and a weighted iteration with and without it")
    ap.add_argument("--score-stats", action="store_true", help="data set (a) only: the score histogram inside the top search and alone, the fit's round trip, an iteration by E-value beside one by raw score")
    ap.add_argument("--mask", action="store_true", help="data set (a) only: the low-complexity mask on the device beside a plain device copy and the host round trip, and an iteration by E-value on the plain and on the masked handle")
    ap.add_argument("--lanes", action="store_true", help="data set (a) only: 64 queries under search_lanes 32 and 16, alternating, full tables and top 10")
    ap.add_argument("--pairs-lanes", action="store_true", help="data set (a) only: pair lists of all, 10 %% and 1 %% of the cross product under search_pairs_lanes 32 and 16, alternating")
    ap.add_argument("--top", action="store_true", help="data set (a) only: the best 100 targets of 64 queries by the full table and by the selection on the device")
    args = ap.parse_args()
    rng = np.random.default_rng(2026)
    eng = swamd.Engine(0)
    dev = "cuda:0"
    out = {"workload": "database search", "device": torch.cuda.get_device_name(0)}

    def search_gcups(query, packed, offs, tag):
        d_q = torch.from_numpy(query.copy()).to(dev)
        d_db = torch.from_numpy(packed.copy()).to(dev)
        res = torch.zeros((len(offs) - 1, 3), dtype=torch.int64, device=dev)
        ms = timed(lambda: eng.search_device(d_q, len(query), d_db, offs, out=res), args.warmup, args.reps)
        cells = float(len(query)) * float(offs[-1] - offs[0])
        out[f"{tag}_ms"] = round(ms, 3)
        out[f"{tag}_gcups"] = round(cells / ms / 1e6, 1)
        out[f"{tag}_grid"] = eng.get_option("last_search_grid")
        return res

    # a random symmetric table over 24 protein letters (the 20 of the data among them), matches 4..11, mismatches -4..2
    letters = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYBZX*", np.uint8)
    mrng = np.random.default_rng(24)   # (its own generator: the data sets stay those of the linear runs)
    tri = np.triu(mrng.integers(-4, 3, (24, 24)), 1)
    sub = swamd.submat_from_letters(letters, (tri + tri.T + np.diag(mrng.integers(4, 12, 24))).astype(np.int8), -4)

    def affine_gcups(query, packed, offs, tag):
        d_q = torch.from_numpy(query.copy()).to(dev)
        d_db = torch.from_numpy(packed.copy()).to(dev)
        res = torch.zeros((len(offs) - 1, 3), dtype=torch.int64, device=dev)
        ms = timed(lambda: eng.search_affine_device(d_q, len(query), d_db, offs, sub, -11, -1, out=res), args.warmup, args.reps)
        cells = float(len(query)) * float(offs[-1] - offs[0])
        out[f"{tag}_affine_ms"] = round(ms, 3)
        out[f"{tag}_affine_gcups"] = round(cells / ms / 1e6, 1)
        out[f"{tag}_affine_grid"] = eng.get_option("last_search_affine_grid")
        out[f"{tag}_affine_over_linear"] = round(out[f"{tag}_affine_gcups"] / out[f"{tag}_gcups"], 3)
        return res

    def align_legs(query, packed, offs, res, tag):
        d_q = torch.from_numpy(query.copy()).to(dev)
        d_db = torch.from_numpy(packed.copy()).to(dev)
        order = swamd.top_hits(res.cpu().numpy(), 1000)
        lens = np.diff(offs)
        for k in (100, 1000):
            hits = order[:k]
            cap = len(query) + int(lens[hits].max())
            bufs = (torch.zeros((k, 7), dtype=torch.int64, device=dev), torch.zeros((k, cap), dtype=torch.uint8, device=dev))
            ms = timed(lambda: eng.align_affine_device(d_q, len(query), d_db, offs, sub, -11, -1, hits, ops_cap=cap, out=bufs), args.warmup, args.reps)
            cells = float(len(query)) * float(lens[hits].sum())
            out[f"{tag}_align{k}_ms"] = round(ms, 3)
            out[f"{tag}_align{k}_gcups"] = round(cells / ms / 1e6, 2)
            out[f"{tag}_align{k}_cells"] = int(cells)
            out[f"{tag}_align{k}_slots"] = eng.get_option("last_align_affine_slots")
            out[f"{tag}_align{k}_ops_mean"] = round(float(bufs[0][:, 6].double().mean().item()), 1)
            # one more call with the kernel's tick stamps on: time in fills and in walks, summed over the waves
            stamps = torch.zeros(2, dtype=torch.int64, device=dev)
            eng.set_option("debug_buf", stamps.data_ptr())
            eng.align_affine_device(d_q, len(query), d_db, offs, sub, -11, -1, hits, ops_cap=cap, out=bufs)
            torch.cuda.synchronize()
            eng.set_option("debug_buf", 0)
            fill_t, walk_t = (float(x) for x in stamps.cpu().numpy())
            out[f"{tag}_align{k}_walk_share"] = round(walk_t / max(1.0, fill_t + walk_t), 4)
        out[f"{tag}_align100_over_affine_search_ms"] = round(out[f"{tag}_align100_ms"] / out[f"{tag}_affine_ms"], 4)

    def batch_gcups(query, b_all, tag, reps):
        npairs, n = b_all.shape
        d_a, d_b, cols, rows = eng.batch_to_device(np.broadcast_to(query, (npairs, len(query))), b_all)
        res = torch.zeros((npairs, 3), dtype=torch.int64, device=dev)
        ms = timed(lambda: eng.batch_device(d_a, d_b, cols, rows, out=(res, None, None)), min(args.warmup, 1), reps)
        out[f"{tag}_ms"] = round(ms, 3)
        out[f"{tag}_gcups"] = round(float(cols) * rows * npairs / ms / 1e6, 1)
        return res

    def multi_legs(packed, offs):
        import time
        d_db = torch.from_numpy(packed.copy()).to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        db = eng.prepare_db(d_db, offs)
        out["multi_prepare_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        small = eng.prepare_db(d_db, offs[:2001])
        qlog = np.clip(np.round(rng.lognormal(np.log(300), 0.6, 64)), 1, 35_000).astype(np.int64)
        for tag, qlens, handle, toffs in [("1", [args.qlen], db, offs), ("8", [args.qlen] * 8, db, offs), ("64", [args.qlen] * 64, db, offs),
                                          ("64_lognormal", list(qlog), db, offs), ("64_short_small_db", [32] * 64, small, offs[:2001])]:
            qoffs = np.zeros(len(qlens) + 1, np.int64)
            qoffs[1:] = np.cumsum(qlens)
            d_q = torch.from_numpy(rng.choice(PROTEIN, int(qoffs[-1])).astype(np.uint8)).to(dev)
            nt = len(toffs) - 1
            res = torch.zeros(len(qlens) * nt * 3, dtype=torch.int64, device=dev)
            ref = torch.zeros((len(qlens), nt, 3), dtype=torch.int64, device=dev)
            ms = timed(lambda: handle.search_affine_device(d_q, qoffs, (sub, -11, -1), out=res), args.warmup, args.reps)

            def one_by_one():
                for k in range(len(qlens)):
                    eng.search_affine_device(d_q[int(qoffs[k]):], int(qlens[k]), d_db, toffs, sub, -11, -1, out=ref[k])
            ms1 = timed(one_by_one, args.warmup, args.reps)
            cells = float(qoffs[-1]) * float(toffs[-1] - toffs[0])
            out[f"multi{tag}_ms"], out[f"single{tag}_ms"] = round(ms, 3), round(ms1, 3)
            out[f"multi{tag}_ms_per_query"], out[f"single{tag}_ms_per_query"] = round(ms / len(qlens), 3), round(ms1 / len(qlens), 3)
            out[f"multi{tag}_gcups"], out[f"single{tag}_gcups"] = round(cells / ms / 1e6, 1), round(cells / ms1 / 1e6, 1)
            out[f"multi{tag}_launches"] = eng.get_option("last_search_multi_launches")
            out[f"multi{tag}_identical"] = bool(torch.equal(res.view(len(qlens), nt, 3), ref))
        db.close()
        small.close()

    def top_leg(packed, offs, nq=64, top=100):
        import time
        d_db = torch.from_numpy(packed.copy()).to(dev)
        db = eng.prepare_db(d_db, offs)
        nt = len(offs) - 1
        qoffs = np.arange(nq + 1, dtype=np.int64) * args.qlen
        d_q = torch.from_numpy(rng.choice(PROTEIN, int(qoffs[-1])).astype(np.uint8)).to(dev)
        scoring = (sub, -11, -1)
        table = torch.zeros(nq * nt * 3, dtype=torch.int64, device=dev)
        bufs = (torch.zeros(nq * top * 3, dtype=torch.int64, device=dev), torch.zeros(nq, dtype=torch.int64, device=dev))

        def full_table():
            res = db.search_affine_device(d_q, qoffs, scoring, out=table)
            eng.synchronize()
            host = res.cpu().numpy()
            hits = np.zeros((nq, top, 3), np.int64)
            for k in range(nq):
                order = swamd.top_hits(host[k], top)
                hits[k, :, 0], hits[k, :, 1], hits[k, :, 2] = order, host[k, order, 0], host[k, order, 1]
            return hits

        def on_device():
            hits, nhits = db.search_affine_top_device(d_q, qoffs, scoring, top, out=bufs)
            eng.synchronize()
            return hits.cpu().numpy(), nhits.cpu().numpy()

        def wall(fn):
            for _ in range(args.warmup):
                last = fn()
            ms = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last = fn()
                ms.append((time.perf_counter() - t0) * 1e3)
            return last, round(float(np.median(ms)), 3), [round(min(ms), 3), round(max(ms), 3)]

        want, out["top_full_table_ms"], out["top_full_table_range_ms"] = wall(full_table)
        (got, nhits), out["top_on_device_ms"], out["top_on_device_range_ms"] = wall(on_device)
        out["top_chunks"] = eng.get_option("last_search_top_chunks")
        out["top_identical"] = bool(np.array_equal(got, want) and (nhits == top).all())
        eng.set_option("search_results_mib", 64)
        (got, nhits), out["top_on_device_64mib_ms"], out["top_on_device_64mib_range_ms"] = wall(on_device)
        out["top_64mib_chunks"] = eng.get_option("last_search_top_chunks")
        out["top_64mib_identical"] = bool(np.array_equal(got, want) and (nhits == top).all())
        eng.set_option("search_results_mib", 1024)
        out["top_ranges_overlap"] = bool(out["top_on_device_range_ms"][1] >= out["top_full_table_range_ms"][0])
        row = nt * 24
        out["top_queries"], out["top_k"], out["top_targets"] = nq, top, nt
        out["top_full_table_result_bytes_computed"] = nq * row
        out["top_on_device_result_bytes_computed"] = min(nq, max(1, (1024 << 20) // row)) * row + nq * (top * 24 + 8 + 8192 + 24)
        out["top_on_device_64mib_result_bytes_computed"] = min(nq, max(1, (64 << 20) // row)) * row + nq * (top * 24 + 8 + 8192 + 24)
        db.close()

    def align_hits_leg(packed, offs, nq=64):
        import time
        d_db = torch.from_numpy(packed.copy()).to(dev)
        db = eng.prepare_db(d_db, offs)
        lens = np.diff(offs)
        longest = int(lens.max())
        qoffs = np.arange(nq + 1, dtype=np.int64) * args.qlen
        d_q = torch.from_numpy(rng.choice(PROTEIN, int(qoffs[-1])).astype(np.uint8)).to(dev)
        scoring = (sub, -11, -1)

        def wall(fn):
            for _ in range(args.warmup):
                last = fn()
            ms = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last = fn()
                ms.append((time.perf_counter() - t0) * 1e3)
            return last, round(float(np.median(ms)), 3), [round(min(ms), 3), round(max(ms), 3)]

        def to_host(aln, ops):
            a = aln.cpu().numpy()
            return a, ops[..., :max(1, int(a[..., 6].max()))].cpu().numpy()

        out["align_hits_queries"], out["align_hits_qlen"] = nq, args.qlen
        for top in (10, 100):
            tag = f"align_hits_top{top}"
            tbufs = (torch.zeros(nq * top * 3, dtype=torch.int64, device=dev), torch.zeros(nq, dtype=torch.int64, device=dev))

            def search():
                r = db.search_affine_top_device(d_q, qoffs, scoring, top, out=tbufs)
                eng.synchronize()
                return r
            (d_hits, d_nhits), out[f"{tag}_search_ms"], out[f"{tag}_search_range_ms"] = wall(search)
            cap = args.qlen + longest
            # both paths write one (aln, ops) buffer of their own and copy it to the host the same way: two copies per run
            one = (torch.zeros((nq * top, 7), dtype=torch.int64, device=dev), torch.zeros((nq * top, cap), dtype=torch.uint8, device=dev))
            per = (torch.zeros((nq * top, 7), dtype=torch.int64, device=dev), torch.zeros((nq * top, cap), dtype=torch.uint8, device=dev))
            views = [(per[0][k * top:(k + 1) * top], per[1][k * top:(k + 1) * top]) for k in range(nq)]

            def per_query():
                hits = d_hits.cpu().numpy()                                  # (the device table to the host: path (1) needs the indices there)
                for k in range(nq):
                    eng.align_affine_device(d_q[int(qoffs[k]):], args.qlen, d_db, offs, sub, -11, -1, hits[k, :, 0], ops_cap=cap, out=views[k])
                eng.synchronize()
                return to_host(per[0].view(nq, top, 7), per[1].view(nq, top, cap))

            def one_call():
                aln, ops = db.align_affine_hits_device(d_q, qoffs, scoring, d_hits, d_nhits, ops_cap=cap, out=one)
                eng.synchronize()
                return to_host(aln, ops)

            want, out[f"{tag}_per_query_ms"], out[f"{tag}_per_query_range_ms"] = wall(per_query)
            (aln, ops), out[f"{tag}_one_call_ms"], out[f"{tag}_one_call_range_ms"] = wall(one_call)
            out[f"{tag}_launches"], out[f"{tag}_tiers"] = eng.get_option("last_align_hits_launches"), eng.get_option("last_align_hits_tiers")
            out[f"{tag}_slots"], out[f"{tag}_lists_filled"] = eng.get_option("last_align_hits_slots"), eng.get_option("last_align_hits_lists")
            wa, wo = want
            same = bool((d_nhits.cpu().numpy() == top).all()) and np.array_equal(wa, aln)
            same = same and all(wo[k, r, :wa[k, r, 6]].tobytes() == ops[k, r, :wa[k, r, 6]].tobytes() for k in range(nq) for r in range(top))
            out[f"{tag}_identical"] = same
            out[f"{tag}_ops_mean"] = round(float(aln[..., 6].mean()), 1)
            out[f"{tag}_hit_len_mean"] = round(float(lens[d_hits.cpu().numpy()[..., 0]].mean()), 1)
            out[f"{tag}_ranges_overlap"] = bool(out[f"{tag}_one_call_range_ms"][1] >= out[f"{tag}_per_query_range_ms"][0])
            out[f"{tag}_per_query_over_one_call"] = round(out[f"{tag}_per_query_ms"] / out[f"{tag}_one_call_ms"], 2)
            out[f"{tag}_one_call_over_search"] = round(out[f"{tag}_one_call_ms"] / out[f"{tag}_search_ms"], 4)
        db.close()

    def spread(fn):
        """Median and range of --reps calls after --warmup, torch events."""
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return round(float(np.median(ms)), 3), [round(min(ms), 3), round(max(ms), 3)]

    def pairs_leg(packed, offs, nq=64):
        d_db = torch.from_numpy(packed.copy()).to(dev)
        db = eng.prepare_db(d_db, offs)
        nt = len(offs) - 1
        lens = np.diff(offs)
        qoffs = np.arange(nq + 1, dtype=np.int64) * args.qlen
        d_q = torch.from_numpy(rng.choice(PROTEIN, int(qoffs[-1])).astype(np.uint8)).to(dev)
        scoring = (sub, -11, -1)
        prng = np.random.default_rng(7)                                      # (its own generator: the lists do not depend on the other legs)
        flat_sparse = prng.choice(nq * nt, nq * nt // 100, replace=False).astype(np.int64)
        flat_full = prng.permutation(nq * nt).astype(np.int64)
        table = torch.zeros(nq * nt * 3, dtype=torch.int64, device=dev)
        out["pairs_queries"], out["pairs_qlen"], out["pairs_targets"] = nq, args.qlen, nt
        out["pairs_full_ms"], out["pairs_full_range_ms"] = spread(lambda: db.search_affine_device(d_q, qoffs, scoring, out=table))
        cells_full = float(qoffs[-1]) * float(offs[-1] - offs[0])
        out["pairs_full_cells"] = int(cells_full)
        out["pairs_full_ps_per_cell"] = round(out["pairs_full_ms"] * 1e9 / cells_full, 4)
        rows = table.view(nq * nt, 3)
        for tag, flat in (("sparse", flat_sparse), ("list", flat_full)):
            pairs = np.stack([flat // nt, flat % nt], axis=1)
            d_pairs = torch.from_numpy(pairs).to(dev)
            d_flat = torch.from_numpy(flat).to(dev)
            res = torch.full((len(flat) * 3,), -1, dtype=torch.int64, device=dev)
            ms, rng_ms = spread(lambda: db.search_affine_pairs_device(d_q, qoffs, scoring, d_pairs, out=res))
            cells = float(args.qlen) * float(lens[pairs[:, 1]].sum())
            out[f"pairs_{tag}_n"], out[f"pairs_{tag}_list_bytes"], out[f"pairs_{tag}_result_bytes"] = len(flat), len(flat) * 16, len(flat) * 24
            out[f"pairs_{tag}_ms"], out[f"pairs_{tag}_range_ms"] = ms, rng_ms
            out[f"pairs_{tag}_cells"] = int(cells)
            out[f"pairs_{tag}_ps_per_cell"] = round(ms * 1e9 / cells, 4)
            out[f"pairs_{tag}_gcups"] = round(cells / ms / 1e6, 1)
            out[f"pairs_{tag}_chunks"], out[f"pairs_{tag}_launches"] = eng.get_option("last_search_pairs_chunks"), eng.get_option("last_search_pairs_launches")
            out[f"pairs_{tag}_identical"] = bool(torch.equal(res.view(len(flat), 3), rows[d_flat]))
            del d_pairs, d_flat, res
        out["pairs_sparse_faster_than_full"] = bool(out["pairs_sparse_ms"] < out["pairs_full_ms"])
        out["pairs_sparse_over_full_ms"] = round(out["pairs_sparse_ms"] / out["pairs_full_ms"], 4)
        out["pairs_list_over_full_per_cell"] = round(out["pairs_list_ps_per_cell"] / out["pairs_full_ps_per_cell"], 4)
        db.close()

    def prefilter_leg(packed, offs, nq=64):
        d_db = torch.from_numpy(packed.copy()).to(dev)
        db = eng.prepare_db(d_db, offs)
        nt = len(offs) - 1
        lens = np.diff(offs)
        qoffs = np.arange(nq + 1, dtype=np.int64) * args.qlen
        d_q = torch.from_numpy(rng.choice(PROTEIN, int(qoffs[-1])).astype(np.uint8)).to(dev)
        scoring = (sub, -11, -1)
        n_all = nq * nt
        cells = float(qoffs[-1]) * float(offs[-1] - offs[0])
        out["prefilter_queries"], out["prefilter_qlen"], out["prefilter_targets"], out["prefilter_cells"] = nq, args.qlen, nt, int(cells)
        # leg i: the full search, unchanged code
        table = torch.zeros(n_all * 3, dtype=torch.int64, device=dev)
        out["prefilter_full_ms"], out["prefilter_full_range_ms"] = spread(lambda: db.search_affine_device(d_q, qoffs, scoring, out=table))
        out["prefilter_full_ps_per_cell"] = round(out["prefilter_full_ms"] * 1e9 / cells, 4)
        rows = table.view(n_all, 3)
        # the ungapped scores of all pairs by both kernels; min_score: the score about 1 % of the pairs reach
        u = {}
        for lanes in (32, 0):
            eng.set_option("prefilter_lanes", lanes)
            _, _, u[lanes] = db.prefilter_ungapped_device(d_q, qoffs, sub, 1, 0, want_scores=True)
            out[f"prefilter_lanes{lanes}_packed_launches"] = eng.get_option("last_prefilter_packed_launches")
            out[f"prefilter_lanes{lanes}_launches"] = eng.get_option("last_prefilter_launches")
        torch.cuda.synchronize()
        flat_u = u[0].view(-1)
        out["prefilter_kernels_identical"] = bool(torch.equal(u[0], u[32]))
        out["prefilter_u_le_max_score_all_pairs"] = bool((flat_u.to(torch.int64) <= rows[:, 1]).all().item())
        min_score = max(1, int(flat_u.float().kthvalue(n_all - n_all // 100).values.item()))
        cap = int((flat_u >= min_score).sum().item())       # (every target of data set (a) has a letter)
        out["prefilter_min_score"], out["prefilter_passing"], out["prefilter_passing_share"] = min_score, cap, round(cap / n_all, 5)
        out["prefilter_u_max"], out["prefilter_u_median"] = int(flat_u.max().item()), int(flat_u.float().median().item())
        del u
        # leg ii: the filter alone, list and count, no score table
        bufs = (torch.empty((cap, 2), dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev), None)
        for lanes, tag in ((32, "lanes32"), (0, "packed")):
            eng.set_option("prefilter_lanes", lanes)
            ms, rng_ms = spread(lambda: db.prefilter_ungapped_device(d_q, qoffs, sub, min_score, cap, out=bufs))
            out[f"prefilter_{tag}_ms"], out[f"prefilter_{tag}_range_ms"] = ms, rng_ms
            out[f"prefilter_{tag}_ps_per_cell"] = round(ms * 1e9 / cells, 4)
            out[f"prefilter_{tag}_gcups"] = round(cells / ms / 1e6, 1)
            out[f"prefilter_{tag}_count_ok"] = bool(int(bufs[1].item()) == cap)
            out[f"prefilter_full_over_{tag}"] = round(out["prefilter_full_ms"] / ms, 2)
            out[f"prefilter_{tag}_faster_than_full"] = bool(ms < out["prefilter_full_ms"])
        out["prefilter_lanes32_over_packed"] = round(out["prefilter_lanes32_ms"] / out["prefilter_packed_ms"], 3)
        # leg iii: the filter and the rescoring of its whole list, nothing read in between
        res = torch.full((cap * 3,), -1, dtype=torch.int64, device=dev)

        def chain():
            d_pairs, _, _ = db.prefilter_ungapped_device(d_q, qoffs, sub, min_score, cap, out=bufs)
            db.search_affine_pairs_device(d_q, qoffs, scoring, d_pairs, out=res)

        out["prefilter_chain_ms"], out["prefilter_chain_range_ms"] = spread(chain)
        out["prefilter_full_over_chain"] = round(out["prefilter_full_ms"] / out["prefilter_chain_ms"], 2)
        pr = bufs[0]
        inside = bool(((pr[:, 0] >= 0) & (pr[:, 0] < nq) & (pr[:, 1] >= 0) & (pr[:, 1] < nt)).all().item())
        flat = pr[:, 0] * nt + pr[:, 1]
        out["prefilter_chain_identical"] = bool(inside and int(flat.unique().numel()) == cap and torch.equal(res.view(cap, 3), rows[flat])
                                                and bool((flat_u[flat] >= min_score).all().item()))
        out["prefilter_chain_rescored_cells"] = int(float(args.qlen) * float(lens[pr[:, 1].cpu().numpy()].sum())) if inside else 0
        db.close()

    def prefiltered_top_leg(packed, offs, nq=64, top=10):
        d_db = torch.from_numpy(packed.copy()).to(dev)
        db = eng.prepare_db(d_db, offs)
        nt = len(offs) - 1
        qoffs = np.arange(nq + 1, dtype=np.int64) * args.qlen
        d_q = torch.from_numpy(rng.choice(PROTEIN, int(qoffs[-1])).astype(np.uint8)).to(dev)
        scoring = (sub, -11, -1)
        n_all = nq * nt
        P = "prefiltered_top"
        out[f"{P}_queries"], out[f"{P}_qlen"], out[f"{P}_targets"], out[f"{P}_top"] = nq, args.qlen, nt, top
        # the full table and the ungapped scores of all pairs: the reference of the checks and the threshold about 1 % of the pairs reach
        table = db.search_affine_device(d_q, qoffs, scoring).view(nq, nt, 3)
        _, _, u = db.prefilter_ungapped_device(d_q, qoffs, sub, 1, 0, want_scores=True)
        torch.cuda.synchronize()
        flat_u = u.view(-1)
        S = max(1, int(flat_u.float().kthvalue(n_all - n_all // 100).values.item()))
        S_low = max(1, int(flat_u.float().kthvalue(n_all - n_all // 10).values.item()))
        cap = int((flat_u >= S).sum().item())               # (every target of data set (a) has a letter)
        out[f"{P}_min_score"], out[f"{P}_passing"], out[f"{P}_passing_share"] = S, cap, round(cap / n_all, 5)
        tbits = max(1, int(nt - 1).bit_length())

        def masked_top(thr):
            """The top rows of the full table among the pairs with U >= thr, by torch: (hits, nhits) as the library lays them out."""
            score = torch.where(u >= thr, table[:, :, 1], torch.full_like(table[:, :, 1], -1))
            key = torch.where(score >= 0, (score << tbits) | (nt - 1 - torch.arange(nt, device=dev)), torch.full_like(score, -1))
            best, target = key.topk(top, dim=1)
            ok = best >= 0
            rows = torch.gather(table, 1, target[:, :, None].expand(nq, top, 3))
            hits = torch.stack([torch.where(ok, target, torch.full_like(target, -1)), torch.where(ok, rows[:, :, 0], torch.zeros_like(target)),
                                torch.where(ok, rows[:, :, 1], torch.zeros_like(target))], dim=2)
            return hits, ok.sum(dim=1)

        want_hits, want_nhits = masked_top(S)
        outs = {k: (torch.zeros(nq * top * 3, dtype=torch.int64, device=dev), torch.zeros(nq, dtype=torch.int64, device=dev)) for k in ("i", "ii", "iii", "iv", "v")}
        # leg i: search and dense selection in one call, the parent's code
        out[f"{P}_full_ms"], out[f"{P}_full_range_ms"] = spread(lambda: db.search_affine_top_device(d_q, qoffs, scoring, top, 0, out=outs["i"]))
        # leg ii: the three calls by hand, nothing read in between
        bufs = (torch.empty((cap, 2), dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev), None)
        res = torch.full((cap * 3,), -1, dtype=torch.int64, device=dev)

        def chain():
            d_pairs, _, _ = db.prefilter_ungapped_device(d_q, qoffs, sub, S, cap, out=bufs)
            r = db.search_affine_pairs_device(d_q, qoffs, scoring, d_pairs, out=res)
            return eng.top_hits_pairs_device(d_pairs, r, cap, nq, nt, top, 0, out=outs["ii"])

        out[f"{P}_chain_ms"], out[f"{P}_chain_range_ms"] = spread(chain)
        out[f"{P}_chain_count"] = int(bufs[1].item())
        # the shares of the hand chain, each alone on the same buffers
        out[f"{P}_filter_ms"], out[f"{P}_filter_range_ms"] = spread(lambda: db.prefilter_ungapped_device(d_q, qoffs, sub, S, cap, out=bufs))
        out[f"{P}_rescore_ms"], out[f"{P}_rescore_range_ms"] = spread(lambda: db.search_affine_pairs_device(d_q, qoffs, scoring, bufs[0], out=res))
        # leg iii: the one call
        npairs = [None]

        def one_call():
            h, n, npairs[0] = db.search_affine_top_prefiltered_device(d_q, qoffs, scoring, S, cap, top, 0, out=outs["iii"])
            return h, n

        out[f"{P}_one_call_ms"], out[f"{P}_one_call_range_ms"] = spread(one_call)
        out[f"{P}_one_call_count"] = int(npairs[0].item())
        out[f"{P}_count_within_cap"] = bool(out[f"{P}_one_call_count"] <= cap and out[f"{P}_chain_count"] <= cap)
        # leg iv: the selection alone over the list of leg ii
        out[f"{P}_select_ms"], out[f"{P}_select_range_ms"] = spread(lambda: eng.top_hits_pairs_device(bufs[0], res.view(cap, 3), cap, nq, nt, top, 0, out=outs["iv"]))
        out[f"{P}_select_launches"], out[f"{P}_select_kernel"] = eng.get_option("last_top_pairs_launches"), eng.get_option("last_top_pairs_kernel")
        out[f"{P}_select_longest_segment"] = int(torch.bincount(bufs[0][:, 0], minlength=nq).max().item())
        # leg v: the dense selection over the full table, for scale
        out[f"{P}_dense_select_ms"], out[f"{P}_dense_select_range_ms"] = spread(lambda: eng.top_hits_device(table, nq, nt, top, 0, out=outs["v"]))
        views = {k: eng._top_views(h, n, nq, top) for k, (h, n) in outs.items()}
        torch.cuda.synchronize()
        out[f"{P}_chain_equals_one_call"] = bool(torch.equal(views["ii"][0], views["iii"][0]) and torch.equal(views["ii"][1], views["iii"][1]))
        for k, tag in (("ii", "chain"), ("iii", "one_call"), ("iv", "select")):
            out[f"{P}_{tag}_equals_masked_table"] = bool(torch.equal(views[k][0], want_hits) and torch.equal(views[k][1], want_nhits))
        found = (views["i"][0][:, :, None, 0] == views["iii"][0][:, None, :, 0]).any(dim=2) & (views["i"][0][:, :, 0] >= 0)
        out[f"{P}_recall"] = round(float(found.sum().item()) / max(1, int((views["i"][0][:, :, 0] >= 0).sum().item())), 4)
        out[f"{P}_one_call_faster_than_full"] = bool(out[f"{P}_one_call_ms"] < out[f"{P}_full_ms"])
        out[f"{P}_full_over_one_call"] = round(out[f"{P}_full_ms"] / out[f"{P}_one_call_ms"], 2)
        out[f"{P}_select_over_rescore"] = round(out[f"{P}_select_ms"] / out[f"{P}_rescore_ms"], 4)
        out[f"{P}_select_over_dense_select"] = round(out[f"{P}_select_ms"] / out[f"{P}_dense_select_ms"], 4)
        # leg vi: legs i and iii, each followed by the alignment of its table
        ops_cap = args.qlen + int(np.diff(offs).max())
        abufs = (torch.zeros((nq * top, 7), dtype=torch.int64, device=dev), torch.zeros((nq * top, ops_cap), dtype=torch.uint8, device=dev))

        def full_aligned():
            h, n = db.search_affine_top_device(d_q, qoffs, scoring, top, 0, out=outs["i"])
            db.align_affine_hits_device(d_q, qoffs, scoring, h, n, ops_cap=ops_cap, out=abufs)

        def one_call_aligned():
            h, n = one_call()
            db.align_affine_hits_device(d_q, qoffs, scoring, h, n, ops_cap=ops_cap, out=abufs)

        out[f"{P}_full_aligned_ms"], out[f"{P}_full_aligned_range_ms"] = spread(full_aligned)
        out[f"{P}_one_call_aligned_ms"], out[f"{P}_one_call_aligned_range_ms"] = spread(one_call_aligned)
        # the streaming sort: the selection alone over the list of a threshold that about 10 % of the pairs reach
        cap_low = int((flat_u >= S_low).sum().item())
        low = (torch.empty((cap_low, 2), dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev), None)
        db.prefilter_ungapped_device(d_q, qoffs, sub, S_low, cap_low, out=low)
        res_low = db.search_affine_pairs_device(d_q, qoffs, scoring, low[0])
        out[f"{P}_low_min_score"], out[f"{P}_low_passing"] = S_low, cap_low
        for t2 in (top, 4096):
            o = (torch.zeros(nq * t2 * 3, dtype=torch.int64, device=dev), torch.zeros(nq, dtype=torch.int64, device=dev))
            out[f"{P}_low_select_top{t2}_ms"], out[f"{P}_low_select_top{t2}_range_ms"] = spread(
                lambda: eng.top_hits_pairs_device(low[0], res_low, cap_low, nq, nt, t2, 0, out=o))
            if t2 == top:
                low_hits, low_nhits = masked_top(S_low)
                got = eng._top_views(o[0], o[1], nq, top)
                out[f"{P}_low_select_equals_masked_table"] = bool(torch.equal(got[0], low_hits) and torch.equal(got[1], low_nhits))
        out[f"{P}_low_select_kernel"] = eng.get_option("last_top_pairs_kernel")
        out[f"{P}_low_longest_segment"] = int(torch.bincount(low[0][:, 0], minlength=nq).max().item())
        db.close()

    def pssm_leg(packed, offs, nq=64):
        d_db = torch.from_numpy(packed.copy()).to(dev)
        db = eng.prepare_db(d_db, offs)
        tiny = eng.prepare_db(d_db, offs[:1] + np.array([0, 1]))             # one target of one letter: a call is its uploads and its profile launch
        nt = len(offs) - 1
        qoffs = np.arange(nq + 1, dtype=np.int64) * args.qlen
        queries = rng.choice(PROTEIN, int(qoffs[-1])).astype(np.uint8)
        d_q = torch.from_numpy(queries).to(dev)
        m, moffs = swamd.pssm_from_queries((queries, qoffs), sub, letters)   # iteration 0: the matrices that reproduce the queries
        d_m = torch.from_numpy(m.reshape(-1).copy()).to(dev)
        scoring, pscoring = (sub, -11, -1), (letters, -4, 127, -11, -1)
        res_a = torch.zeros(nq * nt * 3, dtype=torch.int64, device=dev)
        res_p = torch.zeros(nq * nt * 3, dtype=torch.int64, device=dev)
        one = torch.zeros(nq * 3, dtype=torch.int64, device=dev)
        legs = {"affine": lambda: db.search_affine_device(d_q, qoffs, scoring, out=res_a), "pssm": lambda: db.search_pssm_device(d_m, moffs, pscoring, out=res_p),
                "affine_profile_call": lambda: tiny.search_affine_device(d_q, qoffs, scoring, out=one),
                "pssm_profile_call": lambda: tiny.search_pssm_device(d_m, moffs, pscoring, out=one)}
        reps = max(5, args.reps)
        P = "pssm"
        out[f"{P}_queries"], out[f"{P}_qlen"], out[f"{P}_targets"], out[f"{P}_letters"], out[f"{P}_reps"] = nq, args.qlen, nt, len(letters), reps
        for pair in (("affine", "pssm"), ("affine_profile_call", "pssm_profile_call")):
            ms = {k: [] for k in pair}
            for _ in range(max(1, args.warmup)):
                for k in pair:
                    legs[k]()
            torch.cuda.synchronize()
            for _ in range(reps):                                            # alternating: a drift of the device shows in both alike
                for k in pair:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    legs[k]()
                    e1.record()
                    torch.cuda.synchronize()
                    ms[k].append(e0.elapsed_time(e1))
            for k in pair:
                out[f"{P}_{k}_ms"], out[f"{P}_{k}_range_ms"] = round(float(np.median(ms[k])), 4), [round(min(ms[k]), 4), round(max(ms[k]), 4)]
        out[f"{P}_identical"] = bool(torch.equal(res_a, res_p))
        out[f"{P}_launches"] = eng.get_option("last_search_multi_launches")
        # the expectation: the same sweeps behind a profile that is 257 x 512 bytes per query -- equal within the affine call's own spread
        margin = out[f"{P}_affine_range_ms"][1] - out[f"{P}_affine_range_ms"][0]
        out[f"{P}_margin_ms"] = round(margin, 4)
        out[f"{P}_minus_affine_ms"] = round(out[f"{P}_pssm_ms"] - out[f"{P}_affine_ms"], 4)
        out[f"{P}_within_margin"] = bool(abs(out[f"{P}_minus_affine_ms"]) <= margin)
        db.close()
        tiny.close()

    def pssm_iterate_leg(packed, offs, nq=64, reps=7):
        import time
        d_db = torch.from_numpy(packed.copy()).to(dev)
        db = eng.prepare_db(d_db, offs)
        qoffs = np.arange(nq + 1, dtype=np.int64) * args.qlen
        queries = rng.choice(PROTEIN, int(qoffs[-1])).astype(np.uint8)
        m, moffs = swamd.pssm_from_queries((queries, qoffs), sub, letters)
        d_m = torch.from_numpy(m.reshape(-1).copy()).to(dev)
        pscoring, update, cap = (letters, -4, 127, -11, -1), (sub, 10, 1), 4 * args.qlen
        P = "pssm_iterate"
        out[f"{P}_queries"], out[f"{P}_qlen"], out[f"{P}_targets"], out[f"{P}_reps"], out[f"{P}_ops_cap"] = nq, args.qlen, len(offs) - 1, reps, cap
        for top in (10, 100, 4096):
            hits, nhits = db.search_pssm_top_device(d_m, moffs, pscoring, top, 1)
            aln, ops = db.align_pssm_hits_device(d_m, moffs, pscoring, hits, nhits, ops_cap=cap)
            d_out = torch.empty_like(d_m)
            h2 = (torch.zeros_like(hits), torch.zeros_like(nhits))
            state = {}

            def device_call():
                db.pssm_from_hits_device(d_m, moffs, pscoring, update, hits, nhits, aln, ops, cap, out=d_out)

            def host_round_trip():
                h, n, a, o = hits.cpu().numpy(), nhits.cpu().numpy(), aln.cpu().numpy(), ops.cpu().numpy()
                state["m"] = swamd.pssm_from_hits_host((m, moffs), (packed, offs), pscoring, update, h, n, a, o)
                state["d"] = torch.from_numpy(state["m"].reshape(-1)).to(dev)

            def search_alone():
                db.search_pssm_top_device(d_m, moffs, pscoring, top, 1, out=h2)

            def iteration():
                db.align_pssm_hits_device(d_m, moffs, pscoring, hits, nhits, ops_cap=cap, out=(aln, ops))
                db.pssm_from_hits_device(d_m, moffs, pscoring, update, hits, nhits, aln, ops, cap, out=d_out)
                db.search_pssm_top_device(d_out, moffs, pscoring, top, 1, out=h2)

            def wall(fn):                                                    # a leg with host work: wall clock around a synchronised call
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            for pair in (("device_call", "host_round_trip"), ("search_alone", "iteration")):
                legs = {"device_call": device_call, "host_round_trip": host_round_trip, "search_alone": search_alone, "iteration": iteration}
                ms = {k: [] for k in pair}
                for k in pair:
                    wall(legs[k])                                            # warm-up
                for _ in range(reps):                                        # alternating: a drift of the device shows in both alike
                    for k in pair:
                        ms[k].append(wall(legs[k]))
                for k in pair:
                    out[f"{P}_top{top}_{k}_ms"] = round(float(np.median(ms[k])), 4)
                    out[f"{P}_top{top}_{k}_range_ms"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
            device_call()
            torch.cuda.synchronize()
            out[f"{P}_top{top}_identical"] = bool((d_out.cpu().numpy().reshape(m.shape) == state["m"]).all())
            out[f"{P}_top{top}_over_cap"] = int((aln[:, :, 6] > cap).sum().item())
            out[f"{P}_top{top}_moved"] = bool((state["m"] != m).any())
            out[f"{P}_top{top}_host_over_device"] = round(out[f"{P}_top{top}_host_round_trip_ms"] / out[f"{P}_top{top}_device_call_ms"], 2)
            out[f"{P}_top{top}_iteration_over_search"] = round(out[f"{P}_top{top}_iteration_ms"] / out[f"{P}_top{top}_search_alone_ms"], 3)
        out[f"{P}_identical"] = all(out[f"{P}_top{t}_identical"] for t in (10, 100, 4096))
        db.close()

    def msa_leg(packed, offs, nq=64, reps=7):
        import time
        d_db = torch.from_numpy(packed.copy()).to(dev)
        db = eng.prepare_db(d_db, offs)
        qoffs = np.arange(nq + 1, dtype=np.int64) * args.qlen
        queries = rng.choice(PROTEIN, int(qoffs[-1])).astype(np.uint8)
        d_q = torch.from_numpy(queries.copy()).to(dev)
        scoring, cap, inc = (sub, -11, -1), 4 * args.qlen, 1
        P = "msa"
        out[f"{P}_queries"], out[f"{P}_qlen"], out[f"{P}_targets"], out[f"{P}_reps"], out[f"{P}_ops_cap"] = nq, args.qlen, len(offs) - 1, reps, cap
        for top in (10, 100, 4096):
            hits, nhits = db.search_affine_top_device(d_q, qoffs, scoring, top, 1)
            aln, ops = db.align_affine_hits_device(d_q, qoffs, scoring, hits, nhits, ops_cap=cap)
            _, rows, _, total = db.msa_from_hits_device(d_q, qoffs, inc, hits, nhits, aln, ops, cap, cols=False)      # the sizing call
            torch.cuda.synchronize()
            a3m_bytes = int(total.item())
            cols = torch.empty(int(qoffs[-1]) * top, dtype=torch.uint8, device=dev)
            a3m = torch.empty(max(1, a3m_bytes), dtype=torch.uint8, device=dev)
            state = {}

            def device_call():
                db.msa_from_hits_device(d_q, qoffs, inc, hits, nhits, aln, ops, cap, cols=cols, rows=rows, a3m=a3m, a3m_cap=a3m_bytes, a3m_bytes=total)

            def host_round_trip():
                h, n, a, o = hits.cpu().numpy(), nhits.cpu().numpy(), aln.cpu().numpy(), ops.cpu().numpy()
                state["host"] = swamd.msa_from_hits_host((queries, qoffs), (packed, offs), inc, h, n, a, o, a3m_cap=a3m_bytes)

            def wall(fn):                                                    # wall clock around a synchronised call
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            legs = {"device_call": device_call, "host_round_trip": host_round_trip}
            ms = {k: [] for k in legs}
            for k in legs:
                wall(legs[k])                                                # warm-up
            for _ in range(reps):                                            # alternating: a drift of the device shows in both alike
                for k in legs:
                    ms[k].append(wall(legs[k]))
            for k in legs:
                out[f"{P}_top{top}_{k}_ms"] = round(float(np.median(ms[k])), 4)
                out[f"{P}_top{top}_{k}_range_ms"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
            cols.fill_(0x55); rows.fill_(0x5555555555555555); a3m.fill_(0x55); total.fill_(-1)
            device_call()
            torch.cuda.synchronize()
            hc, hr, ha = state["host"]
            n = nq * top
            out[f"{P}_top{top}_identical"] = bool(cols.cpu().numpy().tobytes() == hc.tobytes() and rows.cpu().numpy()[:3 * n].tobytes() == hr.tobytes()
                                                  and a3m.cpu().numpy()[:a3m_bytes].tobytes() == ha.tobytes() and int(total.item()) == a3m_bytes)
            out[f"{P}_top{top}_launches"] = eng.get_option("last_msa_hits_launches")
            out[f"{P}_top{top}_used_entries"] = int((hr["len"] > 0).sum())
            out[f"{P}_top{top}_inserts"] = int(hr["ninsert"].sum())
            out[f"{P}_top{top}_over_cap"] = int((aln[:, :, 6] > cap).sum().item())
            written = cols.numel() + 24 * n + a3m_bytes
            out[f"{P}_top{top}_bytes_written"] = int(written)
            out[f"{P}_top{top}_d2h_bytes"] = int(hits.numel() * 8 + nhits.numel() * 8 + aln.numel() * 8 + ops.numel())
            out[f"{P}_top{top}_write_gbs"] = round(written / out[f"{P}_top{top}_device_call_ms"] / 1e6, 2)
            out[f"{P}_top{top}_host_over_device"] = round(out[f"{P}_top{top}_host_round_trip_ms"] / out[f"{P}_top{top}_device_call_ms"], 2)
        out[f"{P}_identical"] = all(out[f"{P}_top{t}_identical"] for t in (10, 100, 4096))
        db.close()

    def msa_filter_leg(packed, offs, nq=64, reps=7, per_hit=16, filt=(90, 0)):
        import time
        d_db = torch.from_numpy(packed.copy()).to(dev)
        db = eng.prepare_db(d_db, offs)
        qoffs = np.arange(nq + 1, dtype=np.int64) * args.qlen
        queries = rng.choice(PROTEIN, int(qoffs[-1])).astype(np.uint8)
        d_q = torch.from_numpy(queries.copy()).to(dev)
        m, moffs = swamd.pssm_from_queries((queries, qoffs), sub, letters)
        d_m = torch.from_numpy(m.reshape(-1).copy()).to(dev)
        pscoring, weighting, cap, inc = (letters, -4, 127, -11, -1), (per_hit, 1), 4 * args.qlen, 1
        wupdate = (sub, 10 * per_hit, 1)
        P = "msa_filter"
        out[f"{P}_queries"], out[f"{P}_qlen"], out[f"{P}_targets"], out[f"{P}_reps"], out[f"{P}_ops_cap"] = nq, args.qlen, len(offs) - 1, reps, cap
        out[f"{P}_max_ident_pct"], out[f"{P}_min_cover_pct"] = filt
        for top in (10, 100, 4096):
            hits, nhits = db.search_pssm_top_device(d_m, moffs, pscoring, top, 1)
            aln, ops = db.align_pssm_hits_device(d_m, moffs, pscoring, hits, nhits, ops_cap=cap)
            cols = db.msa_from_hits_device(d_q, moffs, inc, hits, nhits, aln, ops, cap, rows=False)[0]
            d_keep = torch.empty(nq * top, dtype=torch.int32, device=dev)
            d_nkept = torch.empty(nq, dtype=torch.int64, device=dev)
            hf = torch.empty_like(hits)
            d_out = torch.empty_like(d_m)
            d_w = torch.empty((nq, top), dtype=torch.int32, device=dev)
            h2 = (torch.zeros_like(hits), torch.zeros_like(nhits))
            state = {}

            def device_call():
                eng.msa_filter_device(cols, d_q, moffs, top, filt, hits=hits.view(-1), hits_out=hf.view(-1), keep=d_keep, nkept=d_nkept)

            def host_round_trip():                                           # what a caller has today: D2H, the host leg, H2D of the table
                c, h = cols.cpu().numpy(), hits.cpu().numpy()
                state["host"] = swamd.msa_filter_host(c, (queries, qoffs), top, filt[0], filt[1], hits=h)
                state["d"] = torch.from_numpy(state["host"][2].reshape(-1)).to(dev)

            def weighted_iteration():
                db.align_pssm_hits_device(d_m, moffs, pscoring, hits, nhits, ops_cap=cap, out=(aln, ops))
                db.pssm_hit_weights_device(moffs, pscoring, weighting, hits, nhits, aln, ops, cap, out=d_w)
                db.pssm_from_hits_device(d_m, moffs, pscoring, wupdate, hits, nhits, aln, ops, cap, weights=d_w, out=d_out)
                db.search_pssm_top_device(d_out, moffs, pscoring, top, 1, out=h2)

            def filtered_iteration():
                db.align_pssm_hits_device(d_m, moffs, pscoring, hits, nhits, ops_cap=cap, out=(aln, ops))
                db.msa_from_hits_device(d_q, moffs, inc, hits, nhits, aln, ops, cap, cols=cols, rows=False)
                eng.msa_filter_device(cols, d_q, moffs, top, filt, hits=hits.view(-1), hits_out=hf.view(-1), keep=False, nkept=False)
                db.pssm_hit_weights_device(moffs, pscoring, weighting, hf, nhits, aln, ops, cap, out=d_w)
                db.pssm_from_hits_device(d_m, moffs, pscoring, wupdate, hf, nhits, aln, ops, cap, weights=d_w, out=d_out)
                db.search_pssm_top_device(d_out, moffs, pscoring, top, 1, out=h2)

            def wall(fn):                                                    # wall clock around a synchronised call
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            legs = {"device_call": device_call, "host_round_trip": host_round_trip, "weighted_iteration": weighted_iteration,
                    "filtered_iteration": filtered_iteration}
            for group in (("device_call", "host_round_trip"), ("weighted_iteration", "filtered_iteration")):
                ms = {k: [] for k in group}
                first = {k: wall(legs[k]) for k in group}                    # warm-up
                # a host leg of more than 20 s is timed by that one call: seven more would take the better part of an hour
                once = {k for k in group if first[k] > 20e3}
                for _ in range(reps):                                        # alternating: a drift of the device shows in all alike
                    for k in group:
                        if k not in once:
                            ms[k].append(wall(legs[k]))
                for k in group:
                    if k in once:
                        ms[k] = [first[k]]
                    out[f"{P}_top{top}_{k}_ms"] = round(float(np.median(ms[k])), 4)
                    out[f"{P}_top{top}_{k}_range_ms"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
                    out[f"{P}_top{top}_{k}_calls"] = len(ms[k])
            d_keep.fill_(0x55555555); d_nkept.fill_(-1); hf.fill_(0x5555555555555555)
            device_call()
            torch.cuda.synchronize()
            hk, hn, hh = state["host"]
            out[f"{P}_top{top}_identical"] = bool(d_keep.cpu().numpy().tobytes() == hk.tobytes() and d_nkept.cpu().numpy().tobytes() == hn.tobytes()
                                                  and hf.cpu().numpy().tobytes() == hh.tobytes())
            out[f"{P}_top{top}_launches"] = eng.get_option("last_msa_filter_launches")
            out[f"{P}_top{top}_chunks"] = eng.get_option("last_msa_filter_chunks")
            out[f"{P}_top{top}_kept"] = int(hn.sum())
            out[f"{P}_top{top}_rows_with_letters"] = int((cols.cpu().numpy().reshape(-1, args.qlen) != 0x2D).any(axis=1).sum())
            out[f"{P}_top{top}_d2h_bytes"] = int(cols.numel() + hits.numel() * 8)
            out[f"{P}_top{top}_host_over_device"] = round(out[f"{P}_top{top}_host_round_trip_ms"] / out[f"{P}_top{top}_device_call_ms"], 2)
            out[f"{P}_top{top}_filtered_over_weighted"] = round(out[f"{P}_top{top}_filtered_iteration_ms"] / out[f"{P}_top{top}_weighted_iteration_ms"], 4)
        out[f"{P}_identical"] = all(out[f"{P}_top{t}_identical"] for t in (10, 100, 4096))
        db.close()

    def score_stats_leg(packed, offs, nq=64, reps=7, top=100, evalue=1e-3):
        import time
        d_db = torch.from_numpy(packed.copy()).to(dev)
        db = eng.prepare_db(d_db, offs)
        nt = len(offs) - 1
        qoffs = np.arange(nq + 1, dtype=np.int64) * args.qlen
        queries = rng.choice(PROTEIN, int(qoffs[-1])).astype(np.uint8)
        d_q = torch.from_numpy(queries.copy()).to(dev)
        scoring = (sub, -11, -1)
        m, moffs = swamd.pssm_from_queries((queries, qoffs), sub, letters)
        d_m = torch.from_numpy(m.reshape(-1).copy()).to(dev)
        pscoring, cap = (letters, -4, 127, -11, -1), 4 * args.qlen
        P = "score_stats"
        out[f"{P}_queries"], out[f"{P}_qlen"], out[f"{P}_targets"], out[f"{P}_reps"], out[f"{P}_top"], out[f"{P}_evalue"] = nq, args.qlen, nt, reps, top, evalue
        cells = nq * swamd.HIST_CLASSES * swamd.HIST_BINS
        h_plain = (torch.zeros(nq * top * 3, dtype=torch.int64, device=dev), torch.zeros(nq, dtype=torch.int64, device=dev))
        h_stats = (torch.zeros(nq * top * 3, dtype=torch.int64, device=dev), torch.zeros(nq, dtype=torch.int64, device=dev))
        d_hist = torch.empty(cells, dtype=torch.int32, device=dev)
        d_hist2 = torch.empty(cells, dtype=torch.int32, device=dev)
        d_thr = torch.empty(nq * swamd.HIST_CLASSES, dtype=torch.int64, device=dev)
        d_inc = torch.empty(nq * top * 3, dtype=torch.int64, device=dev)
        state = {}

        def wall(fn):                                                        # wall clock around a synchronised call
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def alternate(legs):
            ms = {k: [] for k in legs}
            for k in legs:
                wall(legs[k])                                                # warm-up
            for _ in range(reps):                                            # alternating: a drift of the device shows in all alike
                for k in legs:
                    ms[k].append(wall(legs[k]))
            for k in legs:
                out[f"{P}_{k}_ms"] = round(float(np.median(ms[k])), 4)
                out[f"{P}_{k}_range_ms"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]

        # (1) the histogram inside the bounded-memory search
        alternate({"top": lambda: db.search_affine_top_device(d_q, qoffs, scoring, top, 1, out=h_plain),
                   "top_stats": lambda: db.search_affine_top_stats_device(d_q, qoffs, scoring, top, 1, 0, out=h_stats, hist=d_hist)})
        out[f"{P}_top_stats_over_top"] = round(out[f"{P}_top_stats_ms"] / out[f"{P}_top_ms"], 4)
        out[f"{P}_top_chunks"] = eng.get_option("last_search_top_chunks")
        out[f"{P}_hist_slices"] = eng.get_option("last_score_hist_slices")
        # (2) the histogram alone over the full table, beside a plain read of it
        table = db.search_affine_device(d_q, qoffs, scoring)
        one_cell = table.clone()
        one_cell[:, :, 1] = 41
        d_db1 = torch.zeros(1, dtype=torch.uint8, device=dev)
        db1 = eng.prepare_db(d_db1, np.arange(nt + 1, dtype=np.int64) * 150)   # ... every target in one length class
        table_bytes = table.numel() * 8
        out[f"{P}_table_bytes"] = table_bytes
        for name, t_, h_ in (("search", table, db), ("one_cell", one_cell, db1)):
            for copies in (1, 2, 4):
                eng.set_option("score_hist_copies", copies)
                ms = timed(lambda: eng.score_hist_device(h_, t_.view(-1), nq, 0, hist=d_hist2), 2, 20)
                out[f"{P}_hist_{name}_copies{copies}_ms"] = round(ms, 4)
                out[f"{P}_hist_{name}_copies{copies}_gbs"] = round(table_bytes / ms / 1e6, 1)
            eng.set_option("score_hist_copies", 0)
            ms = timed(lambda: eng.score_hist_device(h_, t_.view(-1), nq, 0, hist=d_hist2), 2, 20)
            out[f"{P}_hist_{name}_ms"], out[f"{P}_hist_{name}_gbs"] = round(ms, 4), round(table_bytes / ms / 1e6, 1)
        ms = timed(lambda: torch.sum(table), 2, 20)
        out[f"{P}_torch_sum_ms"], out[f"{P}_torch_sum_gbs"] = round(ms, 4), round(table_bytes / ms / 1e6, 1)
        eng.score_hist_device(db, table.view(-1), nq, 0, hist=d_hist2)
        torch.cuda.synchronize()
        out[f"{P}_identical"] = bool(torch.equal(d_hist.view(-1), d_hist2.view(-1)) and torch.equal(h_plain[0], h_stats[0]) and torch.equal(h_plain[1], h_stats[1]))
        one = eng.score_hist_device(db1, one_cell.view(-1), nq, 0).cpu().numpy().view(np.uint32)
        out[f"{P}_one_cell_count"] = int(one[:, swamd.length_class(150), 41].min())
        out[f"{P}_identical"] = bool(out[f"{P}_identical"] and (one.sum(axis=(1, 2)) == nt).all() and out[f"{P}_one_cell_count"] == nt)

        # (3) what a round of the inclusion by E-value adds, and (5) the path a caller had before
        def fit_round_trip(evalue=evalue):
            h = d_hist.cpu().numpy().view(np.uint32).reshape(nq, swamd.HIST_CLASSES, swamd.HIST_BINS)
            state["fit"] = swamd.score_fit(h, 0)
            state["thr"] = swamd.score_thresholds(state["fit"], evalue)
            d_thr.copy_(torch.from_numpy(state["thr"].reshape(-1)))
            db.hits_threshold_device(d_thr, nq, top, h_stats[0], h_stats[1], hits_out=d_inc, keep=False, nkept=False)

        def host_histogram():
            state["host_hist"] = swamd.score_hist_host(table.cpu().numpy(), offs, 0)

        alternate({"fit_round_trip": fit_round_trip, "host_histogram": host_histogram})
        out[f"{P}_identical"] = bool(out[f"{P}_identical"] and (state["host_hist"] == d_hist.cpu().numpy().view(np.uint32).reshape(state["host_hist"].shape)).all())
        out[f"{P}_fit_valid"] = int(state["fit"]["valid"].sum())
        out[f"{P}_fit_b_median"], out[f"{P}_fit_sigma_median"] = round(float(np.median(state["fit"]["b"])), 3), round(float(np.median(state["fit"]["sigma"])), 3)
        out[f"{P}_kept_at_evalue"] = int((d_inc.view(nq, top, 3)[:, :, 0] >= 0).sum().item())
        # (4) an iteration by E-value beside one by raw score
        hits, nhits = db.search_pssm_top_device(d_m, moffs, pscoring, top, 1)
        aln, ops = db.align_pssm_hits_device(d_m, moffs, pscoring, hits, nhits, ops_cap=cap)
        d_out = torch.empty_like(d_m)
        h2 = (torch.zeros_like(hits), torch.zeros_like(nhits))
        least = -(1 << 63)

        def score_iteration():
            db.align_pssm_hits_device(d_m, moffs, pscoring, hits, nhits, ops_cap=cap, out=(aln, ops))
            db.pssm_from_hits_device(d_m, moffs, pscoring, (sub, 10, 1), hits, nhits, aln, ops, cap, out=d_out)
            db.search_pssm_top_device(d_out, moffs, pscoring, top, 1, out=h2)

        def evalue_iteration():                                              # the round's histogram is that of the search before it;
            fit_round_trip(1e12)                                             # an E-value no hit misses: both iterations build the same matrix
            db.align_pssm_hits_device(d_m, moffs, pscoring, hits, nhits, ops_cap=cap, out=(aln, ops))
            db.pssm_from_hits_device(d_m, moffs, pscoring, (sub, 10, least), d_inc.view(nq, top, 3), nhits, aln, ops, cap, out=d_out)
            db.search_pssm_top_stats_device(d_out, moffs, pscoring, top, 1, 0, out=h2, hist=d_hist2)

        db.search_pssm_top_stats_device(d_m, moffs, pscoring, top, 1, 0, out=(hits.view(-1), nhits), hist=d_hist)
        h_stats = (hits.view(-1), nhits)
        alternate({"score_iteration": score_iteration, "evalue_iteration": evalue_iteration})
        out[f"{P}_evalue_over_score_iteration"] = round(out[f"{P}_evalue_iteration_ms"] / out[f"{P}_score_iteration_ms"], 4)
        db1.close()
        db.close()

    def mask_leg(packed, offs, nq=64, reps=7, top=100, evalue=1e-3):
        import time
        d_db = torch.from_numpy(packed.copy()).to(dev)
        db = eng.prepare_db(d_db, offs)
        nt, nbytes = len(offs) - 1, int(offs[-1])
        P = "mask"
        out[f"{P}_targets"], out[f"{P}_letters"], out[f"{P}_reps"] = nt, nbytes, reps
        d_out, d_out2, d_host, d_copy = (torch.zeros_like(d_db) for _ in range(4))
        d_n = torch.zeros(nt, dtype=torch.int64, device=dev)
        state = {}

        def wall(fn):                                                        # wall clock around a synchronised call
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def alternate(legs, reps=reps):
            ms = {k: [] for k in legs}
            for k in legs:
                wall(legs[k])                                                # warm-up
            for _ in range(reps):                                            # alternating: a drift of the device shows in all alike
                for k in legs:
                    ms[k].append(wall(legs[k]))
            for k in legs:
                out[f"{P}_{k}_ms"] = round(float(np.median(ms[k])), 4)
                out[f"{P}_{k}_range_ms"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]

        # (1) the device call, with and without the counts, beside a plain device copy of the same bytes
        def host_path():                                                     # what a caller had before: D2H, the host leg, H2D
            h = d_db.cpu().numpy()
            state["host"] = swamd.mask_low_complexity_host((h, offs))
            d_host.copy_(torch.from_numpy(state["host"][0]))

        alternate({"device": lambda: db.mask_low_complexity_device(out=d_out, nmasked=d_n),
                   "device_no_counts": lambda: db.mask_low_complexity_device(out=d_out2, nmasked=False),
                   "clone": lambda: state.__setitem__("clone", torch.clone(d_db)),
                   "copy": lambda: d_copy.copy_(d_db)})
        alternate({"host_path": host_path}, reps=3)
        db.mask_low_complexity_device(out=d_out, nmasked=d_n)
        out[f"{P}_launches"], out[f"{P}_tiles"] = eng.get_option("last_mask_launches"), eng.get_option("last_mask_tiles")
        torch.cuda.synchronize()
        out[f"{P}_identical"] = bool(torch.equal(d_out, d_host) and torch.equal(d_out, d_out2) and (d_n.cpu().numpy() == state["host"][1]).all())
        out[f"{P}_letters_masked"], out[f"{P}_targets_masked"] = int(d_n.sum().item()), int((d_n > 0).sum().item())
        out[f"{P}_device_gbs"] = round(2 * nbytes / out[f"{P}_device_ms"] / 1e6, 1)
        out[f"{P}_clone_gbs"] = round(2 * nbytes / out[f"{P}_clone_ms"] / 1e6, 1)
        out[f"{P}_host_over_device"] = round(out[f"{P}_host_path_ms"] / out[f"{P}_device_ms"], 1)
        out[f"{P}_device_over_clone"] = round(out[f"{P}_device_ms"] / out[f"{P}_clone_ms"], 2)
        # (2) an iteration by E-value (the one of --score-stats) on the plain handle and on the masked one
        dbm = eng.prepare_db(d_out, offs)
        qoffs = np.arange(nq + 1, dtype=np.int64) * args.qlen
        queries = rng.choice(PROTEIN, int(qoffs[-1])).astype(np.uint8)
        m, moffs = swamd.pssm_from_queries((queries, qoffs), sub, letters)
        d_m = torch.from_numpy(m.reshape(-1).copy()).to(dev)
        pscoring, cap, least = (letters, -4, 127, -11, -1), 4 * args.qlen, -(1 << 63)
        cells = nq * swamd.HIST_CLASSES * swamd.HIST_BINS
        d_thr = torch.empty(nq * swamd.HIST_CLASSES, dtype=torch.int64, device=dev)
        d_inc = torch.empty(nq * top * 3, dtype=torch.int64, device=dev)
        d_next = torch.empty_like(d_m)
        legs = {}
        for name, h_ in (("plain", db), ("masked", dbm)):
            hist, hist2 = (torch.empty(cells, dtype=torch.int32, device=dev) for _ in range(2))
            hits, nhits, _ = h_.search_pssm_top_stats_device(d_m, moffs, pscoring, top, 1, 0, hist=hist)
            aln, ops = h_.align_pssm_hits_device(d_m, moffs, pscoring, hits, nhits, ops_cap=cap)
            h2 = (torch.zeros_like(hits).view(-1), torch.zeros_like(nhits))

            def iteration(h_=h_, hist=hist, hist2=hist2, hits=hits, nhits=nhits, aln=aln, ops=ops, h2=h2):
                fit = swamd.score_fit(hist.cpu().numpy().view(np.uint32).reshape(nq, swamd.HIST_CLASSES, swamd.HIST_BINS), 0)
                d_thr.copy_(torch.from_numpy(swamd.score_thresholds(fit, evalue).reshape(-1)))
                h_.hits_threshold_device(d_thr, nq, top, hits.view(-1), nhits, hits_out=d_inc, keep=False, nkept=False)
                h_.align_pssm_hits_device(d_m, moffs, pscoring, hits, nhits, ops_cap=cap, out=(aln, ops))
                h_.pssm_from_hits_device(d_m, moffs, pscoring, (sub, 10, least), d_inc.view(nq, top, 3), nhits, aln, ops, cap, out=d_next)
                h_.search_pssm_top_stats_device(d_next, moffs, pscoring, top, 1, 0, out=h2, hist=hist2)
            legs[f"{name}_iteration"] = iteration
        alternate(legs)
        out[f"{P}_masked_over_plain_iteration"] = round(out[f"{P}_masked_iteration_ms"] / out[f"{P}_plain_iteration_ms"], 4)
        dbm.close()
        db.close()

    def pssm_weights_leg(packed, offs, nq=64, reps=7, per_hit=16):
        import time
        d_db = torch.from_numpy(packed.copy()).to(dev)
        db = eng.prepare_db(d_db, offs)
        qoffs = np.arange(nq + 1, dtype=np.int64) * args.qlen
        queries = rng.choice(PROTEIN, int(qoffs[-1])).astype(np.uint8)
        m, moffs = swamd.pssm_from_queries((queries, qoffs), sub, letters)
        d_m = torch.from_numpy(m.reshape(-1).copy()).to(dev)
        pscoring, update, weighting, cap = (letters, -4, 127, -11, -1), (sub, 10, 1), (per_hit, 1), 4 * args.qlen
        wupdate = (sub, 10 * per_hit, 1)                                     # N[j] counts in units of per_hit
        P = "pssm_weights"
        out[f"{P}_queries"], out[f"{P}_qlen"], out[f"{P}_targets"], out[f"{P}_reps"], out[f"{P}_ops_cap"], out[f"{P}_per_hit"] = nq, args.qlen, len(offs) - 1, reps, cap, per_hit
        for top in (10, 100, 4096):
            hits, nhits = db.search_pssm_top_device(d_m, moffs, pscoring, top, 1)
            aln, ops = db.align_pssm_hits_device(d_m, moffs, pscoring, hits, nhits, ops_cap=cap)
            d_out = torch.empty_like(d_m)
            d_w = torch.empty((nq, top), dtype=torch.int32, device=dev)
            h2 = (torch.zeros_like(hits), torch.zeros_like(nhits))
            state = {}

            def device_call():
                db.pssm_hit_weights_device(moffs, pscoring, weighting, hits, nhits, aln, ops, cap, out=d_w)

            def host_round_trip():
                h, n, a, o = hits.cpu().numpy(), nhits.cpu().numpy(), aln.cpu().numpy(), ops.cpu().numpy()
                state["w"] = swamd.pssm_hit_weights_host(moffs, (packed, offs), pscoring, weighting, h, n, a, o)
                state["d"] = torch.from_numpy(state["w"].reshape(-1)).to(dev)

            def update_alone():
                db.pssm_from_hits_device(d_m, moffs, pscoring, update, hits, nhits, aln, ops, cap, out=d_out)

            def iteration():
                db.align_pssm_hits_device(d_m, moffs, pscoring, hits, nhits, ops_cap=cap, out=(aln, ops))
                db.pssm_from_hits_device(d_m, moffs, pscoring, update, hits, nhits, aln, ops, cap, out=d_out)
                db.search_pssm_top_device(d_out, moffs, pscoring, top, 1, out=h2)

            def weighted_iteration():
                db.align_pssm_hits_device(d_m, moffs, pscoring, hits, nhits, ops_cap=cap, out=(aln, ops))
                db.pssm_hit_weights_device(moffs, pscoring, weighting, hits, nhits, aln, ops, cap, out=d_w)
                db.pssm_from_hits_device(d_m, moffs, pscoring, wupdate, hits, nhits, aln, ops, cap, weights=d_w, out=d_out)
                db.search_pssm_top_device(d_out, moffs, pscoring, top, 1, out=h2)

            def wall(fn):                                                    # wall clock around a synchronised call
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            legs = {"device_call": device_call, "host_round_trip": host_round_trip, "update_alone": update_alone, "iteration": iteration,
                    "weighted_iteration": weighted_iteration}
            for group in (("device_call", "update_alone", "host_round_trip"), ("iteration", "weighted_iteration")):
                ms = {k: [] for k in group}
                for k in group:
                    wall(legs[k])                                            # warm-up
                for _ in range(reps):                                        # alternating: a drift of the device shows in all alike
                    for k in group:
                        ms[k].append(wall(legs[k]))
                for k in group:
                    out[f"{P}_top{top}_{k}_ms"] = round(float(np.median(ms[k])), 4)
                    out[f"{P}_top{top}_{k}_range_ms"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
            d_w.fill_(0x55555555)
            device_call()
            torch.cuda.synchronize()
            w = d_w.cpu().numpy()
            out[f"{P}_top{top}_identical"] = bool(w.tobytes() == state["w"].tobytes())
            out[f"{P}_top{top}_launches"] = eng.get_option("last_pssm_weights_launches")
            out[f"{P}_top{top}_tiles_per_query"] = eng.get_option("last_pssm_weights_tiles")
            out[f"{P}_top{top}_informative"] = int((w > 0).sum())
            out[f"{P}_top{top}_weight_min_max"] = [int(w[w > 0].min()), int(w.max())] if (w > 0).any() else [0, 0]
            out[f"{P}_top{top}_host_over_device"] = round(out[f"{P}_top{top}_host_round_trip_ms"] / out[f"{P}_top{top}_device_call_ms"], 2)
            out[f"{P}_top{top}_device_over_update"] = round(out[f"{P}_top{top}_device_call_ms"] / out[f"{P}_top{top}_update_alone_ms"], 2)
            out[f"{P}_top{top}_weighted_over_unweighted"] = round(out[f"{P}_top{top}_weighted_iteration_ms"] / out[f"{P}_top{top}_iteration_ms"], 4)
        out[f"{P}_identical"] = all(out[f"{P}_top{t}_identical"] for t in (10, 100, 4096))
        db.close()

    def lanes_leg(packed, offs, nq=64, top=10):
        d_db = torch.from_numpy(packed.copy()).to(dev)
        db = eng.prepare_db(d_db, offs)
        nt = len(offs) - 1
        qoffs = np.arange(nq + 1, dtype=np.int64) * args.qlen
        d_q = torch.from_numpy(rng.choice(PROTEIN, int(qoffs[-1])).astype(np.uint8)).to(dev)
        scoring = (sub, -11, -1)
        cells = float(qoffs[-1]) * float(offs[-1] - offs[0])
        P = "lanes"
        out[f"{P}_queries"], out[f"{P}_qlen"], out[f"{P}_targets"], out[f"{P}_top"], out[f"{P}_cells"] = nq, args.qlen, nt, top, int(cells)
        tables = {lanes: torch.zeros(nq * nt * 3, dtype=torch.int64, device=dev) for lanes in (32, 16)}
        hits = {lanes: (torch.zeros(nq * top * 3, dtype=torch.int64, device=dev), torch.zeros(nq, dtype=torch.int64, device=dev)) for lanes in (32, 16)}

        def call(kind, lanes):
            eng.set_option("search_lanes", lanes)
            if kind == "search":
                db.search_affine_device(d_q, qoffs, scoring, out=tables[lanes])
            else:
                db.search_affine_top_device(d_q, qoffs, scoring, top, 0, out=hits[lanes])

        for kind in ("search", "top"):
            ms = {32: [], 16: []}
            for _ in range(max(1, args.warmup)):
                for lanes in (32, 16):
                    call(kind, lanes)
            torch.cuda.synchronize()
            for _ in range(args.reps):                                       # alternating: a drift of the device shows in both alike
                for lanes in (32, 16):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call(kind, lanes)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[lanes].append(e0.elapsed_time(e1))
                    out[f"{P}_{kind}{lanes}_launches"] = eng.get_option("last_search_multi_launches")
                    out[f"{P}_{kind}{lanes}_packed_launches"] = eng.get_option("last_search_multi_packed_launches")
            for lanes in (32, 16):
                med = float(np.median(ms[lanes]))
                out[f"{P}_{kind}{lanes}_ms"], out[f"{P}_{kind}{lanes}_range_ms"] = round(med, 3), [round(min(ms[lanes]), 3), round(max(ms[lanes]), 3)]
                out[f"{P}_{kind}{lanes}_gcups"] = round(cells / med / 1e6, 1)
            out[f"{P}_{kind}_16_over_32"] = round(out[f"{P}_{kind}16_ms"] / out[f"{P}_{kind}32_ms"], 4)
            out[f"{P}_{kind}_ranges_overlap"] = bool(out[f"{P}_{kind}16_range_ms"][1] >= out[f"{P}_{kind}32_range_ms"][0])
        eng.set_option("search_lanes", 32)
        torch.cuda.synchronize()
        out[f"{P}_identical"] = bool(torch.equal(tables[32], tables[16]) and torch.equal(hits[32][0], hits[16][0]) and torch.equal(hits[32][1], hits[16][1])
                                     and out[f"{P}_search16_packed_launches"] > 0 and out[f"{P}_search32_packed_launches"] == 0)
        db.close()

    def pairs_lanes_leg(packed, offs, nq=64, top=10, threshold=60, reps=7):
        d_db = torch.from_numpy(packed.copy()).to(dev)
        db = eng.prepare_db(d_db, offs)
        nt = len(offs) - 1
        lens = np.diff(offs)
        qoffs = np.arange(nq + 1, dtype=np.int64) * args.qlen
        d_q = torch.from_numpy(rng.choice(PROTEIN, int(qoffs[-1])).astype(np.uint8)).to(dev)
        scoring = (sub, -11, -1)
        prng = np.random.default_rng(7)                                      # (the generator and the draws of --pairs: its 1 % list and its full list)
        flat_sparse = prng.choice(nq * nt, nq * nt // 100, replace=False).astype(np.int64)
        flat_full = prng.permutation(nq * nt).astype(np.int64)
        flat_tenth = prng.choice(nq * nt, nq * nt // 10, replace=False).astype(np.int64)
        P = "pairs_lanes"
        out[f"{P}_queries"], out[f"{P}_qlen"], out[f"{P}_targets"], out[f"{P}_reps"] = nq, args.qlen, nt, reps

        def alternate(tag, call, cells=None):
            """Medians and ranges of `reps` calls per mode after a warm-up, the modes alternating: a drift of the device shows in both alike."""
            ms = {32: [], 16: []}
            for _ in range(max(1, args.warmup)):
                for lanes in (32, 16):
                    call(lanes)
            torch.cuda.synchronize()
            for _ in range(reps):
                for lanes in (32, 16):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call(lanes)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[lanes].append(e0.elapsed_time(e1))
                    out[f"{P}_{tag}{lanes}_launches"] = eng.get_option("last_search_pairs_launches")
                    out[f"{P}_{tag}{lanes}_packed_launches"] = eng.get_option("last_search_pairs_packed_launches")
                    out[f"{P}_{tag}{lanes}_packed_items"] = eng.get_option("last_search_pairs_packed_items")
            for lanes in (32, 16):
                med = float(np.median(ms[lanes]))
                out[f"{P}_{tag}{lanes}_ms"], out[f"{P}_{tag}{lanes}_range_ms"] = round(med, 3), [round(min(ms[lanes]), 3), round(max(ms[lanes]), 3)]
                if cells:
                    out[f"{P}_{tag}{lanes}_gcups"] = round(cells / med / 1e6, 1)
            out[f"{P}_{tag}_16_over_32"] = round(out[f"{P}_{tag}16_ms"] / out[f"{P}_{tag}32_ms"], 4)
            out[f"{P}_{tag}_ranges_disjoint_in_favour_of_16"] = bool(out[f"{P}_{tag}16_range_ms"][1] < out[f"{P}_{tag}32_range_ms"][0])
            return out[f"{P}_{tag}16_packed_launches"] > 0 and out[f"{P}_{tag}32_packed_launches"] == 0

        same = True
        for tag, flat in (("all", flat_full), ("tenth", flat_tenth), ("sparse", flat_sparse)):
            pairs = np.stack([flat // nt, flat % nt], axis=1)
            d_pairs = torch.from_numpy(pairs).to(dev)
            res = {lanes: torch.full((len(flat) * 3,), -1, dtype=torch.int64, device=dev) for lanes in (32, 16)}

            def call(lanes):
                eng.set_option("search_pairs_lanes", lanes)
                db.search_affine_pairs_device(d_q, qoffs, scoring, d_pairs, out=res[lanes])

            cells = float(args.qlen) * float(lens[pairs[:, 1]].sum())
            out[f"{P}_{tag}_n"], out[f"{P}_{tag}_cells"] = len(flat), int(cells)
            routed = alternate(tag, call, cells)
            out[f"{P}_{tag}_identical"] = bool(torch.equal(res[32], res[16]) and routed)
            same = same and out[f"{P}_{tag}_identical"]
            del d_pairs, res
        # the one-call pipeline: pre-filter, rescoring, selection
        cap = min(nq * nt, (eng.get_option("search_results_mib") << 20) // 56)
        hits = {lanes: (torch.zeros(nq * top * 3, dtype=torch.int64, device=dev), torch.zeros(nq, dtype=torch.int64, device=dev)) for lanes in (32, 16)}
        count = {}

        def one_call(lanes):
            eng.set_option("search_pairs_lanes", lanes)
            _, _, count[lanes] = db.search_affine_top_prefiltered_device(d_q, qoffs, scoring, threshold, cap, top, 0, out=hits[lanes])

        routed = alternate("one_call", one_call)
        eng.set_option("search_pairs_lanes", 32)
        torch.cuda.synchronize()
        out[f"{P}_one_call_threshold"], out[f"{P}_one_call_cap"], out[f"{P}_one_call_count"] = threshold, cap, int(count[16].item())
        out[f"{P}_one_call_identical"] = bool(torch.equal(hits[32][0], hits[16][0]) and torch.equal(hits[32][1], hits[16][1]) and int(count[32].item()) == int(count[16].item())
                                              and int(count[16].item()) <= cap and routed)
        out[f"{P}_identical"] = bool(same and out[f"{P}_one_call_identical"])
        db.close()

    def align_ckpt_leg(q, packed, offs, nq=64):
        d_db = torch.from_numpy(packed.copy()).to(dev)
        db = eng.prepare_db(d_db, offs)
        lens = np.diff(offs)
        longest = int(lens.max())
        scoring = (sub, -11, -1)
        out["ckpt_queries"], out["ckpt_qlen"] = nq, args.qlen
        # the hit table of 64 queries: one sw_db_align_affine_hits call per mode
        qoffs = np.arange(nq + 1, dtype=np.int64) * args.qlen
        d_qs = torch.from_numpy(rng.choice(PROTEIN, int(qoffs[-1])).astype(np.uint8)).to(dev)
        for top in (10, 100):
            tag = f"ckpt_hits_top{top}"
            d_hits, d_nhits = db.search_affine_top_device(d_qs, qoffs, scoring, top)
            cap = args.qlen + longest
            bufs = [(torch.zeros((nq * top, 7), dtype=torch.int64, device=dev), torch.zeros((nq * top, cap), dtype=torch.uint8, device=dev)) for _ in range(2)]
            for mode in (0, 1):
                db.align_affine_hits_device(d_qs, qoffs, scoring, d_hits, d_nhits, ops_cap=cap, out=bufs[mode], checkpoint=mode)
                out[f"{tag}_mode{mode}_slots"] = eng.get_option("last_align_hits_slots")
            out[f"{tag}_band_rows"] = eng.get_option("last_align_hits_band_rows")
            torch.cuda.synchronize()
            out[f"{tag}_identical"] = bool(torch.equal(bufs[0][0], bufs[1][0]) and torch.equal(bufs[0][1], bufs[1][1]))
            for mode in (0, 1):
                out[f"{tag}_mode{mode}_ms"], out[f"{tag}_mode{mode}_range_ms"] = spread(
                    lambda: db.align_affine_hits_device(d_qs, qoffs, scoring, d_hits, d_nhits, ops_cap=cap, out=bufs[mode], checkpoint=mode))
            out[f"{tag}_mode1_over_mode0"] = round(out[f"{tag}_mode1_ms"] / out[f"{tag}_mode0_ms"], 3)
            assert bool((d_nhits.cpu().numpy() == top).all()), "every row of the table was meant to be full"   # (no entry with target -1 below)
            out[f"{tag}_hit_len_mean"] = round(float(lens[d_hits.cpu().numpy()[..., 0]].mean()), 1)
        db.close()
        # the top hits of one query: sw_align_affine_device per mode, with the waves' tick stamps
        d_q = torch.from_numpy(q.copy()).to(dev)
        res = torch.zeros((len(offs) - 1, 3), dtype=torch.int64, device=dev)
        eng.search_affine_device(d_q, len(q), d_db, offs, sub, -11, -1, out=res)
        order = swamd.top_hits(res.cpu().numpy(), 1000)
        for k in (100, 1000):
            tag = f"ckpt_one_top{k}"
            hits = order[:k]
            cap = len(q) + int(lens[hits].max())
            bufs = [(torch.zeros((k, 7), dtype=torch.int64, device=dev), torch.zeros((k, cap), dtype=torch.uint8, device=dev)) for _ in range(2)]
            for mode in (0, 1):
                stamps = torch.zeros(3, dtype=torch.int64, device=dev)
                eng.set_option("debug_buf", stamps.data_ptr())
                eng.align_affine_device(d_q, len(q), d_db, offs, sub, -11, -1, hits, ops_cap=cap, out=bufs[mode], checkpoint=mode)
                torch.cuda.synchronize()
                eng.set_option("debug_buf", 0)
                t = [float(x) for x in stamps.cpu().numpy()]
                total = max(1.0, sum(t))
                out[f"{tag}_mode{mode}_slots"] = eng.get_option("last_align_affine_slots")
                out[f"{tag}_mode{mode}_slot_bytes"] = eng.get_option("last_align_affine_slot_bytes")
                if mode == 0:
                    out[f"{tag}_mode0_fill_share"], out[f"{tag}_mode0_walk_share"] = round(t[0] / total, 4), round(t[1] / total, 4)
                else:
                    out[f"{tag}_band_rows"] = eng.get_option("last_align_affine_band_rows")
                    out[f"{tag}_mode1_sweep_share"], out[f"{tag}_mode1_walk_share"], out[f"{tag}_mode1_refill_share"] = (round(x / total, 4) for x in t)
                out[f"{tag}_mode{mode}_wave_ticks"] = int(sum(t))
            out[f"{tag}_identical"] = bool(torch.equal(bufs[0][0], bufs[1][0]) and torch.equal(bufs[0][1], bufs[1][1]))
            for mode in (0, 1):
                out[f"{tag}_mode{mode}_ms"], out[f"{tag}_mode{mode}_range_ms"] = spread(
                    lambda: eng.align_affine_device(d_q, len(q), d_db, offs, sub, -11, -1, hits, ops_cap=cap, out=bufs[mode], checkpoint=mode))
            out[f"{tag}_mode1_over_mode0"] = round(out[f"{tag}_mode1_ms"] / out[f"{tag}_mode0_ms"], 3)
            out[f"{tag}_hit_len_mean"], out[f"{tag}_hit_len_max"] = round(float(lens[hits].mean()), 1), int(lens[hits].max())
            out[f"{tag}_ops_mean"] = round(float(bufs[1][0][:, 6].double().mean().item()), 1)

    # (a) protein database, log-normal lengths
    q = rng.choice(PROTEIN, args.qlen).astype(np.uint8)
    lens = np.clip(np.round(rng.lognormal(np.log(300), 0.6, args.targets)), 1, 35_000).astype(np.int64)
    offs = np.zeros(args.targets + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    packed = rng.choice(PROTEIN, int(offs[-1])).astype(np.uint8)
    out["a_letters"] = int(offs[-1])
    out["a_len_median"] = int(np.median(lens))
    out["a_len_max"] = int(lens.max())
    if args.multi or args.top or args.align_hits or args.pairs or args.prefilter or args.prefiltered_top or args.pssm or args.pssm_iterate or args.pssm_weights or args.msa or args.msa_filter or args.score_stats or args.mask or args.lanes or args.pairs_lanes:
        if args.mask:
            mask_leg(packed, offs)
        if args.score_stats:
            score_stats_leg(packed, offs)
        if args.lanes:
            lanes_leg(packed, offs)
        if args.pairs_lanes:
            pairs_lanes_leg(packed, offs)
        if args.pssm:
            pssm_leg(packed, offs)
        if args.pssm_iterate:
            pssm_iterate_leg(packed, offs)
        if args.pssm_weights:
            pssm_weights_leg(packed, offs)
        if args.msa:
            msa_leg(packed, offs)
        if args.msa_filter:
            msa_filter_leg(packed, offs)
        if args.pairs:
            pairs_leg(packed, offs)
        if args.prefilter:
            prefilter_leg(packed, offs)
        if args.prefiltered_top:
            prefiltered_top_leg(packed, offs)
        if args.multi:
            multi_legs(packed, offs)
        if args.align_hits and args.checkpoint:
            align_ckpt_leg(q, packed, offs)
        elif args.align_hits:
            align_hits_leg(packed, offs)
        if args.top:
            top_leg(packed, offs)
        eng.close()
        print(json.dumps(out))
        if args.lanes and not out["lanes_identical"]:
            sys.exit("bench_search.py --lanes: lanes_identical is false")
        if args.pairs_lanes and not out["pairs_lanes_identical"]:
            sys.exit("bench_search.py --pairs-lanes: pairs_lanes_identical is false")
        if args.pssm_iterate and not out["pssm_iterate_identical"]:
            sys.exit("bench_search.py --pssm-iterate: pssm_iterate_identical is false")
        if args.pssm_weights and not out["pssm_weights_identical"]:
            sys.exit("bench_search.py --pssm-weights: pssm_weights_identical is false")
        if args.msa and not out["msa_identical"]:
            sys.exit("bench_search.py --msa: msa_identical is false")
        if args.score_stats and not out["score_stats_identical"]:
            sys.exit("bench_search.py --score-stats: score_stats_identical is false")
        if args.mask and not out["mask_identical"]:
            sys.exit("bench_search.py --mask: mask_identical is false")
        if args.msa_filter and not out["msa_filter_identical"]:
            sys.exit("bench_search.py --msa-filter: msa_filter_identical is false")
        if args.pssm and not out["pssm_identical"]:
            sys.exit("bench_search.py --pssm: pssm_identical is false")
        if args.pairs:   # the required conditions of the pair-list call: a line that misses one is printed, and the run fails
            missed = [k for k in ("pairs_sparse_identical", "pairs_list_identical", "pairs_sparse_faster_than_full") if not out[k]]
            if missed:
                sys.exit("bench_search.py --pairs: " + ", ".join(missed) + " is false")
        if args.prefilter:   # the required conditions of the pre-filter: a line that misses one is printed, and the run fails
            missed = [k for k in ("prefilter_chain_identical", "prefilter_u_le_max_score_all_pairs", "prefilter_kernels_identical", "prefilter_lanes32_count_ok",
                                  "prefilter_packed_count_ok", "prefilter_lanes32_faster_than_full", "prefilter_packed_faster_than_full") if not out[k]]
            if missed:
                sys.exit("bench_search.py --prefilter: " + ", ".join(missed) + " is false")
        if args.prefiltered_top:   # the required conditions of the selection from the list: a line that misses one is printed, and the run fails
            missed = [k for k in ("prefiltered_top_chain_equals_one_call", "prefiltered_top_chain_equals_masked_table", "prefiltered_top_one_call_equals_masked_table",
                                  "prefiltered_top_select_equals_masked_table", "prefiltered_top_low_select_equals_masked_table", "prefiltered_top_count_within_cap",
                                  "prefiltered_top_one_call_faster_than_full") if not out[k]]
            if missed:
                sys.exit("bench_search.py --prefiltered-top: " + ", ".join(missed) + " is false")
        return
    search_gcups(q, packed, offs, "a")
    align_legs(q, packed, offs, affine_gcups(q, packed, offs, "a"), "a")
    if args.only_a:
        eng.close()
        print(json.dumps(out))
        return
    # (b) the same cells, equal lengths
    L = int(round(offs[-1] / args.targets))
    offs_b = np.arange(args.targets + 1, dtype=np.int64) * L
    packed_b = rng.choice(PROTEIN, int(offs_b[-1])).astype(np.uint8)
    out["b_len"] = L
    search_gcups(q, packed_b, offs_b, "b")
    affine_gcups(q, packed_b, offs_b, "b")
    # (c) 4-letter 1024^2: search against the batch kernel on the same data
    qc = rng.choice(DNA, 1024).astype(np.uint8)
    bc = rng.choice(DNA, (args.pairs_c, 1024)).astype(np.uint8)
    rs = search_gcups(qc, bc.reshape(-1), np.arange(args.pairs_c + 1, dtype=np.int64) * 1024, "c_search")
    rb = batch_gcups(qc, bc, "c_batch", args.reps)
    out["c_identical"] = bool(torch.equal(rs, rb))
    # (d) protein equal-length data through sw_batch_device (more than 8 letters: the single-pair path)
    bd = packed_b[: args.pairs_d * L].reshape(args.pairs_d, L)
    batch_gcups(q, bd, "d_batch", 1)
    out["a_over_b"] = round(out["a_gcups"] / out["b_gcups"], 3)
    out["c_search_over_batch"] = round(out["c_search_gcups"] / out["c_batch_gcups"], 3)
    out["a_over_d"] = round(out["a_gcups"] / out["d_batch_gcups"], 2)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
