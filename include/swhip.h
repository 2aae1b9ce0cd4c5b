/*
 * swhip.h -- C-ABI of the MI355X-native Smith-Waterman DP-fill engine (libswhip.so).
 *
 * Drop-in boundary for the reference's hot path.  The reference has no
 * FFI; each entry point below names the reference code it replaces (paths relative to the
 * reference repository root).  Plain pointers and sizes only; no torch / C++ types.
 *
 * Conventions
 *   - every function returns 0 on success, a negative SW_E* code on failure, never exit()s
 *     (the reference's CUDA path prints and exit(0)s, simple-cuda/sw-default-discrete.cu:101-108);
 *     sw_last_error() returns a thread-local description of the last failure.
 *   - cols = len(a) = matrix columns, rows = len(b) = matrix rows (serial_smithW.c:72-77);
 *     H and P are (rows+1) x (cols+1), row-major, row stride cols+1 (serial_smithW.c:192).
 *   - "d_" pointers are DEVICE (HBM) pointers, everything else is host memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Every launch, memset and copy of a call goes to that
 *     stream, behind the previous call of the device (see sw_ctx).  That holds for the fills and for every search, selection and
 *     alignment call alike (every call below that takes a `stream`: the sw_*_device calls and the searches, selections, pre-filter and
 *     alignments of a sw_db; not sw_db_create, sw_db_free or sw_db_info, which enqueue nothing): a context's calls share its pinned
 *     staging copies and device workspaces, so a call enqueued on another stream than the device's previous call first waits, on the
 *     device, for that call.  Calls of one context may therefore follow each other on any streams without a synchronisation in between.
 *     "Asynchronous, no host round trip" has a bound: before it rewrites the pinned copies a call waits on the host for the previous
 *     call's uploads to have left them, and those are ordered behind the call before that one, so the host runs about two calls ahead
 *     of the device, not more; where a workspace has to grow, the call also waits for the stream.
 *   - WRITE extents.  A call writes the outputs it documents and nothing else of the caller's: exactly (rows+1) x (cols+1) elements of
 *     d_H / d_P (a tile: its own rectangle inside the row stride), one sw_result / sw_alignment per problem, the documented number of
 *     granules, flags, path entries and op bytes.  Outputs need no initialisation and no particular alignment beyond that of their
 *     element type (d_H: 4 or 8 bytes, int32 d_P: 4, int8 d_P: any address, sw_result / sw_alignment / granules: 8); base addresses
 *     that are not 8-byte aligned (16 for an int64 d_H) only cost the whole-line stores of the widest fills.
 *   - READ extents, from the kernels' loads.  Input sequences need no alignment except d_b of the fills and batches (16 bytes, below).
 *     sw_batch_device*, sw_search_device, sw_search_affine_device, sw_db_search_affine and sw_align_affine_device read no byte outside
 *     [d_a + k*a_stride, + cols), [d_b + k*b_stride, + rows), [d_query, + qlen) and [d_db + offsets[0], d_db + offsets[ntargets]): the
 *     gaps of padded strides and the bytes around the query and the database are never loaded.  sw_fill_device, sw_fill_device_ex and
 *     sw_fill_band_device read a and b, and besides them at most the rest of the 16-byte ALIGNED windows that hold the first and the last
 *     byte of a, and the last byte of b (their alphabet scan loads whole aligned windows and masks out what is not sequence): up to 15
 *     bytes in front of d_a, up to 15 behind a and up to 15 behind b, none of which can cross a page or leave an allocation, and none of
 *     which influences a result.  sw_fill_tile_device reads its a and b bytes only.  (The Python wrapper's to_device keeps 16 spare
 *     bytes behind a sequence, more than that.)  tests/test_buffer_contract_gpu.py surrounds every input with letters that would raise
 *     the scores if they were taken for sequence data: it proves that results do not depend on those bytes, not that they are never read.
 */
#ifndef SWHIP_H
#define SWHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SW_OK 0
#define SW_EINVAL (-22)   /* bad argument */
#define SW_ENOMEM (-12)   /* host or device allocation failed */
#define SW_EDEVICE (-5)   /* HIP runtime error */
#define SW_ETIMEOUT (-62) /* an in-kernel hand-off wait gave up (never expected) */
#define SW_ENODEV (-19)   /* no usable GPU */

/* predecessor codes, serial_smithW.c:23-27 */
#define SW_PATH (-1)
#define SW_NONE 0
#define SW_UP 1
#define SW_LEFT 2
#define SW_DIAGONAL 3

/* serial_smithW.c:59-61 (matchScore, missmatchScore, gapScore); default {3,-3,-2}. gap must be <= 0. */
typedef struct { int32_t match, mismatch, gap; } sw_scores;

/* max_pos: linear index rows-major of the arg-max cell, lowest index among ties, 0 if H == 0
 * everywhere (what the scan at serial_smithW.c:240-242 yields); max_score = H[max_pos];
 * path_len: cells negated by the traceback (0 until a traceback ran). */
typedef struct { int64_t max_pos; int64_t max_score; int64_t path_len; } sw_result;

/* One per GPU; one host thread drives a ctx at a time.  Fills of one DEVICE are serialised by the library (a fill's
 * workgroups wait for each other, so two fills must not share the CUs): a fill enqueued on another stream than the
 * previous fill of that device first waits, on the device, for that stream.  The search, selection and alignment calls take
 * the same turn (their workspaces are shared between the families of a context).  Contexts of different devices are
 * independent. */
typedef struct sw_ctx sw_ctx;

const char* sw_last_error(void);
const char* sw_version(void);

/* ---- input side ---------------------------------------------------------------------------
 * sw_generate: replaces generate(), serial_smithW.c:334-361, bit-exact incl. its draw order
 * (cols+1 rand() draws for a, then rows+1 for b; glibc TYPE_3 rand() restated, no libc state).
 * seed 1 == serial_smithW.c (which never calls srand).  a holds cols+1 bytes, b rows+1. */
int sw_generate(int64_t cols, int64_t rows, uint32_t seed, char* a, char* b);

/* FASTA input, the step before the path for real sequences (the reference only has
 * generate()).  Reads record `record` (0-based) of the file: '>' starts a record, ';' lines are comments,
 * white space is dropped, letters are upper-cased; a file without '>' is one record.  *len receives the
 * sequence length; seq (may be NULL to query the length) receives at most cap bytes, no terminator. */
int sw_read_fasta(const char* path, int64_t record, char* seq, int64_t cap, int64_t* len);

/* ---- wavefront indexing: nElement / calcFirstDiagElement, omp_smithW.c:260-275, 282-291.
 * m, n are the padded sizes (cols+1, rows+1); i in [1, m+n-3]. */
int64_t sw_nelement(int64_t i, int64_t m, int64_t n);
void sw_first_diag_element(int64_t i, int64_t m, int64_t n, int64_t* si, int64_t* sj);

/* ---- context ------------------------------------------------------------------------------ */
int sw_create(int device, sw_ctx** out);
void sw_destroy(sw_ctx* ctx);

/* ---- the hot path ---------------------------------------------------------------------------
 * sw_fill_device: replaces the fill loop + similarityScore/matchMissmatchScore
 * (serial_smithW.c:141-145, 187-256; omp_smithW.c:203-216) and the rotated family's
 * smithWaterman(a,b,w,h,H,P,&maxloc) (rotated-cuda/sw-rotated-omp.cc:192-209).
 * Asynchronous on `stream`.  d_H/d_P need not be initialised (row 0 / column 0 are written).  d_b must be 16-byte aligned
 * (SW_EINVAL otherwise); d_a may start anywhere.
 *   h_elem_bytes : 4 -> d_H is int32_t*, 8 -> d_H is int64_t* (same values, widened)
 *   d_top        : optional (may be NULL) int32 H values of the row above this band, cols+1
 *                  entries (multi-GPU row bands); NULL == zeros (a whole matrix)
 *   d_result     : device sw_result; max_pos/max_score valid when the stream has drained
 * Placement: H[r][c] and P[r][c] are written within a fraction of a microsecond of each other; when both buffers were
 * mapped to the same class of the physical HBM (the usual outcome of two back-to-back hipMallocs) a 16384^2 fill takes
 * 1.05 ms instead of 0.79 ms on MI355X.  sw_alloc_outputs() below hands out a pair that avoids it.  Results do not depend on it. */
int sw_fill_device(sw_ctx* ctx, const char* d_a, int64_t cols, const char* d_b, int64_t rows,
                   const sw_scores* scores, void* d_H, int h_elem_bytes, int32_t* d_P,
                   const int32_t* d_top, sw_result* d_result, void* stream);

/* Same with a compact predecessor matrix and/or without one of the matrices (the rolling-buffer
 * variants of the reference, rotated-cuda/sw-rotated-omp.cc:214-224, likewise keep only what the caller asks for):
 *   p_elem_bytes 4 -> d_P is int32_t* (identical to sw_fill_device), 1 -> d_P is int8_t* holding the same codes
 *                (0..3; -1..-3 after a traceback): a quarter of the P traffic and footprint;
 *   d_H == NULL  -> H is not written ("P-only": 1 or 4 B/cell, enough for the traceback);
 *   d_P == NULL  -> P is not written; both NULL = score-only.
 * max_pos / max_score are exact in every mode.  Systolic engine only. */
int sw_fill_device_ex(sw_ctx* ctx, const char* d_a, int64_t cols, const char* d_b, int64_t rows,
                      const sw_scores* scores, void* d_H, int h_elem_bytes, void* d_P, int p_elem_bytes,
                      const int32_t* d_top, sw_result* d_result, void* stream);

/* Tile of a bigger matrix (multi-GPU row bands x column chunks).  d_H / d_P point at the
 * tile's corner cell (row above / column left of its first cell) inside matrices of row stride
 * `row_stride` elements; d_top: cols+1 H values of the row above (NULL = zeros), d_left: rows+1 H values
 * of the column to the left (NULL = zeros; d_left[0] is the corner), d_right (optional): receives the
 * rows+1 H values of the tile's last column = the next tile's d_left.  The tile's last row is the next
 * band's d_top.  d_result->max_pos is relative to the corner with the full row stride.
 * Row 0 of the tile belongs to the neighbour above when d_top is given, column 0 to the neighbour on the left when d_left is given:
 * such a row / column is not written, neither in H nor in P (the caller's matrix holds the neighbour's values there already; d_top /
 * d_left carry them to the kernel).  Without d_top row 0, without d_left column 0 is the tile's own and is written: H = 0, P = 0.
 * Nothing outside the (rows+1) x (cols+1) rectangle at the corner is written.  A tile with d_top needs the systolic engine. */
int sw_fill_tile_device(sw_ctx* ctx, const char* d_a, int64_t cols, const char* d_b, int64_t rows,
                        const sw_scores* scores, void* d_H, int h_elem_bytes, int32_t* d_P, int64_t row_stride,
                        const int32_t* d_top, const int32_t* d_left, int32_t* d_right, sw_result* d_result,
                        void* stream);

/* One ROW BAND of a bigger (total_rows+1) x (cols+1) matrix as ONE persistent launch: the multi-GPU decomposition of
 * SURVEY.md 8e (the reference has no multi-GPU code; the order preserved is omp_smithW.c:203-216).  The band's halo
 * row arrives and its last row leaves as 8-byte granules  (uint64)tag << 32 | (uint32)H  , one per column, WHILE the
 * kernel runs: a strip starts as soon as its 64 granules of the row above carry `top_tag`, so the launch can be
 * enqueued before the band above has produced anything, and whoever moves the halo (RCCL recv, a copy, a peer store)
 * may deliver it in any order and chunking -- the data is its own flag.
 *   d_H, d_P      : band-local (rows+1) x (cols+1) storage; row 0 is the halo row (H written, P left alone).  Either
 *                   may be NULL (not written), p_elem_bytes 4 or 1 as in sw_fill_device_ex
 *   d_top_gran    : cols+1 granules of the row above, or NULL for the first band (zeros)
 *   d_bot_gran    : receives cols+1 granules of the band's last row (tag = bot_tag), or NULL
 *   d_bot_done    : optional, one uint32 per 63-column strip (ceil(cols/63)), may be host-pinned memory: set to bot_tag,
 *                   system scope, after the strip's granules were released -- lets a host thread forward finished chunks
 *   tags          : non-zero, and different from what the buffers held before (e.g. a per-fill counter)
 *   reserve_cus   : CUs the launch leaves free for other kernels (halo transfers); 0 = use all
 *   concurrent    : non-zero = do not order this launch behind fills on other streams of the device (the caller keeps
 *                   the sum of the grids within the CUs, option "max_blocks")
 *   d_result      : band-local arg-max (max_pos relative to the band's row 0, stride cols+1)
 * total_rows bounds the scores a halo can carry (range check).  Patience of the halo poll: option "band_wait_ms". */
int sw_fill_band_device(sw_ctx* ctx, const char* d_a, int64_t cols, const char* d_b, int64_t rows, int64_t total_rows,
                        const sw_scores* scores, void* d_H, int h_elem_bytes, void* d_P, int p_elem_bytes,
                        const uint64_t* d_top_gran, uint32_t top_tag, uint64_t* d_bot_gran, uint32_t bot_tag,
                        uint32_t* d_bot_done, int reserve_cus, int concurrent, sw_result* d_result, void* stream);

/* ---- one matrix over several GPUs of ONE process (one process per GPU: smith-waterman_amd/multi.py) ----
 * Row bands, one per entry of `devices` (an id may repeat: the bands then share that GPU's CUs), every band one
 * band-resident launch, all launched at once; finished column chunks of a band's last row are forwarded to the next
 * band with peer copies over xGMI while the kernels run.  a, b: HOST sequences.
 *   sw_multi_create    allocates the band-local matrices (H int32 unless want_h == 0; P int32 or int8)
 *   sw_multi_fill      one fill of the whole matrix (blocking); result: global arg-max by the serial rule
 *   sw_multi_traceback backtrack() across the bands (negates P along the path), total path length
 *   sw_multi_band_info device, rows (lo, hi] and device pointers of band g (band-local (hi-lo+1) x (cols+1), row 0 = halo) */
typedef struct sw_multi sw_multi;
int sw_multi_create(const int* devices, int ndev, const char* a, int64_t cols, const char* b, int64_t rows,
                    int p_elem_bytes, int want_h, sw_multi** out);
int sw_multi_fill(sw_multi* m, const sw_scores* scores, int nchunks, sw_result* result);
int sw_multi_traceback(sw_multi* m, int64_t* path_len);
int sw_multi_band_info(sw_multi* m, int g, int* device, int64_t* row_lo, int64_t* row_hi, void** d_H, void** d_P);
int sw_multi_nbands(sw_multi* m);
double sw_multi_seconds(sw_multi* m);   /* wall time of the last sw_multi_fill */
void sw_multi_free(sw_multi* m);

/* Batch of npairs independent cols x rows problems (BASELINE config 5; the reference handles one pair per process,
 * serial_smithW.c:141-145 per pair).  Runs on the one-pair-per-wave kernel (csrc/sw_batch.hip) when the batch has at most 8
 * distinct letters and the scores fit a signed byte -- the letter count is read back once per call, the one host round trip --
 * and on the single-pair machinery otherwise; results are identical.  Pair k reads a at
 * d_a + k*a_stride and b at d_b + k*b_stride (b_stride a multiple of 16), writes d_results[k] (exact arg-max in
 * every mode) and, where given, its matrices at element offset k*(rows+1)*(cols+1).  d_H and/or d_P may be NULL.  a_stride >= cols and
 * b_stride >= rows may leave gaps between the pairs: the gaps are not read, whatever they hold.  d_b must be 16-byte aligned. */
int sw_batch_device(sw_ctx* ctx, const char* d_a, int64_t a_stride, int64_t cols, const char* d_b, int64_t b_stride,
                    int64_t rows, int64_t npairs, const sw_scores* scores, int32_t* d_H, int32_t* d_P,
                    sw_result* d_results, void* stream);
/* the same with a compact predecessor matrix: p_elem_bytes 1 -> d_P is int8_t* (100 000 x 1025^2 codes = 105 GB) */
int sw_batch_device_ex(sw_ctx* ctx, const char* d_a, int64_t a_stride, int64_t cols, const char* d_b, int64_t b_stride,
                       int64_t rows, int64_t npairs, const sw_scores* scores, int32_t* d_H, void* d_P, int p_elem_bytes,
                       sw_result* d_results, void* stream);
/* backtrack() (serial_smithW.c:262-277) of every pair of a batch: walks pair k's P from d_results[k].max_pos, negates
 * the path, sets d_results[k].path_len; d_paths (optional, npairs x path_cap) receives the visited pair-local indices. */
int sw_batch_traceback_device(sw_ctx* ctx, void* d_P, int p_elem_bytes, int64_t cols, int64_t rows, int64_t npairs,
                              int64_t* d_paths, int64_t path_cap, sw_result* d_results, void* stream);

/* Database search: one query against ntargets sequences of different lengths.  For every target k the reference fill
 * (serial_smithW.c:141-145 for the set-up, 187-256 for the cells: similarityScore + matchMissmatchScore, maxPos by the serial
 * scan's rule) of a = query (cols = qlen), b = target k (rows = its length), score and arg-max only -- what the reference computes
 * per pair, without H and P.
 *   d_query      : device, qlen >= 1 bytes
 *   d_db         : device, the targets back to back; target k = d_db[offsets[k] .. offsets[k+1]), no alignment asked
 *   offsets      : HOST, ntargets + 1 non-decreasing int64 (offsets[0] may be > 0; empty targets allowed); the library
 *                  copies what it needs before returning, so the array may be reused at once.  Here and in every call of the
 *                  search family each offset, count, cap and stride is used as a 64-bit quantity end to end -- on the host, in the
 *                  kernels' addresses and in the workspaces -- and placement beyond 4 GiB is tested (tests/test_far_gpu.py)
 *   d_results    : device, ntargets sw_result in INPUT order: max_score, max_pos = r*(qlen+1)+c in target k's own
 *                  (len_k+1) x (qlen+1) matrix, lowest index among ties, 0 if no cell is positive; path_len = 0
 * Any byte value is a letter (bytes compared as in matchMissmatchScore, serial_smithW.c:251-256).  Asynchronous on
 * `stream`.  Results identical to sw_fill_device(query, target k) for every k.  SW_EINVAL for decreasing offsets, qlen < 1,
 * qlen or a target length above 2^20 - 1, scores the fill would reject for (qlen, longest target), NULL pointers.
 * Runs on csrc/sw_search.hip (targets scheduled longest first over persistent waves; a re-fill of a chosen hit with
 * sw_fill_device + sw_traceback_device gives its path). */
int sw_search_device(sw_ctx* ctx, const char* d_query, int64_t qlen, const char* d_db, const int64_t* offsets,
                     int64_t ntargets, const sw_scores* scores, sw_result* d_results, void* stream);

/* Database search with a substitution matrix and affine gaps (csrc/sw_search_affine.hip): what protein searches use.
 * sw_submat: s[x][y] = score of query byte x against target byte y (any byte value is a letter; the table need not be symmetric).
 * sw_affine: gap_open <= 0 and gap_extend <= 0; a gap of k letters scores gap_open + k * gap_extend.  Per target, with q the query
 * (columns j), t the target (rows i), go = gap_open, ge = gap_extend:
 *   H[0][j] = H[i][0] = 0, E[0][j] = F[i][0] = -inf
 *   E[i][j] = max(E[i-1][j], H[i-1][j] + go) + ge            (a gap that consumes target letters)
 *   F[i][j] = max(F[i][j-1], H[i][j-1] + go) + ge            (a gap that consumes query letters)
 *   H[i][j] = max(0, H[i-1][j-1] + s[q[j-1]][t[i-1]], E[i][j], F[i][j])
 * d_results[k] = {max_pos, max_score, 0} by the rule and layout of sw_search_device: max_score = max H, max_pos = the lowest
 * i*(qlen+1)+j that holds it, 0 if no cell is positive; empty targets give {0,0,0}; input order.  With gap_open = 0 and the table
 * of sw_submat_match(match, mismatch) the results are those of sw_search_device for {match, mismatch, gap_extend}, bit for bit.
 * d_query, d_db, offsets, d_results, stream: as for sw_search_device.  The table is HOST memory, copied before the call returns.
 * SW_EINVAL for NULL pointers, the offsets / length errors of sw_search_device, gap_open > 0 or gap_extend > 0,
 * gap_open + gap_extend < -2^24, and max(largest table entry, 0) * min(qlen, longest target) >= 2^24 (the 24-bit score of the
 * arg-max key).  Score and end cell only; the alignment PATH of chosen hits comes from sw_align_affine_device below, which re-fills
 * them with the same recurrence while it records directions.
 * sw_search_affine_host: the same computation in plain C++ on host memory, no GPU needed (the CPU leg). */
typedef struct { int8_t s[256][256]; } sw_submat;
typedef struct { const sw_submat* sub; int32_t gap_open, gap_extend; } sw_affine;
int sw_search_affine_device(sw_ctx* ctx, const char* d_query, int64_t qlen, const char* d_db, const int64_t* offsets,
                            int64_t ntargets, const sw_affine* scoring, sw_result* d_results, void* stream);
int sw_search_affine_host(const char* query, int64_t qlen, const char* db, const int64_t* offsets, int64_t ntargets,
                          const sw_affine* scoring, sw_result* results);
/* The alignment of chosen hits under affine scoring (csrc/sw_align_affine.hip): Gotoh's recurrence with one direction byte per cell
 * and a walk through its three states.  H, E, F, go, ge, s, rows i (target letters) and columns j (query letters) as above.
 * THE CANONICAL ALIGNMENT of a target.  The walk starts at max_pos (the arg-max of sw_search_affine_device: lowest index among
 * ties) in state H.
 *   State H at (i, j): if H[i][j] == 0, stop -- this cell is the begin corner and not part of the alignment.  Else if
 *     H[i][j] == H[i-1][j-1] + s[q[j-1]][t[i-1]]: emit M, go to H at (i-1, j-1).  Else if H[i][j] == E[i][j]: go to state E at the
 *     same cell, nothing emitted.  Else go to state F at the same cell.  (Tie order diagonal, E, F: the reference's
 *     DIAGONAL > UP > LEFT, serial_smithW.c:221-234.)
 *   State E at (i, j), a gap that consumes target letters: emit D; if E[i][j] == H[i-1][j] + go + ge (opening wins a tie against
 *     extending) go to H at (i-1, j), otherwise stay in E at (i-1, j).
 *   State F at (i, j), a gap that consumes query letters: emit I; if F[i][j] == H[i][j-1] + go + ge go to H at (i, j-1), otherwise
 *     stay in F at (i, j-1).
 * Ops are reported in alignment order, begin to end, one byte each: 'M' (a letter pair, match or mismatch), 'I', 'D'.  With the
 * begin corner (i0, j0) and the end cell (i1, j1) the alignment covers query [j0, j1) and target [i0, i1), 0-based, half open:
 * sw_alignment = {max_pos, max_score, q_begin = j0, t_begin = i0, q_end = j1, t_end = i1, nops}.  A target with nothing positive
 * gives the empty alignment: all zeros, no ops.  The rule makes the alignment unique.  With go = 0 and the table of sw_submat_match
 * the cells visited in state H are backtrack()'s path (serial_smithW.c:262-277) for {match, mismatch, ge}, in the same order.
 *   hits   : HOST, nhits target indices in [0, ntargets), in any order, duplicates allowed; copied before the call returns
 *   d_aln  : device, nhits sw_alignment in the order of `hits`; max_pos / max_score of hit h are what sw_search_affine_device
 *            reports for target hits[h] (the call re-fills every hit in full and finds the arg-max itself: it does not take the
 *            search's results, and stays asynchronous on `stream` without a host round trip)
 *   d_ops  : device, nhits rows of ops_cap bytes: the ops of hit h at d_ops + h * ops_cap, left-justified.  nops is always the true
 *            length; where nops > ops_cap that hit's op bytes are unspecified, and nothing is written outside its own row.
 *            ops_cap >= qlen + longest hit always suffices.  d_ops may be NULL with ops_cap 0: coordinates only.
 * nhits == 0 returns SW_OK and launches nothing.  SW_EINVAL: the argument errors of sw_search_affine_device, an index out of range,
 * NULL hits with nhits > 0, NULL d_aln, a negative ops_cap (or NULL d_ops with ops_cap > 0).  The directions take one byte per cell
 * of a re-filled matrix (longest hit x padded query length per slot) in a per-context workspace that the option
 * "align_workspace_mib" bounds (default 1024): a hit whose own matrix does not fit is SW_EINVAL with a message that names the
 * option; more hits than slots fit are processed slot after slot inside the one call.
 * Under "align_checkpoint" = 1, and under 2 for exactly the calls refused above, a slot holds one band of rows and a checkpoint row
 * per band instead (see sw_set_option): the same sw_alignment and ops byte for byte, and a hit is refused only if that slot -- a few
 * MB for a million rows -- does not fit "align_workspace_mib".  The argument rules stay: a target has at most 2^20 - 1 letters.
 * sw_align_affine_host: the same in plain C++ on host memory (the CPU leg; no workspace bound). */
typedef struct { int64_t max_pos, max_score, q_begin, t_begin, q_end, t_end, nops; } sw_alignment;
int sw_align_affine_device(sw_ctx* ctx, const char* d_query, int64_t qlen, const char* d_db, const int64_t* offsets,
                           int64_t ntargets, const int64_t* hits, int64_t nhits, const sw_affine* scoring,
                           sw_alignment* d_aln, char* d_ops, int64_t ops_cap, void* stream);
int sw_align_affine_host(const char* query, int64_t qlen, const char* db, const int64_t* offsets, int64_t ntargets,
                         const int64_t* hits, int64_t nhits, const sw_affine* scoring,
                         sw_alignment* aln, char* ops, int64_t ops_cap);
/* A prepared database and the search of MANY queries against it (csrc/sw_search_multi.hip).  sw_search_affine_device checks the offsets,
 * sorts the target lengths and builds its schedule anew for every query; a handle does that once, and one call then runs every
 * (query, target) pair of a set of queries from one work counter per launch -- short queries and small databases fill the device together.
 *   sw_db_create  d_db and offsets as for sw_search_device: device bytes back to back, a HOST array of ntargets + 1 non-decreasing
 *                 offsets (offsets[0] may be > 0, empty targets allowed), copied as far as needed.  The handle BORROWS d_db: the caller
 *                 keeps it alive and unchanged until sw_db_free.  The handle owns the schedule on the device (24 bytes per non-empty
 *                 target) and a copy of the ntargets + 1 offsets there (8 bytes per target; the schedule is ordered by length, and
 *                 sw_db_align_affine_hits has to get from a target index to its bytes).  Synchronous.  ntargets == 0 gives a valid,
 *                 empty handle.  SW_EINVAL: NULL pointers, ntargets < 0, the offsets / length errors of sw_search_device.  Free the
 *                 handle before the context's device is reset.
 *   sw_db_info    every out pointer is optional: targets, non-empty targets, the longest target, offsets[ntargets] - offsets[0].
 *   sw_db_search_affine
 *     d_queries : device, the queries back to back: query q = d_queries[qoffsets[q] .. qoffsets[q+1]), no alignment asked
 *     qoffsets  : HOST, nqueries + 1 non-decreasing int64, qoffsets[0] >= 0; copied before the call returns
 *     d_results : device, QUERY-MAJOR, nqueries x ntargets sw_result: d_results[q * ntargets + k] is bit for bit what
 *                 sw_search_affine_device writes for query q and target k -- the recurrence, the arg-max rule, max_pos in that pair's own
 *                 (len_k + 1) x (qlen_q + 1) layout, {0, 0, 0} for empty targets.  Every entry is written.
 *     Asynchronous on `stream`, no host round trip; the table is HOST memory, copied before the call returns.  The host work of a call
 *     is O(nqueries): it never reads the targets' offsets again and never sorts.  Linear gaps: pass sw_submat_match's table with
 *     gap_open = 0, which equals sw_search_device bit for bit (above).  The queries' profiles (257 x padded length bytes each) share a
 *     per-context workspace that the option "search_profile_mib" bounds (default 256, at least 1): queries are taken in consecutive
 *     groups that fit it, and a query whose own profile exceeds it runs as a group of its own -- the option refuses nothing.
 *     SW_EINVAL: NULL pointers, nqueries < 0, decreasing qoffsets or qoffsets[0] < 0, a query of length 0 or above 2^20 - 1, the
 *     scoring errors of sw_search_affine_device with the 24-bit bound taken over the LONGEST query, a handle created on another
 *     context's device.  nqueries == 0 returns SW_OK and launches nothing; a handle without a non-empty target only zeroes the results.
 *     LANES.  The option "search_lanes" (32, the default, or 16) chooses the kernel of this call, of sw_db_search_affine_top and of
 *     their PSSM twins; every byte they write is the same under both.  Under 32 a wave scores one target on 32-bit lanes.  Under 16 a
 *     wave scores TWO targets of one query on packed 16-bit lanes, for every query with
 *         max(max_entry, 0) x min(its length, the handle's longest target) <= 32767
 *     (max_entry: the table's largest entry; for the PSSM calls smax), provided that, for the whole call,
 *         gap_open + 2 gap_extend >= -32768;
 *     a query outside the rule runs on 32-bit lanes inside the same call, and refusals, workspaces, groups and chunks do not depend
 *     on the option.  "last_search_multi_packed_launches" counts the packed launches among the "last_search_multi_launches" of the
 *     last such call: 0 after any call under 32 and after a call that launched nothing.
 *   sw_search_affine_multi_host  the CPU leg: sw_search_affine_host query after query, the same result layout, no GPU needed; every
 *     argument is checked before the first query runs. */
typedef struct sw_db sw_db;
int  sw_db_create(sw_ctx* ctx, const char* d_db, const int64_t* offsets, int64_t ntargets, sw_db** out);
void sw_db_free(sw_db* db);
int  sw_db_info(const sw_db* db, int64_t* ntargets, int64_t* nonempty, int64_t* longest, int64_t* letters);
int  sw_db_search_affine(sw_ctx* ctx, const sw_db* db, const char* d_queries, const int64_t* qoffsets, int64_t nqueries,
                         const sw_affine* scoring, sw_result* d_results, void* stream);
int  sw_search_affine_multi_host(const char* queries, const int64_t* qoffsets, int64_t nqueries, const char* db,
                                 const int64_t* offsets, int64_t ntargets, const sw_affine* scoring, sw_result* results);

/* The best targets of every query, selected on the device (csrc/sw_search_top.hip).  A caller of sw_db_search_affine wants the best few
 * targets per query, not nqueries x ntargets results of 24 bytes; these calls deliver nqueries x top hits.
 *   d_hits  : device, nqueries x top sw_hit = {target, max_pos, max_score}.  Row q holds the hits of query q in RANK ORDER: max_score
 *             descending, then target ascending.  max_pos and max_score of a hit are bit for bit what sw_db_search_affine writes for
 *             that (query, target) pair.
 *   min_score : only targets with max_score >= min_score qualify; with min_score <= 0 every target does, empty ones included, with their
 *             {target, 0, 0}.
 *   d_nhits : device, nqueries int64: d_nhits[q] = min(top, qualifying targets of query q).  The remaining entries of row q are
 *             {-1, 0, 0}.
 * Every entry of d_hits and d_nhits is written and nothing outside them.  The result is unique: the rank order leaves no choice, and
 * no run differs from another although the selection counts and gathers with atomics.  Asynchronous on `stream`, no host round trip;
 * the host work of a call is O(nqueries).
 *   sw_top_hits_device       the selection alone, over any query-major table of nqueries x ntargets sw_result on the device: the output of
 *             sw_db_search_affine, or of sw_search_device / sw_search_affine_device with nqueries = 1.  PRECONDITION, which the call cannot
 *             check on device data: 0 <= max_score < 2^24 for every entry (the bound every search call enforces).  d_results is only read.
 *             SW_EINVAL: NULL pointers, nqueries < 0, ntargets < 0 or ntargets >= 2^31, top < 1 or top > SW_TOP_MAX.
 *   sw_db_search_affine_top  search and selection through a prepared handle, with BOUNDED result memory: the full table never exists.
 *             Arguments as for sw_db_search_affine.  The queries are taken in consecutive chunks whose result rows (24 bytes per target)
 *             fit a per-context workspace that the option "search_results_mib" bounds (default 1024, 1..2^20); every chunk runs through
 *             the many-query search of sw_db_search_affine into the workspace and the selection then writes that chunk's rows of
 *             d_hits; chunks follow each other in the stream and share the workspace.  A query whose single row exceeds the budget is a
 *             chunk of its own -- the option refuses nothing.  Besides the workspace the selection holds 8 KiB of counters per query of
 *             a chunk, for at most 4096 queries.  SW_EINVAL: the argument errors of sw_db_search_affine, top < 1 or top > SW_TOP_MAX,
 *             NULL d_hits or d_nhits.  nqueries == 0 launches nothing; a handle with ntargets == 0 writes nhits = 0 and the {-1, 0, 0}
 *             pattern.  "last_search_top_chunks" and "last_search_top_kernel" (0: every row was sorted whole, at most SW_TOP_MAX targets;
 *             1: radix select) describe the last call.
 *   sw_search_affine_multi_top_host  the CPU leg on host memory, no GPU needed: sw_search_affine_host per query and a sort by the same
 *             rule; arguments as for sw_search_affine_multi_host, every one checked before the first query runs. */
#define SW_TOP_MAX 4096
typedef struct { int64_t target, max_pos, max_score; } sw_hit;
int  sw_top_hits_device(sw_ctx* ctx, const sw_result* d_results, int64_t nqueries, int64_t ntargets, int64_t top, int64_t min_score,
                        sw_hit* d_hits, int64_t* d_nhits, void* stream);
int  sw_db_search_affine_top(sw_ctx* ctx, const sw_db* db, const char* d_queries, const int64_t* qoffsets, int64_t nqueries,
                             const sw_affine* scoring, int64_t top, int64_t min_score, sw_hit* d_hits, int64_t* d_nhits, void* stream);
int  sw_search_affine_multi_top_host(const char* queries, const int64_t* qoffsets, int64_t nqueries, const char* db,
                                     const int64_t* offsets, int64_t ntargets, const sw_affine* scoring, int64_t top, int64_t min_score,
                                     sw_hit* hits, int64_t* nhits);

/* The alignments of the top hits of many queries, from the device hit table as it is (csrc/sw_align_hits.hip): the step behind
 * sw_db_search_affine_top, without a host round trip.  One call aligns every (query, hit) pair of the table; the work is sorted by
 * size on the device and runs from device-side lists.
 *   d_queries, qoffsets, scoring : as for sw_db_search_affine.
 *   d_hits  : device, nqueries x top sw_hit -- typically the output of sw_db_search_affine_top or sw_top_hits_device, but any table is
 *             accepted.  Only `target` is read: as in sw_align_affine_device a hit is re-filled in full and the kernel finds the
 *             arg-max itself.  Duplicate targets are allowed.
 *   d_nhits : device, nqueries int64, or NULL.  Row q uses its first clamp(d_nhits[q], 0, top) entries; with NULL all `top` of them.
 *   d_aln   : device, nqueries x top sw_alignment.  Entry (q, r) of a used hit is bit for bit what sw_align_affine_device writes for
 *             query q and hits = {target}.  Every other entry is all zeros: the entries beyond the row's count and those whose target
 *             lies outside [0, ntargets).  An out-of-range target is never used as an index: it is compared, unsigned, against ntargets
 *             before any load through it.  Every entry of d_aln is written.
 *   d_ops   : device, the ops of entry (q, r) at d_ops + (q * top + r) * ops_cap under the ops_cap / nops rules of
 *             sw_align_affine_device; the ops row of an all-zero entry is not touched.  May be NULL with ops_cap 0: coordinates only.
 * Nothing is written outside d_aln and the used ops rows.  Asynchronous on `stream`; the host reads neither the hits nor the targets'
 * offsets, its work is O(nqueries).  The order in which the device takes the pairs differs between runs, the bytes it writes do not.
 * nqueries == 0 launches nothing; a handle with ntargets == 0 only zeroes d_aln.
 * SW_EINVAL: the argument errors of sw_db_search_affine; top < 1 or top > SW_TOP_MAX; NULL d_hits or d_aln; a negative ops_cap, or NULL
 * d_ops with ops_cap > 0; and a worst case that does not fit: the host cannot know which targets the table names, so the handle's
 * longest target x the padded length of the longest query (a multiple of 256, 512 or 1024 for queries of at most 256, at most 512,
 * longer) has to fit "align_workspace_mib" and the 2 GiB a slot may take -- decided before anything is launched, whatever the table
 * says, with a message that names the option.  Under "align_checkpoint" = 1, and under 2 for exactly the calls refused so, every
 * hit is aligned from one band of direction bytes and checkpoint rows (see sw_set_option): the same bytes in d_aln and d_ops, and a
 * call is refused only if the checkpointed slot of that worst case does not fit the option.  The workspaces are those of sw_align_affine_device and sw_db_search_affine
 * ("align_workspace_mib", "search_profile_mib": queries run in consecutive groups whose profiles fit) plus 24 bytes per entry of a group,
 * at most 96 MiB.  "last_align_hits_launches" (kernel launches), "last_align_hits_tiers" (the (class, size tier) lists planned, one
 * alignment launch each) and "last_align_hits_slots" (direction matrices, summed over those launches) describe the last call, all 0 for
 * a call that launched no alignment; "last_align_hits_lists" is how many of those lists received items, counted on the device:
 * reading it waits for the device.
 *   sw_align_affine_hits_host  the CPU leg: the same result in plain C++ from host tables (sw_align_affine_host per query), no GPU
 *             needed, no workspace bound; every argument is checked before the first alignment. */
int  sw_db_align_affine_hits(sw_ctx* ctx, const sw_db* db, const char* d_queries, const int64_t* qoffsets, int64_t nqueries,
                             const sw_affine* scoring, const sw_hit* d_hits, const int64_t* d_nhits, int64_t top,
                             sw_alignment* d_aln, char* d_ops, int64_t ops_cap, void* stream);
int  sw_align_affine_hits_host(const char* queries, const int64_t* qoffsets, int64_t nqueries, const char* db,
                               const int64_t* offsets, int64_t ntargets, const sw_affine* scoring, const sw_hit* hits,
                               const int64_t* nhits, int64_t top, sw_alignment* aln, char* ops, int64_t ops_cap);

/* The scores of a device LIST of (query, target) pairs against a prepared database (csrc/sw_search_pairs.hip): the rescoring stage
 * behind a pre-filter -- k-mer or seed matching, a previous search round, a clustering step, a re-score under another matrix or other
 * gap costs --, whose list is typically a fraction of a percent of nqueries x ntargets.  sw_db_search_affine runs the whole cross
 * product whatever the list's size; this call runs the listed pairs and nothing else, through the same handle.
 *   d_queries, qoffsets, scoring : as for sw_db_search_affine.
 *   d_pairs   : device, npairs sw_pair = {query, target}, only read.  Entries may come in any order; duplicates are allowed.
 *   d_results : device, npairs sw_result, in the order of d_pairs.  Entry p is bit for bit what sw_db_search_affine writes at
 *               [query * ntargets + target]: the same recurrence, the same arg-max rule, max_pos in that pair's own
 *               (len + 1) x (qlen + 1) layout.  An entry whose query lies outside [0, nqueries), whose target lies outside
 *               [0, ntargets) or whose target is empty gives {0, 0, 0}.  An index is compared against its bound, UNSIGNED, before
 *               anything is loaded through it (the rule of sw_db_align_affine_hits).  Every entry of d_results is written, and
 *               nothing outside it.
 * Asynchronous on `stream`, no host round trip.  The host reads neither the pairs nor the targets' offsets; its work is O(nqueries).
 * The order in which the device takes the pairs may differ between runs, the bytes it writes do not.  npairs == 0 returns SW_OK and
 * launches nothing; nqueries == 0 launches no kernel either (no entry names a query: the results are zeroed); a handle without a
 * non-empty target only zeroes the results.  Linear gaps: pass sw_submat_match's table with gap_open = 0, as everywhere in this family.
 * SW_EINVAL: the argument and scoring errors of sw_db_search_affine, npairs < 0, NULL d_pairs or NULL d_results with npairs > 0.
 * The list is taken in consecutive chunks of at most "search_pairs_chunk" entries (settable, default 2^22, 1..2^31 - 1): a chunk's work
 * items take 24 bytes each in a per-context workspace (96 MiB at the default) and its counters stay inside 32 bits; the queries run in
 * the groups of sw_db_search_affine ("search_profile_mib").  "last_search_pairs_groups", "last_search_pairs_chunks" and
 * "last_search_pairs_launches" (kernel launches, the profile launches included) describe the last call, all 0 for one that launched
 * no kernel.
 *     LANES.  The option "search_pairs_lanes" (32, the default, or 16) chooses the kernel of this call and of the rescoring inside
 *     sw_db_search_affine_top_prefiltered; it is an option of its own, "search_lanes" does not reach a pair list.  Under 16 a query
 *     that is ELIGIBLE has its listed pairs run two per wave on packed 16-bit lanes (csrc/sw_search_pairs16.hip): the device pairs
 *     the pairs of a query whose weights len x padded query length share a power of two, so partners differ in length by less than a
 *     factor of two; a pair left over runs alone.  Eligible is the rule of sw_db_search_affine's "search_lanes" = 16, per query:
 *     max(largest table entry, 0) x min(qlen, longest target OF THE HANDLE) <= 32767 and gap_open + 2 gap_extend >= -32768, and the
 *     packed kernel of the query's width fits the device.  The handle's longest target is a conservative bound for a list -- the list
 *     may name shorter targets only, and the host does not read it --, so a query can stay on 32-bit lanes that a shorter database
 *     would let run packed.  Every other query runs on the 32-bit kernel inside the same call.  The results are the same bytes under
 *     16 and 32, on every run, whichever pairs the device happens to put together.  Under 16 a chunk's items take up to 48 bytes per
 *     entry, and per group of queries 12 x 41 bytes per query of counters.  "last_search_pairs_packed_launches" is the number of
 *     packed score launches of the last call (0 under 32 and for a call that launched none); "last_search_pairs_packed_items" the
 *     number of two-pair work items the device built in it, pairs without a partner included -- counted on the device: reading it
 *     waits for the device, like "last_align_hits_lists".
 * Alignments of listed pairs: sw_top_hits_pairs_device (below) selects the best entries of every query from the scored list into an
 * nqueries x top sw_hit table on the device, and sw_db_align_affine_hits aligns that table.
 *   sw_search_affine_pairs_host  the CPU leg: every entry as sw_search_affine_host computes that pair, in plain C++ on host memory, no
 *               GPU needed; every argument is checked before the first pair (SW_EINVAL also for the offsets / length errors of
 *               sw_search_device). */
typedef struct { int64_t query, target; } sw_pair;
int  sw_db_search_affine_pairs(sw_ctx* ctx, const sw_db* db, const char* d_queries, const int64_t* qoffsets, int64_t nqueries,
                               const sw_affine* scoring, const sw_pair* d_pairs, int64_t npairs, sw_result* d_results, void* stream);
int  sw_search_affine_pairs_host(const char* queries, const int64_t* qoffsets, int64_t nqueries, const char* db,
                                 const int64_t* offsets, int64_t ntargets, const sw_affine* scoring, const sw_pair* pairs,
                                 int64_t npairs, sw_result* results);

/* The ungapped pre-filter (csrc/sw_prefilter.hip): the stage that PRODUCES the pair list sw_db_search_affine_pairs rescores -- the MSV
 * stage of HMMER, the ungapped stage of MMseqs2.  For query q (columns j) and target t (rows i), with the table s used exactly as
 * sw_search_affine_device uses it (next to Gotoh's recurrence above):
 *   D[0][j] = D[i][0] = 0
 *   D[i][j] = max(0, D[i-1][j-1] + s[q[j-1]][t[i-1]])
 *   U(q, t) = max over all cells of D                          (0 for an empty target)
 * the best score of a gapless local alignment, over all diagonals; exact, no seeds, no index.  A gapless alignment is a local
 * alignment, so U <= max_score of sw_search_affine_device for the same table and ANY gap_open, gap_extend <= 0.
 *   d_queries, qoffsets, the handle, the stream : as for sw_db_search_affine; `sub` is HOST memory, copied before the call returns.
 *   min_score : a pair PASSES when its target is not empty and U >= min_score (min_score >= 1).
 *   d_npairs  : device, one int64: the TRUE number of passing pairs, also where it exceeds pairs_cap (the rule of sw_alignment's nops).
 *   d_pairs   : device, pairs_cap sw_pair.  Its first min(*d_npairs, pairs_cap) entries are distinct passing pairs, in no specified
 *               order (the slots come from an atomic cursor, and which pairs a too-small list keeps may differ between runs); every
 *               entry behind them, up to pairs_cap, is {-1, -1}.  Nothing is written outside pairs_cap entries.  May be NULL with
 *               pairs_cap 0: count (and scores) only.
 *   d_scores  : device, optional: nqueries x ntargets int32, QUERY-MAJOR; where it is not NULL every entry is written,
 *               d_scores[q * ntargets + k] = U(q, k), exact.
 * The {-1, -1} tail makes the chain free of a host round trip: sw_db_search_affine_pairs(..., d_pairs, pairs_cap, ...) gives {0, 0, 0}
 * for those entries by its out-of-range rule, so a caller runs it over all pairs_cap entries and never reads *d_npairs in between.
 * Asynchronous on `stream`, no host round trip; the host work of a call is O(nqueries).  The queries run in the groups of
 * sw_db_search_affine ("search_profile_mib").  A query whose scores provably fit 16 bits -- max(largest table entry, 0) x
 * min(its length, the handle's longest target) <= 32767 -- runs two targets per wave on packed 16-bit lanes, any other query on 32-bit
 * lanes; the scores are the same.  "prefilter_lanes" (settable: 0, the default, lets the planner decide; 32 never uses the packed
 * kernel) is the A/B switch; "last_prefilter_groups", "last_prefilter_launches" (score launches) and "last_prefilter_packed_launches"
 * describe the last call, all 0 for one that launched no kernel.
 * SW_EINVAL: the argument errors of sw_db_search_affine (the offsets, the query lengths, the table's 24-bit bound, a handle from
 * another device), NULL sub, min_score < 1, pairs_cap < 0, NULL d_pairs with pairs_cap > 0, NULL d_npairs unless d_pairs is NULL and
 * d_scores is not (so also: everything NULL).  nqueries == 0 or a handle without a non-empty target: SW_OK, *d_npairs = 0, the
 * {-1, -1} tail, zero scores.
 *   sw_prefilter_ungapped_host  the CPU leg: the same on host memory in plain C++, the list in ascending (query, target) order; every
 *               argument is checked before the first pair (SW_EINVAL also for the offsets / length errors of sw_search_device). */
int  sw_db_prefilter_ungapped(sw_ctx* ctx, const sw_db* db, const char* d_queries, const int64_t* qoffsets, int64_t nqueries,
                              const sw_submat* sub, int64_t min_score, sw_pair* d_pairs, int64_t pairs_cap, int64_t* d_npairs,
                              int32_t* d_scores, void* stream);
int  sw_prefilter_ungapped_host(const char* queries, const int64_t* qoffsets, int64_t nqueries, const char* db,
                                const int64_t* offsets, int64_t ntargets, const sw_submat* sub, int64_t min_score,
                                sw_pair* pairs, int64_t pairs_cap, int64_t* npairs, int32_t* scores);

/* The best entries of every query, selected on the device from a scored PAIR LIST (csrc/sw_top_pairs.hip): the step between
 * sw_db_search_affine_pairs and sw_db_align_affine_hits.  sw_top_hits_device needs a dense nqueries x ntargets table; the list of a
 * pre-filter lies in the order of an atomic cursor, unsorted and ungrouped, and this call turns it into the same kind of hit table.
 *   d_pairs, d_results : device, npairs entries each, only read; entry p of the results belongs to entry p of the pairs, exactly as
 *             sw_db_search_affine_pairs leaves them.
 *   An entry QUALIFIES when 0 <= query < nqueries, 0 <= target < ntargets and max_score >= min_score.  Each index is compared UNSIGNED
 *             against its bound before anything is indexed with it (the rule of sw_db_align_affine_hits), so the {-1, -1} tail of
 *             sw_db_prefilter_ungapped drops out by itself: a caller passes all pairs_cap entries and never reads the count.  With
 *             min_score <= 0 every in-range entry qualifies.  PRECONDITION, as for sw_top_hits_device: 0 <= max_score < 2^24 for the
 *             in-range entries; scores are taken modulo 2^24 so that no input carries a key out of its field.
 *   d_hits  : device, nqueries x top sw_hit.  Row q holds the first `top` qualifying entries of query q in the order max_score
 *             descending, then target ascending, then LIST POSITION ascending; hit = {target, max_pos, max_score} copied from the
 *             entry.  The third key makes the output unique for ANY input, duplicates of a pair included, also where a caller made
 *             their results differ: duplicates are kept, each one takes a rank.  The rest of a row is {-1, 0, 0}.
 *   d_nhits : device, nqueries int64: d_nhits[q] = min(top, qualifying entries of query q).
 * Every entry of d_hits and d_nhits is written and nothing outside them.  Asynchronous on `stream`, no host round trip; the host work
 * is O(1): it reads neither the list nor the results.  The same bytes come out on every run, although the entries are grouped with
 * atomics.  The entries are grouped per query in a per-context workspace of 12 bytes per list entry and 8 bytes per query that grows
 * on demand.  A query with many entries is ordered by ONE workgroup, in blocks once it has more than SW_TOP_MAX (top <= 2048) or
 * 2 x SW_TOP_MAX entries: the call is made for lists that are small on purpose.
 * SW_EINVAL: NULL d_hits or d_nhits; NULL d_pairs or d_results with npairs > 0; npairs < 0 or npairs >= 2^31; nqueries < 0;
 * ntargets < 0 or ntargets >= 2^31; top < 1 or top > SW_TOP_MAX.  npairs == 0 writes nhits = 0 and the {-1, 0, 0} pattern;
 * nqueries == 0 launches nothing.  "last_top_pairs_launches" (kernel launches) and "last_top_pairs_kernel" (0: every segment could be
 * sorted whole because npairs <= SW_TOP_MAX; 1: the streaming form was compiled in for the call) describe the last call.
 *   sw_top_hits_pairs_host  the CPU leg: the same table from host memory in plain C++, no GPU needed.
 *
 *   sw_db_search_affine_top_prefiltered  the whole chain in one call: sw_db_prefilter_ungapped (the table of `scoring`, threshold
 *             prefilter_min_score, no d_scores), sw_db_search_affine_pairs over all pairs_cap entries, then the selection above, all on
 *             `stream` with no host read in between.  d_queries, qoffsets, scoring and the handle as for sw_db_search_affine; top,
 *             min_score, d_hits, d_nhits as above.  The rescoring follows the option "search_pairs_lanes" as sw_db_search_affine_pairs
 *             does (the table is the same under 16 and 32); the pre-filter has "prefilter_lanes".
 *             WHAT IT COMPUTES: the table of sw_db_search_affine_top restricted to the pairs with U >= prefilter_min_score (U: the
 *             ungapped score above).  That is a FILTER, not the same hits: a pair whose gapped score is high and whose best gapless
 *             segment is below the threshold is not found.  One case is exact: with prefilter_min_score = 1 and min_score >= 1 the two
 *             tables are identical, because a positive local score needs a positive cell.
 *             d_npairs (device, one int64, not NULL) receives the filter's TRUE count.  Where it exceeds pairs_cap the table is built
 *             from the pairs the list happened to keep: every hit is then still a correct, passing pair, but the table is NEITHER
 *             COMPLETE NOR REPRODUCIBLE.  The call cannot know without a host read: the caller checks the count after the call.
 *             The list and its results live in a per-context workspace of 40 bytes per entry; with the selection's segments that is at
 *             most 56 bytes x pairs_cap, which the option "search_results_mib" bounds: a larger pairs_cap is SW_EINVAL with a message
 *             that names the option.  Every argument is checked before the first launch.  SW_EINVAL besides: the argument errors of
 *             sw_db_search_affine, prefilter_min_score < 1, pairs_cap < 0 or >= 2^31, NULL d_npairs, NULL d_hits or d_nhits, top < 1 or
 *             top > SW_TOP_MAX. */
int  sw_top_hits_pairs_device(sw_ctx* ctx, const sw_pair* d_pairs, const sw_result* d_results, int64_t npairs, int64_t nqueries,
                              int64_t ntargets, int64_t top, int64_t min_score, sw_hit* d_hits, int64_t* d_nhits, void* stream);
int  sw_top_hits_pairs_host(const sw_pair* pairs, const sw_result* results, int64_t npairs, int64_t nqueries, int64_t ntargets,
                            int64_t top, int64_t min_score, sw_hit* hits, int64_t* nhits);
int  sw_db_search_affine_top_prefiltered(sw_ctx* ctx, const sw_db* db, const char* d_queries, const int64_t* qoffsets, int64_t nqueries,
                                         const sw_affine* scoring, int64_t prefilter_min_score, int64_t pairs_cap, int64_t top,
                                         int64_t min_score, sw_hit* d_hits, int64_t* d_nhits, int64_t* d_npairs, void* stream);

/* Queries that are position-specific scoring matrices (PSSMs; csrc/sw_pssm.hip): one row of scores per query COLUMN in place of a letter
 * scored through a table -- the query of a PSI-BLAST iteration, of a profile or domain library.  The three calls below are the twins of
 * sw_db_search_affine, sw_db_search_affine_top and sw_db_align_affine_hits: the same handle, outputs, layouts, options, chunks, tiers and
 * refusals, and the same kernels behind the query profiles; only the profiles are built from another source.
 *   sw_pssm_scoring  letters    : HOST, the nletters target bytes a column has an entry for (1..256, no byte twice)
 *                    other      : the score of a target byte that is not in `letters`, at every column; -128..smax
 *                    smax       : 0..127; every entry above smax is TAKEN AS smax
 *                    gap_open, gap_extend : as in sw_affine
 *   d_pssm    : device, int8.  Column g is the nletters bytes at d_pssm + g * nletters; byte k of a column scores the target byte
 *               letters[k].  No alignment is asked of d_pssm.
 *   qoffsets  : HOST, as everywhere in the family, counted in COLUMNS: query q is the columns [qoffsets[q], qoffsets[q+1]);
 *               qoffsets[0] >= 0 and may be positive.  A call reads no byte outside
 *               [d_pssm + qoffsets[0] * nletters, d_pssm + qoffsets[nqueries] * nletters).
 * The score of query column j (1-based inside its query, column g of d_pssm) against target byte x is
 *   s(j, x) = min(entry, smax)  where x = letters[k], entry = d_pssm[g * nletters + k];   s(j, x) = other  for every other x.
 * With s(j, t[i-1]) in place of s[q[j-1]][t[i-1]] the recurrence, the arg-max rule, the result layouts and the canonical alignment are the
 * ones stated above for sw_search_affine_device and sw_align_affine_device.
 * THE CLAMP.  The host never reads d_pssm, so it cannot bound the entries the way the table calls bound theirs; smax does it by
 * construction.  The 24-bit bound is smax x min(longest query, longest target) < 2^24, and gap_open + gap_extend >= -2^24 as before.
 * Compare sw_top_hits_device: there 0 <= max_score < 2^24 is a PRECONDITION the call cannot check on device data; here the same bound
 * is ENFORCED, whatever bytes d_pssm holds, and a hit table of sw_db_search_pssm_top meets that precondition.  A caller whose entries
 * all lie at or below smax loses nothing; smax = 127 clamps nothing.  The three calls are tested at the edges of this rule as the
 * table calls are at theirs -- entries of -128 and 127, other = -128 and other = smax, smax = 0, 1..256 letters with the bytes 0x00,
 * 0x7F, 0x80 and 0xFF among them and among the bytes that score `other`, on 32-bit and packed 16-bit lanes
 * (tests/test_pssm_range_gpu.py).
 * Asynchronous on `stream`, no host round trip; the host work of a call is O(nqueries) + O(nletters).  Every argument is checked before
 * the first launch.  "last_search_multi_*", "last_search_top_*" and "last_align_hits_*" describe these calls as they describe the twins.
 * SW_EINVAL: the argument errors of the twin; NULL d_pssm, scoring or letters; nletters outside 1..256; a byte twice in letters; smax
 * outside 0..127; other outside -128..smax; the two bounds above.
 *   sw_search_pssm_multi_host, sw_align_pssm_hits_host  the CPU legs: the same results in plain C++ from host memory (pssm: the host
 *               copy of d_pssm, indexed by the same qoffsets), no GPU needed; every argument is checked before the first query runs.
 *   sw_pssm_from_queries  the PSSM that reproduces sequence queries under a table, iteration 0 of an iterative search:
 *               out[(qoffsets[q] - qoffsets[0] + j) * nletters + k] = sub->s[q[j]][letters[k]], q[j] = queries[qoffsets[q] + j].  `out`
 *               holds (qoffsets[nqueries] - qoffsets[0]) * nletters bytes and starts at the FIRST query's first column: pass
 *               d_pssm = (device copy of out) - qoffsets[0] * nletters, or offsets rebased to 0.  With every byte the targets use in
 *               `letters`, other <= smax and smax >= the table's largest entry, the PSSM calls then equal the table calls bit for bit.
 *   sw_read_pssm  the ASCII PSSM that PSI-BLAST writes (-out_ascii_pssm).  The header is the first line whose tokens are all single
 *               letters; the letters are its tokens up to the first repeat (PSI-BLAST prints the alphabet twice: scores, then
 *               percentages), and that repeat has to be of the FIRST letter -- any other is a letter listed twice.  Lines end with
 *               LF or CRLF.  Every following line that starts with an integer is a column: position, residue letter, then nletters
 *               integers; the rest of the line is ignored.  The first other line after a column ends the table.  Entries must fit
 *               int8.  Two-call pattern as in sw_read_fasta_db: with pssm == NULL it reports *nletters, *ncols and the letters only;
 *               otherwise pssm receives ncols * nletters bytes (cap at least that), column-major as d_pssm wants them.  letters_out
 *               holds 256 bytes.  SW_EINVAL with a message for an unreadable or malformed file (no header, no column, a short
 *               column, an entry that is no integer or does not fit int8) and for a cap too small; nothing is read or written out
 *               of bounds whatever the file holds. */
typedef struct {
    const char* letters; int32_t nletters;   /* HOST: the target bytes the PSSM has a row entry for, 1..256, no byte twice */
    int32_t other;                           /* score of a target byte not in `letters`, at every column; -128..smax */
    int32_t smax;                            /* 0..127: every entry above smax is TAKEN AS smax (see above) */
    int32_t gap_open, gap_extend;            /* as in sw_affine */
} sw_pssm_scoring;
int  sw_db_search_pssm(sw_ctx* ctx, const sw_db* db, const int8_t* d_pssm, const int64_t* qoffsets, int64_t nqueries,
                       const sw_pssm_scoring* scoring, sw_result* d_results, void* stream);
int  sw_db_search_pssm_top(sw_ctx* ctx, const sw_db* db, const int8_t* d_pssm, const int64_t* qoffsets, int64_t nqueries,
                           const sw_pssm_scoring* scoring, int64_t top, int64_t min_score, sw_hit* d_hits, int64_t* d_nhits, void* stream);
int  sw_db_align_pssm_hits(sw_ctx* ctx, const sw_db* db, const int8_t* d_pssm, const int64_t* qoffsets, int64_t nqueries,
                           const sw_pssm_scoring* scoring, const sw_hit* d_hits, const int64_t* d_nhits, int64_t top,
                           sw_alignment* d_aln, char* d_ops, int64_t ops_cap, void* stream);
int  sw_search_pssm_multi_host(const int8_t* pssm, const int64_t* qoffsets, int64_t nqueries, const char* db, const int64_t* offsets,
                               int64_t ntargets, const sw_pssm_scoring* scoring, sw_result* results);
int  sw_align_pssm_hits_host(const int8_t* pssm, const int64_t* qoffsets, int64_t nqueries, const char* db, const int64_t* offsets,
                             int64_t ntargets, const sw_pssm_scoring* scoring, const sw_hit* hits, const int64_t* nhits, int64_t top,
                             sw_alignment* aln, char* ops, int64_t ops_cap);
int  sw_pssm_from_queries(const char* queries, const int64_t* qoffsets, int64_t nqueries, const sw_submat* sub, const char* letters,
                          int32_t nletters, int8_t* out);
int  sw_read_pssm(const char* path, char* letters_out, int32_t* nletters, int8_t* pssm, int64_t cap, int64_t* ncols);

/* The NEXT iteration's PSSM, built on the device from aligned hits (csrc/sw_pssm_hits.hip): the step that closes the loop
 *   sw_db_search_pssm_top -> sw_db_align_pssm_hits -> sw_db_pssm_from_hits -> sw_db_search_pssm_top -> ...
 * It takes the hit table, the alignments and the ops exactly as the first two calls leave them on the device and writes a PSSM that
 * goes straight back into the first.  The arithmetic is integers only -- no log, no floats --, so device and host agree bit for bit;
 * a caller who wants true log-odds takes the exact count matrix (d_counts) and does the small float step alone.  The score rule is
 * Gribskov's average profile: a column's new row is the weighted mean of its prior row and of the substitution-table rows of the
 * residues observed in that column.
 *   d_prior, d_pssm_out : device, int8, the layout of d_pssm (column g at + g * nletters), indexed by the same qoffsets.  Only the
 *               columns [qoffsets[0], qoffsets[nqueries]) are written.  d_pssm_out == d_prior (exactly the same buffer) is allowed;
 *               any other overlap is the caller's error.  d_pssm_out may be NULL where d_counts is not.
 *   scoring   : letters, nletters and smax are used (other and the gap costs are checked as everywhere, and not used).
 *   upd       : sub, the table S is taken from; prior_weight 0..65535; include_min_score.
 *   d_hits, d_nhits, top, d_aln, d_ops, ops_cap : the tables of sw_db_align_pssm_hits / sw_db_align_affine_hits; d_ops is required,
 *               ops_cap >= 1.  Only read.
 *   d_weights : device, optional: nqueries x top int32, the weight of entry (q, r); NULL: every weight is 1.
 *   d_counts  : device, optional: (qoffsets[nqueries] - qoffsets[0]) x nletters int32, rebased to the first query's first column like the
 *               output of sw_pssm_from_queries; every entry is written.
 * Notation: query q has qlen columns j (0-based) at column g = qoffsets[q] + j.  P[j][k] = min(prior entry, smax).
 * S[b][k] = sub->s[(uint8) letters[b]][(uint8) letters[k]]: the observed residue plays the query letter.
 * USED ENTRIES.  Entry (q, r) is used when ALL of these hold:  r < clamp(d_nhits[q], 0, top) (d_nhits == NULL: all top entries);
 *   d_hits[q * top + r].target, compared unsigned, < ntargets;  d_aln[q * top + r].max_score >= include_min_score;  0 < nops <= ops_cap;
 *   q_begin and t_begin, compared unsigned, <= qlen and <= the target's length.  Each index is compared before anything is loaded
 *   through it (the rule of sw_db_align_affine_hits).
 * THE WALK of a used entry starts at j = q_begin, i = t_begin and goes through its nops op bytes in order:
 *   'M': if j < qlen and i < len the entry PAIRS column j with the target byte t[i]; then j++, i++.
 *   'I': j++ (consumes a query letter).   'D': i++.   Any other byte consumes nothing.
 *   So the call is defined for ANY bytes in the tables and reads nothing out of bounds; for tables that come from the alignment calls
 *   none of the guards ever fires.
 * WEIGHTS.  w(q, r) = d_weights ? clamp(d_weights[q * top + r], 0, 65535) : 1 -- taken as, like smax: the host cannot check device data.
 * COUNTS.  C[j][k] = the sum of w over the used entries of query q that pair column j with the byte letters[k]; bytes that are not in
 *   `letters` are not counted.  N[j] = sum over k of C[j][k].  A walk visits a column at most once: N[j] <= 4096 x 65535 < 2^28.
 * NEW ENTRY.  den = prior_weight + N[j].  den == 0: out[j][k] = P[j][k].  Otherwise, in int64,
 *   num = prior_weight x P[j][k] + sum over b of C[j][b] x S[b][k],   out[j][k] = clamp(floor((2 num + den) / (2 den)), -128, 127):
 *   round half up with FLOOR division (C's '/' truncates toward zero, which differs for negative numerators).  num reaches
 *   4096 x 65535 x 127 = 3.4e10; tests/test_pssm_hits_gpu.py runs sums beyond 2^32, exact halves of both signs there and both clamps.
 * Integer sums do not depend on their order: the same bytes come out on every run.
 * Asynchronous on `stream`, no host round trip: the host reads none of the device tables; its work is O(nqueries) + O(nletters^2) (S).
 * One small table (S, the code table, the offsets) is uploaded from pinned memory; the context holds TWO such copies and uses them in turn,
 * so a call waits on the host only for the upload of the call before the last one -- a loop can be enqueued one call ahead of the
 * device.  (The search and alignment calls of the loop keep one pinned copy each and wait for their own previous upload, as ever.)
 * tests/test_session_gpu.py enqueues five such calls of different shapes in a row on two streams, unsynchronised.
 * nqueries == 0 launches nothing; a handle with ntargets == 0 uses no entry: the clamped prior comes out and the counts are zero.
 * One launch: one workgroup per (query, tile of columns), a tile's counts in LDS, no global atomics (swp::plan_pssm_hits cuts the
 * tiles).  "last_pssm_hits_launches" reports the kernel launches of the last call.
 * SW_EINVAL, checked before the first launch: the argument errors of sw_db_align_pssm_hits (the offsets, the scoring object, the
 * handle's device, top outside 1..SW_TOP_MAX); NULL d_prior, upd, upd->sub, d_hits, d_aln or d_ops; ops_cap < 1; prior_weight outside
 * 0..65535; both outputs NULL.
 *   sw_pssm_from_hits_host  the CPU leg: the same bytes in plain C++ from host memory, db / offsets / ntargets in the handle's place.
 *   sw_write_pssm  the ASCII layout sw_read_pssm reads (PSI-BLAST's): a title line, the alphabet twice, one line per column with its
 *               position, its residue (consensus[g], or 'X' with consensus == NULL), the nletters scores and nletters zero percentages.
 *               sw_read_pssm on the file returns the same letters and bytes.  SW_EINVAL for what that reader could not read back: a
 *               letter outside A-Z, a-z, '*' (so: at most 53 letters), a letter twice, ncols < 1, a consensus byte that is not a
 *               printable character, a file that cannot be written. */
typedef struct { const sw_submat* sub; int32_t prior_weight; int64_t include_min_score; } sw_pssm_update;
int  sw_db_pssm_from_hits(sw_ctx* ctx, const sw_db* db, const int8_t* d_prior, const int64_t* qoffsets, int64_t nqueries,
                          const sw_pssm_scoring* scoring, const sw_pssm_update* upd, const sw_hit* d_hits, const int64_t* d_nhits, int64_t top,
                          const sw_alignment* d_aln, const char* d_ops, int64_t ops_cap, const int32_t* d_weights, int8_t* d_pssm_out,
                          int32_t* d_counts, void* stream);
int  sw_pssm_from_hits_host(const int8_t* prior, const int64_t* qoffsets, int64_t nqueries, const char* db, const int64_t* offsets,
                            int64_t ntargets, const sw_pssm_scoring* scoring, const sw_pssm_update* upd, const sw_hit* hits,
                            const int64_t* nhits, int64_t top, const sw_alignment* aln, const char* ops, int64_t ops_cap,
                            const int32_t* weights, int8_t* pssm_out, int32_t* counts);
int  sw_write_pssm(const char* path, const char* letters, int32_t nletters, const int8_t* pssm, int64_t ncols, const char* consensus);

/* The WEIGHTS of aligned hits, on the device (csrc/sw_pssm_weights.hip): the d_weights table of sw_db_pssm_from_hits, written from the
 * same device tables, so that the loop
 *   sw_db_search_pssm_top -> sw_db_align_pssm_hits -> sw_db_pssm_hit_weights -> sw_db_pssm_from_hits -> sw_db_search_pssm_top -> ...
 * stays on one stream with no host round trip.  With every weight 1 a family that appears 200 times among the hits outvotes a distant
 * homologue 200 to 1 and the profile collapses onto that family; position-based sequence weights (Henikoff & Henikoff 1994, J. Mol.
 * Biol. 243:574) share a column's vote among the residues seen in it and a residue's share among the sequences that show it.  The
 * rule below is that one in integers only -- no floats --, so device, host leg and a restatement in any language agree bit for bit,
 * and every run writes the same bytes.
 *   scoring   : letters and nletters are used (the rest is checked as everywhere, and not used).
 *   weighting : per_hit 1..65535, the mean weight of an informative hit; include_min_score.
 *   d_hits, d_nhits, top, d_aln, d_ops, ops_cap : as for sw_db_pssm_from_hits.  Only read.
 *   d_weights : device, nqueries x top int32.  EVERY entry is written.
 * For query q of qlen columns j:
 * USED ENTRIES and THE WALK are exactly those of sw_db_pssm_from_hits, with weighting->include_min_score in the place of
 *   upd->include_min_score: the same guards, every index compared, unsigned, before anything is loaded through it; an 'M' PAIRS column
 *   j with the byte t[i] only if j < qlen and i < len.  Only pairs whose byte is in `letters` count below.
 * n[j][k] = the number of used entries that pair column j with letters[k], 0..4096 (the same target twice in the table: two sequences).
 * k_j     = the number of k with n[j][k] > 0, 0..256.
 * F = 2^20, so k_j x n[j][k] <= F and every term below is >= 1.
 * For a used entry r:  m_r = the number of counted pairs it makes;  T_r = the sum over those pairs (j, k) of floor(F / (k_j x n[j][k])),
 *   below 2^40, in int64;  A_r = m_r > 0 ? floor(T_r / m_r) : 0, within 1..2^20: the fixed-point mean, over the columns the hit
 *   covers, of Henikoff's 1 / (k n).  An entry that is not used has A_r = 0.
 * U = the number of entries with A_r > 0;  SUM = the sum of A_r over the query's entries, <= 2^32.
 * THE WEIGHT.  w(q, r) = SUM > 0 ? min(65535, floor((2 x per_hit x U x A_r + SUM) / (2 x SUM))) : 0 -- rounded half up; the numerator stays
 *   below 2^50.  The weights of a query sum to about per_hit x U: the mean weight of an informative hit is per_hit.
 * Entries that are not used, and r at or beyond clamp(d_nhits[q], 0, top), get 0.  The call is defined for ANY bytes in the device
 * tables and reads nothing out of bounds.
 * What follows from the rule (tests/test_pssm_weights_host.py holds it): U identical entries get exactly per_hit each; permuting a
 * query's entries permutes its weights; two copies of one sequence beside one sequence that differs from it in every column get
 * 0.75, 0.75 and 1.5 x per_hit; a query's weights depend on no other query.
 * Downstream, N[j] of sw_db_pssm_from_hits counts in units of per_hit: scale prior_weight with it.
 * Asynchronous on `stream`, no host round trip: the host reads none of the device tables; its work is O(nqueries) + O(nletters).  The
 * output feeds sw_db_pssm_from_hits(..., d_weights, ...) on the same stream with nothing in between.  The small table (the code table,
 * the offsets) is uploaded through the two pinned copies of sw_db_pssm_from_hits, in the same turns: a loop can still be enqueued
 * one call ahead of the device.  Two launches behind one memset of the context's nqueries x top x 8 bytes of accumulators: one workgroup
 * per (query, tile of columns) -- counts, then terms, in LDS; one 64-bit integer atomic add per (entry, tile) --, then one workgroup per
 * query (swp::plan_pssm_weights).  "last_pssm_weights_launches" reports the kernel launches of the last call, "last_pssm_weights_tiles"
 * the tiles its longest query was cut into.
 * nqueries == 0 launches nothing; with a handle of ntargets == 0 every weight is 0.
 * SW_EINVAL, checked before the first launch: the argument errors sw_db_pssm_from_hits reports for the same arguments (the offsets, the
 * scoring object, the handle's device, top outside 1..SW_TOP_MAX, NULL d_hits, d_aln or d_ops, ops_cap < 1); NULL weighting or
 * d_weights; per_hit outside 1..65535.
 *   sw_pssm_hit_weights_host  the CPU leg: the same bytes in plain C++ from host memory, db / offsets / ntargets in the handle's place. */
typedef struct { int32_t per_hit; int64_t include_min_score; } sw_pssm_weighting;   /* per_hit 1..65535 */
int  sw_db_pssm_hit_weights(sw_ctx* ctx, const sw_db* db, const int64_t* qoffsets, int64_t nqueries, const sw_pssm_scoring* scoring,
                            const sw_pssm_weighting* weighting, const sw_hit* d_hits, const int64_t* d_nhits, int64_t top,
                            const sw_alignment* d_aln, const char* d_ops, int64_t ops_cap, int32_t* d_weights, void* stream);
int  sw_pssm_hit_weights_host(const int64_t* qoffsets, int64_t nqueries, const char* db, const int64_t* offsets, int64_t ntargets,
                              const sw_pssm_scoring* scoring, const sw_pssm_weighting* weighting, const sw_hit* hits, const int64_t* nhits,
                              int64_t top, const sw_alignment* aln, const char* ops, int64_t ops_cap, int32_t* weights);

/* The QUERY-ANCHORED ALIGNMENT of aligned hits, on the device (csrc/sw_msa_hits.hip): what an iterative search is usually run for --
 * the multiple alignment of the hits with one column per query position, as jackhmmer and HHblits write it (A3M) -- from the tables
 * sw_db_align_affine_hits / sw_db_align_pssm_hits leave on the device, without bringing the nqueries x top x ops_cap op rows to the host.
 *   d_queries : device, the query letters as the sequence calls take them (query q at d_queries + qoffsets[q]); NULL for PSSM
 *               queries, which have no letters: nident is then 0.  Used for nident only.
 *   include_min_score, d_hits, d_nhits, top, d_aln, d_ops, ops_cap : as for sw_db_pssm_from_hits.  Only read.
 * USED ENTRIES and THE WALK are exactly those of sw_db_pssm_from_hits, with include_min_score in the place of upd->include_min_score:
 *   the same guards, every index compared, unsigned, before anything is loaded through it; an 'M' PAIRS column j with the byte t[i]
 *   only if j < qlen and i < len.  A VALID INSERT is a 'D' op met with i < len and j <= qlen: the target byte t[i] stands between
 *   columns j - 1 and j.  The call is defined for ANY bytes in the device tables and reads and writes nothing out of bounds.
 * COLUMN ROWS, d_cols (optional): device, (qoffsets[nqueries] - qoffsets[0]) x top bytes; EVERY byte is written.  Row (q, r) has qlen
 *   bytes at d_cols + (qoffsets[q] - qoffsets[0]) x top + r x qlen: byte j is t[i], verbatim, where the walk pairs column j, and '-'
 *   everywhere else; the row of an entry that is not used is all '-'.  A query's rows are a top x qlen matrix a kernel reads by column.
 * A3M ROWS, d_a3m with d_rows (optional together): the row of a used entry is its column row with the byte of every valid insert
 *   placed before column j, in op order (inserts behind the last column at the end); insert bytes 'A'..'Z' become + 32 (lower case),
 *   every other byte stays.  So column j sits at j + the valid inserts seen before the walk reaches column j (all of them for the
 *   columns behind the walk's end), and len = qlen + ninsert; an entry that is not used has len = 0.
 *   d_rows    : device, nqueries x top sw_msa_row; EVERY one is written.  off: the exclusive prefix sum of len over the entries in (q, r)
 *               order, computed on the device; nmatch: the paired columns; nident: the paired columns with t[i] == the query's letter j
 *               (0 with d_queries == NULL); ninsert: the valid inserts.  An entry that is not used gets {off, 0, 0, 0, 0}.
 *   d_a3m, a3m_cap : device, a3m_cap bytes (d_a3m may be NULL: the rows alone, a sizing call).  The row of entry (q, r) lies at
 *               d_a3m + off; a row with off + len > a3m_cap is not written, and nothing is written at or beyond d_a3m + a3m_cap.
 *   d_a3m_bytes : device, one int64 (optional with d_rows alone): the TRUE total of len, also beyond a3m_cap -- the caller compares and calls again.
 * Bytes only: the same bytes on every run.  Asynchronous on `stream`, no host round trip: the host reads none of the device tables;
 * its work is O(nqueries).  The offsets are uploaded through the two pinned copies of sw_db_pssm_from_hits, in the same turns.
 * Launches (swp::plan_msa_hits): A, one workgroup per (query, slice of entries), writes the column rows and the rows' counts; with
 * d_rows, B scans len in two levels (256 entries per workgroup in LDS, then one workgroup over the sums; no atomics) and C writes off
 * and the A3M rows, one wave per entry.  "last_msa_hits_launches" reports the kernel launches of the last call.
 * nqueries == 0 launches nothing; with a handle of ntargets == 0 no entry is used: '-' everywhere, every len 0.
 * SW_EINVAL, checked before the first launch: the offset and handle errors of sw_db_align_affine_hits; top outside 1..SW_TOP_MAX; NULL
 * d_hits, d_aln or d_ops; ops_cap < 1; every output NULL (d_cols and d_rows both NULL); d_a3m or d_a3m_bytes without d_rows; d_a3m
 * without d_a3m_bytes; a negative a3m_cap.
 *   sw_msa_from_hits_host  the CPU leg: the same bytes in plain C++ from host memory, db / offsets / ntargets in the handle's place
 *               (queries: the letters at queries + qoffsets[q], or NULL).
 *   sw_write_a3m  one query's A3M file from host copies of the tables: with `query` (qlen letters) the file opens with the record
 *               ">qname" and the query's letters, with query == NULL (a PSSM) there is no query record.  Then, for r = 0 .. top - 1 in
 *               order, every entry with rows[r].len > 0 whose row lies inside a3m_cap gets
 *                   >NAME score=S q=B-E t=B-E ident=N/M
 *               (NAME = tnames[target], or the target's index with tnames == NULL; S = max_score; the begins and ends of sw_alignment;
 *               N = nident, M = nmatch) and its row a3m[rows[r].off .. + len).  hits, aln, rows: the query's top entries;
 *               a3m, a3m_cap: the call's whole buffer.  SW_EINVAL: NULL path, qname, hits, aln, rows or a3m, top < 1, qlen < 1, a row
 *               of a target index outside 0..ntargets - 1, a file that cannot be written. */
typedef struct { int64_t off; int32_t len; int32_t nmatch; int32_t nident; int32_t ninsert; } sw_msa_row;
int  sw_db_msa_from_hits(sw_ctx* ctx, const sw_db* db, const char* d_queries, const int64_t* qoffsets, int64_t nqueries,
                         int64_t include_min_score, const sw_hit* d_hits, const int64_t* d_nhits, int64_t top, const sw_alignment* d_aln,
                         const char* d_ops, int64_t ops_cap, char* d_cols, sw_msa_row* d_rows, char* d_a3m, int64_t a3m_cap,
                         int64_t* d_a3m_bytes, void* stream);
int  sw_msa_from_hits_host(const char* queries, const int64_t* qoffsets, int64_t nqueries, const char* db, const int64_t* offsets,
                           int64_t ntargets, int64_t include_min_score, const sw_hit* hits, const int64_t* nhits, int64_t top,
                           const sw_alignment* aln, const char* ops, int64_t ops_cap, char* cols, sw_msa_row* rows, char* a3m,
                           int64_t a3m_cap, int64_t* a3m_bytes);
int  sw_write_a3m(const char* path, const char* qname, const char* query, int64_t qlen, const char* const* tnames, int64_t ntargets,
                  const sw_hit* hits, const sw_alignment* aln, const sw_msa_row* rows, int64_t top, const char* a3m, int64_t a3m_cap);

/* The FILTER of a hit alignment, on the device (csrc/sw_msa_filter.hip): the stage between "align" and "weights / update" that drops
 * the rows that are too short and the rows that are nearly identical to the query or to a better-ranked row (PSI-BLAST's purge,
 * hhfilter -id -cov).  It reads the COLUMN ROWS of sw_db_msa_from_hits exactly as that call writes them into d_cols -- per query q of
 * qlen = qoffsets[q + 1] - qoffsets[q] columns, row r = 0 .. top - 1 has qlen bytes at d_cols + (qoffsets[q] - qoffsets[0]) x top +
 * r x qlen -- and needs no database handle.  Bytes are taken verbatim; '-' (0x2D) means NO LETTER, so a target byte that happens to be
 * 0x2D counts as no letter.
 * THE RULE, per query, integers only:
 *   n_r          : the bytes of row r that are not '-'.
 *   same(r, r')  : the columns j where row r has a letter and row r' holds the same byte.
 *   sameq(r)     : the same count against the query's letters d_queries[qoffsets[q] + j]; only with d_queries != NULL.  For tables that
 *                  come from the alignment calls it equals nident of sw_msa_row.
 *   covered(r)   : n_r >= 1 and 100 x n_r >= min_cover_pct x qlen.
 *   redundant(r | r') : 100 x same(r, r') >= max_ident_pct x n_r -- at least max_ident_pct percent of what row r shows is already
 *                  shown, letter for letter, by r'.  Asymmetric on purpose: the lower-ranked row is measured against its own length.
 *   keep(r), for r = 0 .. top - 1 in rank order, holds when covered(r); and d_queries == NULL or 100 x sameq(r) < max_ident_pct x n_r;
 *                  and redundant(r | r') is false for every r' < r with keep(r').  GREEDY: a row that was dropped suppresses nothing.
 *   sw_msa_filter : max_ident_pct 1..101 (101 drops nothing for identity: same <= n_r), min_cover_pct 0..100.  Every product fits
 *                  int32 (100 x 2^20).  No floats: device, host leg and any restatement agree bit for bit, every run writes the same bytes.
 * Outputs (at least one of d_keep and d_hits_out):
 *   d_keep     : device, nqueries x top int32, 1 or 0, EVERY entry written; the layout of d_weights, so it goes into
 *                sw_db_pssm_from_hits as unit weights.  Optional.
 *   d_hits_out : device, nqueries x top sw_hit, with d_hits (optional together): entry (q, r) is d_hits[q x top + r] with target = -1
 *                where keep is 0, unchanged otherwise.  d_hits_out == d_hits (in place) is allowed.  A dropped entry is not a USED
 *                ENTRY of sw_db_pssm_hit_weights, sw_db_pssm_from_hits and sw_db_msa_from_hits: they see the kept entries only.
 *   d_nkept    : device, nqueries int64: the rows kept.  Optional.
 * Asynchronous on `stream`, no host round trip: the host reads no device table, its work is O(nqueries).  The offsets are uploaded
 * through the two pinned copies of sw_db_pssm_from_hits, in the same turns: a loop can be enqueued one call ahead.  Defined for ANY
 * bytes in d_cols and d_queries; nothing is read or written out of bounds; rows need no alignment (qlen and the bases may be odd).
 * Launches (swp::plan_msa_filter), per chunk of queries whose bit matrices fit the option "msa_filter_workspace_mib" (default 256, at
 * least what one query of top 4096 needs): the PAIR launch, one workgroup per (query, 64 x 64 tile of the triangle r' <= r), leaves
 * bit r' of word (r' / 64, r) set where redundant(r | r'), and the row's own test (cover, query) beside it -- the tiles on the diagonal
 * compare with the query; the GREEDY launch, one workgroup per query, resolves keep in rank order 64 rows at a time and writes the
 * outputs.  "last_msa_filter_launches" and "last_msa_filter_chunks" report the last call.  nqueries == 0 launches nothing.
 * SW_EINVAL, checked before the first launch: the offset errors of sw_db_msa_from_hits (so every query has at least one column); top
 * outside 1..SW_TOP_MAX; NULL d_cols or filter; a percentage out of range; both outputs NULL; d_hits_out without d_hits.
 *   sw_msa_filter_host  the CPU leg: the same bytes in plain C++ from host memory. */
typedef struct { int32_t max_ident_pct; int32_t min_cover_pct; } sw_msa_filter;
int  sw_msa_filter_device(sw_ctx* ctx, const char* d_cols, const char* d_queries, const int64_t* qoffsets, int64_t nqueries, int64_t top,
                          const sw_msa_filter* filter, const sw_hit* d_hits, sw_hit* d_hits_out, int32_t* d_keep, int64_t* d_nkept,
                          void* stream);
int  sw_msa_filter_host(const char* cols, const char* queries, const int64_t* qoffsets, int64_t nqueries, int64_t top,
                        const sw_msa_filter* filter, const sw_hit* hits, sw_hit* hits_out, int32_t* keep, int64_t* nkept);

/* The STATISTICS of a many-query search (csrc/sw_score_hist.hip, csrc/sw_score_stats.cpp): E-values from the scores of the search
 * itself, per query, as SSEARCH estimates them -- this library takes any alphabet, table, gap costs and its own PSSMs, so no tabulated
 * Karlin-Altschul constants exist for it.  Nearly every target is unrelated to the query; the unrelated targets' score grows linearly
 * with the log of the target's length and follows an extreme-value law around that line.  Four steps:
 * 1. THE HISTOGRAM (device and host leg, integers, the same bytes on both and on every run).  Per query SW_HIST_CLASSES x SW_HIST_BINS
 *    uint32 counters, 40 KiB: d_hist[(q x 40 + c) x 256 + s] is the number of NON-EMPTY targets k with class(len_k) == c and
 *    bin(max_score) == s.  class(1) = 0; for L >= 2 with e = floor(log2 L): class(L) = 2 e + ((L >> (e - 1)) & 1) -- half octaves of
 *    the length, L < 2^20 gives c <= 39 (class 1 holds no length).  bin(v) = min(max(v, 0) >> shift, 255), shift 0..SW_HIST_SHIFT_MAX:
 *    bin 255 collects everything at or above it, a negative entry goes to bin 0.  Empty targets are counted nowhere.
 *   sw_score_hist_device  over any query-major nqueries x ntargets table of sw_result on the device; the lengths come from the handle's
 *             device copy of the offsets.  EVERY counter of d_hist is written (the call zeroes the buffer on the stream); nothing
 *             outside d_hist is written.  Asynchronous, no host round trip, host work O(1).  One launch (swp::plan_score_hist): one
 *             workgroup per (query, slice of targets) with a private histogram in LDS, LDS integer adds, then one global uint32 atomic
 *             add per non-zero counter.  The option "score_hist_copies" (0, the default: the planner's choice; 1 / 2 / 4) sets the LDS
 *             histograms per workgroup; "last_score_hist_launches" and "last_score_hist_slices" report the last call.
 *             SW_EINVAL before any launch: NULL pointers, nqueries < 0, shift out of range, a handle of another context's device,
 *             ntargets >= 2^31.  nqueries == 0 launches nothing; ntargets == 0 only zeroes.
 *   sw_score_hist_host    the CPU leg from host memory; also refuses a target length outside 0..2^20 - 1.
 * 2. INSIDE THE BOUNDED-MEMORY SEARCHES.  sw_db_search_affine_top_stats / sw_db_search_pssm_top_stats are sw_db_search_affine_top /
 *    sw_db_search_pssm_top with `shift` and `d_hist` (device, nqueries x 40 x 256 uint32): after the search of each chunk of queries, one
 *    histogram launch runs over the chunk's rows while they are in the workspace, then the selection as before.  d_hits and d_nhits are
 *    byte for byte those of the plain call; d_hist is what sw_score_hist_device gives on the full table, which never exists.
 *    SW_EINVAL in addition: NULL d_hist, shift out of range.  OUT OF SCOPE: the prefiltered search (sw_db_search_affine_top_prefiltered)
 *    scores only the pairs above a cut-off, a censored sample this fit is not made for.
 * 3. THE FIT AND THE E-VALUE (host only, double, ONE implementation for every path; floating point, so deliberately not duplicated on
 *    the device: the bit-for-bit rule covers steps 1, 2 and 4).  A caller brings the histograms to the host: 40 KiB per query and one
 *    synchronisation per round.  Per query: a cell (c, s) with s < 255 has x = c, y = s x 2^shift + (2^shift - 1) / 2 and its count as
 *    weight w; bin 255 never enters a fit (n_censored); n_db is the sum of ALL counters.  One round: W = SUM w, the weighted means mx,
 *    my, b = SUM w (x - mx)(y - my) / SUM w (x - mx)^2 (0 where the denominator is 0), a = my - b mx, r = y - a - b x, sigma^2 =
 *    SUM w r^2 / (W - 2) (sigma = 0 where W <= 2).  The first round takes every cell; three more rounds each give every cell its full
 *    count again, then zero the cells whose z = r / sigma under the PREVIOUS round's fit is > 5 or < -4 (not cumulative; a previous
 *    round without sigma > 0 drops nothing), and refit.  valid = 1 iff the last W >= 30 and sigma > 0; n_fit is the last W.
 *   sw_score_evalue  with z = (score - a - b class(len)) / sigma and gamma Euler's constant:
 *             E = n_db (1 - exp(-exp(-(pi / sqrt 6) z - gamma))), computed as -n_db expm1(-exp(...)); NaN for an invalid fit, a NULL
 *             fit or target_len < 1.
 *   sw_score_thresholds  T[q x 40 + c] = the smallest integer score with E <= evalue in class c: ceil(a + b c + sigma z0) with
 *             z0 = -(sqrt 6 / pi)(ln(-ln(1 - evalue / n_db)) + gamma), then held against sw_score_evalue itself so that
 *             E(T) <= evalue < E(T - 1) as computed.  T = 0 where evalue >= n_db or the fit is invalid: a tiny database drops
 *             nothing.  SW_EINVAL: NULL pointers, nqueries < 0, evalue not above 0.
 * 4. THE THRESHOLDS ON A HIT TABLE (device and host leg, integers, the same bytes).  The shape and the output rules of
 *    sw_msa_filter_device: keep(q, r) = 1 iff r < clamp(d_nhits[q], 0, top) (NULL d_nhits: all top entries); target, compared unsigned,
 *    < ntargets, before any load through it; the target is non-empty; max_score >= d_thresholds[q x 40 + class(len)].
 *    d_hits_out (optional): entry = input entry with target = -1 where keep is 0; d_hits_out == d_hits (in place) is allowed.  d_keep
 *    (optional): nqueries x top int32 1 / 0, EVERY entry written, usable as unit d_weights.  d_nkept (optional): nqueries int64.  At
 *    least one of d_keep and d_hits_out.  A dropped entry is not a USED ENTRY of sw_db_pssm_hit_weights, sw_db_pssm_from_hits,
 *    sw_db_msa_from_hits and the aligners, so per-query, per-length inclusion enters the loop with no signature changed: threshold a
 *    COPY of the table for the column rows, the filter, the weights and the update, with include_min_score at its minimum.
 *    Asynchronous, no host round trip, one launch, one workgroup per query.  SW_EINVAL: NULL ctx, db, d_thresholds or d_hits; a handle
 *    of another context's device; nqueries < 0; top outside 1..SW_TOP_MAX; both outputs NULL; (host leg) NULL offsets, ntargets < 0 or
 *    >= 2^31, a target length out of range.  nqueries == 0 launches nothing. */
#define SW_HIST_CLASSES 40
#define SW_HIST_BINS 256
#define SW_HIST_SHIFT_MAX 16
typedef struct { double a, b, sigma; int64_t n_db, n_fit, n_censored; int32_t valid, shift; } sw_score_fit;
int  sw_score_hist_device(sw_ctx* ctx, const sw_db* db, const sw_result* d_results, int64_t nqueries, int shift, uint32_t* d_hist, void* stream);
int  sw_score_hist_host(const sw_result* results, int64_t nqueries, const int64_t* offsets, int64_t ntargets, int shift, uint32_t* hist);
int  sw_db_search_affine_top_stats(sw_ctx* ctx, const sw_db* db, const char* d_queries, const int64_t* qoffsets, int64_t nqueries,
                                   const sw_affine* scoring, int64_t top, int64_t min_score, sw_hit* d_hits, int64_t* d_nhits, int shift,
                                   uint32_t* d_hist, void* stream);
int  sw_db_search_pssm_top_stats(sw_ctx* ctx, const sw_db* db, const int8_t* d_pssm, const int64_t* qoffsets, int64_t nqueries,
                                 const sw_pssm_scoring* scoring, int64_t top, int64_t min_score, sw_hit* d_hits, int64_t* d_nhits, int shift,
                                 uint32_t* d_hist, void* stream);
int  sw_score_fit_hist(const uint32_t* hist, int64_t nqueries, int shift, sw_score_fit* fit);
double sw_score_evalue(const sw_score_fit* fit, int64_t target_len, int64_t score);
int  sw_score_thresholds(const sw_score_fit* fit, int64_t nqueries, double evalue, int64_t* thresholds /* nqueries x 40 */);
int  sw_hits_threshold_device(sw_ctx* ctx, const sw_db* db, const int64_t* d_thresholds, int64_t nqueries, int64_t top, const sw_hit* d_hits,
                              const int64_t* d_nhits, sw_hit* d_hits_out, int32_t* d_keep, int64_t* d_nkept, void* stream);
int  sw_hits_threshold_host(const int64_t* offsets, int64_t ntargets, const int64_t* thresholds, int64_t nqueries, int64_t top,
                            const sw_hit* hits, const int64_t* nhits, sw_hit* hits_out, int32_t* keep, int64_t* nkept);

/* LOW-COMPLEXITY MASKING of a database, on the device (csrc/sw_mask.hip): the stage in front of the search loop.  Compositionally
 * biased stretches (poly-Q, SGSGSG..., collagen-like repeats) score high against each other without being related, and the E-values
 * above make it worse: such targets are the outliers the trimmed fit removes from the null line.  The call writes a MASKED COPY of a
 * handle's bytes with the same offsets; the caller makes a second handle over it (sw_db_create(ctx, d_out, offsets, ntargets, &masked))
 * and searches, selects, aligns and updates on that one, while hit tables and ops carry indices, not letters, so sw_db_msa_from_hits
 * can still be given the UNMASKED handle: the A3M keeps the original letters (what BLAST calls soft masking).
 * THE RULE is the first stage of SEG (Wootton & Federhen 1993) -- trigger windows, extended through overlapping windows of slightly
 * higher complexity -- restated in integers.  SEG's second stage, which trims each raw segment by a log-probability optimisation, is
 * floating point and deliberately left out: this masker is somewhat GREEDIER AT THE SEGMENT ENDS than `seg`.  Per target t[0 .. len):
 *   sw_mask_params : window W, 2..64 (SEG: 12); trigger_mbits K1 and extend_mbits K2, 0 <= K1 <= K2, entropy in thousandths of a bit
 *                (SEG: 2200, 2500); letters / nletters, the alphabet, 1..32 distinct bytes -- every other byte is NO LETTER;
 *                mask_byte, what a masked position becomes.
 *   G          : G[c] = floor(c x log2(c) x 65536 + 0.5), c = 0..64, G[0] = G[1] = 0: 65 integer literals in csrc/sw_mask_table.h,
 *                which the kernel and the host leg both include; never computed at run time.
 *   valid(i)   : i + W <= len and none of t[i .. i + W) is a no-letter.  Windows never cross a target's end.
 *   D(i)       : for a valid start, G[W] - SUM_k G[c_k], c_k the count of letters[k] in the window: W x 65536 x the window's Shannon
 *                entropy in bits, an integer >= 0.
 *   low1(i)    : valid(i) and 1000 x D(i) <= K1 x W x 65536, that is D(i) <= floor(K1 x W x 65536 / 1000); low2(i) the same with K2.
 *                The host computes the two right-hand sides once in 64-bit integers; the kernel compares int32.
 *   run        : a maximal sequence of consecutive starts s .. e with low2; TRIGGERED when low1 holds for at least one of them.
 *   masked(p)  : p lies in [s, e + W) of a triggered run.
 *   out[p]     : mask_byte where masked(p), t[p] verbatim otherwise, for any byte 0..255.
 *   So: a target shorter than W is never masked, an empty target contributes nothing.  No floats: device, host leg and any
 *   restatement agree bit for bit, every run writes the same bytes.
 * sw_db_mask_low_complexity:
 *   db         : a handle over the UNMASKED bytes.
 *   d_out      : device memory laid out like the handle's d_db: byte p of d_out answers byte p of d_db.  Exactly
 *                [offsets[0], offsets[ntargets]) is written, nothing outside.  d_out == d_db (in place) is REFUSED; buffers that
 *                overlap in part are the caller's error and are not detected.
 *   d_nmasked  : device, ntargets int64, optional: the masked positions per target, EVERY entry written, 0 for an empty target.
 *   Asynchronous on `stream`, no host round trip, host work O(1): the lengths come from the handle's device copy of the offsets.
 *   (As with every workspace of the context: the first call that needs a larger one than any call before waits for the stream once
 *   and allocates.)
 *   Flat over the concatenated bytes in tiles of swp::kMaskTile positions (swp::plan_mask), whatever the targets' lengths; per
 *   position two bits (low1, low2) and the mask bit in a workspace of the context.  Launches: WINDOWS (one workgroup per tile: letter
 *   classes and target ends staged in LDS, a lane slides over consecutive starts with its counts in LDS, a summary per tile), CARRIES
 *   (one workgroup: for every tile border, whether the run that crosses it is triggered anywhere, however far away), APPLY (triggers
 *   spread through runs a 64-position word at a time by add-with-carry, dilated by W, the bytes written) and, with d_nmasked, COUNT
 *   (population counts of the mask bits between a target's offsets; no atomics).  "last_mask_launches" and "last_mask_tiles" report
 *   the last call, "mask_tile" (read-only) the positions of a tile.  A handle without letters launches nothing but the zeroes of d_nmasked.
 *   QUERIES need no call of their own: a handle over the query bytes (sw_db_create on d_queries and the query offsets) costs next to
 *   nothing; on the host sw_mask_low_complexity_host serves them as it serves targets.
 *   SW_EINVAL before any launch: NULL pointers; a handle of another context's device; d_out == d_db; window outside 2..64;
 *   trigger_mbits < 0, extend_mbits < trigger_mbits, or a value for which K x W x 65536 leaves int64; nletters outside 1..32 or a
 *   letter named twice.
 * sw_mask_low_complexity_host: the CPU leg, the rule restated window by window in plain C++ from host memory.  seq and out are indexed
 *   by the offsets themselves (seq + offsets[t]); out == seq is refused likewise; SW_EINVAL besides for negative or decreasing offsets. */
typedef struct {
    int64_t trigger_mbits, extend_mbits;
    int32_t window, nletters;
    unsigned char letters[32];
    unsigned char mask_byte;
} sw_mask_params;
int  sw_db_mask_low_complexity(sw_ctx* ctx, const sw_db* db, const sw_mask_params* params, char* d_out, int64_t* d_nmasked, void* stream);
int  sw_mask_low_complexity_host(const char* seq, const int64_t* offsets, int64_t ntargets, const sw_mask_params* params, char* out,
                                 int64_t* nmasked);

/* Tables.  sw_submat_match: s[x][y] = x == y ? match : mismatch (matchMissmatchScore, serial_smithW.c:251-256; both must fit int8:
 * the builder returns nothing, so it clamps them to -128..127 -- a caller that takes them from a user checks the range first, as
 * smithW and the Python wrapper do, which refuse such scores).  sw_submat_from_letters: `scores` is n x n, row = query letter, over the n bytes of
 * `letters`; every pair with a byte not in `letters` scores `other` (n 1..256, no letter twice, other within int8).
 * sw_read_submat: the NCBI text format -- '#' comment lines and blank lines are skipped, a header line of letters, then rows of
 * one letter followed by n integers (row = query letter); lower-case letters in the file are upper-cased, every entry must fit
 * int8, every row must have n entries and name a header letter; `other` is the smallest entry of the file.  No table is built in. */
void sw_submat_match(int match, int mismatch, sw_submat* out);
int sw_submat_from_letters(const char* letters, int n, const int8_t* scores, int other, sw_submat* out);
int sw_read_submat(const char* path, sw_submat* out);

/* Every record of a FASTA file in one pass, under the parsing rules of sw_read_fasta.  Two-call pattern:
 * with seq == NULL it reports the counts only (*nrecords, *total_len).  Otherwise seq receives total_len bytes (seq_cap
 * at least that) and offsets nrecords + 1 entries (offsets_cap at least that): record k = seq[offsets[k] .. offsets[k+1]),
 * so the output goes straight into sw_search_device.  A file without any record reports 0 records. */
int sw_read_fasta_db(const char* path, char* seq, int64_t seq_cap, int64_t* offsets, int64_t offsets_cap,
                     int64_t* nrecords, int64_t* total_len);

/* Host-buffer convenience wrapper around sw_fill_device (alloc, H2D, fill, D2H, sync).
 * H, P: caller-owned int32 (rows+1)*(cols+1); either may be NULL to skip its copy-out. */
int sw_fill_host(sw_ctx* ctx, const char* a, int64_t cols, const char* b, int64_t rows,
                 const sw_scores* scores, int32_t* H, int32_t* P, sw_result* result);

/* Adaptive dispatch (the reference's per-diagonal choice of serial / OpenMP / offload,
 * omp_smithW-v7-adaptive.cpp:304-396): tiny problems are filled on the host by sw_fill_cpu (the reference recurrence,
 * serial_smithW.c:141-145,187-244), everything else on ctx's GPU (ctx may be NULL: host only); the traceback runs on
 * the host P either way, so H, P, max_pos, max_score and path_len come back exactly as serial_smithW leaves them.
 * used_gpu (optional) reports the choice. */
int sw_align_auto(sw_ctx* ctx, const char* a, int64_t cols, const char* b, int64_t rows, const sw_scores* scores,
                  int32_t* H, int32_t* P, sw_result* result, int* used_gpu);
int sw_fill_cpu(const char* a, int64_t cols, const char* b, int64_t rows, const sw_scores* scores, int32_t* H, int32_t* P,
                sw_result* result);
/* The same with the reference's THREE executors (omp_smithW-v7-adaptive.cpp:304-396: serial / OpenMP / offload per diagonal):
 * executor 0 = host fill, 1 = one GPU (ctx if given, else a context made on devices[0]), 2 = row bands over all `ndev` devices
 * (sw_multi_*; an id may repeat).  N GPUs are used from multi_min_cells cells on (0 = 4e9, about 65536^2: below that a single pair
 * is bound by its strip chain, which more GPUs do not shorten) or when H + P do not fit devices[0].  Same outputs as sw_align_auto. */
int sw_align_auto_multi(sw_ctx* ctx, const int* devices, int ndev, const char* a, int64_t cols, const char* b, int64_t rows,
                        const sw_scores* scores, int32_t* H, int32_t* P, sw_result* result, int* executor, int64_t multi_min_cells);

/* ---- traceback: replaces backtrack(), serial_smithW.c:262-277.  Negates P along the path.  One wave walks 64 x 64 windows of P
 * held in registers (csrc/sw_traceback.hip): ~35 ns per step instead of a memory latency.
 * d_path (optional) receives the visited linear indices (capacity path_cap);
 * d_result->path_len is set.  P[max_pos]==NONE (UB in the reference) == empty path. */
int sw_traceback_device(sw_ctx* ctx, int32_t* d_P, int64_t cols, int64_t rows, int64_t max_pos,
                        int64_t* d_path, int64_t path_cap, sw_result* d_result, void* stream);
int sw_traceback_host(int32_t* P, int64_t cols, int64_t rows, int64_t max_pos,
                      int64_t* path, int64_t path_cap, int64_t* path_len);
/* the same on an int32 (p_elem_bytes 4) or compact int8 (1) predecessor matrix */
int sw_traceback_device_ex(sw_ctx* ctx, void* d_P, int p_elem_bytes, int64_t cols, int64_t rows, int64_t max_pos,
                           int64_t* d_path, int64_t path_cap, sw_result* d_result, void* stream);
int sw_traceback_host_ex(void* P, int p_elem_bytes, int64_t cols, int64_t rows, int64_t max_pos,
                         int64_t* path, int64_t path_cap, int64_t* path_len);

/* Compact predecessor matrix back to the reference's layout (a compact P "must still round-trip to the
 * int32 H/P layout"): d_P32[k] = (int32_t)d_P8[k] for k < count -- codes 0..3, and -1..-3 along a traced path.  The two
 * buffers must not overlap. */
int sw_p8_to_p32_device(sw_ctx* ctx, const void* d_P8, int32_t* d_P32, int64_t count, void* stream);

/* 2-bit predecessor matrix (the reference's own "keep less" variant is the rolling-buffer fill,
 * rotated-cuda/sw-rotated-omp.cc:214-224): the codes 0..3 of serial_smithW.c:23-27 need two bits, so 262144^2 predecessors take
 * 17 GB instead of 69 GB (int8) or 275 GB (the reference's int32).  Layout: 4 cells per byte, cell k (row-major linear index, as in
 * P) in bits 2*(k&3)..2*(k&3)+1 of byte k>>2.  Two bits cannot hold the sign backtrack() leaves on a path (P[pos] *= PATH,
 * serial_smithW.c:271): a traced path is a bitmap beside the matrix, bit k&31 of 32-bit word k>>5.
 *   SW_P2_BYTES(count) / SW_PATHBITS_BYTES(count): buffer sizes for `count` cells (whole 32-cell groups)
 *   sw_p_to_p2_device   packs an int8 (p_elem_bytes 1) or int32 (4) matrix; negative (traced) cells set their bit in d_pathbits
 *                       (optional, may be NULL; every word of it is written)
 *   sw_p2_to_p32_device the round trip to the reference layout: d_P32[k] = code, negated where d_pathbits (optional) marks it
 *   sw_traceback_p2_device  backtrack() on the packed matrix: marks the path in d_pathbits (optional; zeroed by the caller),
 *                       writes the visited indices to d_path (optional) and d_result->path_len -- same walk, same kernel family
 *                       as sw_traceback_device */
#define SW_P2_BYTES(count) ((((size_t)(count) + 31) / 32) * 8)
#define SW_PATHBITS_BYTES(count) ((((size_t)(count) + 31) / 32) * 4)
int sw_p_to_p2_device(sw_ctx* ctx, const void* d_P, int p_elem_bytes, void* d_P2, uint32_t* d_pathbits, int64_t count, void* stream);
int sw_p2_to_p32_device(sw_ctx* ctx, const void* d_P2, const uint32_t* d_pathbits, int32_t* d_P32, int64_t count, void* stream);
int sw_traceback_p2_device(sw_ctx* ctx, const void* d_P2, int64_t cols, int64_t rows, int64_t max_pos, uint32_t* d_pathbits,
                           int64_t* d_path, int64_t path_cap, sw_result* d_result, void* stream);

/* ---- verification helpers (not on the timed path) ------------------------------------------
 * Position-weighted row checksums of a device matrix with (rows1 x m) elements:
 *   cs[i] = sum_j (uint64)(uint32)X[i][j] * ((j+1) * 0x9E3779B97F4A7C15)  (mod 2^64)
 * elem_bytes 1, 4 or 8 (1: int8 values are sign-extended first, so a compact P checksums like its int32
 * widening; 8: low 32 bits are summed and the high half must be the sign extension, otherwise cs[i] is
 * forced to ~0). d_cs: rows1 uint64 on the device. */
int sw_row_checksums_device(sw_ctx* ctx, const void* d_X, int elem_bytes, int64_t rows1, int64_t m,
                            uint64_t* d_cs, void* stream);

/* ---- output buffers placed for speed -------------------------------------------------------
 * Physical HBM falls into a few coarse classes (regions of tens of GiB; three on MI355X), and two store streams into the SAME class
 * run ~1.4x slower than into different ones.  A fill stores H[r][c] and P[r][c] together: a 16384^2 fill takes 0.79 ms with H and P
 * in different classes and 1.05 ms with both in one -- the usual outcome of two back-to-back hipMallocs.  sw_alloc_outputs places the
 * pair:
 *   trials <= 0  (default) candidates for P -- three plain ones, then behind temporary spacer allocations of 8-160 GiB (taken only while
 *                8 GiB of head room remain, released at once) -- are classified against H with a two-stream store probe
 *                (csrc/sw_place.hip; ~0.3 ms per candidate, no fill of the caller's problem, d_a / d_b not needed); the first one in
 *                another class is kept (matrices of many GiB span classes themselves: 8 sample windows, the best of five candidates).
 *                Below 512 MiB of output a plain pair (such a fill is not bound by its stores).  The search runs against a time budget,
 *                option "placement_budget_ms" (default 1500): fresh memory costs 0.3 ms per allocation and the call takes 2-5 ms, but
 *                memory that was in use before is wiped by the driver (~30 GiB/s) before it is handed out again, nothing tells
 *                beforehand, and a spacer can then cost seconds -- so a spacer is tried only while its WORST case (40 ms per GiB)
 *                still fits the budget (the default admits spacers up to 37 GiB), and when the budget is spent the best
 *                candidate seen is handed out (sw_get_option "last_placement_ratio_x1000": ~1300-1450 = different classes,
 *                ~2000 = one class).  A caller that fills many times into the pair raises the budget (bench.py: 20 s).
 *   trials == 1  a plain pair.
 *   trials  > 1  round 3's search: up to `trials` candidates, three fills of the caller's problem into each on the DEFAULT stream
 *                (d_a / d_b must be ready), the fastest kept.
 * trial_ms (optional; max(trials, 16) floats) receives per candidate the time of the probe (or of a trial fill), 0 for those not
 * needed.  The contents of the returned buffers are undefined.  Release with sw_free_outputs (d_P may sit inside a larger allocation).
 * (sw_multi_create and sw_fill_host place their matrices the same way; results never depend on placement.) */
int sw_alloc_outputs(sw_ctx* ctx, const char* d_a, int64_t cols, const char* d_b, int64_t rows, const sw_scores* scores,
                     int h_elem_bytes, int p_elem_bytes, int trials, void** d_H, void** d_P, float* trial_ms);
int sw_free_outputs(sw_ctx* ctx, void* d_H, void* d_P);
/* The classifier of sw_alloc_outputs for buffers the caller allocated itself: how much slower two store streams into (d_X, d_Y) run
 * together than one stream into d_X alone -- *ratio ~1.3-1.45: the two lie in different classes of the HBM, ~2.0: in the same one (a fill
 * that writes H into one and P into the other is then ~1.3x slower).  Samples windows of up to 128 MiB (8 of them for buffers of more
 * than 6 GiB) and WRITES them: call it before the buffers hold anything.  Runs on the current device, default stream, ~0.2 ms per window;
 * ms_together (optional): the time of the two-stream probe. */
int sw_place_pair_ratio(void* d_X, size_t xbytes, void* d_Y, size_t ybytes, float* ratio, float* ms_together);

/* ---- device memory plumbing for hosts without a HIP binding (cgo / JNI / ctypes callers) --- */
int sw_device_malloc(sw_ctx* ctx, size_t bytes, void** d_ptr);
int sw_device_free(sw_ctx* ctx, void* d_ptr);
int sw_memcpy_h2d(sw_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int sw_memcpy_d2h(sw_ctx* ctx, void* dst, const void* d_src, size_t bytes);
int sw_synchronize(sw_ctx* ctx, void* stream);   /* waits for `stream`; reports kernel faults */

/* ---- tuning knobs (0 = built-in default) --------------------------------------------------
 * None of them changes a result bit; they only move time.
 *   "engine"            0 systolic (default), 1 strip_scan
 *   "strips_per_group"  systolic: strips (producer waves) per workgroup, 1 or 2 (0: 1 for a single pair with up to
 *                       4.5 strips per CU or a batch that fits the CUs at once, else 2)
 *   "consumers"         systolic: consumer waves per strip: 2, 3, 4; also 6, 7 with one strip per group (0: with one strip per
 *                       group 4 up to ~3.5e8 cells and 6 above, with two strips 4; 8 is taken as 7).  The two-columns-per-lane
 *                       kernel (whole-matrix or band fills of one pair, any number of rows; csrc/sw_systolic2.inc) takes 4..7 from
 *                       this option (0: 7 behind scout workgroups, else 5 up to ~3.5e8 cells, 6 above) and runs 9 minus that many
 *                       importer waves
 *   "store_policy"      systolic H/P stores: 0 by problem size and strip geometry (streaming up to 6e8 cells and wherever whole lines are stored),
 *                       1 write-back, 2 streaming (nt)
 *   "importers"         systolic, one strip per workgroup: waves polling the left neighbour's edge column, besides the one that
 *                       always does (0: 4 up to ~3.5e8 cells, 2 above; at most what 12 waves per workgroup leave)
 *   "xcd_order"         systolic: 1 = neighbouring strip groups run on the same XCD
 *   "pace_ps"           systolic: strip 0 releases one row per this many picoseconds (0 = unpaced)
 *   "xcd_chain"         two-column kernel without scout workgroups: the strips of a pass dealt per XCD, edge columns through that XCD's
 *                       L2 (0: from 384 strips on, 1 on, 2 off)
 *   "filler_hop_ps", "filler_tau_ps", "filler_bw_gbs"   two-column kernel behind scout workgroups: pacing of the workgroups that
 *                       write H / P -- estimate of a strip hand-off (2400000 ps; 0 = no pacing), time per row of
 *                       an unhindered strip (25000 ps), store bandwidth the strips share (4200 GB/s)
 *   "band_wait_ms"      sw_fill_band_device: how long a strip waits for its halo granules before the launch aborts
 *                       with SW_ETIMEOUT (default 20000)
 *   "s2w"               two-column kernel: strips every 126 columns, or every 110 -- 126 wide, overlapping by 16 columns, so that every
 *                       64-byte line of a matrix row lies inside one strip and is stored whole, by one instruction;
 *                       0: the library chooses (110, with streaming stores, for matrices with H written and P int32, absent, or int8 beside an int32 H -- even
 *                       widths but for int32 H + int32 P -- that
 *                       are too wide for scout workgroups: more than ~21 500 columns, 18 700 with an int64 H), 126 / 110 force one
 *   "split_blk", "split_from"   two-column kernel behind scouts: from strip `split_from` on, the strip's scout writes the matrix
 *                       blocks from `split_blk` on itself (0: the library chooses)
 *   "probe_foreign_pairs"  1: an H / P pair the library did not allocate is probed once, at its first fill (big int32 fills behind scouts only): the
 *                       probe WRITES both buffers -- the fill overwrites them anyway -- and synchronises the stream (~0.3 ms); a pair found to
 *                       lie in one class of the HBM is then filled with overlapping strips (16384^2: ~310 instead of ~235 GCUPS).  Default 0
 *                       (pairs from sw_alloc_outputs are known without it)
 *   "placement_hold_gib"  sw_alloc_outputs: where no candidate pair lies in two classes of the HBM (the usual case once most of a device's memory
 *                       has been in use: the driver then hands out the little clean memory it has, all of one class), P may be allocated with up
 *                       to this many GiB of slack and slid inside its own allocation to where the probe is good; the slack stays allocated
 *                       while the pair lives (sw_get_option "last_placement_held_gib").  Default 0; pairs of many GiB take up to 32 by themselves
 *   "placement_budget_ms"  sw_alloc_outputs: how long the search for an H / P pair in different classes of the HBM may take at worst (default 1500; 2-5 ms on memory that needs no wiping)
 *   "max_blocks"        cap of the resident grid (0 = all CUs); concurrent band launches partition the CUs with it
 *   "waves_per_block", "debug_flags", "debug_buf", "batch_lds"   development aids (debug_flags: the bits of swk::DebugFlag in
 *                       smith-waterman_amd/csrc/sw_debug.h)
 * sw_get_option also answers "last_grid", "last_strips", "last_strips2" (strips of the two-column kernel), "last_perm" (1: the last fill's
 * scores and size allowed the perm producer; the letter count, found on the device, still has to), "last_scouts"
 * (scout workgroups of the last fill), "last_xcd_mode" (1: that fill dealt its roles per XCD), "last_scan_all" (1: every workgroup of that fill
 * scanned the alphabet for itself, 0: the shared scan behind a grid barrier), "xcd_round_robin" (1: sw_create saw
 * workgroup i of a launch on XCD i % 8), "last_batch_kernel" (0: the last batch ran on the fall-back, 1: one pair per wave, 2: two pairs per
 * wave on packed lanes), "last_search_kernel" (the last search: 2 * (columns per lane / 8) + 1 for the wide profile), "last_search_affine_kernel"
 * (the last affine search: columns per lane / 8) and "last_search_affine_grid" (its workgroups), "last_align_affine_kernel" (the
 * last sw_align_affine_device call: columns per lane / 8) and "last_align_affine_slots" (its direction matrices, one per wave at
 * work); "align_workspace_mib" (settable, default 1024) bounds the direction workspace of that call;
 * "align_checkpoint" (settable, default 0) chooses how sw_align_affine_device and sw_db_align_affine_hits keep the directions of a
 * hit: 0 the whole matrix, one byte per cell, as described at the two calls; 1 checkpointed: a score-only sweep saves H and E of
 * every B-th row (8 bytes per column), and only the bands of B rows the walk enters are re-filled with direction bytes, each resumed
 * from the checkpoint above it, so a slot takes qpad * (min(B, len) + 8 * (ceil(len / B) - 1)) bytes instead of qpad * len and the
 * results are the same byte for byte (the argument rules of the two calls stay as they are: no target above 2^20 - 1 letters is
 * accepted, checkpointed or not); 2 checkpointed for exactly the calls that 0 would refuse for size, the whole matrix otherwise
 * (decided on the host once per call, before any launch).  "align_checkpoint_rows" (settable, default 0) is B: 0 leaves it to the
 * planner (the power of two from 256 to 2^20 that makes the slot smallest), otherwise a power of two in 64..2^20, anything else is
 * SW_EINVAL.  "last_align_affine_checkpointed" (0 / 1), "last_align_affine_band_rows" (B, 0 for whole matrices) and
 * "last_align_affine_slot_bytes" describe the last sw_align_affine_device call, "last_align_hits_checkpointed" and
 * "last_align_hits_band_rows" (the largest B over its launches) the last sw_db_align_affine_hits call.  "debug_buf" and
 * "align_checkpoint": a checkpointed sw_align_affine_device call adds THREE words of wave ticks (sweep, walk, re-fills) where the
 * whole-matrix call adds two, and under 2 the caller does not know beforehand which runs -- whenever "align_checkpoint" is not 0 the
 * buffer "debug_buf" names must hold at least three 8-byte words;
 * "search_profile_mib" (settable,
 * default 256) bounds the profiles of a group of sw_db_search_affine, "last_search_multi_groups", "last_search_multi_launches" and
 * "last_search_multi_grid" (workgroups of its last launch) describe the last such call; "search_lanes" (settable, 32 or 16, default
 * 32) sends the queries of the many-query search whose scores fit 16 bits to the kernel that runs two targets per wave on packed lanes
 * (sw_db_search_affine above has the rule) and "last_search_multi_packed_launches" counts those launches; "search_results_mib" (settable, default 1024,
 * 1..2^20) bounds the result rows a chunk of sw_db_search_affine_top holds, "last_search_top_chunks" and "last_search_top_kernel"
 * describe the last sw_db_search_affine_top / sw_top_hits_device call; "last_align_hits_launches", "last_align_hits_tiers",
 * "last_align_hits_slots" and "last_align_hits_lists" the last sw_db_align_affine_hits call; "search_pairs_chunk" (settable, default
 * 2^22, 1..2^31 - 1) is the most entries of a pair list that sw_db_search_affine_pairs bins at a time, "last_search_pairs_groups",
 * "last_search_pairs_chunks" and "last_search_pairs_launches" describe the last such call, "search_pairs_lanes" (settable, 32 or 16,
 * default 32) sends the listed pairs of the queries whose scores fit 16 bits to the kernel that runs two pairs per wave on packed lanes
 * (sw_db_search_affine_pairs above has the rule), "last_search_pairs_packed_launches" counts those launches and
 * "last_search_pairs_packed_items" the two-pair work items the device built (reading it waits for the device); "prefilter_lanes" (settable, 0 or 32) and
 * "last_prefilter_groups", "last_prefilter_launches", "last_prefilter_packed_launches" belong to sw_db_prefilter_ungapped (above);
 * "last_top_pairs_launches" and "last_top_pairs_kernel" describe the last sw_top_hits_pairs_device call, and "search_results_mib" also
 * bounds the pairs_cap of sw_db_search_affine_top_prefiltered (56 bytes per entry); "score_hist_copies" (settable: 0, the default, the
 * planner's choice, or 1 / 2 / 4) sets the LDS histograms a workgroup of the score histogram keeps, "last_score_hist_launches" and
 * "last_score_hist_slices" (slices of targets per query) describe the last sw_score_hist_device / _top_stats call.
 * "debug_search_pairs_items_ptr" (an
 * accessor for tests) is the device address of that call's item workspace, which a call leaves as its last (chunk, group) filled it:
 * 24-byte items {int64 start, int64 out, int32 len, int32 entry}, the classes' lists back to back (under "search_pairs_lanes" = 16 the
 * two-pair items of a group with packed queries come first, 48 bytes each, the 24-byte items behind them). */
int sw_set_option(sw_ctx* ctx, const char* name, int64_t value);
int64_t sw_get_option(sw_ctx* ctx, const char* name);

#ifdef __cplusplus
}
#endif
#endif
