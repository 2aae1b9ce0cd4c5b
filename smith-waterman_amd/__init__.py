"""smith-waterman_amd -- host-side mirror (ctypes) of the C-ABI in include/swhip.h.

The product is libswhip.so (hand-written gfx950 HIP kernels + a C-ABI); this module is plumbing
for tests / bench / Python callers: torch provides device memory and streams only.  There is NO
CPU fallback: if libswhip.so is missing, importing the library handle raises.

Names follow the reference (paths relative to the reference repository):
  generate()            serial_smithW.c:334-361
  Engine.fill()         fill loop + similarityScore, serial_smithW.c:141-145,187-256;
                        smithWaterman(a,b,w,h,H,P,&maxloc), rotated-cuda/sw-rotated-omp.cc:192-209
  Engine.traceback()    backtrack(), serial_smithW.c:262-277
  n_element / first_diag_element    omp_smithW.c:260-291
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import weakref
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SWHIP_LIBRARY") or os.path.join(_HERE, "libswhip.so")  # override: A/B builds of the kernels

NONE, UP, LEFT, DIAGONAL, PATH = 0, 1, 2, 3, -1
DEFAULT_SCORES = (3, -3, -2)  # serial_smithW.c:59-61


class SwError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"swhip error {code}: {msg}")
        self.code = code


class _Scores(ctypes.Structure):
    _fields_ = [("match", ctypes.c_int32), ("mismatch", ctypes.c_int32), ("gap", ctypes.c_int32)]


class _Result(ctypes.Structure):
    _fields_ = [("max_pos", ctypes.c_int64), ("max_score", ctypes.c_int64), ("path_len", ctypes.c_int64)]


class _Affine(ctypes.Structure):   # sw_affine: the table by pointer
    _fields_ = [("sub", ctypes.c_void_p), ("gap_open", ctypes.c_int32), ("gap_extend", ctypes.c_int32)]


class _PssmScoring(ctypes.Structure):   # sw_pssm_scoring: the letters by pointer
    _fields_ = [("letters", ctypes.c_void_p), ("nletters", ctypes.c_int32), ("other", ctypes.c_int32), ("smax", ctypes.c_int32),
                ("gap_open", ctypes.c_int32), ("gap_extend", ctypes.c_int32)]


class _PssmUpdate(ctypes.Structure):   # sw_pssm_update: the table by pointer
    _fields_ = [("sub", ctypes.c_void_p), ("prior_weight", ctypes.c_int32), ("include_min_score", ctypes.c_int64)]


class _PssmWeighting(ctypes.Structure):   # sw_pssm_weighting
    _fields_ = [("per_hit", ctypes.c_int32), ("include_min_score", ctypes.c_int64)]


class _MsaFilter(ctypes.Structure):   # sw_msa_filter
    _fields_ = [("max_ident_pct", ctypes.c_int32), ("min_cover_pct", ctypes.c_int32)]


class _MaskParams(ctypes.Structure):   # sw_mask_params
    _fields_ = [("trigger_mbits", ctypes.c_int64), ("extend_mbits", ctypes.c_int64), ("window", ctypes.c_int32), ("nletters", ctypes.c_int32),
                ("letters", ctypes.c_ubyte * 32), ("mask_byte", ctypes.c_ubyte)]


# every symbol include/swhip.h declares: (restype, argtypes)
_vp, _i64, _i32, _u32, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_uint32, ctypes.c_size_t
ABI = {
    "sw_last_error": (ctypes.c_char_p, []),
    "sw_version": (ctypes.c_char_p, []),
    "sw_generate": (_i32, [_i64, _i64, _u32, _vp, _vp]),
    "sw_read_fasta": (_i32, [ctypes.c_char_p, _i64, _vp, _i64, ctypes.POINTER(_i64)]),
    "sw_read_fasta_db": (_i32, [ctypes.c_char_p, _vp, _i64, _vp, _i64, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    "sw_nelement": (_i64, [_i64, _i64, _i64]),
    "sw_first_diag_element": (None, [_i64, _i64, _i64, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    "sw_create": (_i32, [_i32, ctypes.POINTER(_vp)]),
    "sw_destroy": (None, [_vp]),
    "sw_fill_device": (_i32, [_vp, _vp, _i64, _vp, _i64, ctypes.POINTER(_Scores), _vp, _i32, _vp, _vp, _vp, _vp]),
    "sw_fill_tile_device": (_i32, [_vp, _vp, _i64, _vp, _i64, ctypes.POINTER(_Scores), _vp, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "sw_batch_device": (_i32, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _i64, ctypes.POINTER(_Scores), _vp, _vp, _vp, _vp]),
    "sw_batch_device_ex": (_i32, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _i64, ctypes.POINTER(_Scores), _vp, _vp, _i32, _vp, _vp]),
    "sw_search_device": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, ctypes.POINTER(_Scores), _vp, _vp]),
    "sw_search_affine_device": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, ctypes.POINTER(_Affine), _vp, _vp]),
    "sw_search_affine_host": (_i32, [_vp, _i64, _vp, _vp, _i64, ctypes.POINTER(_Affine), _vp]),
    "sw_db_create": (_i32, [_vp, _vp, _vp, _i64, ctypes.POINTER(_vp)]),
    "sw_db_free": (None, [_vp]),
    "sw_db_info": (_i32, [_vp, ctypes.POINTER(_i64), ctypes.POINTER(_i64), ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    "sw_db_search_affine": (_i32, [_vp, _vp, _vp, _vp, _i64, ctypes.POINTER(_Affine), _vp, _vp]),
    "sw_search_affine_multi_host": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, ctypes.POINTER(_Affine), _vp]),
    "sw_db_search_affine_pairs": (_i32, [_vp, _vp, _vp, _vp, _i64, ctypes.POINTER(_Affine), _vp, _i64, _vp, _vp]),
    "sw_search_affine_pairs_host": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, ctypes.POINTER(_Affine), _vp, _i64, _vp]),
    "sw_db_prefilter_ungapped": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp]),
    "sw_prefilter_ungapped_host": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp]),
    "sw_top_hits_device": (_i32, [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp]),
    "sw_db_search_affine_top": (_i32, [_vp, _vp, _vp, _vp, _i64, ctypes.POINTER(_Affine), _i64, _i64, _vp, _vp, _vp]),
    "sw_search_affine_multi_top_host": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, ctypes.POINTER(_Affine), _i64, _i64, _vp, _vp]),
    "sw_top_hits_pairs_device": (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp]),
    "sw_top_hits_pairs_host": (_i32, [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp]),
    "sw_db_search_affine_top_prefiltered": (_i32, [_vp, _vp, _vp, _vp, _i64, ctypes.POINTER(_Affine), _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    "sw_db_align_affine_hits": (_i32, [_vp, _vp, _vp, _vp, _i64, ctypes.POINTER(_Affine), _vp, _vp, _i64, _vp, _vp, _i64, _vp]),
    "sw_align_affine_hits_host": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, ctypes.POINTER(_Affine), _vp, _vp, _i64, _vp, _vp, _i64]),
    "sw_db_search_pssm": (_i32, [_vp, _vp, _vp, _vp, _i64, ctypes.POINTER(_PssmScoring), _vp, _vp]),
    "sw_db_search_pssm_top": (_i32, [_vp, _vp, _vp, _vp, _i64, ctypes.POINTER(_PssmScoring), _i64, _i64, _vp, _vp, _vp]),
    "sw_db_align_pssm_hits": (_i32, [_vp, _vp, _vp, _vp, _i64, ctypes.POINTER(_PssmScoring), _vp, _vp, _i64, _vp, _vp, _i64, _vp]),
    "sw_search_pssm_multi_host": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, ctypes.POINTER(_PssmScoring), _vp]),
    "sw_align_pssm_hits_host": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, ctypes.POINTER(_PssmScoring), _vp, _vp, _i64, _vp, _vp, _i64]),
    "sw_pssm_from_queries": (_i32, [_vp, _vp, _i64, _vp, _vp, _i32, _vp]),
    "sw_read_pssm": (_i32, [ctypes.c_char_p, _vp, ctypes.POINTER(ctypes.c_int32), _vp, _i64, ctypes.POINTER(_i64)]),
    "sw_db_pssm_from_hits": (_i32, [_vp, _vp, _vp, _vp, _i64, ctypes.POINTER(_PssmScoring), ctypes.POINTER(_PssmUpdate), _vp, _vp, _i64, _vp, _vp, _i64, _vp,
                                    _vp, _vp, _vp]),
    "sw_pssm_from_hits_host": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, ctypes.POINTER(_PssmScoring), ctypes.POINTER(_PssmUpdate), _vp, _vp, _i64, _vp, _vp,
                                      _i64, _vp, _vp, _vp]),
    "sw_db_pssm_hit_weights": (_i32, [_vp, _vp, _vp, _i64, ctypes.POINTER(_PssmScoring), ctypes.POINTER(_PssmWeighting), _vp, _vp, _i64, _vp, _vp, _i64, _vp,
                                      _vp]),
    "sw_pssm_hit_weights_host": (_i32, [_vp, _i64, _vp, _vp, _i64, ctypes.POINTER(_PssmScoring), ctypes.POINTER(_PssmWeighting), _vp, _vp, _i64, _vp, _vp,
                                        _i64, _vp]),
    "sw_db_msa_from_hits": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp]),
    "sw_msa_from_hits_host": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    "sw_msa_filter_device": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, ctypes.POINTER(_MsaFilter), _vp, _vp, _vp, _vp, _vp]),
    "sw_msa_filter_host": (_i32, [_vp, _vp, _vp, _i64, _i64, ctypes.POINTER(_MsaFilter), _vp, _vp, _vp, _vp]),
    "sw_db_mask_low_complexity": (_i32, [_vp, _vp, ctypes.POINTER(_MaskParams), _vp, _vp, _vp]),
    "sw_mask_low_complexity_host": (_i32, [_vp, _vp, _i64, ctypes.POINTER(_MaskParams), _vp, _vp]),
    "sw_score_hist_device": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp, _vp]),
    "sw_score_hist_host": (_i32, [_vp, _i64, _vp, _i64, _i32, _vp]),
    "sw_db_search_affine_top_stats": (_i32, [_vp, _vp, _vp, _vp, _i64, ctypes.POINTER(_Affine), _i64, _i64, _vp, _vp, _i32, _vp, _vp]),
    "sw_db_search_pssm_top_stats": (_i32, [_vp, _vp, _vp, _vp, _i64, ctypes.POINTER(_PssmScoring), _i64, _i64, _vp, _vp, _i32, _vp, _vp]),
    "sw_score_fit_hist": (_i32, [_vp, _i64, _i32, _vp]),
    "sw_score_evalue": (ctypes.c_double, [_vp, _i64, _i64]),
    "sw_score_thresholds": (_i32, [_vp, _i64, ctypes.c_double, _vp]),
    "sw_hits_threshold_device": (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sw_hits_threshold_host": (_i32, [_vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
    "sw_write_a3m": (_i32, [ctypes.c_char_p, ctypes.c_char_p, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64]),
    "sw_write_pssm": (_i32, [ctypes.c_char_p, _vp, ctypes.c_int32, _vp, _i64, _vp]),
    "sw_align_affine_device": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, ctypes.POINTER(_Affine), _vp, _vp, _i64, _vp]),
    "sw_align_affine_host": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, ctypes.POINTER(_Affine), _vp, _vp, _i64]),
    "sw_submat_match": (None, [_i32, _i32, _vp]),
    "sw_submat_from_letters": (_i32, [_vp, _i32, _vp, _i32, _vp]),
    "sw_read_submat": (_i32, [ctypes.c_char_p, _vp]),
    "sw_batch_traceback_device": (_i32, [_vp, _vp, _i32, _i64, _i64, _i64, _vp, _i64, _vp, _vp]),
    "sw_fill_band_device": (_i32, [_vp, _vp, _i64, _vp, _i64, _i64, ctypes.POINTER(_Scores), _vp, _i32, _vp, _i32, _vp, _u32, _vp, _u32, _vp,
                                   _i32, _i32, _vp, _vp]),
    "sw_multi_create": (_i32, [ctypes.POINTER(_i32), _i32, _vp, _i64, _vp, _i64, _i32, _i32, ctypes.POINTER(_vp)]),
    "sw_multi_fill": (_i32, [_vp, ctypes.POINTER(_Scores), _i32, ctypes.POINTER(_Result)]),
    "sw_multi_traceback": (_i32, [_vp, ctypes.POINTER(_i64)]),
    "sw_multi_band_info": (_i32, [_vp, _i32, ctypes.POINTER(_i32), ctypes.POINTER(_i64), ctypes.POINTER(_i64), ctypes.POINTER(_vp), ctypes.POINTER(_vp)]),
    "sw_multi_nbands": (_i32, [_vp]),
    "sw_multi_seconds": (ctypes.c_double, [_vp]),
    "sw_multi_free": (None, [_vp]),
    "sw_align_auto": (_i32, [_vp, _vp, _i64, _vp, _i64, ctypes.POINTER(_Scores), _vp, _vp, ctypes.POINTER(_Result), ctypes.POINTER(_i32)]),
    "sw_align_auto_multi": (_i32, [_vp, ctypes.POINTER(_i32), _i32, _vp, _i64, _vp, _i64, ctypes.POINTER(_Scores), _vp, _vp, ctypes.POINTER(_Result),
                                   ctypes.POINTER(_i32), _i64]),
    "sw_p_to_p2_device": (_i32, [_vp, _vp, _i32, _vp, _vp, _i64, _vp]),
    "sw_p2_to_p32_device": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "sw_traceback_p2_device": (_i32, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp]),
    "sw_fill_cpu": (_i32, [_vp, _i64, _vp, _i64, ctypes.POINTER(_Scores), _vp, _vp, ctypes.POINTER(_Result)]),
    "sw_fill_host": (_i32, [_vp, _vp, _i64, _vp, _i64, ctypes.POINTER(_Scores), _vp, _vp, ctypes.POINTER(_Result)]),
    "sw_traceback_device": (_i32, [_vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp]),
    "sw_traceback_host": (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, ctypes.POINTER(_i64)]),
    "sw_traceback_host_ex": (_i32, [_vp, _i32, _i64, _i64, _i64, _vp, _i64, ctypes.POINTER(_i64)]),
    "sw_traceback_device_ex": (_i32, [_vp, _vp, _i32, _i64, _i64, _i64, _vp, _i64, _vp, _vp]),
    "sw_fill_device_ex": (_i32, [_vp, _vp, _i64, _vp, _i64, ctypes.POINTER(_Scores), _vp, _i32, _vp, _i32, _vp, _vp, _vp]),
    "sw_row_checksums_device": (_i32, [_vp, _vp, _i32, _i64, _i64, _vp, _vp]),
    "sw_p8_to_p32_device": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "sw_alloc_outputs": (_i32, [_vp, _vp, _i64, _vp, _i64, ctypes.POINTER(_Scores), _i32, _i32, _i32, ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                ctypes.POINTER(ctypes.c_float)]),
    "sw_free_outputs": (_i32, [_vp, _vp, _vp]),
    "sw_place_pair_ratio": (_i32, [_vp, _sz, _vp, _sz, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]),
    "sw_device_malloc": (_i32, [_vp, _sz, ctypes.POINTER(_vp)]),
    "sw_device_free": (_i32, [_vp, _vp]),
    "sw_memcpy_h2d": (_i32, [_vp, _vp, _vp, _sz]),
    "sw_memcpy_d2h": (_i32, [_vp, _vp, _vp, _sz]),
    "sw_synchronize": (_i32, [_vp, _vp]),
    "sw_set_option": (_i32, [_vp, ctypes.c_char_p, _i64]),
    "sw_get_option": (_i64, [_vp, ctypes.c_char_p]),
}

SW_TOP_MAX = 4096   # include/swhip.h: the most hits per query a selecting call takes
# sw_msa_row (include/swhip.h), 24 bytes: an entry's A3M row is a3m[off : off + len]
MSA_ROW = np.dtype([("off", np.int64), ("len", np.int32), ("nmatch", np.int32), ("nident", np.int32), ("ninsert", np.int32)])
# the score histogram of a query (include/swhip.h): SW_HIST_CLASSES x SW_HIST_BINS uint32 counters; sw_score_fit, 56 bytes
HIST_CLASSES, HIST_BINS, HIST_SHIFT_MAX = 40, 256, 16
SCORE_FIT = np.dtype([("a", np.float64), ("b", np.float64), ("sigma", np.float64), ("n_db", np.int64), ("n_fit", np.int64),
                      ("n_censored", np.int64), ("valid", np.int32), ("shift", np.int32)])

_lib = None


def lib() -> ctypes.CDLL:
    """Load libswhip.so (built in-tree by `make -C smith-waterman_amd`). Fails loudly if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not built: run `make -C {_HERE}` (hipcc --offload-arch=gfx950); "
                              "there is no CPU fallback")
        try:  # torch bundles its own HIP/HSA runtime: let it load first so the process has ONE
            import torch  # noqa: F401  (libswhip.so then binds to the already-loaded libamdhip64)
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in ABI.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def _check(rc: int):
    if rc != 0:
        raise SwError(rc, lib().sw_last_error().decode())


def generate(cols: int, rows: int, seed: int = 1):
    """Random DNA pair exactly as the reference's generate() (seed 1 == serial_smithW.c).
    Returns (a, b) as uint8 arrays of length cols / rows."""
    a = np.zeros(cols + 1, np.uint8)
    b = np.zeros(rows + 1, np.uint8)
    _check(lib().sw_generate(cols, rows, seed, a.ctypes.data, b.ctypes.data))
    return a[:cols].copy(), b[:rows].copy()


def read_fasta(path: str, record: int = 0):
    """One record of a FASTA file as a uint8 array (upper-cased, white space dropped); see sw_read_fasta."""
    n = _i64()
    _check(lib().sw_read_fasta(os.fsencode(path), record, None, 0, ctypes.byref(n)))
    seq = np.zeros(max(1, n.value), np.uint8)
    _check(lib().sw_read_fasta(os.fsencode(path), record, seq.ctypes.data, n.value, ctypes.byref(n)))
    return seq[:n.value].copy()


def read_fasta_db(path: str):
    """Every record of a FASTA file in one pass (sw_read_fasta_db): (packed uint8 sequence bytes, int64 offsets of nrecords + 1
    entries); record k = packed[offsets[k]:offsets[k+1]], the layout Engine.search takes."""
    nrec, total = _i64(), _i64()
    _check(lib().sw_read_fasta_db(os.fsencode(path), None, 0, None, 0, ctypes.byref(nrec), ctypes.byref(total)))
    seq = np.zeros(max(1, total.value), np.uint8)
    offs = np.zeros(nrec.value + 1, np.int64)
    _check(lib().sw_read_fasta_db(os.fsencode(path), seq.ctypes.data, len(seq), offs.ctypes.data, len(offs), ctypes.byref(nrec),
                                  ctypes.byref(total)))
    return seq[:total.value].copy(), offs


def _pack_targets(targets):
    """A list of sequences, or a (packed, offsets) pair -> (packed uint8, int64 offsets)."""
    if isinstance(targets, tuple) and len(targets) == 2 and not isinstance(targets[0], (str, bytes, bytearray)):
        packed = np.ascontiguousarray(targets[0], np.uint8).reshape(-1)
        offs = np.ascontiguousarray(targets[1], np.int64).reshape(-1)
        return packed, offs
    seqs = [_as_seq(t) for t in targets]
    offs = np.zeros(len(seqs) + 1, np.int64)
    if seqs:
        offs[1:] = np.cumsum([len(x) for x in seqs])
    packed = np.concatenate(seqs) if seqs and offs[-1] > 0 else np.zeros(0, np.uint8)
    return np.ascontiguousarray(packed, np.uint8), offs


def submat_match(match: int, mismatch: int):
    """(256, 256) int8 table s[x][y] = match if x == y else mismatch (sw_submat_match).  Both must fit int8: the C builder would
    clamp them, which is a different scoring from the one asked for, so that is an error here."""
    for name, v in (("match", match), ("mismatch", mismatch)):
        if not -128 <= int(v) <= 127:
            raise ValueError(f"submat_match: {name} = {v} does not fit int8")
    out = np.zeros((256, 256), np.int8)
    lib().sw_submat_match(match, mismatch, out.ctypes.data)
    return out


def submat_from_letters(letters, scores, other: int):
    """(256, 256) int8 table from an n x n score array over `letters` (row = query letter); every pair with a byte that is not listed
    scores `other` (sw_submat_from_letters)."""
    lt = _as_seq(letters)
    sc = np.ascontiguousarray(scores, np.int8)
    if sc.shape != (len(lt), len(lt)):
        raise ValueError(f"scores must be {len(lt)} x {len(lt)}")
    out = np.zeros((256, 256), np.int8)
    _check(lib().sw_submat_from_letters(lt.ctypes.data, len(lt), sc.ctypes.data, int(other), out.ctypes.data))
    return out


def read_submat(path: str):
    """(256, 256) int8 table from a substitution matrix in the NCBI text format (sw_read_submat)."""
    out = np.zeros((256, 256), np.int8)
    _check(lib().sw_read_submat(os.fsencode(path), out.ctypes.data))
    return out


def _affine(submat, gap_open: int, gap_extend: int):
    """(the table kept alive, the sw_affine that points at it)"""
    sub = np.ascontiguousarray(submat, np.int8)
    if sub.shape != (256, 256):
        raise ValueError("the substitution matrix must be (256, 256) int8")
    return sub, _Affine(sub.ctypes.data, int(gap_open), int(gap_extend))


def search_affine_host(query, targets, submat, gap_open: int, gap_extend: int, top=None):
    """sw_search_affine_host: the affine search in plain C++ on the host (no GPU).  Arguments and results as Engine.search_affine."""
    q = np.ascontiguousarray(_as_seq(query))
    packed, offs = _pack_targets(targets)
    ntargets = len(offs) - 1
    db = packed if len(packed) else np.zeros(1, np.uint8)
    res = np.zeros((max(1, ntargets), 3), np.int64)
    sub, sc = _affine(submat, gap_open, gap_extend)
    _check(lib().sw_search_affine_host(q.ctypes.data, len(q), db.ctypes.data, offs.ctypes.data, ntargets, ctypes.byref(sc), res.ctypes.data))
    out = res[:ntargets]
    return (out, top_hits(out, top)) if top is not None else out


def search_affine_multi_host(queries, targets, scoring):
    """sw_search_affine_multi_host: every query against every target in plain C++ on the host (no GPU).  Arguments and result as
    Database.search_affine: queries a list of sequences or a (packed, offsets) pair, scoring = (submat, gap_open, gap_extend); returns the
    (nqueries, ntargets, 3) int64 array of (max_pos, max_score, path_len = 0)."""
    qpacked, qoffs = _pack_targets(queries)
    packed, offs = _pack_targets(targets)
    nq, ntargets = len(qoffs) - 1, len(offs) - 1
    qs = qpacked if len(qpacked) else np.zeros(1, np.uint8)
    db = packed if len(packed) else np.zeros(1, np.uint8)
    res = np.zeros((max(1, nq * ntargets), 3), np.int64)
    sub, sc = _affine(*scoring)
    _check(lib().sw_search_affine_multi_host(qs.ctypes.data, qoffs.ctypes.data, nq, db.ctypes.data, offs.ctypes.data, ntargets, ctypes.byref(sc),
                                             res.ctypes.data))
    return res[:nq * ntargets].reshape(nq, ntargets, 3)


def _pair_list(pairs):
    """A host pair list as the C-ABI takes it: (npairs, 2) int64 of (query, target), from an array or a list of tuples."""
    pr = np.asarray(pairs, np.int64)
    if pr.size == 0:
        pr = pr.reshape(0, 2)
    if pr.ndim != 2 or pr.shape[1] != 2:
        raise ValueError("pairs must be (npairs, 2) int64 of (query, target)")
    return np.ascontiguousarray(pr)


def search_affine_pairs_host(queries, targets, scoring, pairs):
    """sw_search_affine_pairs_host: the scores of a list of (query, target) pairs in plain C++ on the host (no GPU).  Arguments and
    result as Database.search_affine_pairs: returns the (npairs, 3) int64 array of (max_pos, max_score, path_len = 0) in list order."""
    qpacked, qoffs = _pack_targets(queries)
    packed, offs = _pack_targets(targets)
    pr = _pair_list(pairs)
    qs = qpacked if len(qpacked) else np.zeros(1, np.uint8)
    db = packed if len(packed) else np.zeros(1, np.uint8)
    res = np.zeros((max(1, len(pr)), 3), np.int64)
    sub, sc = _affine(*scoring)
    _check(lib().sw_search_affine_pairs_host(qs.ctypes.data, qoffs.ctypes.data, len(qoffs) - 1, db.ctypes.data, offs.ctypes.data, len(offs) - 1,
                                             ctypes.byref(sc), pr.ctypes.data if len(pr) else None, len(pr), res.ctypes.data))
    return res[:len(pr)]


def _submat(submat):
    sub = np.ascontiguousarray(submat, np.int8)
    if sub.shape != (256, 256):
        raise ValueError("the substitution matrix must be (256, 256) int8")
    return sub


def prefilter_ungapped_host(queries, targets, submat, min_score: int, cap=None, want_scores: bool = True):
    """sw_prefilter_ungapped_host: the ungapped pre-filter in plain C++ on the host (no GPU).  queries and targets as for
    search_affine_multi_host.  Returns (pairs, npairs, scores): the first min(npairs, cap) rows of the (cap, 2) int64 list are the
    passing (query, target) pairs in ascending order, the rest is (-1, -1); npairs is the true count; scores is the
    (nqueries, ntargets) int32 table of U, or None.  cap defaults to nqueries x ntargets."""
    qpacked, qoffs = _pack_targets(queries)
    packed, offs = _pack_targets(targets)
    nq, ntargets = len(qoffs) - 1, len(offs) - 1
    cap = nq * ntargets if cap is None else int(cap)
    qs = qpacked if len(qpacked) else np.zeros(1, np.uint8)
    db = packed if len(packed) else np.zeros(1, np.uint8)
    sub = _submat(submat)
    pairs = np.zeros((max(1, cap), 2), np.int64)
    scores = np.zeros(max(1, nq * ntargets), np.int32) if want_scores else None
    n = _i64(0)
    _check(lib().sw_prefilter_ungapped_host(qs.ctypes.data, qoffs.ctypes.data, nq, db.ctypes.data, offs.ctypes.data, ntargets, sub.ctypes.data,
                                            int(min_score), pairs.ctypes.data if cap > 0 else None, cap, ctypes.byref(n),
                                            scores.ctypes.data if want_scores else None))
    return pairs[:max(0, cap)], n.value, (scores[:nq * ntargets].reshape(nq, ntargets) if want_scores else None)


def search_affine_multi_top_host(queries, targets, scoring, top: int, min_score: int = 0):
    """sw_search_affine_multi_top_host: the best `top` targets of every query in plain C++ on the host (no GPU).  Arguments and results
    as Database.search_affine_top: returns (hits (nqueries, top, 3) int64 of (target, max_pos, max_score), nhits (nqueries,) int64)."""
    qpacked, qoffs = _pack_targets(queries)
    packed, offs = _pack_targets(targets)
    nq, ntargets, k = len(qoffs) - 1, len(offs) - 1, max(0, int(top))
    qs = qpacked if len(qpacked) else np.zeros(1, np.uint8)
    db = packed if len(packed) else np.zeros(1, np.uint8)
    hits = np.zeros((max(1, nq * k), 3), np.int64)
    nhits = np.zeros(max(1, nq), np.int64)
    sub, sc = _affine(*scoring)
    _check(lib().sw_search_affine_multi_top_host(qs.ctypes.data, qoffs.ctypes.data, nq, db.ctypes.data, offs.ctypes.data, ntargets, ctypes.byref(sc),
                                                 int(top), int(min_score), hits.ctypes.data, nhits.ctypes.data))
    return hits[:nq * k].reshape(nq, k, 3), nhits[:nq]


def top_hits_pairs_host(pairs, results, nqueries: int, ntargets: int, top: int, min_score: int = 0):
    """sw_top_hits_pairs_host: the best `top` entries of every query of a scored pair list in plain C++ on the host (no GPU).  pairs an
    (npairs, 2) int64 array of (query, target), results the (npairs, 3) int64 array of (max_pos, max_score, path_len) that belongs to
    it entry for entry.  An entry qualifies when its query and target lie inside nqueries and ntargets and max_score >= min_score; a
    row is ordered by score descending, then target ascending, then list position.  Returns (hits (nqueries, top, 3) int64 of
    (target, max_pos, max_score), unused entries (-1, 0, 0); nhits (nqueries,) int64)."""
    pr = _pair_list(pairs)
    res = np.ascontiguousarray(results, np.int64).reshape(-1, 3)
    if len(res) != len(pr):
        raise ValueError("results must hold one (max_pos, max_score, path_len) row per pair")
    nq, k = max(0, int(nqueries)), max(0, int(top))
    hits = np.zeros((max(1, nq * k), 3), np.int64)
    nhits = np.zeros(max(1, nq), np.int64)
    _check(lib().sw_top_hits_pairs_host(pr.ctypes.data if len(pr) else None, res.ctypes.data if len(pr) else None, len(pr), int(nqueries), int(ntargets),
                                        int(top), int(min_score), hits.ctypes.data, nhits.ctypes.data))
    return hits[:nq * k].reshape(nq, k, 3), nhits[:nq]


def _ops_list(aln, ops, cap):
    """The ops rows of an alignment call as a list of bytes, each cut to its nops."""
    return [ops[h, :aln[h, 6]].tobytes() if aln[h, 6] <= cap else b"" for h in range(len(aln))]


def _hits_and_cap(offs, hits, qlen):
    hits = np.ascontiguousarray(hits, np.int64).reshape(-1)
    ntargets = len(offs) - 1
    inside = hits[(hits >= 0) & (hits < ntargets)]
    longest = int(np.diff(offs)[inside].max()) if len(inside) else 0
    return hits, max(1, qlen + longest)


def align_affine_host(query, targets, submat, gap_open: int, gap_extend: int, hits):
    """sw_align_affine_host: the alignments of the targets `hits` in plain C++ on the host (no GPU).  Arguments and results as
    Engine.align_affine."""
    q = np.ascontiguousarray(_as_seq(query))
    packed, offs = _pack_targets(targets)
    db = packed if len(packed) else np.zeros(1, np.uint8)
    hits, cap = _hits_and_cap(offs, hits, len(q))
    aln = np.zeros((max(1, len(hits)), 7), np.int64)
    ops = np.zeros((max(1, len(hits)), cap), np.uint8)
    sub, sc = _affine(submat, gap_open, gap_extend)
    _check(lib().sw_align_affine_host(q.ctypes.data, len(q), db.ctypes.data, offs.ctypes.data, len(offs) - 1, hits.ctypes.data, len(hits),
                                      ctypes.byref(sc), aln.ctypes.data, ops.ctypes.data, cap))
    aln = aln[:len(hits)]
    return aln, _ops_list(aln, ops, cap)


def _hit_table(hits, nhits, nq: int):
    """A host hit table as the C-ABI takes it: (nq, top, 3) int64 of (target, max_pos, max_score) -- or (nq, top) target indices, which
    are widened -- and the counts (or None)."""
    hits = np.asarray(hits, np.int64)
    if hits.ndim == 2:
        hits = np.stack([hits, np.zeros_like(hits), np.zeros_like(hits)], axis=-1)
    if hits.ndim != 3 or hits.shape[0] != nq or hits.shape[2] != 3:
        raise ValueError(f"hits must be ({nq}, top, 3) or ({nq}, top) int64")
    if nhits is not None:
        nhits = np.ascontiguousarray(nhits, np.int64).reshape(-1)
        if len(nhits) != nq:
            raise ValueError(f"nhits must hold {nq} counts")
    return np.ascontiguousarray(hits), nhits


def align_affine_hits_host(queries, targets, scoring, hits, nhits=None):
    """sw_align_affine_hits_host: the alignments of a hit table in plain C++ on the host (no GPU).  Arguments and results as
    Database.align_affine_hits."""
    qpacked, qoffs = _pack_targets(queries)
    packed, offs = _pack_targets(targets)
    nq = len(qoffs) - 1
    hits, nhits = _hit_table(hits, nhits, nq)
    top = hits.shape[1]
    qs = qpacked if len(qpacked) else np.zeros(1, np.uint8)
    db = packed if len(packed) else np.zeros(1, np.uint8)
    cap = max(1, int(np.diff(qoffs).max(initial=0)) + int(np.diff(offs).max(initial=0)))
    aln = np.zeros((max(1, nq * top), 7), np.int64)
    ops = np.zeros((max(1, nq * top), cap), np.uint8)
    sub, sc = _affine(*scoring)
    _check(lib().sw_align_affine_hits_host(qs.ctypes.data, qoffs.ctypes.data, nq, db.ctypes.data, offs.ctypes.data, len(offs) - 1, ctypes.byref(sc),
                                           hits.ctypes.data, nhits.ctypes.data if nhits is not None else None, top, aln.ctypes.data, ops.ctypes.data, cap))
    aln = aln[:nq * top]
    return aln.reshape(nq, top, 7), _ops_rows(aln, ops, cap, nq, top)


def _pssm_scoring(scoring):
    """(the letters kept alive, the sw_pssm_scoring that points at them) from (letters, other, smax, gap_open, gap_extend)."""
    letters, other, smax, gap_open, gap_extend = scoring
    lt = np.ascontiguousarray(_as_seq(letters))
    buf = np.concatenate([lt, np.zeros(1, np.uint8)])   # (never an empty buffer: the library, not a NULL pointer, refuses nletters = 0)
    return buf, _PssmScoring(buf.ctypes.data, len(lt), int(other), int(smax), int(gap_open), int(gap_extend))


def _pack_pssm(pssm, nletters: int):
    """A list of per-query (columns, nletters) int8 matrices, or a ((total columns, nletters) int8, int64 offsets) pair whose offsets
    count columns of the array -> (int8 array of total columns x nletters, int64 offsets)."""
    if isinstance(pssm, tuple) and len(pssm) == 2:
        m = np.ascontiguousarray(pssm[0], np.int8).reshape(-1, nletters)
        return m, np.ascontiguousarray(pssm[1], np.int64).reshape(-1)
    ms = [np.ascontiguousarray(m, np.int8).reshape(-1, nletters) for m in pssm]
    offs = np.zeros(len(ms) + 1, np.int64)
    if ms:
        offs[1:] = np.cumsum([len(m) for m in ms])
    return (np.concatenate(ms) if ms else np.zeros((0, nletters), np.int8)), offs


def pssm_from_queries(queries, submat, letters):
    """sw_pssm_from_queries: the PSSMs that reproduce sequence queries under a table -- column j of query q is the table's row of
    letter q[j] at `letters`.  Returns (pssm (total columns, nletters) int8, offsets int64 starting at 0), what the *_pssm calls take."""
    qpacked, qoffs = _pack_targets(queries)
    lt = np.ascontiguousarray(_as_seq(letters))
    sub = _submat(submat)
    n = int(qoffs[-1] - qoffs[0])
    out = np.zeros((max(1, n), max(1, len(lt))), np.int8)
    qs = qpacked if len(qpacked) else np.zeros(1, np.uint8)
    _check(lib().sw_pssm_from_queries(qs.ctypes.data, qoffs.ctypes.data, len(qoffs) - 1, sub.ctypes.data, lt.ctypes.data if len(lt) else None, len(lt),
                                      out.ctypes.data))
    return out[:n], qoffs - qoffs[0]


def read_pssm(path: str):
    """sw_read_pssm: the ASCII PSSM that PSI-BLAST writes.  Returns (letters uint8 (nletters,), pssm int8 (columns, nletters))."""
    letters = np.zeros(256, np.uint8)
    nl, ncols = ctypes.c_int32(), _i64()
    _check(lib().sw_read_pssm(os.fsencode(path), letters.ctypes.data, ctypes.byref(nl), None, 0, ctypes.byref(ncols)))
    m = np.zeros((ncols.value, nl.value), np.int8)
    _check(lib().sw_read_pssm(os.fsencode(path), letters.ctypes.data, ctypes.byref(nl), m.ctypes.data, m.size, ctypes.byref(ncols)))
    return letters[:nl.value].copy(), m


def write_pssm(path: str, letters, pssm, consensus=None):
    """sw_write_pssm: a (columns, nletters) int8 matrix in the ASCII layout read_pssm reads back.  consensus: one printable byte per
    column (the residue printed beside the position), or None for 'X'."""
    lt = np.ascontiguousarray(_as_seq(letters))
    m = np.ascontiguousarray(pssm, np.int8).reshape(-1, max(1, len(lt)))
    cons = None
    if consensus is not None:
        cons = np.ascontiguousarray(_as_seq(consensus))
        if len(cons) != len(m):
            raise ValueError(f"consensus must hold one byte per column ({len(m)})")
    buf = np.concatenate([lt, np.zeros(1, np.uint8)])
    _check(lib().sw_write_pssm(os.fsencode(path), buf.ctypes.data, len(lt), m.ctypes.data if m.size else None, len(m),
                               cons.ctypes.data if cons is not None and len(cons) else None))


def _pssm_update(update):
    """(the table kept alive, the sw_pssm_update that points at it) from (submat, prior_weight, include_min_score)."""
    submat, prior_weight, include_min_score = update
    sub = _submat(submat)
    return sub, _PssmUpdate(sub.ctypes.data, int(prior_weight), int(include_min_score))


def _ops_table(ops, nq: int, top: int):
    """The ops of a hit table as the C-ABI takes them: a (nq, top, ops_cap) uint8 array, or the list per query of `top` bytes objects
    the align calls return -> ((nq * top, ops_cap) uint8, ops_cap)."""
    if isinstance(ops, np.ndarray):
        o = np.ascontiguousarray(ops, np.uint8).reshape(max(1, nq * top), -1)
        return o, o.shape[1]
    cap = max([1] + [len(b) for row in ops for b in row])
    o = np.zeros((max(1, nq * top), cap), np.uint8)
    for q, row in enumerate(ops):
        for r, b in enumerate(row):
            o[q * top + r, :len(b)] = np.frombuffer(b, np.uint8)
    return o, cap


def _pack_hit_tables(hits, nhits, aln, ops, nq: int):
    """The host tables of a call that reads a hit table's alignments, as the C-ABI takes them -> (hits, nhits, top, aln, ops, ops_cap):
    hits and nhits of _hit_table, aln (nq * top, 7) int64 -- one row of zeros where there is no entry: never an empty buffer --, ops and
    ops_cap of _ops_table."""
    hits, nhits = _hit_table(hits, nhits, nq)
    top = hits.shape[1]
    a = np.ascontiguousarray(aln, np.int64).reshape(-1, 7)
    if len(a) != nq * top:
        raise ValueError(f"aln must be ({nq}, {top}, 7) int64")
    o, cap = _ops_table(ops, nq, top)
    return hits, nhits, top, a if len(a) else np.zeros((1, 7), np.int64), o, cap


def pssm_from_hits_host(prior, targets, scoring, update, hits, nhits, aln, ops, weights=None, want_counts: bool = False):
    """sw_pssm_from_hits_host: the next iteration's PSSM from aligned hits in plain C++ on the host (no GPU).  Arguments and results as
    Database.pssm_from_hits."""
    lt, sc = _pssm_scoring(scoring)
    sub, up = _pssm_update(update)
    nl = max(1, sc.nletters)
    m, qoffs = _pack_pssm(prior, nl)
    packed, offs = _pack_targets(targets)
    nq = len(qoffs) - 1
    hits, nhits, top, aa, o, cap = _pack_hit_tables(hits, nhits, aln, ops, nq)
    w = None
    if weights is not None:
        w = np.ascontiguousarray(weights, np.int32).reshape(-1)
        if len(w) != nq * top:
            raise ValueError(f"weights must be ({nq}, {top}) int32")
    mm = m if m.size else np.zeros((1, nl), np.int8)
    db = packed if len(packed) else np.zeros(1, np.uint8)
    ncols = int(qoffs[-1] - qoffs[0])
    out = mm.copy()
    counts = np.zeros((max(1, ncols), nl), np.int32)
    _check(lib().sw_pssm_from_hits_host(mm.ctypes.data, qoffs.ctypes.data, nq, db.ctypes.data, offs.ctypes.data, len(offs) - 1, ctypes.byref(sc),
                                        ctypes.byref(up), hits.ctypes.data if hits.size else aa.ctypes.data, nhits.ctypes.data if nhits is not None else None,
                                        top, aa.ctypes.data, o.ctypes.data, cap, w.ctypes.data if w is not None and len(w) else None, out.ctypes.data,
                                        counts.ctypes.data))
    out = out[:len(m)]
    return (out, counts[:ncols]) if want_counts else out


def _pssm_weighting(weighting):
    """The sw_pssm_weighting from (per_hit, include_min_score)."""
    per_hit, include_min_score = weighting
    return _PssmWeighting(int(per_hit), int(include_min_score))


def _query_offsets(qoffsets_or_pssm, nletters: int):
    """The int64 column offsets of the queries: an offsets array, or a PSSM as search_pssm takes it (only its offsets are used)."""
    if isinstance(qoffsets_or_pssm, np.ndarray) and qoffsets_or_pssm.ndim == 1:
        return np.ascontiguousarray(qoffsets_or_pssm, np.int64)
    return _pack_pssm(qoffsets_or_pssm, nletters)[1]


def pssm_hit_weights_host(qoffsets_or_pssm, targets, scoring, weighting, hits, nhits, aln, ops):
    """sw_pssm_hit_weights_host: the position-based weights of aligned hits in plain C++ on the host (no GPU).  Arguments and result as
    Database.pssm_hit_weights."""
    lt, sc = _pssm_scoring(scoring)
    wt = _pssm_weighting(weighting)
    qoffs = _query_offsets(qoffsets_or_pssm, max(1, sc.nletters))
    packed, offs = _pack_targets(targets)
    nq = len(qoffs) - 1
    hits, nhits, top, aa, o, cap = _pack_hit_tables(hits, nhits, aln, ops, nq)
    db = packed if len(packed) else np.zeros(1, np.uint8)
    w = np.zeros(max(1, nq * top), np.int32)
    _check(lib().sw_pssm_hit_weights_host(qoffs.ctypes.data, nq, db.ctypes.data, offs.ctypes.data, len(offs) - 1, ctypes.byref(sc), ctypes.byref(wt),
                                          hits.ctypes.data if hits.size else aa.ctypes.data, nhits.ctypes.data if nhits is not None else None, top,
                                          aa.ctypes.data, o.ctypes.data, cap, w.ctypes.data))
    return w[:nq * top].reshape(nq, top)


def _msa_queries(queries):
    """The queries of an msa_from_hits call -> (packed letters or None, int64 offsets): a list of sequences or a (packed, offsets) pair;
    a 1-D int64 array is the column offsets of PSSM queries, which have no letters."""
    if isinstance(queries, np.ndarray) and queries.ndim == 1 and queries.dtype == np.int64:
        return None, np.ascontiguousarray(queries)
    return _pack_targets(queries)


def msa_from_hits_host(queries, targets, include_min_score, hits, nhits, aln, ops, a3m_cap=None):
    """sw_msa_from_hits_host: the query-anchored alignment of aligned hits in plain C++ on the host (no GPU).  Arguments and results as
    Database.msa_from_hits."""
    qpacked, qoffs = _msa_queries(queries)
    packed, offs = _pack_targets(targets)
    nq = len(qoffs) - 1
    hits, nhits, top, aa, o, cap = _pack_hit_tables(hits, nhits, aln, ops, nq)
    db = packed if len(packed) else np.zeros(1, np.uint8)
    ncols = int(qoffs[-1] - qoffs[0])
    cols = np.zeros(max(1, ncols * top), np.uint8)
    rows = np.zeros(max(1, nq * top), MSA_ROW)
    total = _i64(0)

    def call(c, a3m, a3m_cap):
        _check(lib().sw_msa_from_hits_host(qpacked.ctypes.data if qpacked is not None and len(qpacked) else None, qoffs.ctypes.data, nq, db.ctypes.data,
                                           offs.ctypes.data, len(offs) - 1, int(include_min_score), hits.ctypes.data if hits.size else aa.ctypes.data,
                                           nhits.ctypes.data if nhits is not None else None, top, aa.ctypes.data, o.ctypes.data, cap, c, rows.ctypes.data,
                                           a3m, a3m_cap, ctypes.addressof(total)))
    if a3m_cap is None:
        call(None, None, 0)   # the sizing call: the rows and the total
        a3m_cap = total.value
    a3m = np.zeros(max(1, int(a3m_cap)), np.uint8)
    call(cols.ctypes.data, a3m.ctypes.data, int(a3m_cap))
    return cols[:ncols * top], rows[:nq * top].reshape(nq, top), a3m[:int(a3m_cap)]


def _msa_filter(filter):
    """The sw_msa_filter from (max_ident_pct, min_cover_pct)."""
    max_ident_pct, min_cover_pct = filter
    return _MsaFilter(int(max_ident_pct), int(min_cover_pct))


def _msa_filter_args(cols, queries_or_qoffsets, top: int, hits):
    """The host arguments of a filter call, checked: (cols uint8, query letters or None, int64 offsets, nq, top, (nq, top, 3) hits or None)."""
    qpacked, qoffs = _msa_queries(queries_or_qoffsets)
    nq, top = len(qoffs) - 1, int(top)
    c = np.ascontiguousarray(cols, np.uint8).reshape(-1)
    need = int(qoffs[-1] - qoffs[0]) * max(0, top)
    if len(c) < need:
        raise ValueError(f"cols must hold at least {need} bytes")
    if qpacked is not None and len(qpacked) < int(qoffs[-1]):
        raise ValueError(f"the query letters must hold at least {int(qoffs[-1])} bytes")
    if hits is not None:
        hits, _ = _hit_table(hits, None, nq)
        if hits.shape[1] != top:
            raise ValueError(f"hits must be ({nq}, {top}, 3) int64")
    return c, qpacked, qoffs, nq, top, hits


def msa_filter_host(cols, queries_or_qoffsets, top: int, max_ident_pct: int, min_cover_pct: int, hits=None):
    """sw_msa_filter_host: the filter of the column rows in plain C++ on the host (no GPU).  Arguments and results as Engine.msa_filter."""
    c, qpacked, qoffs, nq, top, hits = _msa_filter_args(cols, queries_or_qoffsets, top, hits)
    f = _msa_filter((max_ident_pct, min_cover_pct))
    one = np.zeros(1, np.uint8)
    keep = np.zeros(max(1, nq * max(0, top)), np.int32)
    nkept = np.zeros(max(1, nq), np.int64)
    out = np.zeros_like(hits) if hits is not None else None
    _check(lib().sw_msa_filter_host((c if len(c) else one).ctypes.data, qpacked.ctypes.data if qpacked is not None and len(qpacked) else None,
                                    qoffs.ctypes.data, nq, top, ctypes.byref(f), hits.ctypes.data if hits is not None and hits.size else None,
                                    out.ctypes.data if out is not None and out.size else None, keep.ctypes.data, nkept.ctypes.data))
    return keep[:nq * top].reshape(nq, top), nkept[:nq], out


def _target_offsets(targets_or_offsets):
    """The int64 offsets of the targets: from a 1-D integer array of offsets as it is, else as _pack_targets gives them."""
    if isinstance(targets_or_offsets, np.ndarray) and targets_or_offsets.ndim == 1 and targets_or_offsets.dtype.kind in "iu" \
            and targets_or_offsets.dtype != np.uint8:
        return np.ascontiguousarray(targets_or_offsets, np.int64)
    return _pack_targets(targets_or_offsets)[1]


def score_hist_host(results, targets_or_offsets, shift: int = 0):
    """sw_score_hist_host: the score histogram of a result table in plain C++ on the host (no GPU).  results: the (nqueries, ntargets,
    3) int64 table of (max_pos, max_score, path_len) a search returns; targets_or_offsets: the targets as for search_affine, or their
    1-D int64 offsets (only the lengths count).  Returns (nqueries, 40, 256) uint32: [q, c, s] counts the non-empty targets of
    half-octave length class c whose score lies in bin s = min(max(score, 0) >> shift, 255) (include/swhip.h states the rule)."""
    offs = _target_offsets(targets_or_offsets)
    ntargets = len(offs) - 1
    res = np.ascontiguousarray(results, np.int64)
    if res.ndim != 3 or res.shape[1] != ntargets or res.shape[2] != 3:
        raise ValueError(f"results must be (nqueries, {ntargets}, 3) int64")
    nq = res.shape[0]
    hist = np.zeros((max(1, nq), HIST_CLASSES, HIST_BINS), np.uint32)
    one = np.zeros(3, np.int64)
    _check(lib().sw_score_hist_host((res if res.size else one).ctypes.data, nq, offs.ctypes.data, ntargets, int(shift), hist.ctypes.data))
    return hist[:nq]


MASK_LETTERS = b"ACDEFGHIKLMNPQRSTVWY"


def _mask_params(window=12, trigger_mbits=2200, extend_mbits=2500, letters=MASK_LETTERS, mask_byte=ord("X")):
    """The sw_mask_params of the masking calls; the defaults are SEG's window and bounds over the 20 amino acids.  The C side checks the
    ranges; here only what the struct cannot hold is refused."""
    if isinstance(letters, str):
        letters = letters.encode("latin-1")
    letters = bytes(bytearray(letters))
    if len(letters) > 32:
        raise ValueError("letters: at most 32 letters")
    if isinstance(mask_byte, (str, bytes, bytearray)):
        if len(mask_byte) != 1:
            raise ValueError("mask_byte must be one byte")
        mask_byte = ord(mask_byte) if isinstance(mask_byte, str) else mask_byte[0]
    if not 0 <= int(mask_byte) <= 255:
        raise ValueError("mask_byte must be 0..255")
    for name, v in (("window", window), ("trigger_mbits", trigger_mbits), ("extend_mbits", extend_mbits)):
        bits = 31 if name == "window" else 63
        if not -(1 << bits) <= int(v) < (1 << bits):
            raise ValueError(f"{name} = {v} does not fit its field")
    mp = _MaskParams(int(trigger_mbits), int(extend_mbits), int(window), len(letters))
    for k, b in enumerate(letters):
        mp.letters[k] = b
    mp.mask_byte = int(mask_byte)
    return mp


def mask_low_complexity_host(targets, window=12, trigger_mbits=2200, extend_mbits=2500, letters=MASK_LETTERS, mask_byte=ord("X"), out=None):
    """sw_mask_low_complexity_host: the low-complexity mask in plain C++ on the host (no GPU); it serves queries as it serves targets.
    targets: a list of sequences or a (packed uint8, int64 offsets) pair; the rule and its parameters are stated in include/swhip.h.
    Returns (masked, nmasked): the packed bytes with mask_byte at the masked positions -- a copy of the input outside
    [offsets[0], offsets[-1]), or `out` (uint8, as long as the packed input), of which only that range is written -- and the (ntargets,)
    int64 masked positions per target."""
    packed, offs = _pack_targets(targets)
    if len(offs) == 0:
        offs = np.zeros(1, np.int64)
    if len(packed) < int(offs[-1]):
        raise ValueError(f"the packed bytes must hold at least {int(offs[-1])} bytes")
    nt = len(offs) - 1
    mp = _mask_params(window, trigger_mbits, extend_mbits, letters, mask_byte)
    if out is None:
        out = packed.copy()
    if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < len(packed):
        raise ValueError(f"out must be a contiguous uint8 array of at least {len(packed)} bytes")
    one, one_out = np.zeros(1, np.uint8), np.zeros(1, np.uint8)
    nmasked = np.zeros(max(1, nt), np.int64)
    _check(lib().sw_mask_low_complexity_host((packed if len(packed) else one).ctypes.data, offs.ctypes.data, nt, ctypes.byref(mp),
                                             (out if out.size else one_out).ctypes.data, nmasked.ctypes.data))
    return out, nmasked[:nt]


def _hists(hist):
    hist = np.ascontiguousarray(hist, np.uint32)
    if hist.ndim == 2:
        hist = hist[None]
    if hist.ndim != 3 or hist.shape[1:] != (HIST_CLASSES, HIST_BINS):
        raise ValueError(f"hist must be (nqueries, {HIST_CLASSES}, {HIST_BINS}) uint32")
    return hist


def score_fit(hist, shift: int = 0):
    """sw_score_fit_hist: per query the line score = a + b x class(length) through the unrelated targets' scores and its spread sigma,
    from the histograms of score_hist / search_affine_top_stats ((nqueries, 40, 256) uint32; `shift` as they were taken with).  Host
    only, double.  Returns a numpy record array of SCORE_FIT: a, b, sigma, n_db, n_fit, n_censored, valid, shift."""
    hist = _hists(hist)
    nq = hist.shape[0]
    fit = np.zeros(max(1, nq), SCORE_FIT)
    one = np.zeros(1, np.uint32)
    _check(lib().sw_score_fit_hist((hist if hist.size else one).ctypes.data, nq, int(shift), fit.ctypes.data))
    return fit[:nq]


def _fits(fit):
    fit = np.ascontiguousarray(np.atleast_1d(fit))
    if fit.dtype != SCORE_FIT:
        raise ValueError("fit must be the SCORE_FIT records score_fit returns")
    return fit


def score_thresholds(fit, evalue: float):
    """sw_score_thresholds: (nqueries, 40) int64, [q, c] the smallest integer score of a target of length class c whose E-value for query
    q is <= evalue; 0 where evalue >= n_db or the fit is invalid."""
    fit = _fits(fit)
    thr = np.zeros((max(1, len(fit)), HIST_CLASSES), np.int64)
    _check(lib().sw_score_thresholds((fit if len(fit) else np.zeros(1, SCORE_FIT)).ctypes.data, len(fit), float(evalue), thr.ctypes.data))
    return thr[:len(fit)]


def score_evalue(fit, target_len: int, score: int) -> float:
    """sw_score_evalue: the E-value of `score` against a target of target_len letters under ONE query's fit (a SCORE_FIT record); NaN
    for an invalid fit."""
    fit = _fits(fit)
    if len(fit) != 1:
        raise ValueError("fit must be one SCORE_FIT record")
    return float(lib().sw_score_evalue(fit.ctypes.data, int(target_len), int(score)))


def length_class(length: int) -> int:
    """The half-octave class of a target's length (include/swhip.h): 0 for 1, else 2 e + the bit below the leading one, e = floor(log2)."""
    length = int(length)
    if length < 2:
        return 0
    e = length.bit_length() - 1
    return 2 * e + ((length >> (e - 1)) & 1)


def hits_threshold_host(targets_or_offsets, thresholds, hits, nhits=None):
    """sw_hits_threshold_host: the thresholds of score_thresholds applied to a hit table in plain C++ on the host (no GPU).  Arguments
    and results as Database.hits_threshold, the targets as for score_hist_host."""
    offs = _target_offsets(targets_or_offsets)
    thr = np.ascontiguousarray(thresholds, np.int64)
    if thr.ndim != 2 or thr.shape[1] != HIST_CLASSES:
        raise ValueError(f"thresholds must be (nqueries, {HIST_CLASSES}) int64")
    nq = thr.shape[0]
    hits, nhits = _hit_table(hits, nhits, nq)
    top = hits.shape[1]
    keep = np.zeros((max(1, nq), max(1, top)), np.int32)
    nkept = np.zeros(max(1, nq), np.int64)
    out = np.zeros((max(1, nq), max(1, top), 3), np.int64)
    one = np.zeros(HIST_CLASSES, np.int64)
    _check(lib().sw_hits_threshold_host(offs.ctypes.data, len(offs) - 1, (thr if thr.size else one).ctypes.data, nq, top,
                                        (hits if hits.size else one).ctypes.data, nhits.ctypes.data if nhits is not None else None,
                                        out.ctypes.data, keep.ctypes.data, nkept.ctypes.data))
    return keep[:nq, :top], nkept[:nq], out[:nq, :top]


def write_a3m(path: str, qname: str, query, tnames, hits, aln, rows, a3m):
    """sw_write_a3m: one query's A3M file.  query: its letters, or an int (the number of columns of a PSSM query: no query record);
    tnames: the names of ALL targets, or None for their indices; hits, aln, rows: the query's (top, 3), (top, 7) and (top,) MSA_ROW
    entries; a3m: the whole byte buffer the rows' off count from."""
    q = None if isinstance(query, (int, np.integer)) else np.ascontiguousarray(_as_seq(query))
    qlen = int(query) if q is None else len(q)
    h = np.ascontiguousarray(hits, np.int64).reshape(-1, 3)
    al = np.ascontiguousarray(aln, np.int64).reshape(-1, 7)
    rw = np.ascontiguousarray(rows, MSA_ROW).reshape(-1)
    buf = np.ascontiguousarray(a3m, np.uint8).reshape(-1)
    if not (len(h) == len(al) == len(rw)):
        raise ValueError("hits, aln and rows must hold the same number of entries")
    names, nt = None, int(h[:, 0].max(initial=-1)) + 1
    if tnames is not None:
        nt = len(tnames)
        names = (ctypes.c_char_p * max(1, nt))(*[os.fsencode(n) if isinstance(n, str) else bytes(n) for n in tnames])
    one = np.zeros(1, np.uint8)
    _check(lib().sw_write_a3m(os.fsencode(path), qname.encode(), q.ctypes.data if q is not None and len(q) else None, qlen,
                              ctypes.cast(names, _vp) if names is not None else None, nt, h.ctypes.data if len(h) else None, al.ctypes.data if len(al) else None,
                              rw.ctypes.data if len(rw) else None, len(h), (buf if len(buf) else one).ctypes.data, len(buf)))


def search_pssm_multi_host(pssm, targets, scoring):
    """sw_search_pssm_multi_host: every PSSM against every target in plain C++ on the host (no GPU).  Arguments and result as
    Database.search_pssm."""
    lt, sc = _pssm_scoring(scoring)
    m, qoffs = _pack_pssm(pssm, max(1, sc.nletters))
    packed, offs = _pack_targets(targets)
    nq, ntargets = len(qoffs) - 1, len(offs) - 1
    mm = m if m.size else np.zeros((1, 1), np.int8)
    db = packed if len(packed) else np.zeros(1, np.uint8)
    res = np.zeros((max(1, nq * ntargets), 3), np.int64)
    _check(lib().sw_search_pssm_multi_host(mm.ctypes.data, qoffs.ctypes.data, nq, db.ctypes.data, offs.ctypes.data, ntargets, ctypes.byref(sc),
                                           res.ctypes.data))
    return res[:nq * ntargets].reshape(nq, ntargets, 3)


def align_pssm_hits_host(pssm, targets, scoring, hits, nhits=None):
    """sw_align_pssm_hits_host: the alignments of a hit table under PSSM queries in plain C++ on the host (no GPU).  Arguments and
    results as Database.align_pssm_hits."""
    lt, sc = _pssm_scoring(scoring)
    m, qoffs = _pack_pssm(pssm, max(1, sc.nletters))
    packed, offs = _pack_targets(targets)
    nq = len(qoffs) - 1
    hits, nhits = _hit_table(hits, nhits, nq)
    top = hits.shape[1]
    mm = m if m.size else np.zeros((1, 1), np.int8)
    db = packed if len(packed) else np.zeros(1, np.uint8)
    cap = max(1, int(np.diff(qoffs).max(initial=0)) + int(np.diff(offs).max(initial=0)))
    aln = np.zeros((max(1, nq * top), 7), np.int64)
    ops = np.zeros((max(1, nq * top), cap), np.uint8)
    _check(lib().sw_align_pssm_hits_host(mm.ctypes.data, qoffs.ctypes.data, nq, db.ctypes.data, offs.ctypes.data, len(offs) - 1, ctypes.byref(sc),
                                         hits.ctypes.data, nhits.ctypes.data if nhits is not None else None, top, aln.ctypes.data, ops.ctypes.data, cap))
    aln = aln[:nq * top]
    return aln.reshape(nq, top, 7), _ops_rows(aln, ops, cap, nq, top)


def _ops_rows(aln, ops, cap, nq: int, top: int):
    flat = _ops_list(aln.reshape(-1, 7), ops, cap)
    return [flat[q * top:(q + 1) * top] for q in range(nq)]


def format_alignment(query, target, aln_row, ops):
    """The three display lines of an alignment (an sw_alignment row and its ops): the query with '-' where the target has letters
    of its own, a midline ('|' under equal letters, a space otherwise), the target with '-'.  For a PSSM query pass its consensus --
    any string with one letter per column -- as `query`."""
    q, t = _as_seq(query), _as_seq(target)
    j, i = int(aln_row[2]), int(aln_row[3])
    top, mid, bot = [], [], []
    for op in bytes(ops):
        if op == ord("M"):
            top.append(chr(q[j])); bot.append(chr(t[i])); mid.append("|" if q[j] == t[i] else " ")
            j += 1; i += 1
        elif op == ord("I"):
            top.append(chr(q[j])); bot.append("-"); mid.append(" ")
            j += 1
        else:
            top.append("-"); bot.append(chr(t[i])); mid.append(" ")
            i += 1
    return "".join(top), "".join(mid), "".join(bot)


def top_hits(results, k: int):
    """Indices of the k best targets of search results: score descending, then index ascending."""
    scores = np.asarray(results)[:, 1]
    order = np.lexsort((np.arange(len(scores)), -scores))
    return order[: max(0, min(int(k), len(scores)))]


def n_element(i: int, m: int, n: int) -> int:
    return int(lib().sw_nelement(i, m, n))


def first_diag_element(i: int, m: int, n: int):
    si, sj = _i64(), _i64()
    lib().sw_first_diag_element(i, m, n, ctypes.byref(si), ctypes.byref(sj))
    return int(si.value), int(sj.value)


def traceback_host(P: np.ndarray, max_pos: int):
    """backtrack() on a host int32 (or compact int8) P, modified in place. Returns the visited linear indices."""
    rows1, m = P.shape
    assert P.dtype in (np.int32, np.int8) and P.flags.c_contiguous
    path = np.zeros(rows1 + m + 2, np.int64)
    n = _i64()
    _check(lib().sw_traceback_host_ex(P.ctypes.data, P.dtype.itemsize, m - 1, rows1 - 1, int(max_pos), path.ctypes.data, len(path),
                                      ctypes.byref(n)))
    return path[: n.value].copy()


def _as_seq(x) -> np.ndarray:
    if isinstance(x, (bytes, bytearray)):
        return np.frombuffer(bytes(x), np.uint8)
    if isinstance(x, str):
        return np.frombuffer(x.encode(), np.uint8)
    return np.ascontiguousarray(x, dtype=np.uint8)


@dataclass
class Fill:
    """Device-resident result of one DP fill. H: (rows+1, cols+1) int32|int64, P: int32|int8, both torch
    CUDA tensors (either may be None: not written); res: int64[3] tensor (max_pos, max_score, path_len)."""
    H: "torch.Tensor"
    P: "torch.Tensor"
    res: "torch.Tensor"
    cols: int
    rows: int

    def free(self):
        """Release a pair that came from Engine.alloc_outputs now (sw_free_outputs); the tensors must not be used afterwards."""
        owner = getattr(self, "_owner", None)
        self.H = self.P = None
        if owner is not None:
            owner.free()
            self._owner = None

    def result(self):
        r = self.res.cpu().tolist()
        if r[2] < 0:
            raise SwError(-62, f"in-kernel hand-off wait timed out (code {-r[2]})")
        return {"max_pos": r[0], "max_score": r[1], "path_len": r[2]}


class _RawDevice:
    """A device allocation of the library seen by torch (zero-copy, __cuda_array_interface__)."""

    def __init__(self, ptr, shape, typestr, owner):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2}
        self._owner = owner


class _Outputs:
    """Keeps a sw_alloc_outputs pair alive; released with sw_free_outputs when the last tensor that views it is dropped (the tensors
    hold this object through _RawDevice), by Fill.free(), or at the latest by Engine.close().  The engine only keeps a WEAK
    reference: a pair whose Fill was dropped is freed by the garbage collector, not held until the engine goes."""

    def __init__(self, engine, dH, dP):
        self.engine, self.dH, self.dP = engine, dH, dP
        engine._outputs.add(self)

    def free(self):
        """sw_free_outputs, once (the pair must not outlive its context)."""
        if self.dH is None and self.dP is None:
            return
        try:
            if self.engine._h:
                lib().sw_free_outputs(self.engine._h, self.dH, self.dP)
        except Exception:
            pass
        self.dH = self.dP = None

    __del__ = free


class Database:
    """A prepared database (sw_db): Engine.prepare_db makes one.  The checks of the offsets and the schedule of the targets are done once;
    search_affine then takes any number of queries per call.  Keeps the device bytes of the database alive; close() (or leaving the
    `with` block) frees the handle."""

    def __init__(self, engine: "Engine", d_db, offsets):
        self.engine, self.d_db = engine, d_db
        offs = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        if len(offs) == 0:
            offs = np.zeros(1, np.int64)
        self.ntargets = len(offs) - 1
        h = _vp()
        _check(lib().sw_db_create(engine._h, d_db.data_ptr(), offs.ctypes.data, self.ntargets, ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            try:
                lib().sw_db_free(self._h)
            except Exception:  # interpreter shutdown: module globals are already gone
                pass
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self):
        """{"ntargets", "nonempty", "longest", "letters"} of the handle (sw_db_info)."""
        v = [_i64() for _ in range(4)]
        _check(lib().sw_db_info(self._h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("ntargets", "nonempty", "longest", "letters"), (x.value for x in v)))

    def mask_low_complexity(self, window=12, trigger_mbits=2200, extend_mbits=2500, letters=MASK_LETTERS, mask_byte=ord("X")):
        """The low-complexity mask of the handle's bytes on the device (sw_db_mask_low_complexity; include/swhip.h states the rule).
        Returns (masked, nmasked): a fresh uint8 device tensor laid out like the handle's bytes -- mask_byte at the masked positions,
        zero outside [offsets[0], offsets[-1]) -- and the (ntargets,) int64 device tensor of the masked positions per target.
        Engine.prepare_db(masked, offsets) makes the handle to search; keep this one for msa_from_hits (the original letters)."""
        masked, nmasked = self.mask_low_complexity_device(None, None, window, trigger_mbits, extend_mbits, letters, mask_byte)
        return masked, nmasked[:self.ntargets]

    def mask_low_complexity_device(self, out=None, nmasked=None, window=12, trigger_mbits=2200, extend_mbits=2500, letters=MASK_LETTERS,
                                   mask_byte=ord("X")):
        """sw_db_mask_low_complexity into caller tensors; asynchronous on torch's current stream, nothing comes to the host.  out: a
        contiguous uint8 tensor at least as long as the handle's bytes and not those bytes themselves (None: a zeroed one); nmasked: a
        contiguous int64 tensor of at least ntargets elements, None for a fresh one, False for none.  Returns (out, nmasked)."""
        eng = self.engine
        t = eng.torch
        dev = f"cuda:{eng.device}"
        if out is None:
            out = t.zeros_like(self.d_db)
        if out.dtype != t.uint8 or not out.is_contiguous() or out.numel() < self.d_db.numel():
            raise ValueError(f"out must be a contiguous uint8 tensor of at least {self.d_db.numel()} elements")
        if nmasked is None:
            nmasked = t.empty(max(1, self.ntargets), dtype=t.int64, device=dev)
        elif nmasked is False:
            nmasked = None
        if nmasked is not None and (nmasked.dtype != t.int64 or not nmasked.is_contiguous() or nmasked.numel() < self.ntargets):
            raise ValueError(f"nmasked must be a contiguous int64 tensor of at least {self.ntargets} elements")
        mp = _mask_params(window, trigger_mbits, extend_mbits, letters, mask_byte)
        _check(lib().sw_db_mask_low_complexity(eng._h, self._h, ctypes.byref(mp), out.data_ptr(), nmasked.data_ptr() if nmasked is not None else None,
                                               eng._stream()))
        return out, nmasked

    def search_affine(self, queries, scoring):
        """Every query against every target (sw_db_search_affine).  queries: a list of sequences or a (packed uint8, int64 offsets) pair;
        scoring = (submat, gap_open, gap_extend) as for Engine.search_affine.  Returns the (nqueries, ntargets, 3) int64 numpy array of
        (max_pos, max_score, path_len = 0), both axes in input order.  Engine.set_option("search_lanes", 16) runs two targets per
        wave on packed 16-bit lanes for every query whose scores fit them (include/swhip.h has the rule); the result is the same
        byte for byte."""
        eng = self.engine
        t = eng.torch
        qpacked, qoffs = _pack_targets(queries)
        d_q = t.from_numpy(qpacked.copy() if len(qpacked) else np.zeros(1, np.uint8)).to(f"cuda:{eng.device}")
        res = self.search_affine_device(d_q, qoffs, scoring)
        eng.synchronize()
        return res.cpu().numpy()

    def search_affine_device(self, d_queries, qoffsets, scoring, out=None):
        """sw_db_search_affine on device-resident queries (a torch uint8 tensor), host int64 offsets and a host table; asynchronous on
        torch's current stream.  Returns the (nqueries, ntargets, 3) int64 result tensor (a view of `out`, a flat int64 tensor of at
        least nqueries * ntargets * 3 elements, if given)."""
        sub, sc = _affine(*scoring)
        return self._search_call(lib().sw_db_search_affine, d_queries, qoffsets, sc, out)

    def _search_call(self, fn, d_source, qoffsets, sc, out):
        """sw_db_search_affine / sw_db_search_pssm: the queries' letters or their matrices in d_source, the scoring object that goes with them."""
        eng = self.engine
        t = eng.torch
        qoffs = np.ascontiguousarray(qoffsets, np.int64).reshape(-1)
        if len(qoffs) == 0:
            qoffs = np.zeros(1, np.int64)
        nq, n = len(qoffs) - 1, (len(qoffs) - 1) * self.ntargets * 3
        res = out if out is not None else t.zeros(max(3, n), dtype=t.int64, device=f"cuda:{eng.device}")
        if res.dtype != t.int64 or not res.is_contiguous() or res.numel() < n:
            raise ValueError(f"out must be a contiguous int64 tensor of at least {n} elements ({nq} queries x {self.ntargets} targets x 3)")
        _check(fn(eng._h, self._h, d_source.data_ptr(), qoffs.ctypes.data, nq, ctypes.byref(sc), res.data_ptr(), eng._stream()))
        return res[:n].view(nq, self.ntargets, 3)

    def _pssm_to_device(self, pssm, nletters: int):
        """Host PSSMs (see _pack_pssm) -> (flat int8 device tensor, int64 offsets in columns)."""
        eng = self.engine
        t = eng.torch
        m, qoffs = _pack_pssm(pssm, max(1, nletters))
        return t.from_numpy(m.reshape(-1).copy() if m.size else np.zeros(1, np.int8)).to(f"cuda:{eng.device}"), qoffs

    def search_pssm(self, pssm, scoring):
        """Every PSSM query against every target (sw_db_search_pssm).  pssm: a list of per-query (columns, nletters) int8 matrices, or a
        ((total columns, nletters) int8, int64 column offsets) pair; scoring = (letters, other, smax, gap_open, gap_extend): entry k of a
        column scores the target byte letters[k], every other byte scores `other`, entries above smax count as smax.  Returns the
        (nqueries, ntargets, 3) int64 numpy array of (max_pos, max_score, path_len = 0), as search_affine does.  "search_lanes" = 16
        applies as there, with smax in the place of the table's largest entry."""
        d_m, qoffs = self._pssm_to_device(pssm, len(_as_seq(scoring[0])))
        res = self.search_pssm_device(d_m, qoffs, scoring)
        self.engine.synchronize()
        return res.cpu().numpy()

    def search_pssm_device(self, d_pssm, qoffsets, scoring, out=None):
        """sw_db_search_pssm on a device-resident matrix (a torch int8 tensor: column g is the nletters bytes at g * nletters) and host
        int64 column offsets; asynchronous on torch's current stream.  Result and `out` as for search_affine_device."""
        lt, sc = _pssm_scoring(scoring)
        return self._search_call(lib().sw_db_search_pssm, d_pssm, qoffsets, sc, out)

    def search_affine_pairs(self, queries, scoring, pairs):
        """The scores of a list of (query, target) pairs (sw_db_search_affine_pairs): queries and scoring as for search_affine; pairs an
        (npairs, 2) int64 array or a list of (query, target) tuples, any order, duplicates allowed.  Returns the (npairs, 3) int64 numpy
        array of (max_pos, max_score, path_len = 0) in list order; an entry that names no query, no target or an empty target is zero.
        Engine.set_option("search_pairs_lanes", 16) runs two listed pairs of a query per wave on packed 16-bit lanes where the query is
        eligible (include/swhip.h says when); the results are the same bytes under 16 and 32."""
        eng = self.engine
        t = eng.torch
        dev = f"cuda:{eng.device}"
        qpacked, qoffs = _pack_targets(queries)
        pr = _pair_list(pairs)
        d_q = t.from_numpy(qpacked.copy() if len(qpacked) else np.zeros(1, np.uint8)).to(dev)
        d_pairs = t.from_numpy(pr.copy() if len(pr) else np.zeros((1, 2), np.int64)).to(dev)[:len(pr)]
        res = self.search_affine_pairs_device(d_q, qoffs, scoring, d_pairs)
        eng.synchronize()
        return res.cpu().numpy()

    def search_affine_pairs_device(self, d_queries, qoffsets, scoring, d_pairs, out=None):
        """sw_db_search_affine_pairs on device-resident queries and a device pair list, a contiguous torch int64 tensor of shape
        (npairs, 2); asynchronous on torch's current stream, nothing comes to the host.  Returns the (npairs, 3) int64 result tensor
        (a view of `out`, a flat int64 tensor of at least npairs * 3 elements, if given).  The option "search_pairs_lanes" applies as for
        search_affine_pairs; after a call under 16 "last_search_pairs_packed_launches" and "last_search_pairs_packed_items" say what ran
        packed (reading the second waits for the device)."""
        eng = self.engine
        t = eng.torch
        qoffs = np.ascontiguousarray(qoffsets, np.int64).reshape(-1)
        if len(qoffs) == 0:
            qoffs = np.zeros(1, np.int64)
        if d_pairs.dtype != t.int64 or not d_pairs.is_contiguous() or d_pairs.dim() != 2 or d_pairs.shape[1] != 2:
            raise ValueError("d_pairs must be a contiguous int64 tensor of shape (npairs, 2)")
        npairs = d_pairs.shape[0]
        n = npairs * 3
        res = out if out is not None else t.zeros(max(3, n), dtype=t.int64, device=f"cuda:{eng.device}")
        if res.dtype != t.int64 or not res.is_contiguous() or res.numel() < n:
            raise ValueError(f"out must be a contiguous int64 tensor of at least {n} elements ({npairs} pairs x 3)")
        sub, sc = _affine(*scoring)
        _check(lib().sw_db_search_affine_pairs(eng._h, self._h, d_queries.data_ptr(), qoffs.ctypes.data, len(qoffs) - 1, ctypes.byref(sc),
                                               d_pairs.data_ptr() if npairs else None, npairs, res.data_ptr(), eng._stream()))
        return res.view(-1)[:n].view(npairs, 3)

    def prefilter_ungapped(self, queries, submat, min_score: int):
        """The ungapped pre-filter on host queries (sw_db_prefilter_ungapped) with a list that holds every pair: returns numpy
        (pairs, scores), the passing (query, target) pairs sorted ascending as an (npairs, 2) int64 array and the (nqueries, ntargets)
        int32 table of U."""
        eng = self.engine
        t = eng.torch
        qpacked, qoffs = _pack_targets(queries)
        nq = len(qoffs) - 1
        d_q = t.from_numpy(qpacked.copy() if len(qpacked) else np.zeros(1, np.uint8)).to(f"cuda:{eng.device}")
        pairs, npairs, scores = self.prefilter_ungapped_device(d_q, qoffs, submat, min_score, nq * self.ntargets, want_scores=True)
        eng.synchronize()
        pr = pairs.cpu().numpy()[:int(npairs.item())]
        return pr[np.lexsort((pr[:, 1], pr[:, 0]))], scores.cpu().numpy()

    def prefilter_ungapped_device(self, d_queries, qoffsets, submat, min_score: int, cap: int, want_scores: bool = False, out=None):
        """sw_db_prefilter_ungapped on device-resident queries; asynchronous on torch's current stream, nothing comes to the host.
        Returns (pairs, npairs, scores): a (cap, 2) int64 tensor whose first min(npairs, cap) rows are distinct passing pairs in no
        specified order and whose other rows are (-1, -1), a 1-element int64 tensor with the true count, and the (nqueries, ntargets)
        int32 tensor of U or None.  `out`: such a triple of an earlier call to write into again.  The list goes as it is, all cap rows,
        to search_affine_pairs_device: the (-1, -1) rows give zeros there."""
        eng = self.engine
        t = eng.torch
        dev = f"cuda:{eng.device}"
        qoffs = np.ascontiguousarray(qoffsets, np.int64).reshape(-1)
        if len(qoffs) == 0:
            qoffs = np.zeros(1, np.int64)
        nq, cap = len(qoffs) - 1, int(cap)
        if cap < 0:
            raise ValueError("cap must not be negative")
        if out is not None:
            pairs, npairs, scores = out
        else:
            pairs = t.empty((cap, 2), dtype=t.int64, device=dev)
            npairs = t.zeros(1, dtype=t.int64, device=dev)
            scores = t.empty((nq, self.ntargets), dtype=t.int32, device=dev) if want_scores else None
        if pairs.dtype != t.int64 or not pairs.is_contiguous() or tuple(pairs.shape) != (cap, 2):
            raise ValueError(f"the pair list must be a contiguous int64 tensor of shape ({cap}, 2)")
        if npairs.dtype != t.int64 or npairs.numel() != 1:
            raise ValueError("the pair count must be a 1-element int64 tensor")
        if want_scores and (scores is None or scores.dtype != t.int32 or not scores.is_contiguous() or tuple(scores.shape) != (nq, self.ntargets)):
            raise ValueError(f"the scores must be a contiguous int32 tensor of shape ({nq}, {self.ntargets})")
        sub = _submat(submat)
        _check(lib().sw_db_prefilter_ungapped(eng._h, self._h, d_queries.data_ptr(), qoffs.ctypes.data, nq, sub.ctypes.data, int(min_score),
                                              pairs.data_ptr() if cap > 0 else None, cap, npairs.data_ptr(),
                                              scores.data_ptr() if want_scores and scores.numel() else None, eng._stream()))
        return pairs, npairs, (scores if want_scores else None)

    def search_affine_top(self, queries, scoring, top: int, min_score: int = 0):
        """The best `top` targets of every query, selected on the device (sw_db_search_affine_top): the full result table never exists
        and only the hits come back.  queries and scoring as for search_affine.  Returns numpy (hits (nqueries, top, 3) int64 of
        (target, max_pos, max_score) in rank order -- score descending, then target ascending; unused entries (-1, 0, 0) --,
        nhits (nqueries,) int64).  Only targets with max_score >= min_score qualify.  The option "search_lanes" applies to the search
        of every chunk as it does to search_affine; the hits are the same under 16 and 32."""
        eng = self.engine
        t = eng.torch
        qpacked, qoffs = _pack_targets(queries)
        d_q = t.from_numpy(qpacked.copy() if len(qpacked) else np.zeros(1, np.uint8)).to(f"cuda:{eng.device}")
        hits, nhits = self.search_affine_top_device(d_q, qoffs, scoring, top, min_score)
        eng.synchronize()
        return hits.cpu().numpy(), nhits.cpu().numpy()

    def search_affine_top_device(self, d_queries, qoffsets, scoring, top: int, min_score: int = 0, out=None):
        """sw_db_search_affine_top on device-resident queries; asynchronous on torch's current stream.  Returns torch (hits (nqueries,
        top, 3), nhits (nqueries,)), views of `out` = (flat int64 tensor of at least nqueries * top * 3 elements, int64 tensor of at
        least nqueries elements) if given."""
        sub, sc = _affine(*scoring)
        return self._search_top_call(lib().sw_db_search_affine_top, d_queries, qoffsets, sc, top, min_score, out)

    def _search_top_call(self, fn, d_source, qoffsets, sc, top: int, min_score: int, out):
        """sw_db_search_affine_top / sw_db_search_pssm_top (see _search_call)."""
        eng = self.engine
        qoffs = np.ascontiguousarray(qoffsets, np.int64).reshape(-1)
        if len(qoffs) == 0:
            qoffs = np.zeros(1, np.int64)
        nq = len(qoffs) - 1
        hits, nhits = eng._top_out(nq, top, out)
        _check(fn(eng._h, self._h, d_source.data_ptr(), qoffs.ctypes.data, nq, ctypes.byref(sc), int(top), int(min_score), hits.data_ptr(), nhits.data_ptr(),
                  eng._stream()))
        return eng._top_views(hits, nhits, nq, top)

    def search_pssm_top(self, pssm, scoring, top: int, min_score: int = 0):
        """The best `top` targets of every PSSM query (sw_db_search_pssm_top): pssm and scoring as for search_pssm, results as for
        search_affine_top; "search_lanes" = 16 applies as for search_pssm."""
        d_m, qoffs = self._pssm_to_device(pssm, len(_as_seq(scoring[0])))
        hits, nhits = self.search_pssm_top_device(d_m, qoffs, scoring, top, min_score)
        self.engine.synchronize()
        return hits.cpu().numpy(), nhits.cpu().numpy()

    def search_pssm_top_device(self, d_pssm, qoffsets, scoring, top: int, min_score: int = 0, out=None):
        """sw_db_search_pssm_top on a device-resident matrix; asynchronous on torch's current stream.  Results and `out` as for
        search_affine_top_device."""
        lt, sc = _pssm_scoring(scoring)
        return self._search_top_call(lib().sw_db_search_pssm_top, d_pssm, qoffsets, sc, top, min_score, out)

    def search_affine_top_stats(self, queries, scoring, top: int, min_score: int = 0, shift: int = 0):
        """search_affine_top with the score histogram of every query, collected on the device inside the call, chunk by chunk, while
        the chunk's rows are in the workspace (sw_db_search_affine_top_stats).  Returns numpy (hits, nhits, hist (nqueries, 40, 256)
        uint32): hits and nhits are those of search_affine_top, hist is score_hist_host of the full table, which never exists.
        score_fit, score_thresholds and score_evalue turn hist into E-values."""
        eng = self.engine
        t = eng.torch
        qpacked, qoffs = _pack_targets(queries)
        d_q = t.from_numpy(qpacked.copy() if len(qpacked) else np.zeros(1, np.uint8)).to(f"cuda:{eng.device}")
        hits, nhits, hist = self.search_affine_top_stats_device(d_q, qoffs, scoring, top, min_score, shift)
        eng.synchronize()
        return hits.cpu().numpy(), nhits.cpu().numpy(), hist.cpu().numpy().view(np.uint32)

    def search_affine_top_stats_device(self, d_queries, qoffsets, scoring, top: int, min_score: int = 0, shift: int = 0, out=None, hist=None):
        """sw_db_search_affine_top_stats on device-resident queries; asynchronous on torch's current stream.  Returns torch (hits, nhits,
        hist (nqueries, 40, 256) int32 -- the uint32 counters' bits); `out` as for search_affine_top_device, `hist` a contiguous int32
        tensor of at least nqueries x 10240 elements, or None for a fresh one."""
        sub, sc = _affine(*scoring)
        return self._search_top_stats_call(lib().sw_db_search_affine_top_stats, d_queries, qoffsets, sc, top, min_score, shift, out, hist)

    def _search_top_stats_call(self, fn, d_source, qoffsets, sc, top: int, min_score: int, shift: int, out, hist):
        """sw_db_search_affine_top_stats / sw_db_search_pssm_top_stats (see _search_top_call)."""
        eng = self.engine
        qoffs = np.ascontiguousarray(qoffsets, np.int64).reshape(-1)
        if len(qoffs) == 0:
            qoffs = np.zeros(1, np.int64)
        nq = len(qoffs) - 1
        hits, nhits = eng._top_out(nq, top, out)
        hist = eng._hist_out(nq, hist)
        _check(fn(eng._h, self._h, d_source.data_ptr(), qoffs.ctypes.data, nq, ctypes.byref(sc), int(top), int(min_score), hits.data_ptr(), nhits.data_ptr(),
                  int(shift), hist.data_ptr(), eng._stream()))
        return eng._top_views(hits, nhits, nq, top) + (hist.view(-1)[:nq * HIST_CLASSES * HIST_BINS].view(nq, HIST_CLASSES, HIST_BINS),)

    def search_pssm_top_stats(self, pssm, scoring, top: int, min_score: int = 0, shift: int = 0):
        """search_pssm_top with the score histogram of every query (sw_db_search_pssm_top_stats); results as for
        search_affine_top_stats."""
        d_m, qoffs = self._pssm_to_device(pssm, len(_as_seq(scoring[0])))
        hits, nhits, hist = self.search_pssm_top_stats_device(d_m, qoffs, scoring, top, min_score, shift)
        self.engine.synchronize()
        return hits.cpu().numpy(), nhits.cpu().numpy(), hist.cpu().numpy().view(np.uint32)

    def search_pssm_top_stats_device(self, d_pssm, qoffsets, scoring, top: int, min_score: int = 0, shift: int = 0, out=None, hist=None):
        """sw_db_search_pssm_top_stats on a device-resident matrix; results, `out` and `hist` as for search_affine_top_stats_device."""
        lt, sc = _pssm_scoring(scoring)
        return self._search_top_stats_call(lib().sw_db_search_pssm_top_stats, d_pssm, qoffsets, sc, top, min_score, shift, out, hist)

    def hits_threshold(self, thresholds, hits, nhits=None):
        """The thresholds of score_thresholds applied to a hit table (sw_hits_threshold_device): an entry is kept when it is a used entry
        -- below the query's count, target inside the handle and not empty -- and its score reaches thresholds[q, class(length of its
        target)].  thresholds: (nqueries, 40) int64; hits: the (nqueries, top, 3) table; nhits: the counts or None (all top entries).
        Returns numpy (keep (nqueries, top) int32, nkept (nqueries,) int64, the hit table with target = -1 in the dropped entries)."""
        eng = self.engine
        t = eng.torch
        dev = f"cuda:{eng.device}"
        thr = np.ascontiguousarray(thresholds, np.int64)
        if thr.ndim != 2 or thr.shape[1] != HIST_CLASSES:
            raise ValueError(f"thresholds must be (nqueries, {HIST_CLASSES}) int64")
        nq = thr.shape[0]
        hits, nhits = _hit_table(hits, nhits, nq)
        top = hits.shape[1]
        d_thr = t.from_numpy(thr.reshape(-1).copy() if thr.size else np.zeros(1, np.int64)).to(dev)
        d_hits = t.from_numpy(hits.reshape(-1).copy() if hits.size else np.zeros(3, np.int64)).to(dev)
        d_n = t.from_numpy(nhits.copy() if len(nhits) else np.zeros(1, np.int64)).to(dev) if nhits is not None else None
        keep, nkept, out = self.hits_threshold_device(d_thr, nq, top, d_hits, d_n, hits_out=d_hits)
        eng.synchronize()
        return (keep.cpu().numpy()[:nq * top].reshape(nq, top), nkept.cpu().numpy()[:nq], out.cpu().numpy()[:nq * top * 3].reshape(nq, top, 3))

    def hits_threshold_device(self, d_thresholds, nqueries: int, top: int, hits, nhits=None, hits_out=None, keep=None, nkept=None):
        """sw_hits_threshold_device on device tensors; asynchronous on torch's current stream, nothing comes to the host.  d_thresholds:
        int64, nqueries x 40; hits: int64, nqueries x top x 3; nhits: int64 counts or None; hits_out: the tensor that receives the table
        with target = -1 in the dropped entries -- `hits` itself for in place, None for none; keep / nkept: as for
        Engine.msa_filter_device.  Returns (keep, nkept, hits_out), None where there is none."""
        eng = self.engine
        t = eng.torch
        dev = f"cuda:{eng.device}"
        nq, top = int(nqueries), int(top)
        n = max(0, nq) * max(0, top)
        for x, need, what in ((d_thresholds, nq * HIST_CLASSES, "d_thresholds"), (hits, n * 3, "hits"), (hits_out, n * 3, "hits_out"), (nhits, nq, "nhits")):
            if x is not None and (x.dtype != t.int64 or not x.is_contiguous() or x.numel() < need):
                raise ValueError(f"{what} must be a contiguous int64 tensor of at least {need} elements")
        if keep is None:
            keep = t.empty(max(1, n), dtype=t.int32, device=dev)
        elif keep is False:
            keep = None
        if keep is not None and (keep.dtype != t.int32 or not keep.is_contiguous() or keep.numel() < n):
            raise ValueError(f"keep must be a contiguous int32 tensor of at least {n} elements")
        if nkept is None:
            nkept = t.empty(max(1, nq), dtype=t.int64, device=dev)
        elif nkept is False:
            nkept = None
        if nkept is not None and (nkept.dtype != t.int64 or not nkept.is_contiguous() or nkept.numel() < nq):
            raise ValueError(f"nkept must be a contiguous int64 tensor of at least {nq} elements")
        ptr = lambda x: x.data_ptr() if x is not None else None
        _check(lib().sw_hits_threshold_device(eng._h, self._h, ptr(d_thresholds), nq, top, ptr(hits), ptr(nhits), ptr(hits_out), ptr(keep), ptr(nkept),
                                              eng._stream()))
        return keep, nkept, hits_out

    def search_affine_top_prefiltered(self, queries, scoring, prefilter_min_score: int, top: int, min_score: int = 0, cap=None):
        """Filter, rescoring and selection in one call on host queries (sw_db_search_affine_top_prefiltered): the table of
        search_affine_top restricted to the pairs whose ungapped score reaches prefilter_min_score.  cap, the length of the pair list,
        defaults to nqueries x ntargets; SwError if more pairs pass than it holds.  Returns numpy (hits, nhits, npairs).  The rescoring
        follows the option "search_pairs_lanes" as search_affine_pairs does; the hits are the same under 16 and 32."""
        eng = self.engine
        t = eng.torch
        qpacked, qoffs = _pack_targets(queries)
        nq = len(qoffs) - 1
        cap = nq * self.ntargets if cap is None else int(cap)
        d_q = t.from_numpy(qpacked.copy() if len(qpacked) else np.zeros(1, np.uint8)).to(f"cuda:{eng.device}")
        hits, nhits, npairs = self.search_affine_top_prefiltered_device(d_q, qoffs, scoring, prefilter_min_score, cap, top, min_score)
        eng.synchronize()
        n = int(npairs.item())
        if n > cap:
            raise SwError(-22, f"search_affine_top_prefiltered: {n} pairs pass the pre-filter, the list holds {cap}: raise cap or prefilter_min_score")
        return hits.cpu().numpy(), nhits.cpu().numpy(), n

    def search_affine_top_prefiltered_device(self, d_queries, qoffsets, scoring, prefilter_min_score: int, cap: int, top: int, min_score: int = 0,
                                             out=None):
        """sw_db_search_affine_top_prefiltered on device-resident queries; asynchronous on torch's current stream, nothing comes to the
        host.  Returns torch (hits (nqueries, top, 3), nhits (nqueries,), npairs (1,)): the table and the pre-filter's TRUE count --
        where it exceeds cap the table is neither complete nor reproducible, the caller checks.  `out` = (hits, nhits) as for
        search_affine_top_device.  The rescoring follows the option "search_pairs_lanes" (search_affine_pairs_device)."""
        eng = self.engine
        t = eng.torch
        qoffs = np.ascontiguousarray(qoffsets, np.int64).reshape(-1)
        if len(qoffs) == 0:
            qoffs = np.zeros(1, np.int64)
        nq = len(qoffs) - 1
        hits, nhits = eng._top_out(nq, top, out)
        npairs = t.zeros(1, dtype=t.int64, device=f"cuda:{eng.device}")
        sub, sc = _affine(*scoring)
        _check(lib().sw_db_search_affine_top_prefiltered(eng._h, self._h, d_queries.data_ptr(), qoffs.ctypes.data, nq, ctypes.byref(sc),
                                                         int(prefilter_min_score), int(cap), int(top), int(min_score), hits.data_ptr(),
                                                         nhits.data_ptr(), npairs.data_ptr(), eng._stream()))
        return eng._top_views(hits, nhits, nq, top) + (npairs,)

    def align_affine_hits(self, queries, scoring, hits, nhits=None, checkpoint=None):
        """The alignments of a hit table (sw_db_align_affine_hits): queries and scoring as for search_affine; hits a (nqueries, top, 3)
        int64 array of (target, max_pos, max_score) as search_affine_top returns it -- or (nqueries, top) target indices --, nhits the
        (nqueries,) counts or None for whole rows.  Returns (aln, ops): aln the (nqueries, top, 7) int64 numpy array of (max_pos,
        max_score, q_begin, t_begin, q_end, t_end, nops), all zeros for unused entries and targets outside the database; ops a list per
        query of `top` bytes objects over b"MID".  checkpoint: the option "align_checkpoint" (0, 1, 2) for this call alone."""
        t = self.engine.torch
        qpacked, qoffs = _pack_targets(queries)
        d_q = t.from_numpy(qpacked.copy() if len(qpacked) else np.zeros(1, np.uint8)).to(f"cuda:{self.engine.device}")
        return self._align_hits_from_host(self.align_affine_hits_device, d_q, qoffs, scoring, hits, nhits, checkpoint)

    def _align_hits_from_host(self, device_call, d_source, qoffs, scoring, hits, nhits, checkpoint):
        """align_affine_hits / align_pssm_hits behind the upload of their queries: the host hit table to the device, the call, the
        results back."""
        eng = self.engine
        t = eng.torch
        dev = f"cuda:{eng.device}"
        nq = len(qoffs) - 1
        hits, nhits = _hit_table(hits, nhits, nq)
        top = hits.shape[1]
        d_hits = t.from_numpy(hits.reshape(-1).copy() if hits.size else np.zeros(3, np.int64)).to(dev)
        d_nhits = t.from_numpy(nhits.copy()).to(dev) if nhits is not None and len(nhits) else None
        cap = max(1, int(np.diff(qoffs).max(initial=0)) + self.info()["longest"])
        aln, ops = device_call(d_source, qoffs, scoring, d_hits.view(nq, top, 3) if hits.size else d_hits, d_nhits, ops_cap=cap, top=top, checkpoint=checkpoint)
        eng.synchronize()
        aln = aln.cpu().numpy()
        return aln, _ops_rows(aln, ops.cpu().numpy().reshape(-1, cap), cap, nq, top)

    def align_pssm_hits(self, pssm, scoring, hits, nhits=None, checkpoint=None):
        """The alignments of a hit table under PSSM queries (sw_db_align_pssm_hits): pssm and scoring as for search_pssm, everything
        else as for align_affine_hits."""
        d_m, qoffs = self._pssm_to_device(pssm, len(_as_seq(scoring[0])))
        return self._align_hits_from_host(self.align_pssm_hits_device, d_m, qoffs, scoring, hits, nhits, checkpoint)

    def align_pssm_hits_device(self, d_pssm, qoffsets, scoring, hits, nhits, ops_cap: int = 0, out=None, top=None, checkpoint=None):
        """sw_db_align_pssm_hits on a device-resident matrix and a device hit table; everything else as for align_affine_hits_device."""
        lt, sc = _pssm_scoring(scoring)
        return self._align_hits_call(lib().sw_db_align_pssm_hits, d_pssm, qoffsets, sc, hits, nhits, ops_cap, out, top, checkpoint)

    def _upload_hit_tables(self, hits, nhits, aln, ops, nq: int):
        """The host tables of pssm_from_hits, pssm_hit_weights and msa_from_hits (_pack_hit_tables) as device tensors -> (top, ops_cap,
        d_hits, d_nhits, d_aln, d_ops)."""
        t, dev = self.engine.torch, f"cuda:{self.engine.device}"
        hits, nhits, top, a, o, cap = _pack_hit_tables(hits, nhits, aln, ops, nq)
        d_hits = t.from_numpy(hits.reshape(-1).copy() if hits.size else np.zeros(3, np.int64)).to(dev)
        d_nhits = t.from_numpy(nhits.copy()).to(dev) if nhits is not None and len(nhits) else None
        return top, cap, d_hits, d_nhits, t.from_numpy(a.reshape(-1).copy()).to(dev), t.from_numpy(o.reshape(-1).copy()).to(dev)

    def _hit_table_args(self, qoffsets, hits, nhits, top, aln=None, ops=None, ops_cap=0):
        """What every call on a device hit table checks first -> (qoffs, nq, top, n = nq * top): the int64 offsets; `top`, from the
        table's shape where it is not given; hits and nhits; with `aln`, the alignments and ops of a call that READS them (the
        alignment calls, which write them, check their `out` themselves)."""
        t = self.engine.torch
        qoffs = np.ascontiguousarray(qoffsets, np.int64).reshape(-1)
        if len(qoffs) == 0:
            qoffs = np.zeros(1, np.int64)
        nq = len(qoffs) - 1
        if top is None:
            if hits.dim() != 3:
                raise ValueError("hits must be (nqueries, top, 3), or `top` given")
            top = hits.shape[1]
        top = int(top)
        n = nq * max(0, top)
        if hits.dtype != t.int64 or not hits.is_contiguous() or hits.numel() < n * 3:
            raise ValueError(f"hits must be a contiguous int64 tensor of at least {nq} x {top} x 3 elements")
        if nhits is not None and (nhits.dtype != t.int64 or not nhits.is_contiguous() or nhits.numel() < nq):
            raise ValueError(f"nhits must be a contiguous int64 tensor of at least {nq} elements")
        if aln is not None:
            if aln.dtype != t.int64 or not aln.is_contiguous() or aln.numel() < n * 7:
                raise ValueError(f"aln must be a contiguous int64 tensor of at least {n * 7} elements")
            if ops is not None and (ops.dtype != t.uint8 or not ops.is_contiguous() or ops.numel() < n * max(0, int(ops_cap))):
                raise ValueError(f"ops must be a contiguous uint8 tensor of at least {n * max(0, int(ops_cap))} elements")
        return qoffs, nq, top, n

    def pssm_from_hits(self, prior, scoring, update, hits, nhits, aln, ops, weights=None, want_counts: bool = False):
        """The next iteration's PSSM from aligned hits (sw_db_pssm_from_hits).  prior and scoring as for search_pssm; update =
        (submat, prior_weight, include_min_score); hits, nhits as search_pssm_top returns them, aln and ops as align_pssm_hits returns
        them (ops: the list per query of bytes objects, or a (nqueries, top, ops_cap) uint8 array); weights a (nqueries, top) int32
        array or None for 1.  Returns the new (total columns, nletters) int8 matrix -- the columns in front of the first query are the
        prior's --, with want_counts (matrix, counts): the (columns of the queries, nletters) int32 counts.  include/swhip.h states the
        rule: a column's new row is the rounded weighted mean of its prior row and the table rows of the residues aligned to it."""
        eng = self.engine
        t = eng.torch
        dev = f"cuda:{eng.device}"
        nl = max(1, len(_as_seq(scoring[0])))
        m, qoffs = _pack_pssm(prior, nl)
        nq = len(qoffs) - 1
        d_m = t.from_numpy(m.reshape(-1).copy() if m.size else np.zeros(1, np.int8)).to(dev)
        top, cap, d_hits, d_nhits, d_aln, d_ops = self._upload_hit_tables(hits, nhits, aln, ops, nq)
        d_w = t.from_numpy(np.ascontiguousarray(weights, np.int32).reshape(-1).copy()).to(dev) if weights is not None and nq * top else None
        counts = t.zeros(max(1, int(qoffs[-1] - qoffs[0]) * nl), dtype=t.int32, device=dev) if want_counts else None
        out = self.pssm_from_hits_device(d_m, qoffs, scoring, update, d_hits, d_nhits, d_aln, d_ops, cap, weights=d_w, top=top, counts=counts)
        eng.synchronize()
        res = out.cpu().numpy().reshape(-1, nl)[:len(m)]
        return (res, counts.cpu().numpy().reshape(-1, nl)[:int(qoffs[-1] - qoffs[0])]) if want_counts else res

    def pssm_from_hits_device(self, d_prior, qoffsets, scoring, update, hits, nhits, aln, ops, ops_cap: int, weights=None, out=None, top=None,
                              counts=None):
        """sw_db_pssm_from_hits on device-resident tables: the prior (a torch int8 tensor in the layout of d_pssm), the hit table and
        counts of search_pssm_top_device, the alignments and ops of align_pssm_hits_device, optional int32 weights; asynchronous on
        torch's current stream, nothing comes to the host.  out: the int8 tensor that receives the new matrix (the columns of the
        queries are written, nothing else), None for a fresh copy of the prior, or d_prior itself (in place); False: counts only.
        counts: an int32 tensor of at least (columns of the queries) x nletters elements, or None.  Returns `out` (counts with
        out=False)."""
        eng = self.engine
        t = eng.torch
        lt, sc = _pssm_scoring(scoring)
        sub, up = _pssm_update(update)
        qoffs, nq, top, n = self._hit_table_args(qoffsets, hits, nhits, top, aln, ops, ops_cap)
        nl = max(1, sc.nletters)
        if d_prior.dtype != t.int8 or not d_prior.is_contiguous() or d_prior.numel() < int(qoffs[-1]) * nl:
            raise ValueError(f"d_prior must be a contiguous int8 tensor of at least {int(qoffs[-1]) * nl} elements")
        if weights is not None and (weights.dtype != t.int32 or not weights.is_contiguous() or weights.numel() < n):
            raise ValueError(f"weights must be a contiguous int32 tensor of at least {n} elements")
        if out is None:
            out = d_prior.clone()
        elif out is False:
            out = None
        if out is not None and (out.dtype != t.int8 or not out.is_contiguous() or out.numel() < int(qoffs[-1]) * nl):
            raise ValueError(f"out must be a contiguous int8 tensor of at least {int(qoffs[-1]) * nl} elements")
        ncnt = int(qoffs[-1] - qoffs[0]) * nl
        if counts is not None and (counts.dtype != t.int32 or not counts.is_contiguous() or counts.numel() < ncnt):
            raise ValueError(f"counts must be a contiguous int32 tensor of at least {ncnt} elements")
        _check(lib().sw_db_pssm_from_hits(eng._h, self._h, d_prior.data_ptr(), qoffs.ctypes.data, nq, ctypes.byref(sc), ctypes.byref(up), hits.data_ptr(),
                                          nhits.data_ptr() if nhits is not None else None, top, aln.data_ptr(), ops.data_ptr() if ops is not None else None,
                                          int(ops_cap), weights.data_ptr() if weights is not None else None, out.data_ptr() if out is not None else None,
                                          counts.data_ptr() if counts is not None else None, eng._stream()))
        return out if out is not None else counts

    def pssm_hit_weights(self, scoring, weighting, qoffsets_or_pssm, hits, nhits, aln, ops):
        """The position-based (Henikoff) weights of aligned hits (sw_db_pssm_hit_weights): the `weights` of pssm_from_hits.  scoring as
        for search_pssm; weighting = (per_hit, include_min_score); qoffsets_or_pssm: the int64 column offsets of the queries, or the
        PSSM as search_pssm takes it (only its offsets are used); hits, nhits, aln, ops as for pssm_from_hits.  Returns the (nqueries,
        top) int32 weights.  include/swhip.h states the rule."""
        eng = self.engine
        qoffs = _query_offsets(qoffsets_or_pssm, max(1, len(_as_seq(scoring[0]))))
        nq = len(qoffs) - 1
        top, cap, d_hits, d_nhits, d_aln, d_ops = self._upload_hit_tables(hits, nhits, aln, ops, nq)
        out = self.pssm_hit_weights_device(qoffs, scoring, weighting, d_hits, d_nhits, d_aln, d_ops, cap, top=top)
        eng.synchronize()
        return out.cpu().numpy()[:nq * top].reshape(nq, top)

    def pssm_hit_weights_device(self, qoffsets, scoring, weighting, hits, nhits, aln, ops, ops_cap: int, out=None, top=None):
        """sw_db_pssm_hit_weights on device-resident tables: the hit table and counts of search_pssm_top_device, the alignments and ops
        of align_pssm_hits_device; asynchronous on torch's current stream, nothing comes to the host.  out: the int32 tensor of at
        least nqueries x top elements that receives the weights (every entry is written), None for a fresh (nqueries, top) one.
        Returns `out`: the `weights` of pssm_from_hits_device."""
        eng = self.engine
        t = eng.torch
        lt, sc = _pssm_scoring(scoring)
        wt = _pssm_weighting(weighting)
        qoffs, nq, top, n = self._hit_table_args(qoffsets, hits, nhits, top, aln, ops, ops_cap)
        if out is None:
            out = t.empty((nq, max(0, top)) if n else (1,), dtype=t.int32, device=f"cuda:{eng.device}")
        if out.dtype != t.int32 or not out.is_contiguous() or out.numel() < n:
            raise ValueError(f"out must be a contiguous int32 tensor of at least {n} elements")
        _check(lib().sw_db_pssm_hit_weights(eng._h, self._h, qoffs.ctypes.data, nq, ctypes.byref(sc), ctypes.byref(wt), hits.data_ptr(),
                                            nhits.data_ptr() if nhits is not None else None, top, aln.data_ptr(), ops.data_ptr() if ops is not None else None,
                                            int(ops_cap), out.data_ptr(), eng._stream()))
        return out

    def msa_from_hits(self, queries, include_min_score, hits, nhits, aln, ops):
        """The query-anchored alignment of aligned hits (sw_db_msa_from_hits).  queries: the sequences as for search_affine, or the 1-D
        int64 column offsets of PSSM queries (no letters: nident is 0); hits, nhits, aln, ops as for pssm_from_hits.  Returns (cols,
        rows, a3m) as numpy arrays: cols, uint8, query q's (top, qlen) matrix of column rows at (qoffsets[q] - qoffsets[0]) * top;
        rows, (nqueries, top) of MSA_ROW; a3m, uint8, entry (q, r)'s A3M row at rows[q, r]["off"], rows[q, r]["len"] bytes.
        include/swhip.h states the rule.  Two calls: one for the rows and the size, one for the bytes."""
        eng = self.engine
        t = eng.torch
        dev = f"cuda:{eng.device}"
        qpacked, qoffs = _msa_queries(queries)
        nq = len(qoffs) - 1
        d_q = t.from_numpy(qpacked.copy()).to(dev) if qpacked is not None and len(qpacked) else None
        top, cap, d_hits, d_nhits, d_aln, d_ops = self._upload_hit_tables(hits, nhits, aln, ops, nq)
        tables = (d_q, qoffs, include_min_score, d_hits, d_nhits, d_aln, d_ops, cap)
        _, rows, _, total = self.msa_from_hits_device(*tables, top=top, cols=False)
        eng.synchronize()
        a3m = t.zeros(max(1, int(total.item())), dtype=t.uint8, device=dev)
        cols, rows, a3m, total = self.msa_from_hits_device(*tables, top=top, rows=rows, a3m=a3m, a3m_cap=int(total.item()), a3m_bytes=total)
        eng.synchronize()
        ncols = int(qoffs[-1] - qoffs[0])
        return (cols.cpu().numpy()[:ncols * top], rows.cpu().numpy().view(MSA_ROW).reshape(-1)[:nq * top].reshape(nq, top),
                a3m.cpu().numpy()[:int(total.item())])

    def msa_from_hits_device(self, d_queries, qoffsets, include_min_score, hits, nhits, aln, ops, ops_cap: int, top=None, cols=None, rows=None,
                             a3m=None, a3m_cap=None, a3m_bytes=None):
        """sw_db_msa_from_hits on device-resident tables: the query letters (a uint8 tensor, query q at qoffsets[q]; None for PSSM
        queries), the hit table and counts of search_*_top_device, the alignments and ops of align_*_hits_device; asynchronous on
        torch's current stream, nothing comes to the host.  cols: the uint8 tensor of at least (columns of the queries) x top elements
        that receives the column rows, None for a fresh one, False for none.  rows: the int64 tensor of at least nqueries x top x 3
        elements that receives the sw_msa_row table (24 bytes per entry: view its numpy copy as MSA_ROW), None for a fresh one, False
        for none (the column rows alone).  a3m: the uint8 tensor that receives the A3M rows, None for none (the rows and the total
        alone: a sizing call); a3m_cap: the bytes of it the call may write (default: all).  a3m_bytes: the int64 tensor that receives
        the true total, None for a fresh one.  Returns (cols, rows, a3m, a3m_bytes), None where there is none."""
        eng = self.engine
        t = eng.torch
        dev = f"cuda:{eng.device}"
        qoffs, nq, top, n = self._hit_table_args(qoffsets, hits, nhits, top, aln, ops, ops_cap)
        if d_queries is not None and (d_queries.dtype != t.uint8 or not d_queries.is_contiguous() or d_queries.numel() < int(qoffs[-1])):
            raise ValueError(f"d_queries must be a contiguous uint8 tensor of at least {int(qoffs[-1])} elements")
        ncols = int(qoffs[-1] - qoffs[0]) * max(0, top)
        if cols is None:
            cols = t.empty(max(1, ncols), dtype=t.uint8, device=dev)
        elif cols is False:
            cols = None
        if cols is not None and (cols.dtype != t.uint8 or not cols.is_contiguous() or cols.numel() < ncols):
            raise ValueError(f"cols must be a contiguous uint8 tensor of at least {ncols} elements")
        if rows is None:
            rows = t.empty(max(1, n) * 3, dtype=t.int64, device=dev)
        elif rows is False:
            rows = None
        if rows is not None and (rows.dtype != t.int64 or not rows.is_contiguous() or rows.numel() < n * 3):
            raise ValueError(f"rows must be a contiguous int64 tensor of at least {n * 3} elements")
        if a3m is not None and (a3m.dtype != t.uint8 or not a3m.is_contiguous()):
            raise ValueError("a3m must be a contiguous uint8 tensor")
        if a3m_cap is None:
            a3m_cap = a3m.numel() if a3m is not None else 0
        if a3m is not None and a3m.numel() < int(a3m_cap):
            raise ValueError(f"a3m must hold at least a3m_cap = {int(a3m_cap)} elements")
        if a3m_bytes is None and rows is not None:
            a3m_bytes = t.zeros(1, dtype=t.int64, device=dev)
        if a3m_bytes is not None and (a3m_bytes.dtype != t.int64 or a3m_bytes.numel() < 1):
            raise ValueError("a3m_bytes must be an int64 tensor of at least one element")
        _check(lib().sw_db_msa_from_hits(eng._h, self._h, d_queries.data_ptr() if d_queries is not None else None, qoffs.ctypes.data, nq,
                                         int(include_min_score), hits.data_ptr(), nhits.data_ptr() if nhits is not None else None, top, aln.data_ptr(),
                                         ops.data_ptr() if ops is not None else None, int(ops_cap), cols.data_ptr() if cols is not None else None,
                                         rows.data_ptr() if rows is not None else None, a3m.data_ptr() if a3m is not None else None, int(a3m_cap),
                                         a3m_bytes.data_ptr() if a3m_bytes is not None else None, eng._stream()))
        return cols, rows, a3m, a3m_bytes

    def align_affine_hits_device(self, d_queries, qoffsets, scoring, hits, nhits, ops_cap: int = 0, out=None, top=None, checkpoint=None):
        """sw_db_align_affine_hits on device-resident queries and a device hit table -- the (nqueries, top, 3) int64 tensor and the
        (nqueries,) counts that search_affine_top_device or Engine.top_hits_device return (nhits may be None: whole rows; `top` is needed
        only where the table's shape does not tell it); asynchronous on torch's current stream, nothing comes to the host.  Returns
        (aln, ops): the (nqueries, top, 7) int64 tensor and the (nqueries, top, ops_cap) uint8 tensor (None with ops_cap = 0:
        coordinates only); out = (aln, ops) reuses given tensors.  checkpoint: the option "align_checkpoint" for this call alone."""
        sub, sc = _affine(*scoring)
        return self._align_hits_call(lib().sw_db_align_affine_hits, d_queries, qoffsets, sc, hits, nhits, ops_cap, out, top, checkpoint)

    def _align_hits_call(self, fn, d_source, qoffsets, sc, hits, nhits, ops_cap, out, top, checkpoint):
        """sw_db_align_affine_hits / sw_db_align_pssm_hits (see _search_call)."""
        eng = self.engine
        t = eng.torch
        qoffs, nq, top, n = self._hit_table_args(qoffsets, hits, nhits, top)
        dev = f"cuda:{eng.device}"
        aln, ops = out if out is not None else (t.zeros((max(1, n), 7), dtype=t.int64, device=dev),
                                                t.zeros((max(1, n), ops_cap), dtype=t.uint8, device=dev) if ops_cap > 0 else None)
        if aln.dtype != t.int64 or not aln.is_contiguous() or aln.numel() < n * 7:
            raise ValueError(f"out: aln must be a contiguous int64 tensor of at least {n * 7} elements")
        if ops is not None and (ops.dtype != t.uint8 or not ops.is_contiguous() or ops.numel() < n * ops_cap):
            raise ValueError(f"out: ops must be a contiguous uint8 tensor of at least {n * ops_cap} elements")
        with eng._checkpoint(checkpoint):
            _check(fn(eng._h, self._h, d_source.data_ptr(), qoffs.ctypes.data, nq, ctypes.byref(sc), hits.data_ptr(),
                      nhits.data_ptr() if nhits is not None else None, top, aln.data_ptr(), ops.data_ptr() if ops is not None else None, ops_cap, eng._stream()))
        return (aln.view(-1)[:n * 7].view(nq, max(0, top), 7),
                ops.view(-1)[:n * ops_cap].view(nq, max(0, top), ops_cap) if ops is not None else None)


class Engine:
    """One GPU's fill engine (sw_ctx). Uses torch only for device buffers / current stream."""

    def __init__(self, device: int = 0):
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("smith-waterman_amd.Engine needs a GPU (no CPU fallback exists)")
        self.torch = torch
        self.device = device
        torch.cuda.set_device(device)
        h = _vp()
        self._outputs = weakref.WeakSet()   # live sw_alloc_outputs pairs (weak: dropping a Fill frees its pair; close() frees survivors)
        _check(lib().sw_create(device, ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            for o in list(getattr(self, "_outputs", [])):
                o.free()
            try:
                lib().sw_destroy(self._h)
            except Exception:  # interpreter shutdown: module globals are already gone
                pass
            self._h = None

    __del__ = close

    def set_option(self, name: str, value: int):
        _check(lib().sw_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        return int(lib().sw_get_option(self._h, name.encode()))

    @contextlib.contextmanager
    def _checkpoint(self, mode):
        """The option "align_checkpoint" set to `mode` for one call and restored after it (None: left as it is)."""
        if mode is None:
            yield
            return
        before = self.get_option("align_checkpoint")
        self.set_option("align_checkpoint", mode)
        try:
            yield
        finally:
            self.set_option("align_checkpoint", before)

    def _stream(self):
        return _vp(self.torch.cuda.current_stream(self.device).cuda_stream)

    def to_device(self, seq):
        """Sequence -> uint8 device tensor with 16 zeroed spare bytes behind it, at an address torch aligns to 512 bytes: the fills want b
        16-byte aligned and may load the rest of the aligned 16-byte window that holds the last byte of a sequence (include/swhip.h,
        READ extents); results never depend on those bytes."""
        t = self.torch
        s = _as_seq(seq)
        d = t.zeros(len(s) + 16, dtype=t.uint8, device=f"cuda:{self.device}")
        if len(s):
            d[: len(s)] = t.from_numpy(s.copy())
        return d, len(s)

    def alloc(self, cols: int, rows: int, h_dtype=None, p_dtype=None, want_h: bool = True, want_p: bool = True):
        """Plain output buffers (torch allocations): H int32|int64, P int32 (the reference layout) or int8 (compact P, same
        codes); either may be left out (matrix-less fills).  For the placement that makes a big fill fast see alloc_outputs."""
        t = self.torch
        h_dtype = h_dtype or t.int32
        p_dtype = p_dtype or t.int32
        assert p_dtype in (t.int32, t.int8)
        dev = f"cuda:{self.device}"
        H = t.empty((rows + 1, cols + 1), dtype=h_dtype, device=dev) if want_h else None
        P = t.empty((rows + 1, cols + 1), dtype=p_dtype, device=dev) if want_p else None
        return Fill(H, P, t.zeros(3, dtype=t.int64, device=dev), cols, rows)

    def alloc_outputs(self, d_a, d_b, cols: int, rows: int, h_dtype=None, p_dtype=None, trials: int = 0, scores=DEFAULT_SCORES):
        """Output buffers through the C-ABI allocator sw_alloc_outputs (what a C caller gets): candidate placements
        tried with real fills of this problem, the fastest kept.  Returns (Fill, [ms of every candidate tried])."""
        t = self.torch
        h_dtype = h_dtype or t.int32
        p_dtype = p_dtype or t.int32
        n = trials if trials > 0 else 16
        ms = (ctypes.c_float * n)()
        dH, dP = _vp(), _vp()
        sc = _Scores(*scores)
        self.synchronize()
        _check(lib().sw_alloc_outputs(self._h, d_a.data_ptr(), cols, d_b.data_ptr(), rows, ctypes.byref(sc), 8 if h_dtype == t.int64 else 4,
                                      1 if p_dtype == t.int8 else 4, trials, ctypes.byref(dH), ctypes.byref(dP), ms))
        owner = _Outputs(self, dH.value, dP.value)
        shape = (rows + 1, cols + 1)
        H = t.as_tensor(_RawDevice(dH.value, shape, "<i8" if h_dtype == t.int64 else "<i4", owner), device=f"cuda:{self.device}")
        P = t.as_tensor(_RawDevice(dP.value, shape, "|i1" if p_dtype == t.int8 else "<i4", owner), device=f"cuda:{self.device}")
        out = Fill(H, P, t.zeros(3, dtype=t.int64, device=f"cuda:{self.device}"), cols, rows)
        out._owner = owner
        return out, [x for x in ms if x > 0]

    def fill_into(self, out: Fill, d_a, d_b, scores=DEFAULT_SCORES, top=None):
        """Asynchronous fill on torch's current stream into pre-allocated buffers."""
        t = self.torch
        sc = _Scores(*scores)
        hb = 8 if (out.H is not None and out.H.dtype == t.int64) else 4
        _check(lib().sw_fill_device_ex(self._h, d_a.data_ptr(), out.cols, d_b.data_ptr(), out.rows, ctypes.byref(sc),
                                       out.H.data_ptr() if out.H is not None else None, hb,
                                       out.P.data_ptr() if out.P is not None else None, out.P.element_size() if out.P is not None else 4,
                                       top.data_ptr() if top is not None else None, out.res.data_ptr(), self._stream()))
        return out

    def fill(self, a, b, scores=DEFAULT_SCORES, h_dtype=None, top=None, p_dtype=None, want_h: bool = True, want_p: bool = True) -> Fill:
        d_a, cols = self.to_device(a)
        d_b, rows = self.to_device(b)
        out = self.alloc(cols, rows, h_dtype, p_dtype, want_h=want_h, want_p=want_p)
        if top is not None:
            top = self.torch.as_tensor(np.ascontiguousarray(top, np.int32)).to(f"cuda:{self.device}")
        self.fill_into(out, d_a, d_b, scores, top)
        self.synchronize()
        return out

    def fill_tile(self, H, P, i0: int, j0: int, trows: int, tcols: int, d_a, d_b, res, scores=DEFAULT_SCORES,
                  top=None, left=None, right=None):
        """Asynchronous fill of the tile rows i0+1..i0+trows x cols j0+1..j0+tcols of the matrices H, P
        (torch CUDA tensors with row stride H.shape[1]).  d_a / d_b: the FULL padded device sequences;
        top: int32 tensor with tcols+1 H values of row i0 (or None), left: trows+1 values of column j0,
        right: output tensor (trows+1) for column j0+tcols.  i0 must be a multiple of 16."""
        t = self.torch
        assert i0 % 16 == 0, "tile rows must start at a multiple of 16 (16-byte aligned b window)"
        sc = _Scores(*scores)
        stride = H.shape[1]
        hb = 8 if H.dtype == t.int64 else 4
        corner = i0 * stride + j0
        _check(lib().sw_fill_tile_device(
            self._h, d_a.data_ptr() + j0, tcols, d_b.data_ptr() + i0, trows, ctypes.byref(sc),
            H.data_ptr() + corner * hb, hb, P.data_ptr() + corner * 4, stride,
            top.data_ptr() if top is not None else None, left.data_ptr() if left is not None else None,
            right.data_ptr() if right is not None else None, res.data_ptr(), self._stream()))

    def fill_band(self, d_a, cols, d_b, rows, total_rows, H, P, res, top_gran=None, top_tag=0, bot_gran=None, bot_tag=0, bot_done=None,
                  reserve_cus=0, concurrent=False, scores=DEFAULT_SCORES):
        """Asynchronous band-resident launch (sw_fill_band_device): H/P (rows+1, cols+1) band-local tensors or None;
        top_gran / bot_gran: int64 tensors with cols+1 granules (tag << 32 | H); bot_done: int32 tensor, one per strip
        (device, or pinned host memory)."""
        t = self.torch
        sc = _Scores(*scores)
        hb = 8 if (H is not None and H.dtype == t.int64) else 4
        ptr = lambda x: x.data_ptr() if x is not None else None
        _check(lib().sw_fill_band_device(self._h, d_a.data_ptr(), cols, d_b.data_ptr(), rows, total_rows, ctypes.byref(sc), ptr(H), hb,
                                         ptr(P), P.element_size() if P is not None else 4, ptr(top_gran), top_tag, ptr(bot_gran), bot_tag,
                                         ptr(bot_done), reserve_cus, 1 if concurrent else 0, res.data_ptr(), self._stream()))

    def batch(self, a_all, b_all, scores=DEFAULT_SCORES, store: bool = False, p_dtype=None, store_h=None, traceback: bool = False,
              want_paths: bool = False):
        """npairs independent problems (BASELINE config 5).  a_all: (npairs, cols) uint8, b_all: (npairs, rows).
        store: write P (int32, or int8 with p_dtype=torch.int8) and -- unless store_h is False -- H of every pair.
        traceback: also run backtrack() per pair (needs P); results[:, 2] then holds the path lengths.
        Returns (results[npairs,3] int64 tensor, H, P) -- plus the paths tensor (npairs, cols+rows+2) when want_paths."""
        d_a, d_b, cols, rows = self.batch_to_device(a_all, b_all)
        return self.batch_device(d_a, d_b, cols, rows, scores, store, p_dtype, store_h, traceback, want_paths)

    def batch_to_device(self, a_all, b_all):
        """Host sequences of a batch -> device tensors in the layout sw_batch_device wants: b_stride a multiple of 16 (rows of b zero padded;
        the batch kernels read none of the padding), a at its tight stride."""
        t = self.torch
        a_all = np.ascontiguousarray(a_all, np.uint8)
        b_all = np.ascontiguousarray(b_all, np.uint8)
        npairs, cols = a_all.shape
        rows = b_all.shape[1]
        dev = f"cuda:{self.device}"
        bstr = (rows + 15) // 16 * 16
        d_a = t.from_numpy(a_all).to(dev)
        bpad = np.zeros((npairs, bstr), np.uint8)
        bpad[:, :rows] = b_all
        return d_a, t.from_numpy(bpad).to(dev), cols, rows

    def batch_device(self, d_a, d_b, cols: int, rows: int, scores=DEFAULT_SCORES, store: bool = False, p_dtype=None, store_h=None,
                     traceback: bool = False, want_paths: bool = False, out=None, paths=None):
        """sw_batch_device_ex (+ sw_batch_traceback_device) on sequences already resident in HBM (batch_to_device).  d_a / d_b are
        (npairs, a_stride) / (npairs, b_stride) uint8 tensors: the strides may exceed cols / rows (b_stride a multiple of 16).  `out`:
        (res, H, P) tensors of an earlier call to write into again; `paths`: an (npairs, cols + rows + 2) int64 tensor for want_paths."""
        t = self.torch
        npairs = d_a.shape[0]
        dev = f"cuda:{self.device}"
        if out is not None:
            res, H, P = out
        else:
            res = t.zeros((npairs, 3), dtype=t.int64, device=dev)
            H = P = None
            if store:
                if store_h is None or store_h:
                    H = t.empty((npairs, rows + 1, cols + 1), dtype=t.int32, device=dev)
                P = t.empty((npairs, rows + 1, cols + 1), dtype=p_dtype or t.int32, device=dev)
        sc = _Scores(*scores)
        _check(lib().sw_batch_device_ex(self._h, d_a.data_ptr(), d_a.shape[1], cols, d_b.data_ptr(), d_b.shape[1], rows, npairs, ctypes.byref(sc),
                                        H.data_ptr() if H is not None else None, P.data_ptr() if P is not None else None,
                                        P.element_size() if P is not None else 4, res.data_ptr(), self._stream()))
        if traceback:
            assert P is not None, "the traceback walks P"
            cap = cols + rows + 2
            if want_paths and paths is None:
                paths = t.zeros((npairs, cap), dtype=t.int64, device=dev)
            _check(lib().sw_batch_traceback_device(self._h, P.data_ptr(), P.element_size(), cols, rows, npairs,
                                                   paths.data_ptr() if paths is not None else None, cap, res.data_ptr(), self._stream()))
        self.synchronize()
        if bool((res[:, 2] < 0).any().item()):
            raise SwError(-62, "in-kernel hand-off wait timed out")
        return (res, H, P, paths) if want_paths else (res, H, P)

    def search(self, query, targets, scores=DEFAULT_SCORES, top=None):
        """Database search (sw_search_device): one query against many targets of any length and alphabet.  targets: a list of
        sequences or a (packed uint8, int64 offsets) pair (read_fasta_db).  Returns the (ntargets, 3) int64 numpy array
        (max_pos, max_score, path_len = 0) in input order -- and, with top=K, also the K best target indices (score descending,
        then index ascending)."""
        t = self.torch
        q = _as_seq(query)
        packed, offs = _pack_targets(targets)
        ntargets = len(offs) - 1
        dev = f"cuda:{self.device}"
        d_q = t.from_numpy(q.copy()).to(dev)
        d_db = t.from_numpy(packed.copy() if len(packed) else np.zeros(1, np.uint8)).to(dev)
        res = self.search_device(d_q, len(q), d_db, offs, scores)
        self.synchronize()
        out = res.cpu().numpy()
        return (out, top_hits(out, top)) if top is not None else out

    def search_device(self, d_query, qlen: int, d_db, offsets, scores=DEFAULT_SCORES, out=None):
        """sw_search_device on device-resident query / packed targets (torch uint8 tensors), host int64 offsets; asynchronous on
        torch's current stream.  Returns the (ntargets, 3) int64 result tensor (`out` if given)."""
        t = self.torch
        offs = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        if len(offs) == 0:
            offs = np.zeros(1, np.int64)
        ntargets = len(offs) - 1
        res = out if out is not None else t.zeros((max(1, ntargets), 3), dtype=t.int64, device=f"cuda:{self.device}")
        sc = _Scores(*scores)
        _check(lib().sw_search_device(self._h, d_query.data_ptr(), qlen, d_db.data_ptr(), offs.ctypes.data, ntargets, ctypes.byref(sc),
                                      res.data_ptr(), self._stream()))
        return res[:ntargets]

    def search_affine(self, query, targets, submat, gap_open: int, gap_extend: int, top=None):
        """Database search with a substitution matrix and affine gaps (sw_search_affine_device).  submat: (256, 256) int8,
        s[query byte][target byte] (read_submat, submat_match, submat_from_letters); a gap of k letters scores gap_open + k * gap_extend.
        targets and the return value as for search()."""
        t = self.torch
        q = _as_seq(query)
        packed, offs = _pack_targets(targets)
        dev = f"cuda:{self.device}"
        d_q = t.from_numpy(q.copy()).to(dev)
        d_db = t.from_numpy(packed.copy() if len(packed) else np.zeros(1, np.uint8)).to(dev)
        res = self.search_affine_device(d_q, len(q), d_db, offs, submat, gap_open, gap_extend)
        self.synchronize()
        out = res.cpu().numpy()
        return (out, top_hits(out, top)) if top is not None else out

    def search_affine_device(self, d_query, qlen: int, d_db, offsets, submat, gap_open: int, gap_extend: int, out=None):
        """sw_search_affine_device on device-resident query / packed targets (torch uint8 tensors), host int64 offsets and a host
        (256, 256) int8 table; asynchronous on torch's current stream.  Returns the (ntargets, 3) int64 result tensor (`out` if given)."""
        t = self.torch
        offs = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        if len(offs) == 0:
            offs = np.zeros(1, np.int64)
        ntargets = len(offs) - 1
        res = out if out is not None else t.zeros((max(1, ntargets), 3), dtype=t.int64, device=f"cuda:{self.device}")
        sub, sc = _affine(submat, gap_open, gap_extend)
        _check(lib().sw_search_affine_device(self._h, d_query.data_ptr(), qlen, d_db.data_ptr(), offs.ctypes.data, ntargets, ctypes.byref(sc),
                                             res.data_ptr(), self._stream()))
        return res[:ntargets]

    def _top_out(self, nq: int, top: int, out):
        """The (hits, nhits) buffers of a selecting call: `out` checked, or fresh ones."""
        t = self.torch
        n = nq * max(0, int(top)) * 3
        if out is None:
            dev = f"cuda:{self.device}"
            return t.zeros(max(3, n), dtype=t.int64, device=dev), t.zeros(max(1, nq), dtype=t.int64, device=dev)
        hits, nhits = out
        for x, need, what in ((hits, n, "hits"), (nhits, nq, "nhits")):
            if x.dtype != t.int64 or not x.is_contiguous() or x.numel() < need:
                raise ValueError(f"out: {what} must be a contiguous int64 tensor of at least {need} elements")
        return hits, nhits

    @staticmethod
    def _top_views(hits, nhits, nq: int, top: int):
        k = max(0, int(top))
        return hits.view(-1)[:nq * k * 3].view(nq, k, 3), nhits.view(-1)[:nq]

    def top_hits_device(self, d_results, nqueries: int, ntargets: int, top: int, min_score: int = 0, out=None):
        """sw_top_hits_device: the best `top` targets of every row of a query-major (nqueries, ntargets, 3) int64 result tensor on the
        device (what Database.search_affine_device or search_affine_device returns); asynchronous on torch's current stream.  Every
        max_score must lie in 0 .. 2^24 - 1.  Returns torch (hits (nqueries, top, 3) of (target, max_pos, max_score), nhits (nqueries,));
        `out` as for Database.search_affine_top_device."""
        hits, nhits = self._top_out(int(nqueries), top, out)
        _check(lib().sw_top_hits_device(self._h, d_results.data_ptr(), int(nqueries), int(ntargets), int(top), int(min_score), hits.data_ptr(),
                                        nhits.data_ptr(), self._stream()))
        return self._top_views(hits, nhits, int(nqueries), top)

    def top_hits_pairs_device(self, d_pairs, d_results, npairs: int, nqueries: int, ntargets: int, top: int, min_score: int = 0, out=None):
        """sw_top_hits_pairs_device: the best `top` entries of every query of a scored pair list on the device -- d_pairs (npairs, 2) and
        d_results (npairs, 3) int64 tensors as Database.prefilter_ungapped_device and search_affine_pairs_device leave them, all cap
        rows: the (-1, -1) rows drop out.  Asynchronous on torch's current stream.  Returns torch (hits (nqueries, top, 3) of (target,
        max_pos, max_score), nhits (nqueries,)); `out` as for Database.search_affine_top_device."""
        hits, nhits = self._top_out(int(nqueries), top, out)
        _check(lib().sw_top_hits_pairs_device(self._h, d_pairs.data_ptr() if npairs else None, d_results.data_ptr() if npairs else None, int(npairs),
                                              int(nqueries), int(ntargets), int(top), int(min_score), hits.data_ptr(), nhits.data_ptr(), self._stream()))
        return self._top_views(hits, nhits, int(nqueries), top)

    def _hist_out(self, nq: int, hist):
        """The histogram buffer of a statistics call: `hist` checked, or a fresh one (int32: the uint32 counters' bits)."""
        t = self.torch
        n = nq * HIST_CLASSES * HIST_BINS
        if hist is None:
            return t.empty(max(1, n), dtype=t.int32, device=f"cuda:{self.device}")
        if hist.dtype != t.int32 or not hist.is_contiguous() or hist.numel() < n:
            raise ValueError(f"hist must be a contiguous int32 tensor of at least {n} elements")
        return hist

    def score_hist(self, database, results, shift: int = 0):
        """The score histogram of a host result table on the device (sw_score_hist_device): results the (nqueries, ntargets, 3) int64
        table of a search of `database` (a Database; its offsets give the lengths).  Returns (nqueries, 40, 256) uint32, the bytes of
        score_hist_host."""
        t = self.torch
        res = np.ascontiguousarray(results, np.int64)
        if res.ndim != 3 or res.shape[1] != database.ntargets or res.shape[2] != 3:
            raise ValueError(f"results must be (nqueries, {database.ntargets}, 3) int64")
        d_res = t.from_numpy(res.reshape(-1).copy() if res.size else np.zeros(3, np.int64)).to(f"cuda:{self.device}")
        hist = self.score_hist_device(database, d_res, res.shape[0], shift)
        self.synchronize()
        return hist.cpu().numpy().view(np.uint32)

    def score_hist_device(self, database, d_results, nqueries: int, shift: int = 0, hist=None):
        """sw_score_hist_device on a device-resident query-major result table (int64, nqueries x ntargets x 3, what
        Database.search_affine_device returns); asynchronous on torch's current stream.  Every counter is written.  Returns the
        (nqueries, 40, 256) int32 tensor of the uint32 counters' bits, a view of `hist` if given (see _hist_out)."""
        t = self.torch
        nq = int(nqueries)
        need = max(0, nq) * database.ntargets * 3
        if d_results is not None and (d_results.dtype != t.int64 or not d_results.is_contiguous() or d_results.numel() < need):
            raise ValueError(f"d_results must be a contiguous int64 tensor of at least {need} elements")
        hist = self._hist_out(max(0, nq), hist)
        _check(lib().sw_score_hist_device(self._h, database._h, d_results.data_ptr() if d_results is not None else None, nq, int(shift),
                                          hist.data_ptr(), self._stream()))
        return hist.view(-1)[:max(0, nq) * HIST_CLASSES * HIST_BINS].view(max(0, nq), HIST_CLASSES, HIST_BINS)

    def msa_filter(self, cols, queries_or_qoffsets, top: int, max_ident_pct: int, min_cover_pct: int, hits=None):
        """The filter of a hit alignment (sw_msa_filter_device): which rows of the column rows of Database.msa_from_hits are kept --
        covered to min_cover_pct percent, less than max_ident_pct percent identical to the query and to every kept row of better rank
        (include/swhip.h states the rule).  cols: the uint8 column rows; queries_or_qoffsets: the sequences as for search_affine, or
        the 1-D int64 column offsets (no letters: no row is compared with the query); hits: the (nqueries, top, 3) hit table, or
        None.  Returns numpy (keep (nqueries, top) int32, nkept (nqueries,) int64, the hit table with target = -1 in the dropped
        entries or None)."""
        t = self.torch
        dev = f"cuda:{self.device}"
        c, qpacked, qoffs, nq, top, hits = _msa_filter_args(cols, queries_or_qoffsets, top, hits)
        d_cols = t.from_numpy(c.copy() if len(c) else np.zeros(1, np.uint8)).to(dev)
        d_q = t.from_numpy(qpacked.copy()).to(dev) if qpacked is not None and len(qpacked) else None
        d_hits = t.from_numpy(hits.reshape(-1).copy()).to(dev) if hits is not None and hits.size else None
        keep, nkept, out = self.msa_filter_device(d_cols, d_q, qoffs, top, (max_ident_pct, min_cover_pct), hits=d_hits, hits_out=d_hits)
        self.synchronize()
        return (keep.cpu().numpy()[:nq * top].reshape(nq, top), nkept.cpu().numpy()[:nq],
                out.cpu().numpy()[:nq * top * 3].reshape(nq, top, 3) if out is not None else None)

    def msa_filter_device(self, d_cols, d_queries, qoffsets, top: int, filter, hits=None, hits_out=None, keep=None, nkept=None):
        """sw_msa_filter_device on device-resident column rows (the uint8 tensor Database.msa_from_hits_device fills) and query letters
        (a uint8 tensor, query q at qoffsets[q]; None: no row is compared with the query); asynchronous on torch's current stream,
        nothing comes to the host.  filter: (max_ident_pct, min_cover_pct).  hits: the int64 hit table of nqueries x top x 3 elements,
        hits_out: the tensor that receives it with target = -1 in the dropped entries -- `hits` itself for in place, None for none.
        keep: the int32 tensor of at least nqueries x top elements that receives 1 / 0 per entry, None for a fresh one, False for none;
        nkept: the int64 tensor of at least nqueries elements that receives the rows kept, None for a fresh one, False for none.
        Returns (keep, nkept, hits_out), None where there is none."""
        t = self.torch
        dev = f"cuda:{self.device}"
        qoffs = np.ascontiguousarray(qoffsets, np.int64).reshape(-1)
        if len(qoffs) == 0:
            qoffs = np.zeros(1, np.int64)
        nq, top = len(qoffs) - 1, int(top)
        n = nq * max(0, top)
        ncols = int(qoffs[-1] - qoffs[0]) * max(0, top)
        if d_cols is not None and (d_cols.dtype != t.uint8 or not d_cols.is_contiguous() or d_cols.numel() < ncols):
            raise ValueError(f"d_cols must be a contiguous uint8 tensor of at least {ncols} elements")
        if d_queries is not None and (d_queries.dtype != t.uint8 or not d_queries.is_contiguous() or d_queries.numel() < int(qoffs[-1])):
            raise ValueError(f"d_queries must be a contiguous uint8 tensor of at least {int(qoffs[-1])} elements")
        for x, what in ((hits, "hits"), (hits_out, "hits_out")):
            if x is not None and (x.dtype != t.int64 or not x.is_contiguous() or x.numel() < n * 3):
                raise ValueError(f"{what} must be a contiguous int64 tensor of at least {nq} x {top} x 3 elements")
        if keep is None:
            keep = t.empty(max(1, n), dtype=t.int32, device=dev)
        elif keep is False:
            keep = None
        if keep is not None and (keep.dtype != t.int32 or not keep.is_contiguous() or keep.numel() < n):
            raise ValueError(f"keep must be a contiguous int32 tensor of at least {n} elements")
        if nkept is None:
            nkept = t.empty(max(1, nq), dtype=t.int64, device=dev)
        elif nkept is False:
            nkept = None
        if nkept is not None and (nkept.dtype != t.int64 or not nkept.is_contiguous() or nkept.numel() < nq):
            raise ValueError(f"nkept must be a contiguous int64 tensor of at least {nq} elements")
        f = _msa_filter(filter)
        _check(lib().sw_msa_filter_device(self._h, d_cols.data_ptr() if d_cols is not None else None,
                                          d_queries.data_ptr() if d_queries is not None else None, qoffs.ctypes.data, nq, top, ctypes.byref(f),
                                          hits.data_ptr() if hits is not None else None, hits_out.data_ptr() if hits_out is not None else None,
                                          keep.data_ptr() if keep is not None else None, nkept.data_ptr() if nkept is not None else None,
                                          self._stream()))
        return keep, nkept, hits_out

    def prepare_db(self, db, offsets=None) -> Database:
        """A prepared database (sw_db_create) for Database.search_affine.  db: a list of sequences, a (packed, offsets) pair, or --
        with `offsets` given -- a torch uint8 device tensor of the targets back to back, which the handle keeps alive and which must
        not change while the handle lives.  Use as a context manager or close() it."""
        t = self.torch
        if offsets is None:
            packed, offsets = _pack_targets(db)
            db = t.from_numpy(packed.copy() if len(packed) else np.zeros(1, np.uint8)).to(f"cuda:{self.device}")
        elif not isinstance(db, t.Tensor):
            packed = np.ascontiguousarray(db, np.uint8).reshape(-1)
            db = t.from_numpy(packed.copy() if len(packed) else np.zeros(1, np.uint8)).to(f"cuda:{self.device}")
        return Database(self, db, offsets)

    def align_affine(self, query, targets, submat, gap_open: int, gap_extend: int, hits, checkpoint=None):
        """The alignments of the targets `hits` (indices, any order, duplicates allowed) under affine scoring
        (sw_align_affine_device): every hit is re-filled with direction bytes and walked by the canonical rule of include/swhip.h.
        Returns (aln, ops): aln an (nhits, 7) int64 numpy array (max_pos, max_score, q_begin, t_begin, q_end, t_end, nops), ops a
        list of bytes over b"MID" in alignment order.  checkpoint: the option "align_checkpoint" for this call alone (0 whole direction
        matrices, 1 checkpointed, 2 checkpointed where 0 would refuse the call for size)."""
        t = self.torch
        q = _as_seq(query)
        packed, offs = _pack_targets(targets)
        dev = f"cuda:{self.device}"
        d_q = t.from_numpy(q.copy()).to(dev)
        d_db = t.from_numpy(packed.copy() if len(packed) else np.zeros(1, np.uint8)).to(dev)
        hits, cap = _hits_and_cap(offs, hits, len(q))
        aln, ops = self.align_affine_device(d_q, len(q), d_db, offs, submat, gap_open, gap_extend, hits, ops_cap=cap, checkpoint=checkpoint)
        self.synchronize()
        aln = aln.cpu().numpy()
        return aln, _ops_list(aln, ops.cpu().numpy(), cap)

    def align_affine_device(self, d_query, qlen: int, d_db, offsets, submat, gap_open: int, gap_extend: int, hits, ops_cap: int = 0, out=None,
                            checkpoint=None):
        """sw_align_affine_device on device-resident query / packed targets (torch uint8 tensors), host int64 offsets, host hits and
        a host table; asynchronous on torch's current stream.  Returns (aln, ops): the (nhits, 7) int64 tensor and the
        (nhits, ops_cap) uint8 tensor (None with ops_cap = 0: coordinates only); out = (aln, ops) reuses given tensors.
        checkpoint: the option "align_checkpoint" for this call alone."""
        t = self.torch
        offs = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        if len(offs) == 0:
            offs = np.zeros(1, np.int64)
        hits = np.ascontiguousarray(hits, np.int64).reshape(-1)
        nhits, dev = len(hits), f"cuda:{self.device}"
        aln, ops = out if out is not None else (t.zeros((max(1, nhits), 7), dtype=t.int64, device=dev),
                                                t.zeros((max(1, nhits), ops_cap), dtype=t.uint8, device=dev) if ops_cap > 0 else None)
        sub, sc = _affine(submat, gap_open, gap_extend)
        with self._checkpoint(checkpoint):
            _check(lib().sw_align_affine_device(self._h, d_query.data_ptr(), qlen, d_db.data_ptr(), offs.ctypes.data, len(offs) - 1, hits.ctypes.data, nhits,
                                                ctypes.byref(sc), aln.data_ptr(), ops.data_ptr() if ops is not None else None, ops_cap, self._stream()))
        return aln[:nhits], (ops[:nhits] if ops is not None else None)

    def traceback(self, out: Fill, max_pos: int | None = None, want_path: bool = True):
        """backtrack() on the device P (negates the path in place). Returns the path indices."""
        t = self.torch
        if max_pos is None:
            max_pos = out.result()["max_pos"]
        cap = out.cols + out.rows + 2
        path = t.zeros(cap if want_path else 1, dtype=t.int64, device=out.P.device)
        _check(lib().sw_traceback_device_ex(self._h, out.P.data_ptr(), out.P.element_size(), out.cols, out.rows, int(max_pos),
                                            path.data_ptr() if want_path else None, cap, out.res.data_ptr(), self._stream()))
        self.synchronize()
        n = int(out.res[2].item())
        return path[:n].cpu().numpy() if want_path else n

    def row_checksums(self, X):
        t = self.torch
        cs = t.zeros(X.shape[0], dtype=t.int64, device=X.device)
        _check(lib().sw_row_checksums_device(self._h, X.data_ptr(), X.element_size(), X.shape[0], X.shape[1],
                                             cs.data_ptr(), self._stream()))
        self.synchronize()
        return cs.cpu().numpy().view(np.uint64)

    def widen_p(self, P8):
        """int8 predecessor matrix -> the reference's int32 layout (sw_p8_to_p32_device)."""
        t = self.torch
        out = t.empty(P8.shape, dtype=t.int32, device=P8.device)
        _check(lib().sw_p8_to_p32_device(self._h, P8.data_ptr(), out.data_ptr(), P8.numel(), self._stream()))
        return out

    def pack_p2(self, P, want_bits: bool = True):
        """int8 / int32 predecessor matrix -> the 2-bit format (sw_p_to_p2_device): (P2 uint8 tensor with 4 cells per byte, path bitmap
        int32 tensor with 1 bit per cell -- set where P was negative, i.e. on a traced path -- or None)."""
        t = self.torch
        n = P.numel()
        P2 = t.empty(((n + 31) // 32) * 8, dtype=t.uint8, device=P.device)
        bits = t.empty((n + 31) // 32, dtype=t.int32, device=P.device) if want_bits else None
        _check(lib().sw_p_to_p2_device(self._h, P.data_ptr(), P.element_size(), P2.data_ptr(), bits.data_ptr() if want_bits else None, n, self._stream()))
        return P2, bits

    def unpack_p2(self, P2, bits, shape):
        """2-bit matrix (+ optional path bitmap) -> the reference's int32 layout (sw_p2_to_p32_device)."""
        t = self.torch
        out = t.empty(shape, dtype=t.int32, device=P2.device)
        _check(lib().sw_p2_to_p32_device(self._h, P2.data_ptr(), bits.data_ptr() if bits is not None else None, out.data_ptr(), out.numel(), self._stream()))
        return out

    def traceback_p2(self, P2, cols: int, rows: int, max_pos: int, bits=None, want_path: bool = True):
        """backtrack() on a 2-bit matrix: the path is marked in `bits` (zeroed by the caller) instead of negating P.  Returns the path
        indices (or the length)."""
        t = self.torch
        cap = cols + rows + 2
        path = t.zeros(cap if want_path else 1, dtype=t.int64, device=P2.device)
        res = t.zeros(3, dtype=t.int64, device=P2.device)
        _check(lib().sw_traceback_p2_device(self._h, P2.data_ptr(), cols, rows, int(max_pos), bits.data_ptr() if bits is not None else None,
                                            path.data_ptr() if want_path else None, cap, res.data_ptr(), self._stream()))
        self.synchronize()
        n = int(res[2].item())
        return path[:n].cpu().numpy() if want_path else n

    def synchronize(self):
        _check(lib().sw_synchronize(self._h, self._stream()))


def smith_waterman(a, b, scores=DEFAULT_SCORES, device: int = 0, backtrack: bool = True):
    """Whole-pipeline convenience with host arrays, shaped like the reference's program:
    returns dict(H, P, max_pos, max_score, path) with P negated along the path when backtrack."""
    eng = Engine(device)
    try:
        out = eng.fill(a, b, scores)
        r = out.result()
        path = eng.traceback(out, r["max_pos"]) if backtrack else np.zeros(0, np.int64)
        return {"H": out.H.cpu().numpy(), "P": out.P.cpu().numpy(), "max_pos": r["max_pos"],
                "max_score": r["max_score"], "path": path}
    finally:
        eng.close()


class MultiFill:
    """One matrix over several GPUs of this process (sw_multi_*): row bands, band-resident launches, peer-copied halos.
    devices may repeat an id (bands then share that GPU)."""

    def __init__(self, devices, a, b, p_dtype="int32", want_h=True):
        self.a, self.b = _as_seq(a).copy(), _as_seq(b).copy()
        self.cols, self.rows = len(self.a), len(self.b)
        self.pbytes = 1 if str(p_dtype).endswith("int8") else 4
        dv = (_i32 * len(devices))(*devices)
        h = _vp()
        _check(lib().sw_multi_create(dv, len(devices), self.a.ctypes.data, self.cols, self.b.ctypes.data, self.rows, self.pbytes, 1 if want_h else 0,
                                     ctypes.byref(h)))
        self._h = h
        self.want_h = want_h

    def fill(self, scores=DEFAULT_SCORES, nchunks=64):
        sc, r = _Scores(*scores), _Result()
        _check(lib().sw_multi_fill(self._h, ctypes.byref(sc), nchunks, ctypes.byref(r)))
        return {"max_pos": r.max_pos, "max_score": r.max_score, "seconds": lib().sw_multi_seconds(self._h)}

    def traceback(self):
        n = _i64()
        _check(lib().sw_multi_traceback(self._h, ctypes.byref(n)))
        return n.value

    def bands(self):
        """[(device, lo, hi, H (numpy or None), P (numpy int32))] copied to the host."""
        out = []
        for g in range(lib().sw_multi_nbands(self._h)):
            dev, lo, hi, dH, dP = _i32(), _i64(), _i64(), _vp(), _vp()
            _check(lib().sw_multi_band_info(self._h, g, ctypes.byref(dev), ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(dH), ctypes.byref(dP)))
            shape = (hi.value - lo.value + 1, self.cols + 1)
            import torch
            with torch.cuda.device(dev.value):
                H = None
                if self.want_h:
                    H = np.zeros(shape, np.int32)
                    torch.cuda.synchronize()
                    _hip_d2h(H, dH.value)
                P = np.zeros(shape, np.int8 if self.pbytes == 1 else np.int32)
                _hip_d2h(P, dP.value)
            out.append((dev.value, lo.value, hi.value, H, P.astype(np.int32)))
        return out

    def band_tensors(self):
        """[(device, lo, hi, H, P)] as torch tensors that alias the band-local device matrices (no copy; H None when not kept).
        Row 0 of a band is its halo row (= row lo of the whole matrix)."""
        import torch
        out = []
        for g in range(lib().sw_multi_nbands(self._h)):
            dev, lo, hi, dH, dP = _i32(), _i64(), _i64(), _vp(), _vp()
            _check(lib().sw_multi_band_info(self._h, g, ctypes.byref(dev), ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(dH), ctypes.byref(dP)))
            shape = (hi.value - lo.value + 1, self.cols + 1)
            H = torch.as_tensor(_RawDevice(dH.value, shape, "<i4", self), device=f"cuda:{dev.value}") if self.want_h else None
            P = torch.as_tensor(_RawDevice(dP.value, shape, "|i1" if self.pbytes == 1 else "<i4", self), device=f"cuda:{dev.value}")
            out.append((dev.value, lo.value, hi.value, H, P))
        return out

    def close(self):
        if getattr(self, "_h", None):
            lib().sw_multi_free(self._h)
            self._h = None

    __del__ = close


def _hip_d2h(arr: np.ndarray, dptr: int):
    import torch
    n = arr.nbytes
    t = torch.as_tensor(_RawDevice(dptr, (n,), "|u1", None), device="cuda")
    arr.view(np.uint8).reshape(-1)[:] = t.cpu().numpy()


def fill_host(engine: "Engine", a, b, scores=DEFAULT_SCORES):
    """sw_fill_host: the drop-in for the reference's fill loop on HOST buffers -- what `main` owns after its two
    callocs (serial_smithW.c:96-103) goes in, H, P and maxPos come back in the reference's layout.  Returns dict with H, P, max_pos, max_score."""
    a, b = _as_seq(a).copy(), _as_seq(b).copy()
    cols, rows = len(a), len(b)
    H = np.zeros((rows + 1, cols + 1), np.int32)
    P = np.zeros((rows + 1, cols + 1), np.int32)
    sc, r = _Scores(*scores), _Result()
    _check(lib().sw_fill_host(engine._h, a.ctypes.data, cols, b.ctypes.data, rows, ctypes.byref(sc), H.ctypes.data, P.ctypes.data, ctypes.byref(r)))
    return {"H": H, "P": P, "max_pos": r.max_pos, "max_score": r.max_score}


def align_auto(a, b, scores=DEFAULT_SCORES, engine: "Engine | None" = None, devices=None, multi_min_cells: int = 0):
    """sw_align_auto: host fill for tiny problems, the GPU of `engine` otherwise; host traceback.  With `devices` (a list of GPU ids,
    ids may repeat) sw_align_auto_multi: host / one GPU / row bands over all of them, chosen by size.  Returns dict like
    smith_waterman() plus used_gpu and executor (0 host, 1 one GPU, 2 several)."""
    a, b = _as_seq(a).copy(), _as_seq(b).copy()
    cols, rows = len(a), len(b)
    H = np.zeros((rows + 1, cols + 1), np.int32)
    P = np.zeros((rows + 1, cols + 1), np.int32)
    sc, r, used = _Scores(*scores), _Result(), _i32()
    h = engine._h if engine is not None else None
    if devices is None:
        _check(lib().sw_align_auto(h, a.ctypes.data, cols, b.ctypes.data, rows, ctypes.byref(sc), H.ctypes.data, P.ctypes.data, ctypes.byref(r),
                                   ctypes.byref(used)))
        ex = 1 if used.value else 0
    else:
        dv = (_i32 * max(1, len(devices)))(*devices)
        _check(lib().sw_align_auto_multi(h, dv, len(devices), a.ctypes.data, cols, b.ctypes.data, rows, ctypes.byref(sc), H.ctypes.data, P.ctypes.data,
                                         ctypes.byref(r), ctypes.byref(used), multi_min_cells))
        ex = used.value
    return {"H": H, "P": P, "max_pos": r.max_pos, "max_score": r.max_score, "path_len": r.path_len, "used_gpu": ex > 0, "executor": ex}
