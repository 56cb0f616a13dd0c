"""ctypes binding of the C ABI (include/consent_amd.h) + the host-side mirror of CONSENT's operator.

Mirrors ``computeConsensusReadCorrection`` / ``computeConsensusAssemblyPolishing``
(reference src/correctionMSA.h:8,10): same argument names and meaning, batched over windows.
"""
import ctypes as C
import os

import numpy as np

WIN_CONSENSUS, WIN_TEMPLATE, WIN_OVERFLOW = 0, 1, 2
# cw_sw_run (include/consent_amd.h): a row's status, its columns, the flag, the capacities
SW_ALIGNED, SW_NO_INDELS, SW_STOP, SW_IS_REF = 0, 1, 2, 3
SW_SCORE, SW_REF_BEGIN, SW_REF_END, SW_QUERY_BEGIN, SW_QUERY_END, SW_INS, SW_DEL, SW_STATUS, SW_ROW = 0, 1, 2, 3, 4, 5, 6, 7, 8
SW_WANT_INDELS = 1
SW_QMAX, SW_RMAX, SW_DIR_BYTES = 32768, 16383, 1 << 20
# cw_sw_path_run: the statuses only it writes, its flag, the op codes, the per-wave traceback scratch
SW_NO_PATH, SW_PATH_OPEN, SW_PATH_SLOT = 4, 5, 6
SW_PATH_EQX = 4
SW_OP_M, SW_OP_I, SW_OP_D, SW_OP_EQ, SW_OP_X = 0, 1, 2, 7, 8
SW_PATH_BYTES = 2 << 20
SW_OP_LETTERS = {SW_OP_M: "M", SW_OP_I: "I", SW_OP_D: "D", SW_OP_EQ: "=", SW_OP_X: "X"}
# cw_pileup_run: the status only it writes, its flag, the words of a column
SW_PILE_SLOT = 7
PILE_ACCUMULATE = 8
PILE_A, PILE_C, PILE_G, PILE_T, PILE_DEL, PILE_INS, PILE_BEGIN, PILE_END, PILE_COL = 0, 1, 2, 3, 4, 5, 6, 7, 8
# cw_sw_cut_run: the status only it writes
SW_CUT_SLOT = 8
# cw_strand_run: a sequence's strand value, the default k and its range
STRAND_FWD, STRAND_REV, STRAND_IS_REF, STRAND_NONE = 0, 1, 2, 3
STRAND_K, STRAND_KMIN, STRAND_KMAX = 11, 8, 15
# cw_seed_run: a row's columns, the bin shift, the diagonals of a window; Engine.place's default threshold (its docstring has the measurement)
SEED_STATUS, SEED_HITS, SEED_DIAG, SEED_OTHER, SEED_ROW = 0, 1, 2, 3, 4
SEED_SHIFT = 6
SEED_SPAN = 2 << SEED_SHIFT
SEED_MIN_HITS, SEED_MIN_K = 14, 11  # (the threshold holds from this k up)
# cw_locate_*: the default k, the longest reference; Engine.locate's default threshold and the k it is measured for (its docstring has the measurement)
LOCATE_K, LOCATE_RMAX = 15, (1 << 28) - 1
LOCATE_MIN_HITS, LOCATE_MIN_K = 4, 15
# cw_overlap_*: the defaults of cw_overlap_params, the row and the statuses; Engine.overlaps' default threshold and the k it is measured for, the shortest planted
# overlap it finds without exception and how far an end lies from the truth (tests/test_overlap_cpu.py measures all three)
OVL_K, OVL_SAMPLE, OVL_MAX_OCC = 15, 3, 512
OVL_TARGET, OVL_STRAND, OVL_HITS, OVL_DIAG, OVL_Q_START, OVL_Q_END, OVL_T_START, OVL_T_END, OVL_ROW = 0, 1, 2, 3, 4, 5, 6, 7, 8
OVL_OK, OVL_NONE, OVL_SLOT, OVL_DENSE, OVL_BAD_INDEX = 0, 1, 2, 3, 4
OVL_MIN_HITS, OVL_MIN_K, OVL_MIN_OVERLAP, OVL_END_SLACK = 2, 15, 2000, 143
# cw_seed_spans: a placed query's span is its window's diagonals over the whole query, widened by SPAN_PAD + (query length >> SPAN_PAD_SHIFT) on either side;
# the shift is measured (tests/test_sw_span_cpu.py)
SPAN_PAD, SPAN_PAD_SHIFT = 64, 4
_HERE = os.path.dirname(os.path.abspath(__file__))


def sw_ops_bound(query_len, ref_len):
    """CW_SW_OPS_BOUND: a slot of this many ops holds any path of the pair."""
    return query_len + ref_len


def sw_cuts(ref_len, window):
    """CW_SW_CUTS: the words of a query's slot -- the windows of its reference + 1 (numpy-friendly)."""
    ref_len = np.asarray(ref_len, np.int64)
    return ref_len // window + (ref_len % window != 0) + 1


class EngineError(RuntimeError):
    pass


class Params(C.Structure):
    """cw_params: merSize, solidThresh, commonKMers, minAnchors, maxMSA (reference main.cpp:17-26 names)."""

    _fields_ = [("k", C.c_uint32), ("solid", C.c_uint32), ("common_kmers", C.c_uint32), ("min_anchors", C.c_uint32), ("max_msa", C.c_uint32)]


class Batch(C.Structure):
    _fields_ = [
        ("n_windows", C.c_uint32),
        ("n_seqs", C.c_uint32),
        ("n_words", C.c_uint64),
        ("win_first_seq", C.c_void_p),
        ("seq_len", C.c_void_p),
        ("seq_word_off", C.c_void_p),
        ("bases", C.c_void_p),
    ]


class SwPaths(C.Structure):
    """cw_sw_paths: the op slots of cw_sw_path_run."""

    _fields_ = [("ops", C.c_void_p), ("ops_off", C.c_void_p), ("n_ops", C.c_void_p)]


class Pileup(C.Structure):
    """cw_pileup: the column slots of cw_pileup_run."""

    _fields_ = [("counts", C.c_void_p), ("col_off", C.c_void_p)]


class SwCuts(C.Structure):
    """cw_sw_cuts: the cut-point slots of cw_sw_cut_run and the window size."""

    _fields_ = [("cuts", C.c_void_p), ("cut_off", C.c_void_p), ("window", C.c_uint32)]


class Strands(C.Structure):
    """cw_strands: the outputs of cw_strand_run (hits may be NULL) and k (0 = STRAND_K)."""

    _fields_ = [("strand", C.c_void_p), ("hits", C.c_void_p), ("k", C.c_uint32)]


class Seeds(C.Structure):
    """cw_seeds: the outputs of cw_seed_run (strand may be NULL) and k (0 = STRAND_K)."""

    _fields_ = [("rows", C.c_void_p), ("strand", C.c_void_p), ("k", C.c_uint32)]


class LocateRef(C.Structure):
    """cw_locate_ref: the packed reference, its length, the caller's table of cw_locate_table_words(len) words, and k (0 = LOCATE_K)."""

    _fields_ = [("bases", C.c_void_p), ("len", C.c_uint64), ("table", C.c_void_p), ("k", C.c_uint32)]


class OverlapParams(C.Structure):
    """cw_overlap_params: k (0 = OVL_K), sample (0 .. 8), max_occ (0 = OVL_MAX_OCC), min_hits (>= 1)."""

    _fields_ = [("k", C.c_uint32), ("sample", C.c_uint32), ("max_occ", C.c_uint32), ("min_hits", C.c_uint32)]


class OverlapIndexRef(C.Structure):
    """cw_overlap_index: the caller's device memory of cw_overlap_index_words(n_entries) words, the counted entries, the parameters."""

    _fields_ = [("mem", C.c_void_p), ("n_entries", C.c_uint64), ("prm", OverlapParams)]


class Overlaps(C.Structure):
    """cw_overlaps: rows, row_off[n_queries + 1] in rows, n_rows[n_queries], status[n_queries]."""

    _fields_ = [("rows", C.c_void_p), ("row_off", C.c_void_p), ("n_rows", C.c_void_p), ("status", C.c_void_p)]


class SwSpans(C.Structure):
    """cw_sw_spans: per sequence the reference columns [ref_lo, ref_hi) a query may use (the span runs)."""

    _fields_ = [("ref_lo", C.c_void_p), ("ref_hi", C.c_void_p)]


class Result(C.Structure):
    _fields_ = [
        ("cons", C.c_void_p),
        ("cons_off", C.c_void_p),
        ("cons_len", C.c_void_p),
        ("win_status", C.c_void_p),
        ("solid", C.c_void_p),
        ("solid_off", C.c_void_p),
        ("solid_len", C.c_void_p),
    ]


class ReadSet(C.Structure):
    _fields_ = [("n_reads", C.c_uint32), ("read_len", C.c_void_p), ("read_word_off", C.c_void_p), ("bases", C.c_void_p)]


class SynthSpec(C.Structure):
    _fields_ = [
        ("seed", C.c_uint64),
        ("first_window", C.c_uint64),
        ("n_windows", C.c_uint32),
        ("depth", C.c_uint32),
        ("window_len", C.c_uint32),
        ("err_permille", C.c_uint32),
        ("sub_w", C.c_uint32),
        ("ins_w", C.c_uint32),
        ("del_w", C.c_uint32),
        ("seq_stride_words", C.c_uint32),
    ]

    @classmethod
    def pacbio(cls, n_windows, depth, first_window=0, seed=0xC0115E17, window_len=500):
        return cls(seed, first_window, n_windows, depth, window_len, 120, 10, 60, 30, (window_len + 60) // 16 + 2)

    @classmethod
    def ont(cls, n_windows, depth, first_window=0, seed=0xC0115E17, window_len=500):
        return cls(seed, first_window, n_windows, depth, window_len, 120, 30, 30, 40, (window_len + 60) // 16 + 2)


TIER_LISTS = {"Q": 0, "M1": 1, "M2": 2, "L": 3, "H": 5}  # the routed lists by index (csrc/cw_chain.h ch_list_id); tier S has none: it walks the task array
LIST_CLS_SHIFT, LIST_IDX_MASK = 24, 0x00FFFFFF      # an emitted entry: task index | sort class << 24 (csrc/cw_poa.h cw_list_entry)


def lib_path():
    """The in-tree library; CONSENT_AMD_LIB names another build of the same sources (tests/test_gpu_policy.py: a non-default policy)."""
    return os.environ.get("CONSENT_AMD_LIB") or os.path.join(_HERE, "libconsent_amd.so")


_LIB = None
_LIBS = {}  # path -> loaded library
AIDS_LIB = os.path.join(_HERE, "aids", "libconsent_amd.so")  # the -DCW_TEST_AIDS build of the same sources (csrc/cw_env.h): tests and tools only


def use_library(path=None):
    """Make `path` (None: the default, lib_path()) the library every later Engine / helper of this process uses; returns the previous choice.
    What the tests that need a test aid do for their duration (tests/conftest.py `aids`): both builds can be loaded side by side."""
    global _LIB
    prev = _LIB
    _LIB = None
    if path is not None:
        _LIB = _load(path)
    return prev


def load_library():
    """Load libconsent_amd.so.  Fails loudly: there is no fallback implementation."""
    global _LIB
    if _LIB is not None:
        return _LIB
    _LIB = _load(lib_path())
    return _LIB


def _load(p):
    if p in _LIBS:
        return _LIBS[p]
    try:  # PyTorch-ROCm ships its own HIP runtime: let it initialise first so both sides share one runtime and one context
        import torch

        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        pass
    if not os.path.exists(p):
        raise EngineError(f"{p} is missing: build it with `python -m consent_amd._build` (hipcc --offload-arch=gfx950)")
    lib = C.CDLL(p)
    lib.cw_version.restype = C.c_char_p
    lib.cw_strerror.restype = C.c_char_p
    lib.cw_strerror.argtypes = [C.c_int]
    lib.cw_create.argtypes = [C.POINTER(Params), C.c_int, C.POINTER(C.c_void_p)]
    lib.cw_destroy.argtypes = [C.c_void_p]
    lib.cw_destroy.restype = None
    lib.cw_run.argtypes = [C.c_void_p, C.POINTER(Batch), C.POINTER(Result)]
    lib.cw_run_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.POINTER(Result), C.c_void_p]
    if hasattr(lib, "cw_poa_run"):  # (a library built before the POA operator has no such entries)
        lib.cw_poa_run.argtypes = [C.c_void_p, C.POINTER(Batch), C.POINTER(Result)]
        lib.cw_poa_run_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.POINTER(Result), C.c_void_p]
        lib.cw_debug_poa_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_void_p]
    if hasattr(lib, "cw_sw_run"):  # (a library built before the alignment operator has no such entries)
        lib.cw_sw_run.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_uint32]
        lib.cw_sw_run_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_uint32, C.c_void_p]
        lib.cw_debug_sw_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_uint32, C.c_void_p]
    if hasattr(lib, "cw_sw_path_run"):
        lib.cw_sw_path_run.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.POINTER(SwPaths), C.c_uint32]
        lib.cw_sw_path_run_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.POINTER(SwPaths), C.c_uint32, C.c_void_p]
        lib.cw_debug_sw_path_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_uint32, C.c_void_p]
    if hasattr(lib, "cw_pileup_run"):
        lib.cw_pileup_run.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.POINTER(Pileup), C.c_uint32]
        lib.cw_pileup_run_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.POINTER(Pileup), C.c_uint32, C.c_void_p]
    if hasattr(lib, "cw_sw_cut_run"):
        lib.cw_sw_cut_run.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.POINTER(SwCuts)]
        lib.cw_sw_cut_run_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.POINTER(SwCuts), C.c_void_p]
        lib.cw_cut_groups_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.POINTER(SwCuts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_void_p]
    if hasattr(lib, "cw_strand_run"):
        lib.cw_strand_run.argtypes = [C.c_void_p, C.POINTER(Batch), C.POINTER(Strands)]
        lib.cw_strand_run_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.POINTER(Strands), C.c_void_p]
        lib.cw_revcomp.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p]
        lib.cw_revcomp_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p, C.c_void_p]
        lib.cw_debug_strand_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
    if hasattr(lib, "cw_seed_run"):
        lib.cw_seed_run.argtypes = [C.c_void_p, C.POINTER(Batch), C.POINTER(Seeds)]
        lib.cw_seed_run_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.POINTER(Seeds), C.c_void_p]
        lib.cw_debug_seed_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
    if hasattr(lib, "cw_locate_run"):
        lib.cw_locate_table_words.argtypes = [C.c_uint64]
        lib.cw_locate_table_words.restype = C.c_uint64
        lib.cw_locate_build_device.argtypes = [C.c_void_p, C.POINTER(LocateRef), C.c_void_p]
        lib.cw_locate_run_device.argtypes = [C.c_void_p, C.POINTER(LocateRef), C.POINTER(Batch), C.POINTER(Seeds), C.c_void_p]
        lib.cw_locate_run.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(Batch), C.POINTER(Seeds)]
        lib.cw_debug_locate_plan.argtypes = [C.c_uint32, C.c_int, C.c_void_p]
        lib.cw_debug_locate_routes.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(lib, "cw_overlap_run"):
        lib.cw_overlap_index_words.argtypes = [C.c_uint64]
        lib.cw_overlap_index_words.restype = C.c_uint64
        lib.cw_overlap_count_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.POINTER(OverlapParams), C.POINTER(C.c_uint64), C.c_void_p]
        lib.cw_overlap_build_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.POINTER(OverlapIndexRef), C.c_void_p]
        lib.cw_overlap_run_device.argtypes = [C.c_void_p, C.POINTER(OverlapIndexRef), C.POINTER(Batch), C.c_uint32, C.c_uint32, C.POINTER(Overlaps), C.c_void_p]
        lib.cw_overlap_run.argtypes = [C.c_void_p, C.POINTER(Batch), C.POINTER(OverlapParams), C.POINTER(Overlaps)]
        lib.cw_overlap_to_pile_device.argtypes = [C.c_void_p, C.POINTER(Overlaps), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.cw_debug_overlap_plan.argtypes = [C.c_uint32, C.c_int, C.c_void_p]
        lib.cw_debug_overlap_routes.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(lib, "cw_sw_span_run"):
        lib.cw_sw_span_run.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.POINTER(SwSpans), C.c_uint32]
        lib.cw_sw_span_run_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.POINTER(SwSpans), C.c_uint32, C.c_void_p]
        lib.cw_sw_path_span_run.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.POINTER(SwPaths), C.POINTER(SwSpans), C.c_uint32]
        lib.cw_sw_path_span_run_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.POINTER(SwPaths), C.POINTER(SwSpans), C.c_uint32, C.c_void_p]
        lib.cw_pileup_span_run.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.POINTER(Pileup), C.POINTER(SwSpans), C.c_uint32]
        lib.cw_pileup_span_run_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.POINTER(Pileup), C.POINTER(SwSpans), C.c_uint32, C.c_void_p]
        lib.cw_sw_cut_span_run.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.POINTER(SwCuts), C.POINTER(SwSpans)]
        lib.cw_sw_cut_span_run_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.POINTER(SwCuts), C.POINTER(SwSpans), C.c_void_p]
        lib.cw_seed_spans.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.cw_seed_spans_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cw_submit.argtypes = [C.c_void_p, C.POINTER(Batch), C.POINTER(Result), C.POINTER(C.c_int)]
    lib.cw_wait.argtypes = [C.c_void_p, C.c_int]
    lib.cw_host_alloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    lib.cw_host_free.argtypes = [C.c_void_p]
    lib.cw_host_free.restype = None
    lib.cw_poll.argtypes = [C.c_void_p]
    lib.cw_poll.restype = C.c_int
    lib.cw_configure.argtypes = [C.c_void_p, C.c_uint32]
    lib.cw_max_batch_windows.argtypes = [C.c_void_p]
    lib.cw_max_batch_windows.restype = C.c_uint32
    lib.cw_last_timings.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_int)]
    lib.cw_debug_win_info.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    if hasattr(lib, "cw_debug_tier_x"):  # (a library built before tier X has no such entry)
        lib.cw_debug_tier_x.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(lib, "cw_debug_tier_q"):
        lib.cw_debug_tier_q.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(lib, "cw_debug_tier_lists"):
        lib.cw_debug_tier_lists.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p, C.c_uint32,
                                            C.POINTER(C.c_uint32)]
    if hasattr(lib, "cw_debug_solid_table"):
        lib.cw_debug_solid_table.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    if hasattr(lib, "cw_debug_anchor_block"):
        lib.cw_debug_anchor_block.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        lib.cw_debug_ab_layout.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    if hasattr(lib, "cw_debug_segments"):
        lib.cw_debug_segments.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32),
                                          C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.cw_debug_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.cw_extract_piles_device.argtypes = [C.c_void_p, C.POINTER(ReadSet), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_void_p]
    lib.cw_plan_results_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p]
    lib.cw_stitch_device.argtypes = [C.c_void_p, C.POINTER(ReadSet), C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(Batch), C.POINTER(Result), C.c_uint32, C.c_uint32,
                                     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cw_index_reads.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    lib.cw_index_reads_append.argtypes = [C.c_void_p, C.c_char_p]
    lib.cw_read_index_free.argtypes = [C.c_void_p]
    lib.cw_read_index_free.restype = None
    lib.cw_read_index_count.argtypes = [C.c_void_p]
    lib.cw_read_index_count.restype = C.c_uint32
    lib.cw_read_index_view.argtypes = [C.c_void_p, C.POINTER(ReadSet), C.POINTER(C.c_uint64)]
    lib.cw_read_index_find.argtypes = [C.c_void_p, C.c_char_p]
    lib.cw_read_index_find.restype = C.c_int32
    lib.cw_read_index_name.argtypes = [C.c_void_p, C.c_uint32]
    lib.cw_read_index_name.restype = C.c_char_p
    lib.cw_paf_open.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
    lib.cw_paf_next_pile.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.cw_paf_close.argtypes = [C.c_void_p]
    lib.cw_paf_close.restype = None
    lib.cw_paf_reformat.argtypes = [C.c_char_p, C.c_char_p]
    lib.cw_paf_explode.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_uint32)]
    lib.cw_paf_merge.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_uint32]
    lib.cw_window_positions.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.cw_pack_sequence.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint64]
    lib.cw_pack_sequence.restype = C.c_int64
    lib.cw_synth_sizes.argtypes = [C.POINTER(SynthSpec), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    lib.cw_synth_host.argtypes = [C.POINTER(SynthSpec), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cw_synth_device.argtypes = [C.c_void_p, C.POINTER(SynthSpec), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _LIBS[p] = lib
    return lib


# The index kernel's route witness (csrc/cw_index.h enum CwIdxRoute, the same bits by name; csrc/cw_device.h CW_PS_IDX_ROUTE): which way the windows of
# the last batch went through cw_index_kernel.  Only the -DCW_TEST_AIDS library writes it.
INDEX_ROUTE_SLOT = 63
INDEX_ROUTE = {"staged": 1 << 0, "bytes_done": 1 << 1, "nibbles": 1 << 2, "big_ex": 1 << 3, "export_masks": 1 << 4, "export_walk": 1 << 5, "rewalk": 1 << 6,
               "hashed": 1 << 7, "hash_passes": 1 << 8, "hash_gsort": 1 << 9, "wide": 1 << 10, "tfit": 1 << 11, "pg": 1 << 12, "hit_list": 1 << 13, "use_bits": 1 << 14,
               "second_pass": 1 << 15, "bucket_walk": 1 << 16}


# The anchor block of a window (csrc/cw_index.h CwAbCarve: what cw_index_kernel hands to cw_chain_kernel).  ab_layout restates cw_ab_carve<uint64_t>(0, ...):
# tests/test_anchor_ref_cpu.py holds it to cw_debug_ab_layout, and tests/chain_probes.py takes the block's size from it.
AB_HDR, AB_NONE16 = 64, 0xFFFF
AB_PARTS = ("hdr", "ckey", "pres", "dirty", "badm", "rowid", "delta", "P", "end")


def ab_np(N):
    """cw_ab_np: a matrix row's u16 entries -- N rounded up to twice an odd number."""
    Np = (N + 1) & ~1
    return Np + 2 if (Np >> 1) & 1 == 0 else Np


def ab_layout(A, N, n_dirty, n_rows):
    """The nine byte offsets of cw_ab_carve, in the order of AB_PARTS.  Without correction rows there are neither row ids nor rows: P starts at rowid."""
    al = lambda x: (x + 15) & ~15
    o = {"hdr": 0, "ckey": AB_HDR}
    o["pres"] = o["ckey"] + al(4 * A)
    o["dirty"] = o["pres"] + al(8 * A * ((N + 63) // 64))
    o["badm"] = o["dirty"] + al(2 * n_dirty)
    o["rowid"] = o["badm"] + al(8 * A)
    o["delta"] = o["rowid"] + al(A)
    o["P"] = o["delta"] + n_rows * ((A + 15) & ~15) if n_rows else o["rowid"]
    o["end"] = o["P"] + al(2 * A * ab_np(N))
    return tuple(o[n] for n in AB_PARTS)


class AnchorBlock:
    """A window's anchor block as read back (Engine.anchor_block): the header's numbers and numpy views of the parts, cut by ab_layout.  Views of parts the
    kernel does not write under the block's flags (badm without has_bm, the alignment gaps) show whatever the scratch held."""

    def __init__(self, raw):
        self.raw = raw
        self.A, self.N, self.n_dirty, self.flags, self.n_rows = (int(x) for x in raw[:20].view(np.uint32))
        self.use_bits, self.has_bm, self.has_delta = bool(self.flags & 1), bool(self.flags & 2), bool(self.flags & 4)
        A, N = self.A, self.N
        self.Nw, self.Np, self.Ap = (N + 63) // 64, ab_np(N), (A + 15) & ~15
        off = dict(zip(AB_PARTS, ab_layout(A, N, self.n_dirty, self.n_rows)))
        assert off["end"] == len(raw), (off["end"], len(raw))
        cut = lambda name, dtype, count: raw[off[name] : off[name] + count * np.dtype(dtype).itemsize].view(dtype)
        self.ckey = cut("ckey", np.uint32, A)
        self.pres = cut("pres", np.uint64, A * self.Nw).reshape(A, self.Nw)
        self.dirty = cut("dirty", np.uint16, self.n_dirty)
        self.badm = cut("badm", np.uint64, A)
        self.rowid = cut("rowid", np.uint8, A if self.n_rows else 0)
        self.delta = cut("delta", np.uint8, self.n_rows * self.Ap).reshape(self.n_rows, self.Ap)
        self.P = cut("P", np.uint16, A * self.Np).reshape(A, self.Np)


# The chain kernel's route witness (csrc/cw_chain.h enum CwChRoute, csrc/cw_device.h CW_PS_CHAIN_ROUTE): the same for cw_chain_kernel.
CHAIN_ROUTE_SLOT = 45
CHAIN_ROUTE = {"fast": 1 << 0, "rows_lds": 1 << 1, "rows_far": 1 << 2, "pres_lds": 1 << 3, "wide_key": 1 << 4, "far_scan": 1 << 5, "inplace_rows": 1 << 6,
               "inplace_masks": 1 << 7, "inplace_all_dirty": 1 << 8, "inplace_matrix": 1 << 9, "early_flush": 1 << 10, "long_single": 1 << 11, "long_slab": 1 << 12}


# The finish kernel's witness (csrc/cw_finish.h enum CwFinRoute, csrc/cw_device.h CW_PS_FIN_ROUTE .. CW_PS_FIN_NBRS): the route bits, and behind them how often
# fin_link entered a frame and how often it called fin_neighbours, summed over the batch's windows.
FINISH_ROUTE_SLOT = 33
FINISH_ROUTE = {"staged": 1 << 0, "compact": 1 << 1, "global": 1 << 2, "cnt16": 1 << 3, "cnt_global": 1 << 4, "vis_lds": 1 << 5, "vis_global": 1 << 6, "find4": 1 << 7,
                "count_scan": 1 << 8, "head": 1 << 9, "tail": 1 << 10, "linked": 1 << 11, "first_pass": 1 << 12, "second_pass": 1 << 13}


# The re-assembly kernel's witness (csrc/cw_stitch.h enums CwStRoute, CwStBand, CwStRead; cw_debug_stitch_route): per window of the last Engine.stitch call a route
# word, the word of the banded traceback and the numbers of the overlap reconciliation, per read a route word.  Only the -DCW_TEST_AIDS library records it,
# and only under CW_STITCH_TRACE.  The names are those of tests/stitch_ref.py.
STITCH_ROUTE = {n: 1 << i for i, n in enumerate((
    "overflow_skipped", "template_aligned", "template_absent", "al_pos_clamped", "slice_clipped", "no_slice", "no_alignment", "query_clipped", "overlap",
    "guard_short_consensus", "guard_old_shorter", "guard_cur_shorter", "equal_ignoring_case", "by_solid", "by_upper", "old_wins", "tie", "cur_wins", "sub_no_score",
    "indels", "spliced", "emptied", "replaced_longer", "replaced_shorter", "replaced_same", "gap_right", "gap_left", "gap_right_far", "gap_left_far", "last_window"))}
STITCH_BAND = {n: 1 << i for i, n in enumerate(("band_lanes", "band_serial", "rows_global", "dirs_lds", "dirs_global", "band_doubled", "sub_mem_sweep"))}
STITCH_READ = {n: 1 << i for i, n in enumerate(("slot_too_small", "no_window", "outgrown", "last_launch", "no_upper", "one_upper", "trim_shift", "dropped", "handed_over"))}
STITCH_FACTS = ("beg", "end", "overlap", "s1", "s2", "sub_score", "ins", "del", "cut", "cl", "cur_pos", "gap_move")
STITCH_WIT_WORDS = 16
STITCH_GUARD = 64  # bytes behind every out slot of Engine.stitch that no read may touch


# The POA tiers' route witness (csrc/cw_poa.h enums CwPoaRoute and CwPoaRc2, csrc/cw_device.h CW_PS_POA_ROUTE and CW_PS_POA_RC2): which fills, walks, group
# fills, replays and coded row kinds the members of the last batch's tasks took in each slab tier, and why a tier gave a task up (rc 2).  32 route bits a
# tier, two tiers a slot from POA_ROUTE_SLOT; a byte of causes a tier in POA_RC2_SLOT.
POA_ROUTE_SLOT, POA_RC2_SLOT = 69, 126
POA_TIERS = ("S", "M1", "M2", "L", "G", "X")
POA_ROUTE = {"fill_coded": 1 << 0, "fill_pad": 1 << 1, "fill_w1": 1 << 2, "fill_w2": 1 << 3, "fill_w4": 1 << 4, "fill_w8": 1 << 5, "fill_w16": 1 << 6, "fill_w32": 1 << 7,
             "fill_blocks": 1 << 8, "fill_pk1": 1 << 9, "fill_pk2": 1 << 10, "fill_pk4": 1 << 11, "fill_pk8": 1 << 12, "fill_group": 1 << 13, "walk_runs": 1 << 14,
             "walk_dirs": 1 << 15, "walk_tiles": 1 << 16, "walk_coded": 1 << 17, "grp_2": 1 << 18, "grp_3": 1 << 19, "grp_4": 1 << 20, "grp_read": 1 << 21,
             "grp_abandoned": 1 << 22, "replay": 1 << 23, "replay_grp": 1 << 24, "meta_reused": 1 << 25, "row_far": 1 << 26, "row_fan4": 1 << 27, "row_slab": 1 << 28}
POA_RC2 = {"rc2_lcap": 1 << 0, "rc2_first": 1 << 1, "rc2_hcap": 1 << 2, "rc2_ccap": 1 << 3, "rc2_nodes": 1 << 4, "rc2_edges": 1 << 5, "rc2_indeg": 1 << 6}


def poa_route_names(route):
    """Engine.poa_route()'s answer as a set of 'tier.bit' names ('M2.fill_pk2', 'S.rc2_nodes')."""
    out = set()
    for tier, (bits, rc2) in route.items():
        out |= {f"{tier}.{n}" for n, b in POA_ROUTE.items() if bits & b} | {f"{tier}.{n}" for n, b in POA_RC2.items() if rc2 & b}
    return out


def route_names(bits, table=None):
    """The names of the bits of `table` (default INDEX_ROUTE) set in `bits`, for messages."""
    return sorted(n for n, b in (table or INDEX_ROUTE).items() if bits & b)


def _check(lib, rc, what, allow_capacity=False):
    if rc == 0 or (allow_capacity and rc == -4):
        return rc
    raise EngineError(f"{what}: {lib.cw_strerror(rc).decode()} ({rc})")


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


class HostBatch:
    """Host arrays laid out as cw_batch."""

    def __init__(self, win_first_seq, seq_len, seq_word_off, bases):
        self.win_first_seq = np.ascontiguousarray(win_first_seq, np.uint32)
        self.seq_len = np.ascontiguousarray(seq_len, np.uint32)
        self.seq_word_off = np.ascontiguousarray(seq_word_off, np.uint64)
        self.bases = np.ascontiguousarray(bases, np.uint32)

    @property
    def n_windows(self):
        return len(self.win_first_seq) - 1

    def c_struct(self):
        return Batch(self.n_windows, len(self.seq_len), len(self.bases), _ptr(self.win_first_seq), _ptr(self.seq_len), _ptr(self.seq_word_off), _ptr(self.bases))

    def pile(self, w):
        """Decode window w back to a list of ASCII strings (test helper)."""
        out = []
        for s in range(int(self.win_first_seq[w]), int(self.win_first_seq[w + 1])):
            n = int(self.seq_len[s])
            o = int(self.seq_word_off[s])
            words = self.bases[o : o + (n + 15) // 16]
            codes = ((words[:, None] >> (30 - 2 * np.arange(16, dtype=np.uint32))[None, :]) & 3).reshape(-1)[:n]
            out.append(np.frombuffer(b"ACGT", np.uint8)[codes].tobytes().decode())
        return out

    def slice(self, w0, w1):
        s0, s1 = int(self.win_first_seq[w0]), int(self.win_first_seq[w1])
        return HostBatch(self.win_first_seq[w0 : w1 + 1] - s0, self.seq_len[s0:s1], self.seq_word_off[s0:s1], self.bases)


def concat_batches(batches):
    """One HostBatch of the windows of `batches` (HostBatch, slices included), in order: sequences and words appended, offsets moved."""
    wfs, lens, offs, bases = [np.zeros(1, np.uint32)], [], [], []
    s_run = w_run = 0
    for b in batches:
        s0, s1 = int(b.win_first_seq[0]), int(b.win_first_seq[-1])
        wfs.append(b.win_first_seq[1:].astype(np.uint64) - s0 + s_run)
        lens.append(b.seq_len[s0:s1])
        offs.append(b.seq_word_off[s0:s1].astype(np.uint64) + w_run)
        bases.append(b.bases)
        s_run += s1 - s0
        w_run += len(b.bases)
    return HostBatch(np.concatenate(wfs).astype(np.uint32), np.concatenate(lens), np.concatenate(offs), np.concatenate(bases))


def pack_piles(piles):
    """List of piles (each a list of ACGT strings, template first) -> HostBatch (reference 2-bit alphabet, utils.cpp:21-32)."""
    lib = load_library()
    n_seqs = sum(len(p) for p in piles)
    wfs = np.zeros(len(piles) + 1, np.uint32)
    lens = np.zeros(n_seqs, np.uint32)
    offs = np.zeros(n_seqs, np.uint64)
    total_words = sum((len(s) + 15) // 16 for p in piles for s in p)
    bases = np.zeros(max(total_words, 1), np.uint32)
    si = 0
    wo = 0
    for w, p in enumerate(piles):
        wfs[w] = si
        for s in p:
            raw = s.encode()
            lens[si] = len(raw)
            offs[si] = wo
            got = lib.cw_pack_sequence(raw, len(raw), C.c_void_p(bases.ctypes.data + 4 * wo), total_words - wo)
            if got < 0:
                raise EngineError("cw_pack_sequence failed")
            wo += got
            si += 1
    wfs[len(piles)] = si
    return HostBatch(wfs, lens, offs, bases)


def window_positions(tpl_len, overlaps, min_support, window_size, window_overlap):
    """cw_window_positions: `overlaps` is an (n,6) uint32 array of cw_overlap rows; returns [(beg, end), ...]."""
    lib = load_library()
    ov = np.ascontiguousarray(overlaps, np.uint32).reshape(-1, 6)
    n = C.c_uint32()
    cap = tpl_len // max(1, window_size - window_overlap) + 8
    out = np.zeros(2 * cap, np.uint32)
    _check(lib, lib.cw_window_positions(tpl_len, _ptr(ov) if len(ov) else None, len(ov), min_support, window_size, window_overlap, _ptr(out), cap, C.byref(n)), "cw_window_positions")
    return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n.value)]


def synth_host(spec):
    lib = load_library()
    ns, nw = C.c_uint32(), C.c_uint64()
    _check(lib, lib.cw_synth_sizes(C.byref(spec), C.byref(ns), C.byref(nw)), "cw_synth_sizes")
    wfs = np.zeros(spec.n_windows + 1, np.uint32)
    lens = np.zeros(ns.value, np.uint32)
    offs = np.zeros(ns.value, np.uint64)
    bases = np.zeros(nw.value, np.uint32)
    _check(lib, lib.cw_synth_host(C.byref(spec), _ptr(wfs), _ptr(lens), _ptr(offs), _ptr(bases)), "cw_synth_host")
    return HostBatch(wfs, lens, offs, bases)


def write_paf(path, names, lengths, per_query):
    """The PAF file of overlap rows: per_query[q] is the rows (OVL_ROW numbers each) of read q, names and lengths those of every read.  One line per row,
    fields as Engine.overlaps_paf states them.  Returns the number of lines."""
    n = 0
    with open(path, "w") as f:
        for q, rows in enumerate(per_query):
            for t, o, hits, _, qs, qe, ts, te in rows:
                f.write("%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t255\n" % (names[q], lengths[q], qs, qe + 1, "-" if o == STRAND_REV else "+", names[t], lengths[t], ts, te + 1,
                                                                            hits, max(qe + 1 - qs, te + 1 - ts)))
                n += 1
    return n


def paf_reformat(in_path, out_path):
    """reformatPAF (src/reformatPAF.cpp): swap the query and target columns of a PAF file."""
    lib = load_library()
    _check(lib, lib.cw_paf_reformat(os.fsencode(in_path), os.fsencode(out_path)), "cw_paf_reformat")


def paf_explode(in_path, out_prefix):
    """explode (src/explode.cpp): returns the list of chunk files written (out_prefix_1 ...)."""
    lib = load_library()
    n = C.c_uint32()
    _check(lib, lib.cw_paf_explode(os.fsencode(in_path), os.fsencode(out_prefix), C.byref(n)), "cw_paf_explode")
    return [f"{out_prefix}_{i}" for i in range(1, n.value + 1)]


def paf_merge(out_path, headers_path, in_paths):
    """merge (src/merge.cpp): gather every read's lines from the chunks, in the order of the header file."""
    lib = load_library()
    arr = (C.c_char_p * max(len(in_paths), 1))(*[os.fsencode(p) for p in in_paths])
    _check(lib, lib.cw_paf_merge(os.fsencode(out_path), os.fsencode(headers_path), arr, len(in_paths)), "cw_paf_merge")


class ReadIndex:
    """indexReads (utils.cpp:166-205) through the library's host feeder: names, lengths and the 2-bit read set."""

    def __init__(self, path, *more_paths):
        self.lib = load_library()
        h = C.c_void_p()
        _check(self.lib, self.lib.cw_index_reads(os.fsencode(path), C.byref(h)), f"cw_index_reads({path})")
        self.handle = h
        for p in more_paths:
            _check(self.lib, self.lib.cw_index_reads_append(h, os.fsencode(p)), f"cw_index_reads_append({p})")
        n = self.lib.cw_read_index_count(h)
        view, nw = ReadSet(), C.c_uint64()
        _check(self.lib, self.lib.cw_read_index_view(h, C.byref(view), C.byref(nw)), "cw_read_index_view")
        self.names = [self.lib.cw_read_index_name(h, i).decode() for i in range(n)]
        as_np = lambda ptr, ct, cnt: np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(max(cnt, 1),))[:cnt].copy()
        self.seq_len = as_np(view.read_len, C.c_uint32, n)
        self.seq_word_off = as_np(view.read_word_off, C.c_uint64, n)
        self.bases = as_np(view.bases, C.c_uint32, nw.value)

    def find(self, name):
        return self.lib.cw_read_index_find(self.handle, name.encode())

    def sequence(self, i):
        o, n = int(self.seq_word_off[i]), int(self.seq_len[i])
        w = self.bases[o : o + (n + 15) // 16]
        codes = ((w[:, None] >> (30 - 2 * np.arange(16, dtype=np.uint32))) & 3).reshape(-1)[:n]
        return np.frombuffer(b"ACGT", np.uint8)[codes].tobytes().decode()

    def close(self):
        if self.handle:
            self.lib.cw_read_index_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PafReader:
    """getNextReadPile (alignmentPiles.cpp:22-58): iterate over (template id, template length, overlaps (n,6), resMatches (n,))."""

    def __init__(self, path, index, max_support=150):
        self.lib = load_library()
        self.index = index
        self.max_support = max_support
        h = C.c_void_p()
        _check(self.lib, self.lib.cw_paf_open(os.fsencode(path), index.handle, max_support, C.byref(h)), f"cw_paf_open({path})")
        self.handle = h

    def __iter__(self):
        ov = np.zeros((max(self.max_support, 1), 6), np.uint32)
        rm = np.zeros(max(self.max_support, 1), np.uint32)
        tpl, tlen, n = C.c_uint32(), C.c_uint32(), C.c_uint32()
        while True:
            _check(self.lib, self.lib.cw_paf_next_pile(self.handle, C.byref(tpl), C.byref(tlen), _ptr(ov), _ptr(rm), len(ov), C.byref(n)), "cw_paf_next_pile")
            if n.value == 0:
                return
            yield tpl.value, tlen.value, ov[: n.value].copy(), rm[: n.value].copy()

    def close(self):
        if self.handle:
            self.lib.cw_paf_close(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WindowResults:
    def __init__(self, cons, cons_off, cons_len, status, solid=None, solid_off=None, solid_len=None):
        self.cons, self.cons_off, self.cons_len, self.status = cons, cons_off, cons_len, status
        self.solid, self.solid_off, self.solid_len = solid, solid_off, solid_len

    def consensus(self, w):
        o = int(self.cons_off[w])
        return self.cons[o : o + int(self.cons_len[w])].tobytes().decode()

    def solid_kmers(self, w):
        o = int(self.solid_off[w])
        return self.solid[o : o + int(self.solid_len[w])]


def cons_slot_bytes(k, tpl_len):
    """CW_CONS_SLOT_BYTES of include/consent_amd.h: the consensus slot cw_plan_results_device gives a window (numpy-friendly)."""
    tpl = np.asarray(tpl_len, np.int64)
    if k >= 9:
        return np.clip(4 * tpl + 1024, 3072, 32768)
    if k == 8:
        return np.minimum(16 * tpl + 1024, 32768)
    return np.full_like(tpl, 32768)


def alloc_results(batch, want_solid=True, solid_thresh=4, k=9):
    W = batch.n_windows
    wfs = batch.win_first_seq.astype(np.int64)
    tpl = batch.seq_len[wfs[:-1]].astype(np.int64)
    cap = cons_slot_bytes(k, tpl)  # as cw_plan_results_device sizes it (cw_pack.h)
    cons_off = np.zeros(W + 1, np.uint64)
    cons_off[1:] = np.cumsum(cap)
    cons = np.zeros(int(cons_off[-1]), np.uint8)
    cons_len = np.zeros(W, np.uint32)
    status = np.full(W, 255, np.uint8)
    if not want_solid:
        return WindowResults(cons, cons_off, cons_len, status)
    csum = np.concatenate([[0], np.cumsum(batch.seq_len.astype(np.int64))])
    per_win = csum[wfs[1:]] - csum[wfs[:-1]]
    scap = per_win // max(1, solid_thresh) + 16
    solid_off = np.zeros(W + 1, np.uint64)
    solid_off[1:] = np.cumsum(scap)
    solid = np.zeros(int(solid_off[-1]), np.uint32)
    solid_len = np.zeros(W, np.uint32)
    return WindowResults(cons, cons_off, cons_len, status, solid, solid_off, solid_len)


def poa_slot_bytes(longest_member):
    """CW_POA_SLOT_BYTES of include/consent_amd.h: the consensus slot the segment path reserves for members of at most this many bases (numpy-friendly)."""
    return 2 * np.asarray(longest_member, np.int64) + 2


def alloc_poa_results(batch, slot_bytes=None):
    """WindowResults for Engine.poa: one consensus slot per group -- slot_bytes (a number or one per group), default poa_slot_bytes of its longest sequence."""
    G = batch.n_windows
    wfs = batch.win_first_seq.astype(np.int64)
    if slot_bytes is None:
        lens = batch.seq_len.astype(np.int64)
        slot_bytes = poa_slot_bytes(np.array([lens[wfs[g] : wfs[g + 1]].max(initial=0) for g in range(G)], np.int64))
    cons_off = np.zeros(G + 1, np.uint64)
    cons_off[1:] = np.cumsum(np.broadcast_to(np.asarray(slot_bytes, np.int64), (G,)))
    return WindowResults(np.zeros(max(int(cons_off[-1]), 1), np.uint8), cons_off, np.zeros(G, np.uint32), np.full(G, 255, np.uint8))


class SwRows:
    """What Engine.sw returns: `rows`, an (n_seqs, SW_ROW) int32 array with one row per sequence of the batch (columns SW_SCORE .. SW_STATUS), and the map
    from (group, member) -- member 0 is the group's reference -- to its row."""

    def __init__(self, rows, win_first_seq, rc=0):
        self.rows, self.win_first_seq, self.rc = rows, win_first_seq, rc

    def index(self, group, member):
        s = int(self.win_first_seq[group]) + member
        if member < 0 or s >= int(self.win_first_seq[group + 1]):
            raise IndexError(f"group {group} has no member {member}")
        return s

    def row(self, group, member):
        return self.rows[self.index(group, member)]


class SwPathRows(SwRows):
    """What Engine.sw_path returns: SwRows, and per sequence `n_ops` and its slot ops_buf[ops_off[s] : ops_off[s + 1]] of `length << 4 | op` words, of which
    the first n_ops are the path (none unless the row's status is SW_ALIGNED)."""

    def __init__(self, rows, win_first_seq, rc, n_ops, ops_buf, ops_off):
        super().__init__(rows, win_first_seq, rc)
        self.n_ops, self.ops_buf, self.ops_off = n_ops, ops_buf, ops_off

    def ops(self, group, member):
        """The path of (group, member) as a list of (length, op code); empty when the row reports none."""
        s = self.index(group, member)
        if int(self.rows[s, SW_STATUS]) != SW_ALIGNED:
            return []
        o = int(self.ops_off[s])
        return [(int(w) >> 4, int(w) & 15) for w in self.ops_buf[o : o + int(self.n_ops[s])]]

    def cigar(self, group, member):
        """The path as a CIGAR string such as "35M2I10M1D4M" ("=" and "X" in place of "M" when the run had eqx=True)."""
        return "".join(f"{n}{SW_OP_LETTERS[op]}" for n, op in self.ops(group, member))


class PileupRows(SwRows):
    """What Engine.pileup returns: SwRows, and the columns: counts_buf is an (n_columns, PILE_COL) uint32 array in which sequence s, where it is its group's
    reference, owns rows col_off[s] : col_off[s + 1] -- Engine.pileup gives every reference as many columns as it has bases and a query none, so counts_buf
    is the groups' references one after the other whatever their queries, and the counts_buf of one run can be the `into` of another over the same references."""

    def __init__(self, rows, win_first_seq, rc, counts_buf, col_off, seq_len):
        super().__init__(rows, win_first_seq, rc)
        self.counts_buf, self.col_off, self.seq_len = counts_buf, col_off, seq_len

    def counts(self, group):
        """The (ref_len, PILE_COL) counts of the group's reference: columns PILE_A .. PILE_END (empty for a group of none, or when the slot is too short)."""
        r = int(self.win_first_seq[group])
        if r >= int(self.win_first_seq[group + 1]):
            return self.counts_buf[:0]
        o, n = int(self.col_off[r]), int(self.seq_len[r])
        return self.counts_buf[o : o + n] if int(self.col_off[r + 1]) - o >= n else self.counts_buf[:0]

    def coverage(self, group):
        """Per column of the group's reference the number of counted alignments that cover it: A + C + G + T + DEL."""
        return self.counts(group)[:, : PILE_DEL + 1].sum(axis=1, dtype=np.int64)


class SwCutRows(SwRows):
    """What Engine.sw_cut returns: SwRows, and per query its cut points at the reference's window boundaries: sequence s, where it is a query, owns
    cuts_buf[cut_off[s] : cut_off[s + 1]], of which the first sw_cuts(reference length, window) words are written."""

    def __init__(self, rows, win_first_seq, rc, cuts_buf, cut_off, window, batch):
        super().__init__(rows, win_first_seq, rc)
        self.cuts_buf, self.cut_off, self.window, self.batch = cuts_buf, cut_off, window, batch

    def cuts(self, group, member):
        """The T + 1 cut points of query `member` (>= 1) of `group`: query positions, non-decreasing; empty when the slot does not hold them."""
        s = self.index(group, member)
        if member == 0:
            raise IndexError("a reference has no cut points")
        n = int(sw_cuts(int(self.batch.seq_len[int(self.win_first_seq[group])]), self.window))
        o = int(self.cut_off[s])
        return self.cuts_buf[o : o + n] if int(self.cut_off[s + 1]) - o >= n else self.cuts_buf[:0]

    def pieces(self, group, member):
        """The query cut at those points: piece t is what its alignment puts on window t of the reference ('' where it puts nothing)."""
        c = [int(x) for x in self.cuts(group, member)]
        q = self.batch.pile(group)[member]
        return [q[a:b] for a, b in zip(c, c[1:])]


class StrandRows:
    """What Engine.strands returns: `strands`, a uint8 value per sequence of the batch (STRAND_FWD, STRAND_REV, STRAND_IS_REF for a group's reference, STRAND_NONE
    where no vote is possible), `hit_counts`, an (n_seqs, 2) uint32 array of forward and reverse hits, and the map from (group, member) to them as SwRows has it."""

    def __init__(self, strands, hit_counts, win_first_seq, k):
        self.strands, self.hit_counts, self.win_first_seq, self.k = strands, hit_counts, win_first_seq, k

    index = SwRows.index

    def strand(self, group, member):
        return int(self.strands[self.index(group, member)])

    def hits(self, group, member):
        """(forward hits, reverse hits) of (group, member)."""
        f, r = self.hit_counts[self.index(group, member)]
        return int(f), int(r)


class SeedRows(SwRows):
    """What Engine.seeds returns: `rows`, an (n_seqs, SEED_ROW) int32 array -- SEED_STATUS (a STRAND_* value), SEED_HITS, SEED_DIAG, SEED_OTHER -- `strands`, the
    status bytes as cw_revcomp takes them, and .row(group, member) as SwRows has it."""

    def __init__(self, rows, strands, win_first_seq, k):
        super().__init__(rows, win_first_seq)
        self.strands, self.k = strands, k


class LocateIndex:
    """What Engine.locate_index returns: the reference packed on the device (`bases`) and the index built over it (`table`), both torch tensors this handle
    keeps alive; `ref_len`, and `k` as it was given (0 = LOCATE_K).  .c_struct() is the cw_locate_ref the device entry points take."""

    def __init__(self, ref_len, k, bases, table):
        self.ref_len, self.k, self.bases, self.table = ref_len, k, bases, table

    def c_struct(self):
        return LocateRef(self.bases.data_ptr(), self.ref_len, self.table.data_ptr(), self.k)


class OverlapIndex:
    """What Engine.overlap_index returns: the read set on the device (`seq_len`, `seq_word_off`, `bases`) and the index built over it (`mem`), torch tensors
    this handle keeps alive; `lengths` (the reads' lengths on the host), `n_entries`, and k, sample, max_occ as they were given.  .batch() is the cw_batch
    and .c_struct(min_hits) the cw_overlap_index the device entry points take."""

    def __init__(self, lengths, n_words, k, sample, max_occ, n_entries, seq_len, seq_word_off, bases, mem):
        self.lengths, self.n_words, self.k, self.sample, self.max_occ, self.n_entries = lengths, n_words, k, sample, max_occ, n_entries
        self.seq_len, self.seq_word_off, self.bases, self.mem = seq_len, seq_word_off, bases, mem

    def batch(self):
        return Batch(0, len(self.lengths), self.n_words, None, self.seq_len.data_ptr(), self.seq_word_off.data_ptr(), self.bases.data_ptr())

    def c_struct(self, min_hits):
        return OverlapIndexRef(self.mem.data_ptr(), self.n_entries, OverlapParams(self.k, self.sample, self.max_occ, int(min_hits)))


class OverlapRows:
    """What Engine.overlap_rows returns for queries first .. first + count - 1: `rows` (total, OVL_ROW) int32, `row_off` (count + 1, in rows), `n_rows`, `status`.
    .of(j) is the (n_rows[j], OVL_ROW) rows of query first + j."""

    def __init__(self, rows, row_off, n_rows, status, first):
        self.rows, self.row_off, self.n_rows, self.status, self.first = rows, row_off, n_rows, status, first

    def of(self, j):
        a = int(self.row_off[j])
        return self.rows[a : a + (int(self.n_rows[j]) if self.status[j] == OVL_OK else 0)]


class Overlap:
    """One row of Engine.overlaps: read `target` overlaps the query on `strand` (STRAND_FWD, or STRAND_REV: its reverse complement does) with `hits` shared
    sampled k-mers in the best 128 diagonals from `diag`; q_start .. q_end on the query as given and t_start .. t_end on the target, ends inclusive -- the
    dovetail that diagonal implies, up to OVL_END_SLACK bases from an aligned end."""

    __slots__ = ("target", "strand", "hits", "diag", "q_start", "q_end", "t_start", "t_end")

    def __init__(self, target, strand, hits, diag, q_start, q_end, t_start, t_end):
        self.target, self.strand, self.hits, self.diag, self.q_start, self.q_end, self.t_start, self.t_end = target, strand, hits, diag, q_start, q_end, t_start, t_end

    def astuple(self):
        return (self.target, self.strand, self.hits, self.diag, self.q_start, self.q_end, self.t_start, self.t_end)

    def __eq__(self, o):
        return isinstance(o, Overlap) and self.astuple() == o.astuple()

    def __repr__(self):
        return "Overlap(target=%d, strand=%d, hits=%d, diag=%d, q_start=%d, q_end=%d, t_start=%d, t_end=%d)" % self.astuple()


class Placement:
    """One read of Engine.place: `strand` (STRAND_FWD, or STRAND_REV: its reverse complement lies on the reference), `position`, the lowest reference
    coordinate of the densest 128 diagonals -- where the read, turned when REV, begins, give or take its indels; negative when it overhangs the start --
    `hits`, the unique k-mers it shares with the reference there, and `other`, the best the other orientation found."""

    def __init__(self, strand, position, hits, other):
        self.strand, self.position, self.hits, self.other = strand, position, hits, other

    def __eq__(self, o):
        return isinstance(o, Placement) and (self.strand, self.position, self.hits, self.other) == (o.strand, o.position, o.hits, o.other)

    def __repr__(self):
        return f"Placement(strand={self.strand}, position={self.position}, hits={self.hits}, other={self.other})"


class PolishWindow:
    """One window of a polished reference: `members` pieces were aligned beside the reference's own; `status` is the POA's (WIN_CONSENSUS, or WIN_OVERFLOW
    for a group that stopped: `kept_reference` is then True and the window's part of the result is the reference's columns)."""

    def __init__(self, members, status, kept_reference):
        self.members, self.status, self.kept_reference = members, status, kept_reference

    def __repr__(self):
        return f"PolishWindow(members={self.members}, status={self.status}, kept_reference={self.kept_reference})"


class Polished:
    """One reference of Engine.polish: `sequence`, the windows' consensuses joined in order, `windows`, a PolishWindow each, and `strands`, the strand value of
    every read of the group under orient=True (empty without).  From Engine.polish_reads: `placements`, a Placement or None per read (empty otherwise)."""

    def __init__(self, sequence, windows, strands=None, placements=None):
        self.sequence, self.windows, self.strands = sequence, windows, [] if strands is None else strands
        self.placements = [] if placements is None else placements


_COMPLEMENT = str.maketrans("ACGTacgtNn", "TGCAtgcaAA")  # (N is packed as T: its complement is A, as cw_revcomp has it)


def _revcomp(s):
    return s.translate(_COMPLEMENT)[::-1]


def span_arrays(spans, n_seqs):
    """`spans` as the two uint32 arrays of cw_sw_spans: a pair of per-sequence arrays (lo, hi), or one (n_seqs, 2) array.  Values are clipped to 32 bits; a
    negative one is 0."""
    pair = isinstance(spans, (tuple, list)) and len(spans) == 2  # (two sequences: a tuple or list of two is the pair, an array the (n_seqs, 2) form)
    a = np.asarray(spans, dtype=np.int64)
    if a.shape == (n_seqs, 2) and not (pair and np.ndim(spans[0]) == 1):
        a = a.T
    if a.shape != (2, n_seqs):
        raise EngineError(f"spans: a pair of arrays of {n_seqs} values, or one of shape ({n_seqs}, 2)")
    a = np.clip(a, 0, 0xFFFFFFFF).astype(np.uint32)
    return np.ascontiguousarray(a[0]), np.ascontiguousarray(a[1])


def seed_spans_rule(seq_len, ref_len, seed_rows, min_hits=SEED_MIN_HITS, pad=SPAN_PAD, pad_shift=SPAN_PAD_SHIFT):
    """cw_seed_spans' rule on the host (numpy, 64-bit): per sequence of length seq_len on a reference of ref_len, with its seed row (STATUS, HITS, DIAG, ..),
    (lo, hi) = (clamp(DIAG - P, 0, n), clamp(DIAG + SEED_SPAN + m + P, 0, n)), P = pad + (m >> pad_shift), where the row is FWD / REV with HITS >= min_hits;
    (0, 0) elsewhere."""
    m, n = np.asarray(seq_len, np.int64), np.asarray(ref_len, np.int64)
    rows = np.asarray(seed_rows, np.int64).reshape(-1, SEED_ROW)
    placed = (rows[:, SEED_STATUS] <= STRAND_REV) & (rows[:, SEED_STATUS] >= STRAND_FWD) & (rows[:, SEED_HITS] >= int(min_hits))
    P = int(pad) + (m >> int(pad_shift))
    lo = np.clip(rows[:, SEED_DIAG] - P, 0, n)
    hi = np.clip(rows[:, SEED_DIAG] + SEED_SPAN + m + P, 0, n)
    return np.where(placed, lo, 0).astype(np.uint32), np.where(placed, hi, 0).astype(np.uint32)


def _as_batch(groups):
    """`groups` as the operators take them: a HostBatch as it is, a list of lists of ACGT strings packed."""
    return groups if isinstance(groups, HostBatch) else pack_piles(groups)


def _result_struct(r):
    return Result(
        _ptr(r.cons), _ptr(r.cons_off), _ptr(r.cons_len), _ptr(r.status),
        _ptr(r.solid) if r.solid is not None else None,
        _ptr(r.solid_off) if r.solid is not None else None,
        _ptr(r.solid_len) if r.solid is not None else None,
    )


class Engine:
    """One engine per process per GPU (cw_create / cw_destroy)."""

    def __init__(self, params, device=0):
        self.lib = load_library()
        self.params = params
        self.device = device
        self.handle = C.c_void_p()
        _check(self.lib, self.lib.cw_create(C.byref(params), device, C.byref(self.handle)), "cw_create")

    def close(self):
        if self.handle:
            self.lib.cw_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, batch, want_solid=True):
        """Host buffers in, host buffers out (cw_run).  Windows that overflow a capacity carry WIN_OVERFLOW."""
        res = alloc_results(batch, want_solid, self.params.solid, self.params.k)
        b = batch.c_struct()
        r = _result_struct(res)
        _check(self.lib, self.lib.cw_run(self.handle, C.byref(b), C.byref(r)), "cw_run", allow_capacity=True)
        return res

    def submit(self, batch, res):
        """cw_submit: enqueue a host batch (HostBatch + WindowResults from alloc_results); returns (ticket, keep-alive).  Up to two in flight."""
        b = batch.c_struct()
        r = _result_struct(res)
        t = C.c_int(-1)
        _check(self.lib, self.lib.cw_submit(self.handle, C.byref(b), C.byref(r), C.byref(t)), "cw_submit")
        return t.value, (batch, res, b, r)

    def wait(self, ticket):
        """cw_wait: blocks until the batch of `ticket` is done and its WindowResults are filled."""
        _check(self.lib, self.lib.cw_wait(self.handle, ticket), "cw_wait", allow_capacity=True)

    def run_device(self, batch_struct, result_struct, stream=None):
        _check(self.lib, self.lib.cw_run_device(self.handle, C.byref(batch_struct), C.byref(result_struct), stream), "cw_run_device")

    def poa(self, groups, slot_bytes=None):
        """Only the POA (cw_poa_run): `groups` is a list of lists of ACGT strings (or a HostBatch of them); every group's sequences are aligned in the order
        given -- zero-length ones skipped, the first max_msa others taken -- and its consensus returned: WindowResults with consensus(g) and status[g]
        (WIN_CONSENSUS, or WIN_OVERFLOW for a group that stopped).  slot_bytes: the consensus slot, one number or one per group (default: poa_slot_bytes
        of the group's longest sequence, what the window path reserves for a segment)."""
        batch = _as_batch(groups)
        res = alloc_poa_results(batch, slot_bytes)
        b = batch.c_struct()
        r = _result_struct(res)
        _check(self.lib, self.lib.cw_poa_run(self.handle, C.byref(b), C.byref(r)), "cw_poa_run", allow_capacity=True)
        return res

    def poa_device(self, batch_struct, result_struct, stream=None):
        """cw_poa_run_device: as run_device, device pointers in both structs (the result's solid fields NULL), asynchronous on `stream`."""
        _check(self.lib, self.lib.cw_poa_run_device(self.handle, C.byref(batch_struct), C.byref(result_struct), stream), "cw_poa_run_device")

    def _run_spans(self, name, batch, spans, head, tail=()):
        """The host form `name` (cw_sw_run, ..) on (*head, *tail) -- or, with `spans`, its span form (cw_sw_span_run, ..) with the SwSpans of span_arrays()
        between the two.  Returns what it returned: 0, or -4 when a pair stopped."""
        mid = ()
        if spans is not None:
            lo, hi = span_arrays(spans, len(batch.seq_len))
            name, mid = name[: -len("run")] + "span_run", (C.byref(SwSpans(_ptr(lo), _ptr(hi))),)
        return _check(self.lib, getattr(self.lib, name)(self.handle, *head, *mid, *tail), name, allow_capacity=True)

    def sw(self, groups, want_indels=False, spans=None):
        """Only the local alignment (cw_sw_run): `groups` is a list of lists of ACGT strings (or a HostBatch of them); every group's first sequence is its
        reference, every other one a query aligned locally against it.  Returns SwRows: .rows is (n_seqs, SW_ROW) int32 -- score, ref_begin, ref_end,
        query_begin, query_end (inclusive, 0-based; ends -1 when nothing aligns), ins, del (0 unless want_indels), status (SW_ALIGNED, SW_NO_INDELS, SW_STOP
        for a pair beyond SW_QMAX / SW_RMAX, SW_IS_REF for the reference's own row) -- and .row(group, member) finds a row; .rc is cw_sw_run's return value
        (0, or -4 when a pair stopped).
        spans (here and in sw_path(), pileup(), sw_cut()): a pair of per-sequence arrays (lo, hi), or one (n_seqs, 2) array -- query s is aligned against
        reference columns [lo[s], hi[s]) only (cw_sw_span_run and its kin): the result of the run on reference[lo:hi] in the whole reference's coordinates,
        an empty span the row of an empty reference; SW_STOP then for a span, not a reference, of more than SW_RMAX columns.  None: every column, as ever."""
        batch = _as_batch(groups)
        rows = np.zeros((len(batch.seq_len), SW_ROW), np.int32)
        b = batch.c_struct()
        rc = self._run_spans("cw_sw_run", batch, spans, (C.byref(b), _ptr(rows)), (SW_WANT_INDELS if want_indels else 0,))
        return SwRows(rows, batch.win_first_seq, rc)

    def sw_device(self, batch_struct, rows_ptr, flags=0, stream=None):
        """cw_sw_run_device: device pointers in the batch struct, `rows_ptr` a device array of n_seqs * SW_ROW int32; asynchronous on `stream`."""
        _check(self.lib, self.lib.cw_sw_run_device(self.handle, C.byref(batch_struct), rows_ptr, flags, stream), "cw_sw_run_device")

    def sw_span_device(self, batch_struct, rows_ptr, spans_struct, flags=0, stream=None):
        """cw_sw_span_run_device: sw_device() with `spans_struct` (SwSpans, device arrays of n_seqs uint32 each)."""
        _check(self.lib, self.lib.cw_sw_span_run_device(self.handle, C.byref(batch_struct), rows_ptr, C.byref(spans_struct), flags, stream), "cw_sw_span_run_device")

    def sw_path(self, groups, eqx=False, slot_ops=None, spans=None):
        """The local alignment with its path (cw_sw_path_run): `groups` as for sw().  Returns SwPathRows: the rows of sw() with ins / del always filled in,
        .n_ops, .ops(group, member) and .cigar(group, member).  Statuses beyond sw()'s: SW_NO_PATH (the traceback's directions outgrow a wave's scratch),
        SW_PATH_OPEN, SW_PATH_SLOT (the ops outgrow the slot: n_ops is the number needed).  slot_ops: ops a sequence's slot holds, one number or one per
        sequence (default: sw_ops_bound of the sequence and its group's reference, which every path fits)."""
        batch = _as_batch(groups)
        S = len(batch.seq_len)
        if slot_ops is None:
            wfs = np.asarray(batch.win_first_seq, np.int64)
            ref_of = np.repeat(wfs[:-1], np.diff(wfs))
            lens = np.asarray(batch.seq_len, np.int64)
            slot_ops = lens + lens[ref_of] if S else np.zeros(0, np.int64)
        ops_off = np.zeros(S + 1, np.uint64)
        ops_off[1:] = np.cumsum(np.broadcast_to(np.asarray(slot_ops, np.int64), (S,)))
        ops_buf = np.zeros(max(int(ops_off[-1]), 1), np.uint32)
        n_ops = np.zeros(max(S, 1), np.uint32)
        rows = np.zeros((S, SW_ROW), np.int32)
        b = batch.c_struct()
        paths = SwPaths(_ptr(ops_buf), _ptr(ops_off), _ptr(n_ops))
        rc = self._run_spans("cw_sw_path_run", batch, spans, (C.byref(b), _ptr(rows), C.byref(paths)), (SW_PATH_EQX if eqx else 0,))
        return SwPathRows(rows, batch.win_first_seq, rc, n_ops[:S], ops_buf, ops_off)

    def sw_path_device(self, batch_struct, rows_ptr, paths_struct, flags=0, stream=None):
        """cw_sw_path_run_device: device pointers in the batch struct and in `paths_struct` (SwPaths), `rows_ptr` a device array of n_seqs * SW_ROW int32;
        asynchronous on `stream`."""
        _check(self.lib, self.lib.cw_sw_path_run_device(self.handle, C.byref(batch_struct), rows_ptr, C.byref(paths_struct), flags, stream), "cw_sw_path_run_device")

    def sw_path_span_device(self, batch_struct, rows_ptr, paths_struct, spans_struct, flags=0, stream=None):
        """cw_sw_path_span_run_device: sw_path_device() with `spans_struct` (SwSpans, device arrays)."""
        _check(self.lib, self.lib.cw_sw_path_span_run_device(self.handle, C.byref(batch_struct), rows_ptr, C.byref(paths_struct), C.byref(spans_struct), flags, stream),
               "cw_sw_path_span_run_device")

    def pileup(self, groups, into=None, spans=None):
        """The local alignments counted into their reference's columns (cw_pileup_run): `groups` as for sw().  Returns PileupRows: the rows of sw_path() --
        status SW_PILE_SLOT never occurs with the slots made here -- .counts(group), an (ref_len, PILE_COL) array of how many queries put an A, C, G, T on the
        column, skip it, insert after it, begin and end on it, and .coverage(group).  into: a PileupRows of an earlier call over the same references, or its
        counts_buf; the run then adds to those counts (PILE_ACCUMULATE) instead of beginning at zero -- for a reference whose queries are split over calls."""
        batch = _as_batch(groups)
        S = len(batch.seq_len)
        wfs = np.asarray(batch.win_first_seq, np.int64)
        lens = np.asarray(batch.seq_len, np.int64)
        width = np.zeros(S, np.int64)
        refs = wfs[:-1][np.diff(wfs) > 0]
        width[refs] = lens[refs]
        col_off = np.zeros(S + 1, np.uint64)
        col_off[1:] = np.cumsum(width)
        n_cols = int(col_off[-1])
        if into is None:
            counts = np.zeros((max(n_cols, 1), PILE_COL), np.uint32)
        else:
            counts = into.counts_buf if isinstance(into, PileupRows) else into
            if counts.dtype != np.uint32 or not counts.flags.c_contiguous or counts.shape != (max(n_cols, 1), PILE_COL):
                raise EngineError(f"pileup: `into` must be a C-contiguous uint32 array of shape {(max(n_cols, 1), PILE_COL)}: the columns of these references")
        rows = np.zeros((S, SW_ROW), np.int32)
        b = batch.c_struct()
        pile = Pileup(_ptr(counts), _ptr(col_off))
        rc = self._run_spans("cw_pileup_run", batch, spans, (C.byref(b), _ptr(rows), C.byref(pile)), (0 if into is None else PILE_ACCUMULATE,))
        return PileupRows(rows, batch.win_first_seq, rc, counts, col_off, batch.seq_len)

    def pileup_device(self, batch_struct, rows_ptr, pile_struct, flags=0, stream=None):
        """cw_pileup_run_device: device pointers in the batch struct and in `pile_struct` (Pileup; counts 16-byte aligned), `rows_ptr` a device array of
        n_seqs * SW_ROW int32; flags 0 or PILE_ACCUMULATE; asynchronous on `stream`."""
        _check(self.lib, self.lib.cw_pileup_run_device(self.handle, C.byref(batch_struct), rows_ptr, C.byref(pile_struct), flags, stream), "cw_pileup_run_device")

    def pileup_span_device(self, batch_struct, rows_ptr, pile_struct, spans_struct, flags=0, stream=None):
        """cw_pileup_span_run_device: pileup_device() with `spans_struct` (SwSpans, device arrays)."""
        _check(self.lib, self.lib.cw_pileup_span_run_device(self.handle, C.byref(batch_struct), rows_ptr, C.byref(pile_struct), C.byref(spans_struct), flags, stream),
               "cw_pileup_span_run_device")

    def poa_support(self, groups):
        """The support behind every consensus base: poa(groups), then every group's members piled against that group's consensus (packed on the host; two
        calls).  Returns (WindowResults of poa(), PileupRows): .counts(g)[j] are the counts on base j of consensus(g); member k of group g is member k + 1 of
        the pileup's group g.  A group without a consensus has no columns."""
        piles = groups.pile if isinstance(groups, HostBatch) else (lambda g: groups[g])
        n_groups = groups.n_windows if isinstance(groups, HostBatch) else len(groups)
        res = self.poa(groups)
        against = []
        for g in range(n_groups):
            against.append([res.consensus(g)] + list(piles(g)))
        return res, self.pileup(against)

    @staticmethod
    def _cut_slots(batch, window, slot_words=None):
        """cut_off of a batch: a query sw_cuts(its reference, window) words (or slot_words: one number, or one per sequence), a reference none."""
        S = len(batch.seq_len)
        wfs = np.asarray(batch.win_first_seq, np.int64)
        lens = np.asarray(batch.seq_len, np.int64)
        if slot_words is None:
            ref_of = np.repeat(wfs[:-1], np.diff(wfs))
            width = sw_cuts(lens[ref_of], window) if S else np.zeros(0, np.int64)
            width[wfs[:-1][np.diff(wfs) > 0]] = 0
        else:
            width = np.broadcast_to(np.asarray(slot_words, np.int64), (S,))
        cut_off = np.zeros(S + 1, np.uint64)
        cut_off[1:] = np.cumsum(width)
        return cut_off

    def sw_cut(self, groups, window, slot_words=None, spans=None):
        """The local alignments cut at their reference's window boundaries (cw_sw_cut_run): `groups` as for sw(), `window` >= 1 reference columns.  Returns
        SwCutRows: the rows of sw_path(), .cuts(group, member) -- word t the query position at reference column t * window -- and .pieces(group, member).
        Status SW_CUT_SLOT never occurs with the slots made here; slot_words (one number, or one per sequence) makes others."""
        batch = _as_batch(groups)
        S = len(batch.seq_len)
        cut_off = self._cut_slots(batch, max(int(window), 1), slot_words)
        cuts_buf = np.zeros(max(int(cut_off[-1]), 1), np.uint32)
        rows = np.zeros((S, SW_ROW), np.int32)
        b = batch.c_struct()
        cuts = SwCuts(_ptr(cuts_buf), _ptr(cut_off), window)
        rc = self._run_spans("cw_sw_cut_run", batch, spans, (C.byref(b), _ptr(rows), C.byref(cuts)))
        return SwCutRows(rows, batch.win_first_seq, rc, cuts_buf, cut_off, window, batch)

    def sw_cut_device(self, batch_struct, rows_ptr, cuts_struct, stream=None):
        """cw_sw_cut_run_device: device pointers in the batch struct and in `cuts_struct` (SwCuts), `rows_ptr` a device array of n_seqs * SW_ROW int32;
        asynchronous on `stream`."""
        _check(self.lib, self.lib.cw_sw_cut_run_device(self.handle, C.byref(batch_struct), rows_ptr, C.byref(cuts_struct), stream), "cw_sw_cut_run_device")

    def sw_cut_span_device(self, batch_struct, rows_ptr, cuts_struct, spans_struct, stream=None):
        """cw_sw_cut_span_run_device: sw_cut_device() with `spans_struct` (SwSpans, device arrays)."""
        _check(self.lib, self.lib.cw_sw_cut_span_run_device(self.handle, C.byref(batch_struct), rows_ptr, C.byref(cuts_struct), C.byref(spans_struct), stream),
               "cw_sw_cut_span_run_device")

    def cut_groups_device(self, batch_struct, rows_ptr, cuts_struct, grp_first=None, win_first_seq=None, seq_len=None, seq_word_off=None, bases=None,
                          group_cap=0, seq_cap=0, word_cap=0, stream=None):
        """cw_cut_groups_device: the POA batch of every (reference, window) behind a cut run, device pointers throughout.  Returns (rc, output groups,
        sequences, words): rc is 0, or -4 when the totals exceed the capacities -- with capacities of 0 that only sizes the output; one synchronisation."""
        ng, ns, nw = C.c_uint32(), C.c_uint32(), C.c_uint64()
        rc = self.lib.cw_cut_groups_device(self.handle, C.byref(batch_struct), rows_ptr, C.byref(cuts_struct), grp_first, win_first_seq, seq_len, seq_word_off, bases,
                                           group_cap, seq_cap, word_cap, C.byref(ng), C.byref(ns), C.byref(nw), stream)
        if rc not in (0, -4):
            _check(self.lib, rc, "cw_cut_groups_device")
        return rc, ng.value, ns.value, nw.value

    def strands(self, groups, k=0):
        """The strand vote (cw_strand_run): `groups` as for sw().  Per query the positions whose k-mer is among its reference's k-mers, as given and reverse-
        complemented (k = 0: STRAND_K; else STRAND_KMIN .. STRAND_KMAX).  Returns StrandRows: .strand(group, member) is STRAND_REV when the reverse hits are the
        more, else STRAND_FWD; STRAND_IS_REF for a reference, STRAND_NONE where no vote is possible; .hits(group, member) is (forward, reverse)."""
        batch = _as_batch(groups)
        S = len(batch.seq_len)
        strand = np.zeros(max(S, 1), np.uint8)
        hits = np.zeros((max(S, 1), 2), np.uint32)
        b = batch.c_struct()
        out = Strands(_ptr(strand), _ptr(hits), k)
        _check(self.lib, self.lib.cw_strand_run(self.handle, C.byref(b), C.byref(out)), "cw_strand_run")
        return StrandRows(strand[:S], hits[:S], batch.win_first_seq, k)

    def strand_device(self, batch_struct, strands_struct, stream=None):
        """cw_strand_run_device: device pointers in the batch struct and in `strands_struct` (Strands); asynchronous on `stream`."""
        _check(self.lib, self.lib.cw_strand_run_device(self.handle, C.byref(batch_struct), C.byref(strands_struct), stream), "cw_strand_run_device")

    def revcomp(self, groups, strand=None):
        """The batch with the flagged sequences reverse-complemented (cw_revcomp): `strand` is a uint8 value per sequence, of which STRAND_REV flags (a
        StrandRows' .strands, say); None reverses every sequence.  Returns a HostBatch with new `bases` and the arrays of the input otherwise."""
        batch = _as_batch(groups)
        S = len(batch.seq_len)
        if strand is not None:
            strand = np.ascontiguousarray(strand, np.uint8)
            if len(strand) != S:
                raise EngineError(f"revcomp: `strand` must have one value per sequence ({S})")
        out = np.zeros_like(batch.bases)
        b = batch.c_struct()
        _check(self.lib, self.lib.cw_revcomp(self.handle, C.byref(b), _ptr(strand) if strand is not None and S else None, _ptr(out)), "cw_revcomp")
        return HostBatch(batch.win_first_seq, batch.seq_len, batch.seq_word_off, out)

    def revcomp_device(self, batch_struct, strand_ptr, bases_out_ptr, stream=None):
        """cw_revcomp_device: device pointers in the batch struct, `strand_ptr` a device array of n_seqs bytes or None, `bases_out_ptr` a device array laid out as
        the batch's bases and not the same; asynchronous on `stream`."""
        _check(self.lib, self.lib.cw_revcomp_device(self.handle, C.byref(batch_struct), strand_ptr, bases_out_ptr, stream), "cw_revcomp_device")

    def orient(self, groups, k=0):
        """strands() and revcomp() of what it flags: (HostBatch in which every query has its reference's orientation, StrandRows).  Coordinates of what is
        computed from the oriented batch are the oriented query's: position i there is position len - 1 - i of a query that was turned round."""
        batch = _as_batch(groups)
        rows = self.strands(batch, k)
        return self.revcomp(batch, rows.strands), rows

    def seeds(self, groups, k=0):
        """Where every query lies on its reference (cw_seed_run): `groups` as for sw().  Per query, over the k-mers that occur exactly once in its reference
        (k = 0: STRAND_K; else STRAND_KMIN .. STRAND_KMAX), the 128 neighbouring diagonals that hold the most of them, as given and reverse-complemented.
        Returns SeedRows: .row(group, member) is (SEED_STATUS: STRAND_FWD / STRAND_REV of the better orientation, STRAND_IS_REF, STRAND_NONE; SEED_HITS: the
        hits in that window; SEED_DIAG: its lowest diagonal, reference position minus position in the oriented query; SEED_OTHER: the other orientation's
        best), .strands the status bytes, what revcomp() takes."""
        batch = _as_batch(groups)
        S = len(batch.seq_len)
        rows = np.zeros((max(S, 1), SEED_ROW), np.int32)
        strand = np.zeros(max(S, 1), np.uint8)
        b = batch.c_struct()
        out = Seeds(_ptr(rows), _ptr(strand), k)
        _check(self.lib, self.lib.cw_seed_run(self.handle, C.byref(b), C.byref(out)), "cw_seed_run")
        return SeedRows(rows[:S], strand[:S], batch.win_first_seq, k)

    def seed_device(self, batch_struct, seeds_struct, stream=None):
        """cw_seed_run_device: device pointers in the batch struct and in `seeds_struct` (Seeds); asynchronous on `stream`."""
        _check(self.lib, self.lib.cw_seed_run_device(self.handle, C.byref(batch_struct), C.byref(seeds_struct), stream), "cw_seed_run_device")

    def seed_spans(self, groups, seed_rows, min_hits=None, pad=SPAN_PAD, pad_shift=SPAN_PAD_SHIFT):
        """The reference columns every placed query can reach (cw_seed_spans): `groups` as for seeds(), `seed_rows` its SeedRows or their (n_seqs, SEED_ROW)
        array.  Returns (lo, hi), uint32 per sequence: what the `spans` of sw(), sw_path(), pileup() and sw_cut() take -- for the batch ORIENTED by the seed
        run's strands (revcomp(groups, rows.strands)), since SEED_DIAG is the oriented query's.  A reference, a query without a vote or with fewer than
        min_hits (None: SEED_MIN_HITS) gets (0, 0): it is not aligned at all."""
        batch = _as_batch(groups)
        S = len(batch.seq_len)
        rows = np.ascontiguousarray(seed_rows.rows if isinstance(seed_rows, SwRows) else seed_rows, np.int32).reshape(-1, SEED_ROW)
        if len(rows) != S:
            raise EngineError(f"seed_spans: `seed_rows` must have one row per sequence ({S})")
        lo, hi = np.zeros(max(S, 1), np.uint32), np.zeros(max(S, 1), np.uint32)
        b = batch.c_struct()
        _check(self.lib, self.lib.cw_seed_spans(self.handle, C.byref(b), _ptr(rows) if S else None, SEED_MIN_HITS if min_hits is None else int(min_hits), pad, pad_shift,
                                                _ptr(lo), _ptr(hi)), "cw_seed_spans")
        return lo[:S], hi[:S]

    def seed_spans_device(self, batch_struct, seed_rows_ptr, lo_ptr, hi_ptr, min_hits=None, pad=SPAN_PAD, pad_shift=SPAN_PAD_SHIFT, stream=None):
        """cw_seed_spans_device: device pointers in the batch struct, `seed_rows_ptr` a seed run's rows, `lo_ptr` / `hi_ptr` device arrays of n_seqs uint32;
        asynchronous on `stream`."""
        _check(self.lib, self.lib.cw_seed_spans_device(self.handle, C.byref(batch_struct), seed_rows_ptr, SEED_MIN_HITS if min_hits is None else int(min_hits), pad, pad_shift,
                                                       lo_ptr, hi_ptr, stream), "cw_seed_spans_device")

    @staticmethod
    def _tiles(reference, tile):
        tile = int(tile)
        if not 1 <= tile <= SW_RMAX:
            raise EngineError(f"tile must be 1 .. {SW_RMAX} bases")
        return [reference[a : a + tile] for a in range(0, len(reference), tile)]

    def place(self, reference, reads, tile=8192, k=0, min_hits=None):
        """Every read of `reads` (ACGT strings, either strand, any order) placed on `reference`, a string of any length: the reference is cut into tiles of
        `tile` bases (at most SW_RMAX; the last one shorter), one group per tile holds the tile and ALL reads -- the reads' words are packed once and shared
        by the groups -- and one cw_seed_run votes every (read, tile) pair: O(tiles x reads) votes of O(read + tile) each.  Per read the tile with the most
        hits wins, ties to the lowest tile.  Returns a list with one Placement(strand, position = tile start + SEED_DIAG, hits, other) per read, or None where
        its best hits are below min_hits.
        min_hits=None is SEED_MIN_HITS = 14, twice a measured chance level: over the 45 unrelated random pairs of tests/test_seed_cpu.py -- random reads of
        300 to 5 000 bases against random tiles of up to 8 192 bases, and 32 768 random bases against 16 383 -- the plain reference's largest SEED_HITS at the
        default k = 11 is 7 (1 at k = 15), while its planted reads of 300 to 5 000 bases at 10 - 12 % errors have 104 or more (46 at k = 15).  A random k-mer
        is four times rarer with every base of k, so the default holds from k = SEED_MIN_K = 11 up.  Below it does not (46 at k = 8): EngineError unless
        min_hits is given."""
        tiles = self._tiles(reference, tile)
        reads = list(reads)
        if min_hits is None and 0 < int(k) < SEED_MIN_K:
            raise EngineError(f"place: the default min_hits is measured for k >= {SEED_MIN_K}; give min_hits with k = {k}")
        T, R = len(tiles), len(reads)
        if T == 0 or R == 0:
            return [None] * R
        if T > self.max_batch_windows():
            raise EngineError(f"place: {T} tiles exceed the {self.max_batch_windows()} groups of a run; use a longer tile")
        once = pack_piles([tiles + reads])  # every sequence packed once; group g is tile g and the reads' entries again
        pick = np.concatenate([np.concatenate([[g], T + np.arange(R)]) for g in range(T)]).astype(np.int64)
        batch = HostBatch(np.arange(T + 1, dtype=np.uint32) * np.uint32(R + 1), once.seq_len[pick], once.seq_word_off[pick], once.bases)
        rows = self.seeds(batch, k).rows.reshape(T, R + 1, SEED_ROW)[:, 1:, :]
        voted = rows[:, :, SEED_STATUS] <= STRAND_REV
        best = np.argmax(np.where(voted, rows[:, :, SEED_HITS], -1), axis=0)  # (the first of equal maxima: the lowest tile)
        floor = SEED_MIN_HITS if min_hits is None else int(min_hits)
        out = []
        for r in range(R):
            t = int(best[r])
            status, hits, diag, other = (int(v) for v in rows[t, r])
            out.append(Placement(status, t * int(tile) + diag, hits, other) if voted[t, r] and hits >= floor else None)
        return out

    def locate_index(self, reference, k=0):
        """The device index of `reference`, a string of up to LOCATE_RMAX bases, for locate_rows() and locate(): the reference packed and uploaded, a table of
        cw_locate_table_words(len) words, and cw_locate_build_device over both.  k = 0 is LOCATE_K = 15, else STRAND_KMIN .. STRAND_KMAX.  Build once, look any
        number of batches up.  Returns a LocateIndex, which holds the device memory."""
        import torch

        n = len(reference)
        words = int(self.lib.cw_locate_table_words(n))
        if words == 0:
            raise EngineError(f"locate_index: a reference has at most {LOCATE_RMAX} bases")
        dev = torch.device("cuda", self.device)
        packed = pack_piles([[reference]]).bases
        t_bases = torch.from_numpy(np.concatenate([packed, np.zeros(1, np.uint32)]).view(np.int32)).to(dev)
        index = LocateIndex(n, int(k), t_bases, torch.empty(words, dtype=torch.int32, device=dev))
        torch.cuda.synchronize(dev)  # the engine launches on its own stream
        ref = index.c_struct()
        _check(self.lib, self.lib.cw_locate_build_device(self.handle, C.byref(ref), None), "cw_locate_build_device")
        torch.cuda.synchronize(dev)
        return index

    def locate_rows(self, index, reads):
        """cw_locate_run_device of `reads` (ACGT strings, or a HostBatch whose grouping is ignored) against a LocateIndex: SeedRows as seeds() returns them, with
        one row per READ and no reference row -- .rows[s] is read s, .row(0, s) too."""
        import torch

        batch = reads if isinstance(reads, HostBatch) else pack_piles([list(reads)])
        S = len(batch.seq_len)
        one_group = np.array([0, S], np.uint32)
        if S == 0:
            return SeedRows(np.zeros((0, SEED_ROW), np.int32), np.zeros(0, np.uint8), one_group, index.k)
        dev = torch.device("cuda", self.device)

        def up(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

        t_len, t_off = up(batch.seq_len, np.int32), up(batch.seq_word_off, np.int64)
        t_bases = up(np.concatenate([batch.bases, np.zeros(1, np.uint32)]), np.int32)
        t_rows = torch.zeros(S * SEED_ROW, dtype=torch.int32, device=dev)
        t_strand = torch.zeros(S, dtype=torch.uint8, device=dev)
        b = Batch(0, S, len(batch.bases), None, t_len.data_ptr(), t_off.data_ptr(), t_bases.data_ptr())
        torch.cuda.synchronize(dev)
        self.locate_device(index.c_struct(), b, Seeds(t_rows.data_ptr(), t_strand.data_ptr(), 0))
        torch.cuda.synchronize(dev)
        return SeedRows(t_rows.cpu().numpy().reshape(S, SEED_ROW), t_strand.cpu().numpy(), one_group, index.k)

    def locate_device(self, ref_struct, batch_struct, seeds_struct, stream=None):
        """cw_locate_run_device: device pointers in `ref_struct` (LocateRef, built by cw_locate_build_device), in the reads' batch struct and in `seeds_struct`
        (Seeds); asynchronous on `stream`."""
        _check(self.lib, self.lib.cw_locate_run_device(self.handle, C.byref(ref_struct), C.byref(batch_struct), C.byref(seeds_struct), stream), "cw_locate_run_device")

    def locate_routes(self):
        """(reads of the LDS route, reads of the dense route) of the last locate run (cw_debug_locate_routes)."""
        out = np.zeros(2, np.uint32)
        _check(self.lib, self.lib.cw_debug_locate_routes(self.handle, _ptr(out)), "cw_debug_locate_routes")
        return int(out[0]), int(out[1])

    def locate(self, index_or_reference, reads, k=0, min_hits=None):
        """Every read of `reads` (ACGT strings, either strand, any order) placed on a reference of up to LOCATE_RMAX bases through ONE index of its unique k-mers
        (cw_locate_*): O(read) a read, whatever the reference's length, where place() costs O(tiles x reads) votes.  `index_or_reference` is a LocateIndex
        (its k holds; `k` is not read) or a string, indexed here with k (0 = LOCATE_K = 15).  Returns what place() returns: one
        Placement(strand, position = SEED_DIAG, hits, other) per read, or None where no vote is possible or the hits are below min_hits.
        This is not place()'s answer: there a k-mer counts when it is unique in its TILE, here when it is unique in the whole reference -- a stretch present
        twice, 40 000 bases apart, seeds nothing here and seeds in both tiles there.
        min_hits=None is LOCATE_MIN_HITS = 4, twice a measured chance level (tests/test_locate_cpu.py): over 24 unrelated random reads of 300 to 5 000 bases
        against a random reference of 70 000 bases, the largest the CPU test builds, the plain reference's largest SEED_HITS at the default k = 15 is 2 (6 at
        k = 11), while the 24 planted reads of that test at 10 - 12 % errors have 76 or more (138 at k = 11).  For longer references the figure is an
        extrapolation: chance hits grow with n m / 4^k, which at 4.6 Mbp and 5 000 bases is still 21 spread over 72 000 bins.  It holds from
        k = LOCATE_MIN_K = 15 up; below, EngineError unless min_hits is given."""
        reads = list(reads)
        given = isinstance(index_or_reference, LocateIndex)
        kk = index_or_reference.k if given else int(k)
        if min_hits is None and 0 < kk < LOCATE_MIN_K:
            raise EngineError(f"locate: the default min_hits is measured for k >= {LOCATE_MIN_K}; give min_hits with k = {kk}")
        if not reads:
            return []
        index = index_or_reference if given else self.locate_index(index_or_reference, kk)
        floor = LOCATE_MIN_HITS if min_hits is None else int(min_hits)
        out = []
        for status, hits, diag, other in self.locate_rows(index, reads).rows.tolist():
            out.append(Placement(status, diag, hits, other) if status <= STRAND_REV and hits >= floor else None)
        return out

    def overlap_index(self, reads, k=0, sample=OVL_SAMPLE, max_occ=0):
        """The device index of the read set `reads` (ACGT strings, or a HostBatch whose grouping is ignored) for overlap_rows(): the reads uploaded,
        cw_overlap_count_device, memory of cw_overlap_index_words(entries) words and cw_overlap_build_device.  k = 0 is OVL_K = 15, sample 0 .. 8 (0 = every
        k-mer), max_occ = 0 is OVL_MAX_OCC.  Build once, run any number of query ranges.  Returns an OverlapIndex, which holds the device memory."""
        import torch

        batch = reads if isinstance(reads, HostBatch) else pack_piles([list(reads)])
        S = len(batch.seq_len)
        dev = torch.device("cuda", self.device)

        def up(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

        t_len, t_off = up(batch.seq_len if S else np.zeros(1, np.uint32), np.int32), up(batch.seq_word_off if S else np.zeros(1, np.uint64), np.int64)
        t_bases = up(np.concatenate([batch.bases, np.zeros(1, np.uint32)]), np.int32)
        index = OverlapIndex(np.array(batch.seq_len, np.int64), len(batch.bases), int(k), int(sample), int(max_occ), 0, t_len, t_off, t_bases, None)
        torch.cuda.synchronize(dev)  # the engine launches on its own stream
        b, prm, n = index.batch(), OverlapParams(int(k), int(sample), int(max_occ), 1), C.c_uint64()
        _check(self.lib, self.lib.cw_overlap_count_device(self.handle, C.byref(b), C.byref(prm), C.byref(n), None), "cw_overlap_count_device")
        words = int(self.lib.cw_overlap_index_words(n.value))
        if words == 0:
            raise EngineError("overlap_index: more than 2^32 - 1 sampled k-mers; raise `sample`")
        index.n_entries, index.mem = int(n.value), torch.empty(words // 2 + 1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        ref = index.c_struct(1)
        _check(self.lib, self.lib.cw_overlap_build_device(self.handle, C.byref(b), C.byref(ref), None), "cw_overlap_build_device")
        torch.cuda.synchronize(dev)
        return index

    def overlap_device(self, index_struct, batch_struct, first, count, overlaps_struct, stream=None):
        """cw_overlap_run_device: device pointers in `index_struct` (OverlapIndexRef), the reads' batch struct and `overlaps_struct` (Overlaps); asynchronous
        on `stream`."""
        _check(self.lib, self.lib.cw_overlap_run_device(self.handle, C.byref(index_struct), C.byref(batch_struct), first, count, C.byref(overlaps_struct), stream),
               "cw_overlap_run_device")

    def overlap_routes(self):
        """(queries of the LDS route, queries of the dense route) of the last overlap run (cw_debug_overlap_routes)."""
        out = np.zeros(2, np.uint32)
        _check(self.lib, self.lib.cw_debug_overlap_routes(self.handle, _ptr(out)), "cw_debug_overlap_routes")
        return int(out[0]), int(out[1])

    def overlap_rows(self, index, first=0, count=None, min_hits=OVL_MIN_HITS, slots=32, grow=True):
        """cw_overlap_run_device of the queries first .. first + count - 1 (count=None: to the end) of an OverlapIndex: OverlapRows.  `slots` is the rows of
        every query's slot, or an array of them; when a query answers OVL_SLOT and `grow` holds, the run is repeated once with the slots the counts ask for."""
        import torch

        S = len(index.lengths)
        first = int(first)
        count = S - first if count is None else int(count)
        dev = torch.device("cuda", self.device)
        slot = np.full(count, slots, np.uint64) if np.isscalar(slots) else np.asarray(slots, np.uint64)
        while True:
            row_off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(slot, dtype=np.uint64)])
            t_off = torch.from_numpy(row_off.view(np.int64)).to(dev)
            t_rows = torch.zeros(max(int(row_off[-1]) * OVL_ROW, 1), dtype=torch.int32, device=dev)
            t_n = torch.zeros(max(count, 1), dtype=torch.int32, device=dev)
            t_status = torch.zeros(max(count, 1), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            self.overlap_device(index.c_struct(min_hits), index.batch(), first, count, Overlaps(t_rows.data_ptr(), t_off.data_ptr(), t_n.data_ptr(), t_status.data_ptr()))
            torch.cuda.synchronize(dev)
            n_rows, status = t_n.cpu().numpy().view(np.uint32)[:count], t_status.cpu().numpy()[:count]
            if grow and (status == OVL_SLOT).any():
                slot, grow = np.maximum(slot, n_rows.astype(np.uint64)), False
                continue
            return OverlapRows(t_rows.cpu().numpy()[: int(row_off[-1]) * OVL_ROW].reshape(-1, OVL_ROW), row_off, n_rows, status, first)

    def overlap_run_host(self, reads, k=0, sample=OVL_SAMPLE, max_occ=0, min_hits=OVL_MIN_HITS, slots=32):
        """cw_overlap_run, the host form, of every read: (rc, OverlapRows) -- rc is 0 or CW_E_CAPACITY (-4) when a query has OVL_SLOT or OVL_DENSE."""
        batch = reads if isinstance(reads, HostBatch) else pack_piles([list(reads)])
        S = len(batch.seq_len)
        slot = np.full(S, slots, np.uint64) if np.isscalar(slots) else np.asarray(slots, np.uint64)
        row_off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(slot, dtype=np.uint64)])
        rows, n_rows, status = np.zeros((int(row_off[-1]), OVL_ROW), np.int32), np.zeros(max(S, 1), np.uint32), np.zeros(max(S, 1), np.uint8)
        b = Batch(0, S, len(batch.bases), None, _ptr(batch.seq_len), _ptr(batch.seq_word_off), _ptr(batch.bases))
        prm, out = OverlapParams(int(k), int(sample), int(max_occ), int(min_hits)), Overlaps(_ptr(rows) if rows.size else _ptr(np.zeros(1, np.int32)), _ptr(row_off), _ptr(n_rows), _ptr(status))
        rc = _check(self.lib, self.lib.cw_overlap_run(self.handle, C.byref(b), C.byref(prm), C.byref(out)), "cw_overlap_run", allow_capacity=True)
        return rc, OverlapRows(rows, row_off, n_rows[:S], status[:S], 0)

    def overlaps(self, reads, k=0, sample=OVL_SAMPLE, max_occ=0, min_hits=None):
        """Per read of `reads` (ACGT strings, either strand, any order) the reads of the same set that overlap it: a list of Overlap, the most hits first
        (cw_overlap_*: one device index of every sampled k-mer of the set, one run).  `reads` may be an OverlapIndex (its k, sample and max_occ hold).
        min_hits=None is OVL_MIN_HITS = 2, twice a measured chance level (tests/test_overlap_cpu.py): on 120 reads of 1 500 to 5 000 bases at 10 - 12 % errors
        from a random genome of 30 000 bases, at k = 15 and sample = 3, the plain reference's largest HITS between reads whose true intervals lie 1 000 bases
        or more apart is 1, and every planted overlap of OVL_MIN_OVERLAP = 2 000 bases or more is reported with the right strand.  It holds from
        k = OVL_MIN_K = 15 up; below, EngineError unless min_hits is given.  A read outside k .. 32 768 bases has no overlaps and is nobody's."""
        given = isinstance(reads, OverlapIndex)
        kk = reads.k if given else int(k)
        if min_hits is None and 0 < kk < OVL_MIN_K:
            raise EngineError(f"overlaps: the default min_hits is measured for k >= {OVL_MIN_K}; give min_hits with k = {kk}")
        index = reads if given else self.overlap_index(reads, kk, sample, max_occ)
        if len(index.lengths) == 0:
            return []
        got = self.overlap_rows(index, 0, None, OVL_MIN_HITS if min_hits is None else int(min_hits))
        if (got.status >= OVL_SLOT).any():
            raise EngineError(f"overlaps: {int((got.status >= OVL_SLOT).sum())} reads vote for more distinct (target, strand, bin) keys than the run holds; raise sample or lower max_occ")
        return [[Overlap(*row) for row in got.of(j).tolist()] for j in range(len(index.lengths))]

    def overlaps_paf(self, reads, names, path, k=0, sample=OVL_SAMPLE, max_occ=0, min_hits=None):
        """overlaps() written as the PAF file cw_paf_open / cw_run_correction read: one line per row, a query's lines together and in row order -- query name,
        length, Q_START, Q_END + 1 (PAF ends are exclusive), + or -, target name, length, T_START, T_END + 1, residue matches = HITS, block length = the
        longer span, mapping quality 255.  `reads` are ACGT strings, a HostBatch or an OverlapIndex.  Returns the number of lines."""
        per = self.overlaps(reads, k, sample, max_occ, min_hits)
        lens = reads.lengths if isinstance(reads, OverlapIndex) else (reads.seq_len if isinstance(reads, HostBatch) else [len(r) for r in reads])
        return write_paf(path, names, lens, [[o.astuple() for o in rows] for rows in per])

    def polish_reads(self, reference, reads, window=500, tile=8192, k=0, min_hits=None, seeded=False, index=False):
        """`reference`, a contig of any length, polished from an unsorted bag of reads of either strand: place() the reads; every placed read, reverse-
        complemented when STRAND_REV, goes to every tile its footprint [position, position + length + SEED_SPAN) meets; polish() of those groups -- the tile
        first, its reads in the order given -- and the tiles' sequences joined.  `tile` must be a multiple of `window` (EngineError otherwise): windows then
        never straddle tiles, and the result is the contig's polish.  Returns one Polished: .sequence, .windows of all tiles in order, and .placements, a
        Placement or None per read.  The placing costs O(tiles x reads) votes (see place()); the polish aligns a read only against the tiles it lies on.
        seeded=True: place() as above -- the seed run keeps its tiles -- then ONE group, the whole contig and the placed reads, oriented, each confined to the
        span of reference columns its Placement.position gives by cw_seed_spans' rule (seed_spans_rule): polish(that group, spans=...).  No read is aligned
        twice or cut at a tile's edge, no tiles are joined, and `tile` need not be a multiple of `window`.  What the one group costs instead, unmeasured: every
        read's cut slot holds the windows of the WHOLE contig + 1 words, and cw_cut_groups_device looks at every read of the group for every window --
        O(windows x reads) words and tests, where the tiled polish has O(windows x reads of a tile).
        index=True: the placements come from locate() instead of place(), in both forms: one index of the whole contig, O(read) a read (k = 0 is LOCATE_K = 15,
        min_hits=None LOCATE_MIN_HITS; at most LOCATE_RMAX bases).  Everything after the placing is as above.  locate() is not place(): see there."""
        window, tile = int(window), int(tile)
        if window < 1 or (tile % window and not seeded):
            raise EngineError("polish_reads: tile must be a multiple of window")
        reads = list(reads)
        placed = self.locate(reference, reads, k, min_hits) if index else self.place(reference, reads, tile, k, min_hits)
        if seeded:
            if not reference:
                return Polished("", [], placements=placed)
            kept = [(q, p) for q, p in zip(reads, placed) if p is not None]
            group = [reference] + [_revcomp(q) if p.strand == STRAND_REV else q for q, p in kept]
            rows = np.zeros((len(group), SEED_ROW), np.int64)
            rows[0, SEED_STATUS] = STRAND_IS_REF
            for i, (q, p) in enumerate(kept):
                rows[i + 1] = (p.strand, p.hits, p.position, p.other)
            spans = seed_spans_rule([len(x) for x in group], len(reference), rows, min_hits=0)  # (place() has applied the threshold)
            done = self.polish([group], window, spans=spans)[0]
            return Polished(done.sequence, done.windows, placements=placed)
        groups = []
        for g, t in enumerate(self._tiles(reference, tile)):
            a = g * tile
            groups.append([t] + [_revcomp(q) if p.strand == STRAND_REV else q for q, p in zip(reads, placed)
                                 if p is not None and p.position < a + len(t) and p.position + len(q) + SEED_SPAN > a])
        done = self.polish(groups, window) if groups else []
        return Polished("".join(d.sequence for d in done), [w for d in done for w in d.windows], placements=placed)

    def polish(self, groups, window=500, orient=False, k=0, seeded=False, min_hits=None, spans=None):
        """Every group's reference (its first sequence) polished window by window from its other sequences, the reads: the reads are aligned and cut at the
        window boundaries (cw_sw_cut_run_device), every (reference, window) becomes a POA group of the window's columns and the pieces of the reads whose
        alignments span it (cw_cut_groups_device), the POA tiers give every group's consensus (cw_poa_run_device), and the consensuses of a reference's windows
        are joined in order.  Nothing but the result leaves the device.  The reference's columns are the backbone: one voice among the members, and base ties
        go to it; the first max_msa non-empty sequences of a group are aligned, the backbone included.  Returns a list of Polished, one per input group:
        .sequence and .windows (PolishWindow: members, status, kept_reference).  A window whose POA group stops keeps the reference's columns.  Raises
        EngineError when the windows of the batch exceed max_batch_windows(): split the references over calls.
        orient=True: the reads may be of either strand.  The uploaded batch goes through the strand vote (cw_strand_run_device, k as for strands()) and the
        reads it flags are reverse-complemented on the device (cw_revcomp_device) before the cut run; .strands of every Polished then holds its reads' strand
        values, the only extra that leaves the device.  Without it a read of the other strand aligns by chance and its pieces rarely span a window.
        seeded=True: the reads may be of either strand and need not all belong: the seed run (cw_seed_run_device, k as for seeds()) places every read on its
        reference, cw_seed_spans_device turns the rows into spans (min_hits=None: SEED_MIN_HITS, with place()'s guard for k below SEED_MIN_K), the reads
        are turned by the seed run's strand bytes (cw_revcomp_device) and the cut run aligns each inside its span only (cw_sw_cut_span_run_device): a read of
        m bases costs m x (m + a pad) cells, not m x reference, and a read the seed run could not place costs nothing.  .strands as under orient=True.  A
        reference of more than SW_RMAX bases gets STRAND_NONE from the seed run, so empty spans: it comes back unpolished -- polish_reads(seeded=True)
        places by tiles and takes any length.  seeded and orient together: EngineError.
        spans: explicit spans for the cut run, as for sw_cut(); the reads are aligned as given (not with seeded or orient)."""
        import torch

        if seeded and (orient or spans is not None):
            raise EngineError("polish: seeded=True takes neither orient=True nor spans")
        if orient and spans is not None:
            raise EngineError("polish: spans are the given reads' coordinates; orient them first")
        if seeded and min_hits is None and 0 < int(k) < SEED_MIN_K:
            raise EngineError(f"polish: the default min_hits is measured for k >= {SEED_MIN_K}; give min_hits with k = {k}")

        batch = _as_batch(groups)
        window = int(window)
        if window < 1:
            raise EngineError("polish: window must be at least 1")
        G, S = batch.n_windows, len(batch.seq_len)
        if S == 0:
            return [Polished("", []) for _ in range(G)]
        dev = torch.device("cuda", self.device)

        def up(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

        def down(t, dt):
            return t.cpu().numpy().view(dt)

        t_wfs, t_len, t_off = up(batch.win_first_seq, np.int32), up(batch.seq_len, np.int32), up(batch.seq_word_off, np.int64)
        t_bases = up(np.concatenate([batch.bases, np.zeros(1, np.uint32)]), np.int32)
        cut_off = self._cut_slots(batch, window)
        t_coff = up(cut_off, np.int64)
        t_cuts = torch.zeros(max(int(cut_off[-1]), 1), dtype=torch.int32, device=dev)
        t_rows = torch.zeros(S * SW_ROW, dtype=torch.int32, device=dev)
        t_grp = torch.zeros(G + 1, dtype=torch.int32, device=dev)
        b = Batch(G, S, len(batch.bases), t_wfs.data_ptr(), t_len.data_ptr(), t_off.data_ptr(), t_bases.data_ptr())
        cuts = SwCuts(t_cuts.data_ptr(), t_coff.data_ptr(), window)
        if orient or seeded:
            t_strand = torch.zeros(S, dtype=torch.uint8, device=dev)
            t_turned = torch.zeros_like(t_bases)
        if seeded:
            t_seed = torch.zeros(S * SEED_ROW, dtype=torch.int32, device=dev)
        if seeded or spans is not None:
            lo, hi = span_arrays(spans, S) if spans is not None else (np.zeros(S, np.uint32), np.zeros(S, np.uint32))
            t_lo, t_hi = up(lo, np.int32), up(hi, np.int32)
            dspans = SwSpans(t_lo.data_ptr(), t_hi.data_ptr())
        torch.cuda.synchronize(dev)  # the engine launches on its own stream: torch's copies and fills above must have landed
        read_strands = [None] * G
        if orient or seeded:  # the reads the vote flags turned round into a second `bases`: the batch the runs below see
            if seeded:
                self.seed_device(b, Seeds(t_seed.data_ptr(), t_strand.data_ptr(), k))
                self.seed_spans_device(b, t_seed.data_ptr(), t_lo.data_ptr(), t_hi.data_ptr(), min_hits)
            else:
                self.strand_device(b, Strands(t_strand.data_ptr(), None, k))
            self.revcomp_device(b, t_strand.data_ptr(), t_turned.data_ptr())
            b.bases = t_turned.data_ptr()
            wfs = np.asarray(batch.win_first_seq, np.int64)
            torch.cuda.synchronize(dev)
            strand = down(t_strand, np.uint8)
            read_strands = [[int(v) for v in strand[wfs[g] + 1 : wfs[g + 1]]] for g in range(G)]
        if seeded or spans is not None:
            self.sw_cut_span_device(b, t_rows.data_ptr(), cuts, dspans)
        else:
            self.sw_cut_device(b, t_rows.data_ptr(), cuts)
        _, ng, ns, nw = self.cut_groups_device(b, t_rows.data_ptr(), cuts)
        if ng > self.max_batch_windows():
            raise EngineError(f"polish: {ng} windows exceed the {self.max_batch_windows()} groups of a POA run; split the references over calls")
        o_wfs = torch.zeros(ng + 1, dtype=torch.int32, device=dev)
        o_len = torch.zeros(max(ns, 1), dtype=torch.int32, device=dev)
        o_off = torch.zeros(max(ns, 1), dtype=torch.int64, device=dev)
        o_bases = torch.zeros(max(nw, 1) + 1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        rc, ng, ns, nw = self.cut_groups_device(b, t_rows.data_ptr(), cuts, t_grp.data_ptr(), o_wfs.data_ptr(), o_len.data_ptr(), o_off.data_ptr(), o_bases.data_ptr(), ng, ns, nw)
        _check(self.lib, rc, "cw_cut_groups_device")
        torch.cuda.synchronize(dev)
        if ng == 0:
            return [Polished("", [], read_strands[g]) for g in range(G)]
        # the consensus slots: CW_POA_SLOT_BYTES of every group's longest member
        counts = (o_wfs[1:] - o_wfs[:-1]).to(torch.int64)
        gid = torch.repeat_interleave(torch.arange(ng, device=dev), counts)
        longest = torch.zeros(ng, dtype=torch.int64, device=dev).scatter_reduce_(0, gid, o_len[:ns].to(torch.int64), "amax", include_self=True)
        c_off = torch.zeros(ng + 1, dtype=torch.int64, device=dev)
        c_off[1:] = torch.cumsum(2 * longest + 2, 0)
        c_cons = torch.zeros(int(c_off[-1].item()), dtype=torch.uint8, device=dev)
        c_len = torch.zeros(ng, dtype=torch.int32, device=dev)
        c_stat = torch.full((ng,), 255, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        pb = Batch(ng, ns, nw, o_wfs.data_ptr(), o_len.data_ptr(), o_off.data_ptr(), o_bases.data_ptr())
        pr = Result(c_cons.data_ptr(), c_off.data_ptr(), c_len.data_ptr(), c_stat.data_ptr(), None, None, None)
        self.poa_device(pb, pr)
        torch.cuda.synchronize(dev)
        grp, members = down(t_grp, np.uint32), down(counts, np.int64) - 1
        cons, coff, clen, stat = down(c_cons, np.uint8), down(c_off, np.int64), down(c_len, np.uint32), down(c_stat, np.uint8)
        out = []
        for g in range(G):
            w0, w1 = int(grp[g]), int(grp[g + 1])
            ref = batch.pile(g)[0] if w1 > w0 else ""
            parts, wins = [], []
            for t, w in enumerate(range(w0, w1)):
                ok = int(stat[w]) == WIN_CONSENSUS
                parts.append(cons[int(coff[w]) : int(coff[w]) + int(clen[w])].tobytes().decode() if ok else ref[t * window : (t + 1) * window])
                wins.append(PolishWindow(int(members[w]), int(stat[w]), not ok))
            out.append(Polished("".join(parts), wins, read_strands[g]))
        return out

    def extract_piles(self, reads, overlaps, jobs, k):
        """Device-side getAlignmentWindowsSequences (cw_extract_piles_device).  `reads` is a HostBatch-like packing of the read
        set (one "window" holding every read), `overlaps` an (n,6) uint32 array (q_start, q_end, t_read, t_start, t_end, strand;
        ends inclusive), `jobs` an (m,5) uint32 array (tpl_read, q_beg, q_end, ovl_first, ovl_count).  Returns a HostBatch."""
        import torch

        dev = torch.device("cuda", self.device)

        def up(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

        t_len, t_off, t_bases = up(reads.seq_len, np.int32), up(reads.seq_word_off, np.int64), up(np.concatenate([reads.bases, np.zeros(1, np.uint32)]), np.int32)
        ov = np.ascontiguousarray(overlaps, np.uint32).reshape(-1, 6)
        jb = np.ascontiguousarray(jobs, np.uint32).reshape(-1, 5)
        t_ov = up(ov if len(ov) else np.zeros((1, 6), np.uint32), np.int32)
        t_jb = up(jb, np.int32)
        rs = ReadSet(len(reads.seq_len), t_len.data_ptr(), t_off.data_ptr(), t_bases.data_ptr())
        ns, nw = C.c_uint32(), C.c_uint64()
        rc = self.lib.cw_extract_piles_device(self.handle, C.byref(rs), t_ov.data_ptr(), len(ov), t_jb.data_ptr(), len(jb), k, None, None, None, None, 0, 0, C.byref(ns), C.byref(nw), None)
        if rc not in (0, -4):
            _check(self.lib, rc, "cw_extract_piles_device(size)")  # -4 here only says "now you know the sizes"; a real capacity error repeats below
        o_wfs = torch.zeros(len(jb) + 1, dtype=torch.int32, device=dev)
        o_len = torch.zeros(max(ns.value, 1), dtype=torch.int32, device=dev)
        o_off = torch.zeros(max(ns.value, 1), dtype=torch.int64, device=dev)
        o_bases = torch.zeros(max(nw.value, 1) + 1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)  # the engine launches on its own stream: torch's fills above must have landed
        _check(self.lib, self.lib.cw_extract_piles_device(self.handle, C.byref(rs), t_ov.data_ptr(), len(ov), t_jb.data_ptr(), len(jb), k, o_wfs.data_ptr(), o_len.data_ptr(),
                                                          o_off.data_ptr(), o_bases.data_ptr(), ns.value, nw.value, C.byref(ns), C.byref(nw), None), "cw_extract_piles_device")
        torch.cuda.synchronize(dev)
        return HostBatch(o_wfs.cpu().numpy().view(np.uint32), o_len.cpu().numpy().view(np.uint32)[: ns.value], o_off.cpu().numpy().view(np.uint64)[: ns.value],
                         o_bases.cpu().numpy().view(np.uint32)[: max(nw.value, 1)])

    def plan_results(self, batch, fill=0):
        """The result slots of a device-resident batch (cw_plan_results_device): (cons_off, solid_off, cons_total, solid_total), the two exclusive offset arrays
        of n_windows + 1 entries as uint64.  Only the batch's window and length arrays are read.  `fill`: what both arrays hold before the call (a test's
        sentinel: an entry the library did not write comes back as it)."""
        import torch

        dev = torch.device("cuda", self.device)

        def up(a, dt):
            a = np.ascontiguousarray(a)
            return torch.from_numpy((a if a.size else np.zeros(1, a.dtype)).view(dt)).to(dev)

        n = batch.n_windows
        t_wfs, t_len = up(batch.win_first_seq, np.int32), up(batch.seq_len, np.int32)
        o_cons, o_solid = (torch.full((n + 1,), int(np.uint64(fill).astype(np.int64)), dtype=torch.int64, device=dev) for _ in range(2))
        torch.cuda.synchronize(dev)  # the engine launches on its own stream: torch's fills above must have landed
        b = Batch(n, len(batch.seq_len), len(batch.bases), t_wfs.data_ptr(), t_len.data_ptr(), None, None)
        ct, st = C.c_uint64(), C.c_uint64()
        _check(self.lib, self.lib.cw_plan_results_device(self.handle, C.byref(b), o_cons.data_ptr(), o_solid.data_ptr(), C.byref(ct), C.byref(st), None), "cw_plan_results_device")
        torch.cuda.synchronize(dev)
        return o_cons.cpu().numpy().view(np.uint64), o_solid.cpu().numpy().view(np.uint64), ct.value, st.value

    def stitch(self, reads, jobs, win_pos, batch, results, window_size=500, window_overlap=50, do_trim=True, capacity=None):
        """Device-side alignConsensus + trimRead + dropRead (cw_stitch_device).  `reads`: HostBatch-like packing of the read set;
        `jobs`: (n,3) uint32 (read, win_first, win_count); `win_pos`: (W,2) uint32 window (beg,end); `batch`/`results`: the piles
        and what the engine returned for them; `capacity`: bytes of every read's out slot (default: twice the read + 1024).  Behind each slot
        lie STITCH_GUARD bytes that must come back as they were sent (AssertionError otherwise).  Returns [(corrected_read, status)]."""
        import torch

        dev = torch.device("cuda", self.device)

        def up(a, dt):
            a = np.ascontiguousarray(a)
            if a.size == 0:
                a = np.zeros(1, a.dtype)
            return torch.from_numpy(a.view(dt)).to(dev)

        jb = np.ascontiguousarray(jobs, np.uint32).reshape(-1, 3)
        n = len(jb)
        seq_len, seq_off = np.asarray(reads.seq_len), np.asarray(reads.seq_word_off)
        stride = 1
        if capacity is None:
            cap = 2 * seq_len[jb[:, 0]].astype(np.int64) + 1024
        else:
            # a slot's capacity is the distance to the next slot's offset (cw_stitch_device), so the guard behind a slot is a slot of its own: that of a job
            # without windows over an empty read appended to the read set, which writes nothing
            stride = 2
            seq_len, seq_off = np.concatenate([seq_len, np.zeros(1, seq_len.dtype)]), np.concatenate([seq_off, seq_off[-1:] if len(seq_off) else np.zeros(1, np.uint64)])
            both = np.zeros((2 * n, 3), np.uint32)
            both[0::2], both[1::2, 0] = jb, len(seq_len) - 1
            cap = np.full(2 * n, STITCH_GUARD, np.int64)
            cap[0::2] = np.ascontiguousarray(capacity, np.int64).reshape(n)
            jb = both
        t_len, t_off, t_bases = up(seq_len, np.int32), up(seq_off, np.int64), up(np.concatenate([reads.bases, np.zeros(1, np.uint32)]), np.int32)
        rs = ReadSet(len(seq_len), t_len.data_ptr(), t_off.data_ptr(), t_bases.data_ptr())
        b_wfs, b_len, b_off, b_bases = up(batch.win_first_seq, np.int32), up(batch.seq_len, np.int32), up(batch.seq_word_off, np.int64), up(np.concatenate([batch.bases, np.zeros(1, np.uint32)]), np.int32)
        bs = Batch(batch.n_windows, len(batch.seq_len), len(batch.bases), b_wfs.data_ptr(), b_len.data_ptr(), b_off.data_ptr(), b_bases.data_ptr())
        r = results
        r_cons, r_coff, r_clen, r_st = up(r.cons, np.uint8), up(r.cons_off, np.int64), up(r.cons_len, np.int32), up(r.status, np.uint8)
        r_sol, r_soff, r_slen = up(r.solid, np.int32), up(r.solid_off, np.int64), up(r.solid_len, np.int32)
        rstruct = Result(r_cons.data_ptr(), r_coff.data_ptr(), r_clen.data_ptr(), r_st.data_ptr(), r_sol.data_ptr(), r_soff.data_ptr(), r_slen.data_ptr())
        t_jb, t_pos = up(jb, np.int32), up(np.ascontiguousarray(win_pos, np.uint32).reshape(-1), np.int32)
        out_off = np.zeros(len(jb) + 1, np.uint64)
        out_off[1:] = np.cumsum(cap)
        t_ooff = up(out_off, np.int64)
        sent = np.zeros(int(out_off[-1]) + 1, np.uint8)
        for i in range(1, len(jb), stride) if stride == 2 else ():
            sent[int(out_off[i]) : int(out_off[i + 1])] = 0xA5
        t_out = torch.from_numpy(sent).to(dev)
        t_olen = torch.zeros(len(jb) + 1, dtype=torch.int32, device=dev)
        t_ost = torch.full((len(jb) + 1,), 255, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)  # the engine launches on its own stream: torch's fills above must have landed
        _check(self.lib, self.lib.cw_stitch_device(self.handle, C.byref(rs), t_jb.data_ptr(), len(jb), t_pos.data_ptr(), C.byref(bs), C.byref(rstruct), window_size, window_overlap,
                                                   int(bool(do_trim)), t_out.data_ptr(), t_ooff.data_ptr(), t_olen.data_ptr(), t_ost.data_ptr(), None), "cw_stitch_device")
        torch.cuda.synchronize(dev)
        self._stitch_shape = (int(batch.n_windows), len(jb), stride)
        out, olen, ost = t_out.cpu().numpy(), t_olen.cpu().numpy(), t_ost.cpu().numpy()
        for i in range(1, len(jb), stride) if stride == 2 else ():
            lo, hi = int(out_off[i]), int(out_off[i + 1])
            assert (out[lo:hi] == 0xA5).all() and olen[i] == 0 and ost[i] == 0, f"cw_stitch_device: the guard behind the slot of read {i // 2} was written"
        return [(out[int(out_off[i]) : int(out_off[i]) + int(olen[i])].tobytes().decode("latin-1"), int(ost[i])) for i in range(0, len(jb), stride)]

    def stitch_trace(self):
        """The last stitch call's 8 words per window (cw_debug_stitch_trace: al_pos, size_al, score, ref_begin, ref_end, query_begin, query_end, the length
        aligned; 0xFFFFFFFF where no alignment was tried) as an (n_windows, 8) uint32 array.  Needs CW_STITCH_TRACE set during the call, and the
        -DCW_TEST_AIDS library."""
        n_windows = self._stitch_shape[0]
        out = np.zeros((max(n_windows, 1), 8), np.uint32)
        self.lib.cw_debug_stitch_trace.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        _check(self.lib, self.lib.cw_debug_stitch_trace(self.handle, n_windows, _ptr(out)), "cw_debug_stitch_trace")
        return out[:n_windows]

    def stitch_route(self):
        """The last stitch call's route witness (cw_debug_stitch_route): (windows, reads) -- an (n_windows, STITCH_WIT_WORDS) uint32 array (word 0: STITCH_ROUTE
        bits, word 1: STITCH_BAND bits, then STITCH_FACTS) and the reads' STITCH_READ words -- or None where nothing was recorded: the product library, or a
        call without CW_STITCH_TRACE."""
        n_windows, n_jobs, stride = self._stitch_shape
        win, rd = np.zeros((max(n_windows, 1), STITCH_WIT_WORDS), np.uint32), np.zeros(max(n_jobs, 1), np.uint32)
        self.lib.cw_debug_stitch_route.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        self.lib.cw_debug_stitch_route.restype = C.c_int
        rc = self.lib.cw_debug_stitch_route(self.handle, n_windows, n_jobs, _ptr(win), _ptr(rd))
        if rc == 0:
            return None
        if rc < 0:
            _check(self.lib, rc, "cw_debug_stitch_route")
        return win[:n_windows], rd[:n_jobs:stride]

    def configure(self, max_template_len):
        """cw_configure: the longest template (window) this engine will see, before its first run -- templates beyond 1024 + k - 1 bases need a larger
        scratch plan and the chain kernel's long instance (up to 2048 + k - 1 bases)."""
        _check(self.lib, self.lib.cw_configure(self.handle, int(max_template_len)), "cw_configure")

    def max_batch_windows(self):
        """cw_max_batch_windows: the largest batch this engine accepts under its current configuration (at most CW_MAX_BATCH_WINDOWS)."""
        return int(self.lib.cw_max_batch_windows(self.handle))

    def idle(self):
        """cw_poll: True when the last run_device on this engine has completed (never blocks)."""
        rc = self.lib.cw_poll(self.handle)
        if rc < 0:
            _check(self.lib, rc, "cw_poll")
        return rc == 1

    def phase(self):
        """cw_poll as it is: 1 done / nothing launched, 2 running but in its tail, 0 running."""
        rc = self.lib.cw_poll(self.handle)
        if rc < 0:
            _check(self.lib, rc, "cw_poll")
        return rc

    def timings(self):
        ms = (C.c_float * 16)()
        names = (C.c_char_p * 16)()
        n = C.c_int()
        _check(self.lib, self.lib.cw_last_timings(self.handle, ms, names, 16, C.byref(n)), "cw_last_timings")
        return {names[i].decode(): float(ms[i]) for i in range(n.value)}

    def profile(self):
        c = np.zeros(30, np.uint32)  # n_tasks, n_members, 3 cursors, any_overflow, then n_tier / next_tier / n_over / next_over for the six tiers
        p = np.zeros(128, np.uint64)  # phase cycle totals (cw_device.h BatchCounters::prof)
        _check(self.lib, self.lib.cw_debug_profile(self.handle, _ptr(c), len(c), _ptr(p), len(p), None, None), "cw_debug_profile")
        return c, p

    def tier_x_counters(self):
        """Tier X's counters of the last run (cw_debug_tier_x): tasks tier G handed on, tasks aligned, tasks that outgrew tier X too
        (their windows stop on CW_WHY_POA), and the largest alignment it was asked for in int32 cells."""
        c = np.zeros(4, np.uint32)
        _check(self.lib, self.lib.cw_debug_tier_x(self.handle, _ptr(c)), "cw_debug_tier_x")
        return {"routed": int(c[0]), "done": int(c[1]), "stopped": int(c[2]), "max_cells": int(c[3])}

    def tier_q_counters(self):
        """Tier Q's two ranges in the last run (cw_debug_tier_q): `split`, the long entries at the head of its list (16 lanes a task); `short_done`, the short
        tasks behind them that the eight-lane loop finished; `short_handed_on`, those that outgrew it and went to tier S."""
        c = np.zeros(3, np.uint32)
        _check(self.lib, self.lib.cw_debug_tier_q(self.handle, _ptr(c)), "cw_debug_tier_q")
        return {"split": int(c[0]), "short_done": int(c[1]), "short_handed_on": int(c[2])}

    def tier_lists(self):
        """cw_debug_tier_lists: the routed lists of the last run and its task records -- (lists, tasks).  lists[name] for name in TIER_LISTS is (sorted, emitted):
        the list as the tier sort left it (plain task indices) and as it was emitted (task index | sort class << 24), the latter None unless the test-aid
        library ran with CW_KEEP_EMITTED set.  tasks[t] = (window, segment slot, n_members, longest member | mean member length << 16)."""
        n, ne, nt = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(self.lib, self.lib.cw_debug_tier_lists(self.handle, 0, None, None, 0, C.byref(n), C.byref(ne), None, 0, C.byref(nt)), "cw_debug_tier_lists")
        tasks = np.zeros((max(nt.value, 1), 4), np.uint32)
        lists = {}
        for name, li in TIER_LISTS.items():
            _check(self.lib, self.lib.cw_debug_tier_lists(self.handle, li, None, None, 0, C.byref(n), C.byref(ne), None, 0, C.byref(nt)), "cw_debug_tier_lists")
            srt, emi = np.zeros(max(n.value, 1), np.uint32), np.zeros(max(n.value, 1), np.uint32)
            _check(self.lib, self.lib.cw_debug_tier_lists(self.handle, li, _ptr(srt), _ptr(emi), len(srt), C.byref(n), C.byref(ne), _ptr(tasks), len(tasks), C.byref(nt)),
                   "cw_debug_tier_lists")
            lists[name] = (srt[: n.value], emi[: n.value] if ne.value else None)
        return lists, tasks[: nt.value]

    def solid_table(self, w):
        """cw_debug_solid_table: (keys, counts) of window w of the last run -- the index kernel's ascending solid k-mers and their exact pile-wide counts."""
        n = C.c_uint32()
        _check(self.lib, self.lib.cw_debug_solid_table(self.handle, w, None, None, 0, C.byref(n)), "cw_debug_solid_table")
        keys, counts = np.zeros(max(n.value, 1), np.uint32), np.zeros(max(n.value, 1), np.uint32)
        _check(self.lib, self.lib.cw_debug_solid_table(self.handle, w, _ptr(keys), _ptr(counts), len(keys), C.byref(n)), "cw_debug_solid_table")
        return keys[: n.value], counts[: n.value]

    def anchor_block(self, w):
        """cw_debug_anchor_block: window w's anchor block of the last run, as the index kernel handed it to the chain kernel (AnchorBlock)."""
        n = C.c_uint64()
        _check(self.lib, self.lib.cw_debug_anchor_block(self.handle, w, None, 0, C.byref(n)), "cw_debug_anchor_block")
        raw = np.zeros(n.value, np.uint8)
        _check(self.lib, self.lib.cw_debug_anchor_block(self.handle, w, _ptr(raw), len(raw), C.byref(n)), "cw_debug_anchor_block")
        return AnchorBlock(raw[: n.value])

    def index_route(self):
        """The INDEX_ROUTE bits of the last batch's windows, ORed (a window alone in its batch: its route).  Zero from the product library."""
        return int(self.profile()[1][INDEX_ROUTE_SLOT])

    def chain_route(self):
        """The CHAIN_ROUTE bits of the last batch's windows, ORed (a window alone in its batch: its route).  Zero from the product library."""
        return int(self.profile()[1][CHAIN_ROUTE_SLOT])

    def finish_route(self):
        """(FINISH_ROUTE bits of the last batch's windows, ORed; frames fin_link entered; fin_neighbours calls it made) -- a window alone in its batch: its
        own.  Zeros from the product library."""
        p = self.profile()[1]
        return int(p[FINISH_ROUTE_SLOT]), int(p[FINISH_ROUTE_SLOT + 1]), int(p[FINISH_ROUTE_SLOT + 2])

    def poa_route(self):
        """{tier: (POA_ROUTE bits, POA_RC2 bits)} of the last batch's POA tasks, ORed per slab tier S .. X (a group alone in its batch: its own route through
        every tier it visited).  Zeros from the product library."""
        p = self.profile()[1]
        out = {}
        for t, tier in enumerate(POA_TIERS):
            out[tier] = ((int(p[POA_ROUTE_SLOT + t // 2]) >> (32 * (t & 1))) & 0xFFFFFFFF, (int(p[POA_RC2_SLOT]) >> (8 * t)) & 0xFF)
        return out

    def segments(self, w):
        """cw_debug_segments: the chain kernel's segmentation of window w of the last run -- (n_segs, seg_len, tasks).  n_segs is chain anchors + 1, or 0 for a
        window without a chain; seg_len[i] the length of segment i (of a segment that became a POA task: of the tier's consensus); tasks a list, in the order
        of the task array, of (segment index, n_members, longest member, [(sequence counted from the window's first, start, length), ...])."""
        ns, nt, nm = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(self.lib, self.lib.cw_debug_segments(self.handle, w, C.byref(ns), None, 0, None, 0, C.byref(nt), None, 0, C.byref(nm)), "cw_debug_segments")
        seg_len, tasks, members = np.zeros(max(ns.value, 1), np.uint32), np.zeros((max(nt.value, 1), 4), np.uint32), np.zeros((max(nm.value, 1), 3), np.uint32)
        _check(self.lib, self.lib.cw_debug_segments(self.handle, w, C.byref(ns), _ptr(seg_len), len(seg_len), _ptr(tasks), len(tasks), C.byref(nt),
                                                    _ptr(members), len(members), C.byref(nm)), "cw_debug_segments")
        out = []
        for seg, n, mx, first in tasks[: nt.value].tolist():
            out.append((seg, n, mx, [tuple(m) for m in members[first : first + n].tolist()]))
        return ns.value, seg_len[: ns.value], out

    def win_info(self, n_windows):
        a = np.zeros((n_windows, 16), np.uint32)
        _check(self.lib, self.lib.cw_debug_win_info(self.handle, n_windows, _ptr(a)), "cw_debug_win_info")
        return a


def _operator(piles, merSize, commonKMers, minAnchors, solidThresh, maxMSA, device):
    eng = Engine(Params(merSize, solidThresh, commonKMers, minAnchors, maxMSA), device)
    try:
        res = eng.run(pack_piles(piles), want_solid=True)
    finally:
        eng.close()
    out = []
    for w in range(len(piles)):
        if res.status[w] == WIN_OVERFLOW:
            raise EngineError(f"window {w}: capacity overflow")
        out.append((res.consensus(w), res.solid_kmers(w).copy()))
    return out


def compute_consensus_read_correction(readId, piles, pilesPos, minSupport, merSize, commonKMers, minAnchors, solidThresh, windowSize, maxMSA, path="", device=0):
    """Batched mirror of computeConsensusReadCorrection (reference src/correctionMSA.cpp:29-49).

    ``piles`` is a list of window piles (template first).  As in the reference body, ``readId``, ``pilesPos``,
    ``minSupport``, ``windowSize`` and ``path`` do not influence the result.  Returns, per window,
    ``(consensus, solid_kmers)``: the case-annotated consensus and the ascending k-mers whose pile-wide count
    is >= solidThresh (what callers read from the reference's merCounts map).
    """
    return _operator(piles, merSize, commonKMers, minAnchors, solidThresh, maxMSA, device)


def compute_consensus_assembly_polishing(id, readId, piles, pilesPos, minSupport, merSize, commonKMers, minAnchors, solidThresh, windowSize, maxMSA, path="", nbThreads=1, device=0):
    """Batched mirror of computeConsensusAssemblyPolishing (reference src/correctionMSA.cpp:51-71); same body."""
    return _operator(piles, merSize, commonKMers, minAnchors, solidThresh, maxMSA, device)
