"""ctypes access to the CPU oracle (oracle/liboracle.so) and to the reference-built checker (oracle/_ref).
Test infrastructure only."""
import atexit
import ctypes as C
import hashlib
import json
import os

import numpy as np

from consent_amd.engine import Batch, Params, Result, WindowResults, alloc_results, _ptr, _result_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_O = None
_R = None


def oracle():
    global _O
    if _O is None:
        _O = C.CDLL(os.environ.get("CW_ORACLE_LIB") or os.path.join(ROOT, "oracle", "liboracle.so"))
        _O.cwo_run.argtypes = [C.POINTER(Params), C.POINTER(Batch), C.POINTER(Result), C.c_void_p, C.c_int]
    return _O


def ref():
    """The reference's own alignmentWindows/alignmentPiles/utils/reverseComplement TUs (None if not built)."""
    global _R
    p = os.path.join(ROOT, "oracle", "_ref", "libconsent_ref.so")
    if _R is None and os.path.exists(p):
        _R = C.CDLL(p)
    return _R


# Digests of the reference's answers, recorded from oracle/_ref (CW_RECORD_REF_DIGESTS=1 python -m pytest tests -m "not gpu" where it is built):
# the tests that pin the product or the oracle to the reference's own code check against them where oracle/_ref is absent.
REF_DIGESTS = os.path.join(ROOT, "tests", "golden", "ref_digests.json")
_DIGESTS = None
_RECORDED = {}


def _canon(x):
    if isinstance(x, (bytes, bytearray)):
        return {"hex": bytes(x).hex()}
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, np.generic):
        return x.item()
    if isinstance(x, (list, tuple)):
        return [_canon(v) for v in x]
    return x


def digest(x):
    return hashlib.sha256(json.dumps(_canon(x), sort_keys=True).encode()).hexdigest()


class RecordedAnswer:
    """The reference's answer known by its digest only: equal to a value whose digest is the same."""

    __hash__ = None

    def __init__(self, d):
        self.digest = d

    def __eq__(self, other):
        return digest(other) == self.digest

    def __ne__(self, other):
        return not self.__eq__(other)

    def __repr__(self):
        return f"<reference answer sha256:{self.digest[:16]}>"


def ref_answer(inputs, live, have_ref=None):
    """The reference's answer on `inputs` (JSON-like, everything that determines it: file contents, not paths).  With oracle/_ref built
    (have_ref() true; default: libconsent_ref.so loads) it is live(ref()), and its digest is recorded; without it, the digest committed under
    tests/golden/ (a RecordedAnswer).  Inputs never recorded skip."""
    import pytest

    key = digest(inputs)
    if (have_ref() if have_ref else ref() is not None):
        val = live(ref())
        _RECORDED[key] = digest(val)
        return val
    global _DIGESTS
    if _DIGESTS is None:
        _DIGESTS = json.load(open(REF_DIGESTS)) if os.path.exists(REF_DIGESTS) else {}
    if key not in _DIGESTS:
        pytest.skip("oracle/_ref not built and no recorded reference answer for these inputs")
    return RecordedAnswer(_DIGESTS[key])


@atexit.register
def _write_recorded():
    if os.environ.get("CW_RECORD_REF_DIGESTS") and _RECORDED:
        old = json.load(open(REF_DIGESTS)) if os.path.exists(REF_DIGESTS) else {}
        old.update(_RECORDED)
        with open(REF_DIGESTS, "w") as f:
            json.dump(old, f, indent=0, sort_keys=True)
            f.write("\n")


STAT_NAMES = ["kmers", "tpl_anchors", "chain_len", "pair_tests", "segments", "poa_segments", "alignments", "dp_cells", "max_nodes", "max_seg_len", "link_calls", "nbr_calls", "alignments_routed", "dp_cells_routed"]


def oracle_run(params, batch, want_solid=True, threads=1, lib=None):
    """`lib`: another build of the oracle (a ctypes library: a policy build), default the checker."""
    res = alloc_results(batch, want_solid, params.solid, params.k)
    b = batch.c_struct()
    r = _result_struct(res)
    stats = np.zeros(len(STAT_NAMES), np.uint64)
    o = lib or oracle()
    o.cwo_run.argtypes = [C.POINTER(Params), C.POINTER(Batch), C.POINTER(Result), C.c_void_p, C.c_int]
    rc = o.cwo_run(C.byref(params), C.byref(b), C.byref(r), _ptr(stats), threads)
    assert rc in (0, -4), rc
    return res, dict(zip(STAT_NAMES, (int(x) for x in stats)))


def oracle_counts(params, batch, w=0, lib=None):
    """cwo_counts: (keys, counts) of window w -- the oracle's pile-wide k-mer counts that reach params.solid, ascending by key.  `lib`: another build of
    the oracle (a ctypes library), default the checker."""
    o = lib or oracle()
    o.cwo_counts.argtypes = [C.POINTER(Params), C.POINTER(Batch), C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    b = batch.c_struct()
    n = C.c_uint32()
    s0, s1 = int(batch.win_first_seq[w]), int(batch.win_first_seq[w + 1])
    cap = int(batch.seq_len[s0:s1].astype(np.int64).sum()) + 1  # no more different k-mers than bases
    keys, counts = np.zeros(cap, np.uint64), np.zeros(cap, np.uint32)
    rc = o.cwo_counts(C.byref(params), C.byref(b), w, _ptr(keys), _ptr(counts), cap, C.byref(n))
    assert rc == 0 and n.value <= cap, (rc, n.value)
    return keys[: n.value], counts[: n.value]


def oracle_poa(seqs):
    arr = (C.c_char_p * len(seqs))(*[s.encode() for s in seqs])
    lens = np.array([len(s) for s in seqs], np.uint32)
    out = np.zeros(4 * max(lens.max(), 1) + 64, np.uint8)
    n = C.c_uint32()
    rc = oracle().cwo_poa(arr, _ptr(lens), len(seqs), _ptr(out), len(out), C.byref(n))
    assert rc == 0
    return out[: n.value].tobytes().decode()


def oracle_weight_polish(cons, counts, k, solid, weight=True, polish=True):
    keys = np.array(list(counts.keys()), np.uint64)
    cnts = np.array(list(counts.values()), np.uint32)
    out = np.zeros(4 * len(cons) + 256, np.uint8)
    n = C.c_uint32()
    rc = oracle().cwo_weight_polish(cons.encode(), len(cons), _ptr(keys), _ptr(cnts), len(keys), k, solid, int(weight), int(polish), _ptr(out), len(out), C.byref(n))
    assert rc == 0
    return out[: n.value].tobytes().decode()


def _ovl_array(ovls):
    return np.ascontiguousarray(np.array(ovls, np.uint32).reshape(-1, 8))


def window_positions(lib_fn, tpl_len, ovls, min_support, window_size, window_overlap):
    o = _ovl_array(ovls)
    out = np.zeros(2 * (tpl_len // max(1, window_size - window_overlap) + 8), np.uint32)
    n = lib_fn(tpl_len, _ptr(o), len(o), min_support, window_size, window_overlap, _ptr(out), len(out) // 2)
    assert n >= 0
    return [tuple(int(x) for x in out[2 * i : 2 * i + 2]) for i in range(n)]


def window_pile(lib_fn, ovls, tpl, targets, q_beg, q_end, k):
    o = _ovl_array(ovls)
    tg = (C.c_char_p * len(targets))(*[t.encode() for t in targets])
    tl = np.array([len(t) for t in targets], np.uint32)
    out = np.zeros((len(ovls) + 1) * (q_end - q_beg + 200) * 2 + 1024, np.uint8)
    lens = np.zeros(len(ovls) + 2, np.uint32)
    n = lib_fn(_ptr(o), len(o), tpl.encode(), len(tpl), tg, _ptr(tl), len(targets), q_beg, q_end, k, _ptr(out), len(out), _ptr(lens), len(lens))
    assert n >= 0, n
    res, off = [], 0
    for i in range(n):
        res.append(out[off : off + lens[i]].tobytes().decode())
        off += int(lens[i])
    return res
