"""The span runs without a GPU (include/consent_amd.h cw_sw_span_run and its kin, cw_seed_spans): the header declares them and the library exports them, the
binding names them, a NULL engine is refused by all ten before a device is needed (NULL spans need an engine: tests/test_gpu_sw_span.py), the plans hold a pair's span, the plain reference of tests/sw_span_probes.py is what
the header says -- and the pad: CW_SPAN_PAD_SHIFT is the smallest pad of the three candidates under which EVERY planted read the project has aligns inside
its span as on its whole reference."""
import ctypes as C
import os
import re

import numpy as np

import consent_amd as ca
import seed_probes as sdp
import sw_op_probes as sp
import sw_path_probes as pp
import sw_span_probes as ss
from consent_amd import engine as en
from consent_amd.engine import SwCuts, SwPaths, SwSpans, Pileup, _ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
NEW_SYMBOLS = ("cw_sw_span_run", "cw_sw_span_run_device", "cw_sw_path_span_run", "cw_sw_path_span_run_device", "cw_pileup_span_run", "cw_pileup_span_run_device",
               "cw_sw_cut_span_run", "cw_sw_cut_span_run_device", "cw_seed_spans", "cw_seed_spans_device")


def header():
    return open(os.path.join(ROOT, "include", "consent_amd.h")).read()


def test_the_header_declares_the_ten_entry_points_and_the_library_exports_them():
    """tests/test_abi.py's rule for the new symbols: what the header declares (comments stripped, a name before a parenthesis) the library exports."""
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    declared = set(re.findall(r"\b(cw_[a-z0-9_]+)\s*\(", text))
    lib = ca.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared, f"include/consent_amd.h does not declare {name}"
        assert hasattr(lib, name), f"libconsent_amd.so does not export {name}"


def test_the_header_states_the_struct_the_constants_and_the_boundary():
    text = header()
    assert re.search(r"typedef struct cw_sw_spans \{\s*const uint32_t\*\s+ref_lo;[^}]*const uint32_t\*\s+ref_hi;[^}]*\} cw_sw_spans;", text)
    assert re.search(r"#define CW_SPAN_PAD 64u", text)
    assert int(re.search(r"#define CW_SPAN_PAD_SHIFT (\d+)u", text).group(1)) == en.SPAN_PAD_SHIFT and en.SPAN_PAD == ss.PAD == 64
    head = text.split("#ifndef CONSENT_AMD_H")[0]  # the head comment's list of entry points
    assert "cw_sw_span_run" in head and "cw_seed_spans" in head
    assert "ORIENTED" in text.split("typedef struct cw_sw_spans")[0].split("reference spans")[1]  # whose coordinates SEED_DIAG is in


def test_the_binding_names_them():
    for name in ("sw_span_device", "sw_path_span_device", "pileup_span_device", "sw_cut_span_device", "seed_spans", "seed_spans_device"):
        assert hasattr(ca.Engine, name), name
    import inspect

    for name in ("sw", "sw_path", "pileup", "sw_cut"):
        assert inspect.signature(getattr(ca.Engine, name)).parameters["spans"].default is None, name
    pol = inspect.signature(ca.Engine.polish).parameters
    assert pol["seeded"].default is False and pol["spans"].default is None and pol["min_hits"].default is None and pol["orient"].default is False
    assert inspect.signature(ca.Engine.polish_reads).parameters["seeded"].default is False
    assert [f[0] for f in SwSpans._fields_] == ["ref_lo", "ref_hi"]


def test_null_arguments_are_refused_without_a_device():
    """No engine: CW_E_INVALID from all ten before anything is read or written.  This shows the NULL engine only: the refusal of NULL spans and of a NULL
    member needs an engine, so a device, and is tests/test_gpu_sw_span.py's."""
    l = ca.load_library()
    hb = ca.pack_piles([["ACGTACGT", "ACGA"]])
    b = hb.c_struct()
    rows = np.full((2, 8), 77, np.int32)
    lo, hi = np.zeros(2, np.uint32), np.full(2, 8, np.uint32)
    spans = SwSpans(_ptr(lo), _ptr(hi))
    ops, off, n_ops = np.full(24, 77, np.uint32), np.array([0, 12, 24], np.uint64), np.full(2, 77, np.uint32)
    paths = SwPaths(_ptr(ops), _ptr(off), _ptr(n_ops))
    counts, col_off = np.full((8, 8), 77, np.uint32), np.array([0, 8, 8], np.uint64)
    pile = Pileup(_ptr(counts), _ptr(col_off))
    words, cut_off = np.full(8, 77, np.uint32), np.array([0, 0, 8], np.uint64)
    cuts = SwCuts(_ptr(words), _ptr(cut_off), 4)
    assert l.cw_sw_span_run(None, C.byref(b), _ptr(rows), C.byref(spans), 0) == E_INVALID
    assert l.cw_sw_span_run_device(None, C.byref(b), _ptr(rows), C.byref(spans), 0, None) == E_INVALID
    assert l.cw_sw_path_span_run(None, C.byref(b), _ptr(rows), C.byref(paths), C.byref(spans), 0) == E_INVALID
    assert l.cw_sw_path_span_run_device(None, C.byref(b), _ptr(rows), C.byref(paths), C.byref(spans), 0, None) == E_INVALID
    assert l.cw_pileup_span_run(None, C.byref(b), _ptr(rows), C.byref(pile), C.byref(spans), 0) == E_INVALID
    assert l.cw_pileup_span_run_device(None, C.byref(b), _ptr(rows), C.byref(pile), C.byref(spans), 0, None) == E_INVALID
    assert l.cw_sw_cut_span_run(None, C.byref(b), _ptr(rows), C.byref(cuts), C.byref(spans)) == E_INVALID
    assert l.cw_sw_cut_span_run_device(None, C.byref(b), _ptr(rows), C.byref(cuts), C.byref(spans), None) == E_INVALID
    seed_rows = np.zeros((2, 4), np.int32)
    out_lo, out_hi = np.full(2, 77, np.uint32), np.full(2, 77, np.uint32)
    assert l.cw_seed_spans(None, C.byref(b), _ptr(seed_rows), 14, 64, 4, _ptr(out_lo), _ptr(out_hi)) == E_INVALID
    assert l.cw_seed_spans_device(None, C.byref(b), _ptr(seed_rows), 14, 64, 4, _ptr(out_lo), _ptr(out_hi), None) == E_INVALID
    for a in (rows, ops, n_ops, counts, words, out_lo, out_hi):
        assert (a == 77).all()


def test_the_plans_hold_a_span_per_pair():
    """A pair's reference index, its span's first column and its span's columns, and its place in the order: four words a sequence before the wave scratch."""
    seqs = 100000
    out = np.zeros(10, np.uint64)
    assert ca.load_library().cw_debug_sw_plan(1000, seqs, seqs * 10, 256, 0, _ptr(out)) == 0
    assert int(out[1]) >= 4 * 4 * seqs
    out = np.zeros(12, np.uint64)
    assert ca.load_library().cw_debug_sw_path_plan(1000, seqs, seqs * 10, 256, 0, _ptr(out)) == 0
    assert int(out[1]) >= 4 * 4 * seqs


# ---- the rule of cw_seed_spans ------------------------------------------------------------------------------------------------------------------------------------

SEED_CASES = ss.SEED_CASES


def test_the_rule_of_cw_seed_spans_in_plain_integers():
    want = [(936 - 31, 1000 + 128 + 500 + 95), (0, -300 + 128 + 500 + 95), (0, 0), (2800 - 95, 3000), (3000, 3000), (0, 0), (905, 1723), (0, 0), (0, 0),
            (0, 16383), (0, 16383), (2 ** 31 - 900 - 107, 2 ** 31 - 1)]
    for case, w in zip(SEED_CASES, want):
        m, n, row, mh, pad, sh = case
        assert ss.seed_spans(m, n, row, mh, pad, sh) == w, case


def test_the_binding_s_numpy_rule_is_the_same():
    for m, n, row, mh, pad, sh in SEED_CASES:
        lo, hi = en.seed_spans_rule([m], [n], np.array([row], np.int64), mh, pad, sh)
        assert (int(lo[0]), int(hi[0])) == ss.seed_spans(m, n, row, mh, pad, sh), (m, n, row)
    lo, hi = ca.span_arrays(np.array([[1, 5], [2, 6], [3, 7]]), 3)
    assert lo.tolist() == [1, 2, 3] and hi.tolist() == [5, 6, 7] and lo.dtype == np.uint32
    lo, hi = ca.span_arrays(([1, 2, 3], [5, 6, 7]), 3)
    assert lo.tolist() == [1, 2, 3] and hi.tolist() == [5, 6, 7]


# ---- the plain reference ------------------------------------------------------------------------------------------------------------------------------------------

def test_a_whole_span_is_the_run_without_spans_and_an_empty_one_an_empty_reference():
    q, ref = sp.embedded(2, 200, 600)
    e = ss.span_expected(q, ref, 0, 600)
    assert e.row == pp.expected(q, ref)[0] and e.ops == pp.expected(q, ref)[2] and e.row[0] > 0
    assert ss.span_expected(q, ref, 0, 10 ** 9).row == e.row  # hi clamps to n
    import pileup_probes as pl
    import sw_cut_probes as cp

    assert np.array_equal(e.counts, pl.pileup(ref, [q])) and e.cuts(100) == cp.cuts(q, ref, 100)
    for lo, hi in ((300, 300), (400, 300), (600, 900), (10 ** 9, 5)):
        z = ss.span_expected(q, ref, lo, hi)
        assert z.row == (0, 0, -1, 0, -1, 0, 0, pp.ALIGNED) and z.ops == () and not z.counts.any() and z.cuts(100) == [0] * 7, (lo, hi)


def test_a_span_clips_the_alignment_and_counts_nothing_outside():
    ref = ss.ref_of(600)
    lo, hi = 203, 397
    q = ref[lo - 3 : hi + 3]
    e = ss.span_expected(q, ref, lo, hi)
    assert e.row[:5] == (2 * (hi - lo), lo, hi - 1, 3, 3 + hi - lo - 1)  # the three bases on either side would extend it; they do not take part
    assert not e.counts[:lo].any() and not e.counts[hi:].any() and (e.counts[lo:hi, :5].sum(axis=1) == 1).all()
    assert e.cuts(100) == [3, 3, 3, 3 + 300 - lo, 3 + hi - lo, 3 + hi - lo, 3 + hi - lo]  # boundaries 0, 100, .. 600 of the WHOLE reference
    assert ss.span_expected("A" * 40, "A" * 20000, 3, 3 + sp.RMAX + 1).row[7] == ss.STOP and ss.span_expected("A" * 40, "A" * 20000, 3, 3 + sp.RMAX).row[7] != ss.STOP


# ---- the pad ------------------------------------------------------------------------------------------------------------------------------------------------------

# reads tests/test_gpu_sw_span.py leaves out of its end-to-end comparison: (index in sw_span_probes.PAD_INPUTS, read) whose spanned row differs from the full one
# under the chosen pad.  The plain reference finds none.
LISTED = ()


def test_the_pad_shift_is_the_smallest_pad_under_which_every_placed_read_aligns_as_on_its_whole_reference():
    """pad = 64, pad_shift in 4, 3, 2 (the smallest pad first): per candidate the placed reads whose alignment inside the span differs from the alignment on
    the whole draft -- the oracle's seven numbers, which fix the path.  The header's macro and engine.SPAN_PAD_SHIFT are the first candidate without any."""
    table = {sh: ss.pad_mismatches(sh) for sh in ss.PAD_SHIFTS}
    for sh, (total, bad) in table.items():
        print(f"pad_shift = {sh}: {total} placed reads, {len(bad)} differ {bad[:8]}")
    assert all(total == 106 for total, _ in table.values())  # every planted read is placed: 3 x 24 + 12 + 12 + 10
    clean = [sh for sh in ss.PAD_SHIFTS if not table[sh][1]]
    assert clean, "no candidate works: the largest pad is used and the differing reads are LISTED"
    assert en.SPAN_PAD_SHIFT == clean[0]
    assert set(LISTED) == set(table[en.SPAN_PAD_SHIFT][1]) and len(LISTED) * 10 <= 106


def test_the_paths_of_the_contig_s_reads_are_equal_too():
    """What the comparison of numbers rests on, shown on the reads the end-to-end GPU test uses: equal rows, equal ops."""
    for i in (0, 1, 2):
        for q, draft, pos in ss.placed_reads(i):
            lo, hi = ss.seed_spans(len(q), len(draft), (sdp.FWD, 99, pos, 0), 14, ss.PAD, en.SPAN_PAD_SHIFT)
            e, full = ss.span_expected(q, draft, lo, hi), pp.expected(q, draft)
            assert e.row == full[0] and e.ops == full[2] and e.row[0] > 0
