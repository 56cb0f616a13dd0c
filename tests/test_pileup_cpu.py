"""The pileup run without a GPU (include/consent_amd.h cw_pileup_run / cw_pileup_run_device): the symbols and constants exist, a missing engine is refused before
the device is touched -- and the reference the GPU tests compare counts with (tests/pileup_probes.py: the ops of sw_path_probes.reference walked into columns) is
held to its design: every designed pair has exactly the intended ops, the counts obey the invariants any pileup obeys, and the two wrong readings of an insertion
change the answer on the insertion probes, so that an equal GPU answer means something."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import consent_amd as ca
import pileup_probes as pl
import sw_op_probes as sp
import sw_path_probes as pp
from consent_amd import engine as en
from consent_amd.engine import _ptr

E_INVALID = -1


def test_the_new_symbols_and_constants_are_exported():
    l = ca.load_library()
    for name in ("cw_pileup_run", "cw_pileup_run_device"):
        assert hasattr(l, name), name
    assert (ca.SW_PILE_SLOT, ca.PILE_ACCUMULATE) == (7, 8) == (pl.PILE_SLOT, pl.ACCUMULATE)
    assert (ca.PILE_A, ca.PILE_C, ca.PILE_G, ca.PILE_T, ca.PILE_DEL, ca.PILE_INS, ca.PILE_BEGIN, ca.PILE_END, ca.PILE_COL) == tuple(range(9))
    assert (pl.A, pl.C, pl.G, pl.T, pl.DEL, pl.INS, pl.BEGIN, pl.END, pl.COL) == tuple(range(9))
    assert [f[0] for f in ca.Pileup._fields_] == ["counts", "col_off"] and C.sizeof(ca.Pileup) == 16
    for name in ("pileup", "pileup_device", "poa_support"):
        assert hasattr(ca.Engine, name), name
    assert issubclass(ca.PileupRows, ca.SwRows)
    assert (ca.SW_NO_PATH, ca.SW_PATH_OPEN, ca.SW_PATH_SLOT, ca.SW_PATH_EQX) == (4, 5, 6, 4)  # the path run's are kept
    assert [pl.code(c) for c in "ACGTN"] == [0, 1, 2, 3, 3] == [pp.CODE[c] for c in "ACGT"] + [3]


def test_the_header_states_the_enum_the_flag_and_the_struct():
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "consent_amd.h")).read()
    assert re.search(r"enum \{ CW_PILE_A, CW_PILE_C, CW_PILE_G, CW_PILE_T, CW_PILE_DEL, CW_PILE_INS, CW_PILE_BEGIN, CW_PILE_END, CW_PILE_COL = 8 \};", text)
    assert re.search(r"enum \{ CW_SW_PILE_SLOT = 7 \};", text) and re.search(r"#define CW_PILE_ACCUMULATE 8u", text)
    assert re.search(r"typedef struct cw_pileup \{\s*uint32_t\* counts;[^}]*const uint64_t\* col_off;[^}]*\} cw_pileup;", text)
    assert re.search(r"int cw_pileup_run_device\(cw_engine\* e, const cw_batch\* groups, int32_t\* rows, const cw_pileup\* pile, uint32_t flags, void\* hip_stream\);", text)
    assert re.search(r"int cw_pileup_run\(cw_engine\* e, const cw_batch\* groups, int32_t\* rows, const cw_pileup\* pile, uint32_t flags\);", text)


def test_a_missing_engine_is_refused_without_a_device():
    """Without a device there is no engine, so both entry points end at their first check; the checks behind it (flags, NULL arguments, too many groups) need
    an engine and are tests/test_gpu_pileup.py's."""
    l = ca.load_library()
    hb = ca.pack_piles([["ACGTACGT", "ACGA"]])
    b = hb.c_struct()
    rows = np.full((2, 8), 77, np.int32)
    counts, off = np.full((8, 8), pl.FILL, np.uint32), np.array([0, 8, 8], np.uint64)
    pile = en.Pileup(_ptr(counts), _ptr(off))
    for flags in (0, pl.ACCUMULATE):
        assert l.cw_pileup_run(None, C.byref(b), _ptr(rows), C.byref(pile), flags) == E_INVALID
        assert l.cw_pileup_run_device(None, C.byref(b), _ptr(rows), C.byref(pile), flags, None) == E_INVALID
    assert (rows == 77).all() and (counts == pl.FILL).all()


# ---- the probes are as designed ------------------------------------------------------------------------------------------------------------------------------

def test_the_round_edge_probes_are_pure_m_paths_of_their_lengths():
    ref, queries = pl.round_edges()
    assert len(ref) == 600 and tuple(len(q) for q in queries) == pl.ROUND_LENS == (1, 2, 63, 64, 65, 128, 129)
    for q in queries:
        status, ins, dele, ops, _, _ = pp.reference(q, ref)
        assert (status, ins, dele, ops) == (pp.ALIGNED, 0, 0, ((len(q), pp.OP_M),)), len(q)
        score, rb, re_, qb, qe, _, _ = sp.oracle(q, ref)
        assert (score, re_ - rb + 1, qb, qe) == (2 * len(q), len(q), 0, len(q) - 1) and ref[rb : re_ + 1] == q


@pytest.mark.parametrize("deletion", [False, True])
@pytest.mark.parametrize("p", pl.RUN_P)
def test_the_run_start_probes_have_exactly_the_intended_ops(p, deletion):
    """[p M, 3 I, 80 M] (or 3 D): the run's first step is step p of the path, on either side of step 64, the first of the second round."""
    ref, (q,) = pl.run_start(p, deletion)
    status, ins, dele, ops, _, _ = pp.reference(q, ref)
    assert status == pp.ALIGNED and ops == pl.run_ops(p, deletion) == ((p, 0), (3, 2 if deletion else 1), (80, 0)), (p, deletion, ops)
    assert (ins, dele) == ((0, 3) if deletion else (3, 0))
    score, rb, re_, qb, qe, _, _ = sp.oracle(q, ref)
    assert (rb, qb, qe) == (40, 0, len(q) - 1) and re_ == 40 + p + 80 + (3 if deletion else 0) - 1
    counts = pl.pileup(ref, [q])
    run_col = 40 + p  # the first reference column after P
    if deletion:
        assert counts[run_col : run_col + 3, pl.DEL].tolist() == [1, 1, 1] and int(counts[:, pl.DEL].sum()) == 3 and int(counts[:, pl.INS].sum()) == 0
    else:
        assert int(counts[run_col - 1, pl.INS]) == 1 and int(counts[:, pl.INS].sum()) == 1 and int(counts[:, pl.DEL].sum()) == 0
    assert int(counts[40, pl.BEGIN]) == 1 and int(counts[re_, pl.END]) == 1
    assert (pl.RUN_P, pl.RUN_G, pl.RUN_S) == ((62, 63, 64, 65), 3, 80)


def test_the_class_probes_cover_every_launch_class_on_a_reference_beyond_lds():
    ref, queries = pl.classes()
    assert len(ref) == 3000 > sp.LDS_RMAX and tuple(len(q) for q in queries) == (600, 700, 2048, 2100)  # classes 0 (<= 640), 1, 1 (its last length), 2 (> 2048)
    spans = []
    for q in queries:
        assert pl.counts_pair(q, ref), len(q)
        _, rb, re_, _, _, ins, dele = sp.oracle(q, ref)
        assert ins + dele > 0 and re_ - rb + 1 > len(q) * 9 // 10  # a few errors, most of the query aligned
        spans.append((rb, re_))
    assert all(a[1] > b[0] for a, b in zip(spans, spans[1:]))  # on overlapping columns
    ref_d, deep = pl.deep()
    assert len(ref_d) == 600 and len(deep) == 300 and all(len(q) == 500 for q in deep)


def test_the_groups_of_pairs_that_count_nothing_are_as_designed():
    wide, poly, lone, none = pl.nothing_counts()
    assert pp.reference(wide[1], wide[0])[0] == pp.NO_PATH and sp.oracle(wide[1], wide[0])[0] > 0 and not pl.counts_pair(wide[1], wide[0])
    assert wide[2] == "" and pl.counts_pair(wide[3], wide[0]) and pp.reference(wide[3], wide[0])[3] == ((300, pp.OP_M),)
    assert sp.oracle(poly[1], poly[0])[0] == 0 and not pl.counts_pair(poly[1], poly[0])  # nothing aligns
    assert pl.counts_pair(poly[2], poly[0]) and pp.reference(poly[2], poly[0])[3] == ((40, pp.OP_M),) and poly[3] == ""
    assert len(lone) == 1 and len(lone[0]) == 90 and none == []
    counts = pl.pileup(wide[0], wide[1:])
    assert int(counts[:, pl.BEGIN].sum()) == 1 and int(pl.coverage(counts).sum()) == 300 and counts[1000:1300, : pl.T + 1].sum(axis=1).tolist() == [1] * 300


# ---- the reference obeys what any pileup obeys ----------------------------------------------------------------------------------------------------------------

def counted_rows(ref, queries):
    return [sp.oracle(q, ref) for q in queries if pl.counts_pair(q, ref)]


@pytest.mark.parametrize("name", list(pl.small_groups()) + ["deep, its first 20"])
def test_the_reference_pileup_obeys_the_invariants(name):
    if name in pl.small_groups():
        ref, queries = pl.small_groups()[name]
    else:
        ref, queries = pl.deep()[0], pl.deep()[1][:20]
    counts = pl.pileup(ref, queries)
    rows = counted_rows(ref, queries)
    assert counts.shape == (len(ref), 8) and counts.dtype == np.uint32 and len(rows) == len(queries)
    pl.check_invariants(counts, rows)


def test_the_invariants_notice_a_wrong_count():
    ref, queries = pl.run_start(64, True)
    counts, rows = pl.pileup(ref, queries), counted_rows(*pl.run_start(64, True))
    pl.check_invariants(counts, rows)
    for j, w in ((50, pl.A), (110, pl.DEL), (40, pl.BEGIN), (186, pl.END)):
        bad = counts.copy()
        bad[j, w] += 1
        with pytest.raises(AssertionError):
            pl.check_invariants(bad, rows)


# ---- an insertion counts once, on the column before it ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", pl.RUN_P)
def test_the_insertion_probes_tell_the_wrong_readings_of_an_insertion_apart(p):
    """A reference that puts an insertion on the column after it, or counts its bases, answers differently on the I probes -- and equally on the D probes, which
    hold no insertion: a GPU answer equal to the reference's on the I probes has the column and the event count right."""
    ref, queries = pl.run_start(p, False)
    right = pl.pileup(ref, queries)
    after, bases = pl.pileup(ref, queries, ins_after=True), pl.pileup(ref, queries, ins_bases=True)
    col = 40 + p - 1  # the last column consumed before the run
    assert int(right[col, pl.INS]) == 1 and int(right[col + 1, pl.INS]) == 0
    assert not np.array_equal(after, right) and int(after[col, pl.INS]) == 0 and int(after[col + 1, pl.INS]) == 1
    assert not np.array_equal(bases, right) and int(bases[col, pl.INS]) == 3
    for wrong in (after, bases):  # nothing else differs
        assert np.array_equal(np.delete(wrong, pl.INS, axis=1), np.delete(right, pl.INS, axis=1))
    ref_d, queries_d = pl.run_start(p, True)
    assert np.array_equal(pl.pileup(ref_d, queries_d, ins_after=True), pl.pileup(ref_d, queries_d))
    assert np.array_equal(pl.pileup(ref_d, queries_d, ins_bases=True), pl.pileup(ref_d, queries_d))


def test_the_noisy_probes_hold_insertion_runs_of_more_than_one_base_too():
    ref, queries = pl.deep()[0], pl.deep()[1][:20]
    right = pl.pileup(ref, queries)
    assert int(pl.pileup(ref, queries, ins_bases=True)[:, pl.INS].sum()) > int(right[:, pl.INS].sum()) > 0
    assert not np.array_equal(pl.pileup(ref, queries, ins_after=True), right)
