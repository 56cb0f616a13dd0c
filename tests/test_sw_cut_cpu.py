"""The cut run and the polish without a GPU (include/consent_amd.h cw_sw_cut_run / cw_sw_cut_run_device / cw_cut_groups_device; Engine.polish): the symbols and
constants exist, a missing engine and a window of 0 are refused before the device is touched -- and the reference the GPU tests compare with
(tests/sw_cut_probes.py) is held to its design: the run-start probes cut where they were designed to, the two wrong readings of a boundary change the answer on
the insertion probes, the cut points obey what any cut points obey, and the composition of cuts, spanning members and the oracle's POA brings a draft nearer to
its truth where the touching-pieces rule takes it further away."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import consent_amd as ca
import pileup_probes as pl
import sw_cut_probes as cp
import sw_op_probes as sp
import sw_path_probes as pp
from consent_amd import engine as en
from consent_amd.engine import _ptr

E_INVALID = -1
NEW_FUNCTIONS = ("cw_sw_cut_run", "cw_sw_cut_run_device", "cw_cut_groups_device")


def header():
    return open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "consent_amd.h")).read()


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_header_declares_the_new_functions_the_struct_and_the_status():
    text = header()
    assert re.search(r"int cw_sw_cut_run_device\(cw_engine\* e, const cw_batch\* groups, int32_t\* rows, const cw_sw_cuts\* cuts, void\* hip_stream\);", text)
    assert re.search(r"int cw_sw_cut_run\(cw_engine\* e, const cw_batch\* groups, int32_t\* rows, const cw_sw_cuts\* cuts\);", text)
    assert re.search(r"int cw_cut_groups_device\(cw_engine\* e, const cw_batch\* groups, const int32_t\* rows, const cw_sw_cuts\* cuts,\s*uint32_t\* grp_first", text)
    assert re.search(r"typedef struct cw_sw_cuts \{\s*uint32_t\* cuts;[^}]*const uint64_t\* cut_off;[^}]*uint32_t window;[^}]*\} cw_sw_cuts;", text)
    assert re.search(r"enum \{ CW_SW_CUT_SLOT = 8 \};", text)
    assert re.search(r"#define CW_SW_CUTS\(ref_len, window\) \(\(ref_len\) / \(window\) \+ \(\(ref_len\) % \(window\) != 0u\) \+ 1u\)", text)
    for name in ("cw_sw_cut_run / cw_sw_cut_run_device", "cw_cut_groups_device"):  # the head comment's list of entry points
        assert name in text.split("#ifndef CONSENT_AMD_H")[0], name


def test_the_library_exports_them_and_the_binding_names_them():
    l = ca.load_library()
    for name in NEW_FUNCTIONS:
        assert hasattr(l, name), name
    assert ca.SW_CUT_SLOT == 8 == cp.CUT_SLOT and ca.SW_PILE_SLOT == 7
    assert [f[0] for f in ca.SwCuts._fields_] == ["cuts", "cut_off", "window"] and C.sizeof(ca.SwCuts) == 24
    for name in ("sw_cut", "sw_cut_device", "cut_groups_device", "polish"):
        assert hasattr(ca.Engine, name), name
    assert issubclass(ca.SwCutRows, ca.SwRows)
    for n, w in ((0, 1), (1, 1), (3000, 1), (3000, 64), (3000, 500), (3000, 4000), (128, 64), (129, 64), (16383, 0xFFFFFFFF)):
        assert int(ca.sw_cuts(n, w)) == cp.n_windows(n, w) + 1, (n, w)
    assert int(ca.sw_cuts(3000, 1)) == 3001


def test_a_missing_engine_and_a_window_of_none_are_refused_without_a_device():
    """Without a device there is no engine, so every entry point ends at its first check -- whatever the window."""
    l = ca.load_library()
    hb = ca.pack_piles([["ACGTACGT", "ACGA"]])
    b = hb.c_struct()
    rows = np.full((2, 8), 77, np.int32)
    words, off = np.full(8, cp.FILL, np.uint32), np.array([0, 0, 8], np.uint64)
    for window in (0, 4):
        cuts = en.SwCuts(_ptr(words), _ptr(off), window)
        assert l.cw_sw_cut_run(None, C.byref(b), _ptr(rows), C.byref(cuts)) == E_INVALID
        assert l.cw_sw_cut_run_device(None, C.byref(b), _ptr(rows), C.byref(cuts), None) == E_INVALID
        ng, ns, nw = C.c_uint32(7), C.c_uint32(7), C.c_uint64(7)
        assert l.cw_cut_groups_device(None, C.byref(b), _ptr(rows), C.byref(cuts), None, None, None, None, None, 0, 0, 0, C.byref(ng), C.byref(ns), C.byref(nw), None) == E_INVALID
    assert (rows == 77).all() and (words == cp.FILL).all()


# ---- the run-start probes cut where they were designed to --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", pl.RUN_P)
def test_an_insertion_before_a_boundary_belongs_to_the_window_before_it(p):
    """ref_begin = 40, so with W = 40 + p the boundary is the first column after the run: the three inserted bases lie before the cut."""
    ref, (q,) = pl.run_start(p, False)
    assert sp.oracle(q, ref)[1] == 40 and pp.reference(q, ref)[3] == pl.run_ops(p, False)
    right = cp.cuts(q, ref, 40 + p)
    print(f"p = {p}: insertion, W = {40 + p}: {right}")
    assert right == [0, p + 3, p + 83, p + 83] and right[1] == p + 3
    assert cp.pieces(q, ref, 40 + p) == [q[: p + 3], q[p + 3 :], ""]
    # the two wrong readings answer differently here
    next_window, after = cp.cuts(q, ref, 40 + p, ins_next=True), cp.cuts(q, ref, 40 + p, after_step=True)
    assert next_window == [0, p, p + 83, p + 83] and after == [0, p + 4, p + 83, p + 83]
    assert next_window != right != after


def test_the_example_values_of_the_first_probe():
    ref, (q,) = pl.run_start(62, False)
    assert cp.cuts(q, ref, 102) == [0, 65, 145, 145]
    ref, (q,) = pl.run_start(62, True)
    assert cp.cuts(q, ref, 102) == [0, 62, 142, 142]


@pytest.mark.parametrize("p", pl.RUN_P)
def test_a_deletion_over_a_boundary_cuts_at_the_base_that_follows_it(p):
    ref, (q,) = pl.run_start(p, True)
    assert sp.oracle(q, ref)[1] == 40 and pp.reference(q, ref)[3] == pl.run_ops(p, True)
    for k in range(3):  # the boundary on each of the three deleted columns
        W = 40 + p + k
        c = cp.cuts(q, ref, W)
        print(f"p = {p}: deletion, W = {W}: {c}")
        assert c[1] == p and c == [0, p, p + 80, p + 80], (p, k, c)
        assert cp.cuts(q, ref, W, ins_next=True) == c  # no insertion: that reading agrees
        assert cp.cuts(q, ref, W, after_step=True) == c  # a D step consumes no query base: so does this one
    # the first column after the deletion is an M step: there the second wrong reading shows
    W = 40 + p + 3
    assert cp.cuts(q, ref, W)[1] == p and cp.cuts(q, ref, W, after_step=True)[1] == p + 1


# ---- window sizes and boundaries at the ends ----------------------------------------------------------------------------------------------------------------------

def counted(query, ref):
    assert pl.counts_pair(query, ref)
    return sp.oracle(query, ref)


@pytest.mark.parametrize("W", [1, 64, 500, 4000])
def test_the_class_probes_at_every_window_size(W):
    ref, queries = pl.classes()
    for q in queries:
        row = counted(q, ref)
        c = cp.cuts(q, ref, W)
        assert len(c) == cp.n_windows(3000, W) + 1 == {1: 3001, 64: 48, 500: 7, 4000: 2}[W]
        cp.check_invariants(c, row)
        assert "".join(cp.pieces(q, ref, W)) == q[row[3] : row[4] + 1], "the pieces concatenate to the aligned query span"
        if W == 4000:
            assert c == [row[3], row[4] + 1]  # W >= n: one window
        if W == 1:  # a cut a column: piece t is what the path puts on column t -- nothing outside the span, at most an M base and the insertion behind it inside
            assert all(b - a == 0 for t, (a, b) in enumerate(zip(c, c[1:])) if t < row[1] or t > row[2])
            assert sum(b - a == 0 for t, (a, b) in enumerate(zip(c, c[1:])) if row[1] <= t <= row[2]) == row[6], "an empty piece a deleted column"


def test_a_boundary_on_ref_begin_on_ref_end_and_behind_it():
    ref, (q,) = pl.run_start(64, False)
    _, rb, re_, qb, qe, _, _ = counted(q, ref)
    assert (rb, re_, qb, qe) == (40, 183, 0, 146)
    on_begin = cp.cuts(q, ref, 40)  # boundaries 0, 40 = ref_begin, 80, .. 200: the one on ref_begin is query_begin, not a step's
    assert on_begin[:2] == [0, 0] and on_begin[2] == 40 and on_begin[-1] == qe + 1
    on_end = cp.cuts(q, ref, re_)  # boundaries 0, 183 = ref_end, 366 -> T = 2 (n = 224): the last column's step cuts, one base before the end
    assert on_end == [0, qe, qe + 1]
    behind = cp.cuts(q, ref, re_ + 1)  # the boundary on ref_end + 1 is query_end + 1
    assert behind == [0, qe + 1, qe + 1]
    for c in (on_begin, on_end, behind):
        cp.check_invariants(c, (0, rb, re_, qb, qe))


@pytest.mark.parametrize("name", ["round edges", "classes", "deep, its first 12"])
def test_the_cut_points_of_counted_pairs_obey_the_invariants(name):
    ref, queries = pl.round_edges() if name == "round edges" else pl.classes() if name == "classes" else (pl.deep()[0], pl.deep()[1][:12])
    for q in queries:
        row = counted(q, ref)
        for W in (7, 64, 100):
            c = cp.cuts(q, ref, W)
            cp.check_invariants(c, row)
            assert "".join(cp.pieces(q, ref, W)) == q[row[3] : row[4] + 1]


def test_the_invariants_notice_a_wrong_cut():
    ref, (q,) = pl.run_start(63, True)
    row, c = counted(q, ref), cp.cuts(q, ref, 50)
    cp.check_invariants(c, row)
    for t, d in ((0, 1), (len(c) - 1, -1), (2, 200)):
        bad = list(c)
        bad[t] += d
        with pytest.raises(AssertionError):
            cp.check_invariants(bad, row)


def test_a_pair_that_does_not_count_gets_zeros():
    wide, poly, _, _ = pl.nothing_counts()
    assert cp.cuts(wide[1], wide[0], 500) == [0] * (cp.n_windows(len(wide[0]), 500) + 1)  # CW_SW_NO_PATH
    assert cp.cuts(wide[2], wide[0], 500) == [0] * (cp.n_windows(len(wide[0]), 500) + 1)  # the empty query
    assert cp.cuts(poly[1], poly[0], 64) == [0] * 9  # nothing aligns
    assert cp.cuts("ACGT", "", 5) == [0]  # an empty reference: T = 0
    assert all(p == "" for p in cp.pieces(wide[1], wide[0], 500))


# ---- the groups and the polish --------------------------------------------------------------------------------------------------------------------------------------

def test_the_groups_hold_the_windows_columns_and_the_spanning_pieces_only():
    _, grp = cp.polish_input(**cp.SEED9)
    ref = grp[0]
    wins, first = cp.cut_groups([list(grp), [], ["", "ACGT"], [ref[:70]]], 64)
    T = cp.n_windows(len(ref), 64)
    assert first == [0, T, T, T, T + 2] and len(wins) == T + 2
    assert "".join(w[0] for w in wins[:T]) == ref and len(wins[T - 1][0]) == len(ref) - 64 * (T - 1) < 64  # a last window shorter than W
    assert len(wins[0]) == 1 and len(wins[T - 1]) == 1 and max(len(w) for w in wins[:T]) > 10  # end windows with the backbone alone
    assert wins[T:] == [[ref[:64]], [ref[64:70]]]  # a reference alone: its windows, no member
    for t, w in enumerate(wins[:T]):
        want = [cp.pieces(q, ref, 64)[t] for q in grp[1:] if cp.spans(q, ref, 64 * t, min(64 * t + 64, len(ref)))]
        assert w[1:] == [m for m in want if m]
    touching, _ = cp.cut_groups([list(grp)], 64, touching=True)
    assert all(len(a) >= len(b) for a, b in zip(touching, wins)) and sum(map(len, touching)) > sum(map(len, wins[:T]))


def test_the_composition_brings_the_draft_nearer_to_its_truth():
    truth, grp = cp.polish_input(**cp.SEED8)
    assert len(truth) == 1200 and len(grp) == 21
    (polished, members), = cp.polish([list(grp)], 100)
    draft_d, polished_d = cp.edit_distance(grp[0], truth), cp.edit_distance(polished, truth)
    print(f"seed 8, 10 %, W 100: the draft is {draft_d} edits from the truth, the polished draft {polished_d}; members a window {members}")
    assert polished_d < draft_d


def test_the_touching_pieces_rule_takes_the_draft_further_away():
    """By design: a piece that covers half a window is aligned end to end against whole-window members."""
    truth, grp = cp.polish_input(**cp.SEED7)
    (spanning, _), = cp.polish([list(grp)], 200)
    (touching, _), = cp.polish([list(grp)], 200, touching=True)
    draft_d, span_d, touch_d = cp.edit_distance(grp[0], truth), cp.edit_distance(spanning, truth), cp.edit_distance(touching, truth)
    print(f"seed 7, 5 %, W 200: draft {draft_d}, spanning members {span_d}, touching pieces {touch_d}")
    assert span_d < draft_d < touch_d


def test_the_edit_distance_is_levenshteins():
    assert cp.edit_distance("kitten", "sitting") == 3 and cp.edit_distance("", "ACG") == 3 and cp.edit_distance("ACGT", "ACGT") == 0
    assert cp.edit_distance("ACGTACGT", "CGTACG") == 2
