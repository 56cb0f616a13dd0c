"""The alignment operator's cut run (include/consent_amd.h cw_sw_cut_run / cw_sw_cut_run_device; csrc/cw_sw_cut.h): every word of every query's slot equals the
plain reference of tests/sw_cut_probes.py (the ops of sw_path_probes.reference walked to the window boundaries; tests/test_sw_cut_cpu.py holds it to its design),
every row equals Engine.sw_path's, and nothing else is written -- with a run on either side of a boundary and of a round of 64 steps, in all three launch classes
at window sizes from one column to more than the reference, with many waves on one reference, in crowds (by invariants), beside pairs that do not count, with a
slot too short, in any batch composition, through both entry points, between other runs of the engine."""
import ctypes as C
import random

import numpy as np
import pytest

import consent_amd as ca
import oracle_lib
import pileup_probes as pl
import poa_op_probes as pop
import sw_cut_probes as cp
import sw_op_probes as sp
from consent_amd.engine import Batch, SwCuts, _ptr, synth_host

pytestmark = pytest.mark.gpu
E_INVALID, E_CAPACITY = -1, -4
REF_PAD, QUERY_PAD, TAIL = 3, 2, 5  # words of a reference's slot, words a query's slot holds beyond its T + 1, words behind the last slot


@pytest.fixture(scope="module")
def eng():
    e = ca.Engine(ca.Params(*sp.PRM))
    yield e
    e.close()


class Run:
    """One cw_sw_cut_run over slots that held cp.FILL: rows, the words, the slots' offsets."""

    def __init__(self, eng, groups, W, widths=None, expect_rc=(0,)):
        self.groups, self.W = groups, W
        self.hb = hb = ca.pack_piles(groups)
        S = len(hb.seq_len)
        self.first = [int(x) for x in hb.win_first_seq]
        self.need = np.zeros(S, np.int64)  # T + 1 for a query, 0 for a reference
        for g, grp in enumerate(groups):
            for k in range(1, len(grp)):
                self.need[self.first[g] + k] = cp.n_windows(len(grp[0]), W) + 1
        if widths is None:
            widths = np.where(self.need > 0, self.need + QUERY_PAD, REF_PAD)
        self.off = np.zeros(S + 1, np.uint64)
        self.off[1:] = np.cumsum(np.asarray(widths, np.int64))
        self.n_words = int(self.off[-1])
        self.words = np.full(self.n_words + TAIL, cp.FILL, np.uint32)
        self.rows = np.full((S, 8), 99, np.int32)
        b = hb.c_struct()
        cuts = SwCuts(_ptr(self.words), _ptr(self.off), W)
        self.rc = eng.lib.cw_sw_cut_run(eng.handle, C.byref(b), _ptr(self.rows), C.byref(cuts))
        assert self.rc in expect_rc, self.rc
        self.timings = eng.timings()

    def slot(self, s):
        return self.words[int(self.off[s]) : int(self.off[s + 1])]

    def cuts(self, g, k):
        s = self.first[g] + k
        return self.slot(s)[: int(self.need[s])]

    def untouched(self, short=()):
        """Every word the run does not own still holds the fill: a query's slot beyond T + 1, every reference's slot, the words behind the last slot -- and the
        whole slot of the sequences in `short`."""
        assert (self.words[self.n_words :] == cp.FILL).all(), "words behind the last slot were written"
        for s in range(len(self.need)):
            part = self.slot(s) if s in short else self.slot(s)[int(self.need[s]) :]
            assert (part == cp.FILL).all(), f"sequence {s}: words the run does not own were written"


def check(eng, run, what, short=()):
    """Every query's words against the reference, word for word; every row against Engine.sw_path's; nothing else written."""
    path = eng.sw_path(run.groups)
    n_bad = n_pairs = 0
    for g, grp in enumerate(run.groups):
        for k in range(1, len(grp)):
            if run.first[g] + k in short:
                continue
            want, got = cp.cuts(grp[k], grp[0], run.W), [int(x) for x in run.cuts(g, k)]
            n_pairs += 1
            n_bad += want != got
            assert want == got, f"{what}: W = {run.W}, group {g} query {k}: first difference at word {next(t for t, (a, b) in enumerate(zip(want, got)) if a != b)}: {got[:8]} .., the reference {want[:8]} .."
    print(f"{what}: W = {run.W}: {n_pairs} queries, {n_bad} differ")
    keep = np.ones(len(run.rows), bool)
    keep[list(short)] = False
    assert np.array_equal(run.rows[keep], path.rows[keep]), f"{what}: rows differ from cw_sw_path_run's at {np.flatnonzero((run.rows != path.rows).any(axis=1) & keep)[:5]}"
    run.untouched(short=short)
    return path


# ---- 1. a run at a boundary, on either side of a round of 64 steps ------------------------------------------------------------------------------------------------

def test_a_run_on_either_side_of_a_boundary_and_of_a_round(eng):
    named = cp.run_groups()
    groups = [x[1] for x in named]
    runs = {W: Run(eng, groups, W) for W in range(40 + pl.RUN_P[0], 40 + pl.RUN_P[-1] + 3)}  # every W the probes were designed for
    for W, run in runs.items():
        check(eng, run, "run starts")
    for g, (_, _, p, deletion) in enumerate(named):
        if deletion:
            for k in range(3):
                assert [int(x) for x in runs[40 + p + k].cuts(g, 1)] == [0, p, p + 80, p + 80], (p, k)
        else:
            assert [int(x) for x in runs[40 + p].cuts(g, 1)] == [0, p + 3, p + 83, p + 83], p
        assert tuple(int(x) for x in runs[40 + p].rows[2 * g + 1, 5:8]) == ((0, 3, 0) if deletion else (3, 0, 0))
    assert {"sw_order", "cut", "cut_wide", "cut_long", "total"} <= set(runs[102].timings), runs[102].timings
    assert not {"pile", "sw_path", "sw_align", "pile_clear"} & set(runs[102].timings)


# ---- 2. the launch classes, a reference beyond LDS, window sizes ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [1, 64, 500])
def test_all_three_launch_classes_at_a_window_size(eng, W):
    groups = [cp.as_group(pl.classes())]
    run = Run(eng, groups, W)
    check(eng, run, "classes")
    assert (run.rows[1:, 7] == ca.SW_ALIGNED).all() and len(run.cuts(0, 1)) == {1: 3001, 64: 48, 500: 7}[W]
    t = run.timings
    assert t["cut"] > 0 and t["cut_wide"] > 0 and t["cut_long"] > 0, t


def test_a_window_longer_than_the_reference(eng):
    run = Run(eng, [cp.as_group(pl.classes())], 4000)
    check(eng, run, "classes, one window")
    for k in range(1, 5):
        assert [int(x) for x in run.cuts(0, k)] == [int(run.rows[k, 3]), int(run.rows[k, 4]) + 1]


# ---- 3. rounds of 64 steps -----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [1, 64])
def test_paths_that_end_at_the_edges_of_a_round(eng, W):
    run = Run(eng, [cp.as_group(pl.round_edges())], W)
    check(eng, run, "round edges")
    assert [int(r[2] - r[1] + 1) for r in run.rows[1:]] == list(pl.ROUND_LENS)


# ---- 4. many waves on one reference ------------------------------------------------------------------------------------------------------------------------------------

def test_forty_queries_on_one_reference(eng):
    run = Run(eng, [cp.as_group(pl.deep(40))], 100)
    check(eng, run, "deep(40)")
    assert (run.rows[1:, 7] == ca.SW_ALIGNED).all() and len(run.rows) == 41


# ---- 5. pairs that do not count ---------------------------------------------------------------------------------------------------------------------------------------------

def test_pairs_that_do_not_count_get_zeros(eng):
    groups = [list(g) for g in pl.nothing_counts()]
    run = Run(eng, groups, 500)
    check(eng, run, "nothing counts")
    wide, poly, lone = run.first[0], run.first[1], run.first[2]
    assert [int(x) for x in run.rows[wide : wide + 4, 7]] == [ca.SW_IS_REF, ca.SW_NO_PATH, ca.SW_ALIGNED, ca.SW_ALIGNED] and run.rows[wide + 1, 0] > 0
    T = cp.n_windows(len(groups[0][0]), 500)
    assert (run.cuts(0, 1) == 0).all() and (run.cuts(0, 2) == 0).all() and len(run.cuts(0, 1)) == T + 1  # NO_PATH, the empty query
    assert (run.cuts(1, 1) == 0).all() and (run.cuts(1, 3) == 0).all() and run.cuts(1, 2).any()  # nothing aligns, empty; the aligned one beside them
    assert int(run.rows[lone, 7]) == ca.SW_IS_REF and len(run.rows) == sum(len(g) for g in groups)  # a reference alone, a group of none
    on_empty = Run(eng, [["", "ACGT", ""]], 7)  # an empty reference: T = 0, one zero each
    assert [int(x) for x in on_empty.cuts(0, 1)] == [0] and [int(x) for x in on_empty.cuts(0, 2)] == [0]
    on_empty.untouched()
    empty = eng.sw_cut([[], []], 100)  # no sequence at all: nothing to run
    assert empty.rc == 0 and empty.rows.shape == (0, 8)
    rng = random.Random(0xCA9)  # a pair beyond a capacity: CW_E_CAPACITY from the host entry point, zeros for it, the other pair cut
    ref, (q,) = pl.run_start(63, True)
    stop = Run(eng, [[ref, q, pop.rand_seq(rng, sp.QMAX + 1)]], 103, expect_rc=(E_CAPACITY,))
    assert int(stop.rows[2, 7]) == ca.SW_STOP and (stop.cuts(0, 2) == 0).all() and [int(x) for x in stop.cuts(0, 1)] == cp.cuts(q, ref, 103)
    stop.untouched()


# ---- 6. a slot too short ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_slot_one_word_short_stops_its_pair_and_no_other(eng):
    ref, queries = pl.round_edges()
    wide, _, _, _ = pl.nothing_counts()
    groups = [[ref] + list(queries[:4]), [wide[0], wide[1], wide[3]]]
    W = 64
    full = Run(eng, groups, W)
    widths = np.where(full.need > 0, full.need + QUERY_PAD, REF_PAD)
    short_counting, short_other = full.first[0] + 2, full.first[1] + 1  # a pair that counts, and the NO_PATH pair
    widths[short_counting] -= QUERY_PAD + 1
    widths[short_other] -= QUERY_PAD + 1
    run = Run(eng, groups, W, widths=widths)
    assert run.rc == 0  # not an error
    path = check(eng, run, "short slots", short=(short_counting, short_other))
    assert int(run.rows[short_counting, 7]) == ca.SW_CUT_SLOT and np.array_equal(run.rows[short_counting, :7], path.rows[short_counting, :7])
    assert int(path.rows[short_counting, 7]) == ca.SW_ALIGNED
    assert int(run.rows[short_other, 7]) == ca.SW_NO_PATH and np.array_equal(run.rows[short_other], path.rows[short_other])  # keeps its status
    assert (run.slot(short_counting) == cp.FILL).all() and (run.slot(short_other) == cp.FILL).all()
    empty_slot = Run(eng, [[ref, queries[2]]], W, widths=[REF_PAD, 0])
    assert int(empty_slot.rows[1, 7]) == ca.SW_CUT_SLOT and (empty_slot.words == cp.FILL).all()
    # Engine.sw_cut: slot_words makes such slots, the default ones hold every query
    rows = eng.sw_cut(groups, W)
    assert not (rows.rows[:, 7] == ca.SW_CUT_SLOT).any() and [int(x) for x in rows.cuts(0, 2)] == cp.cuts(queries[1], ref, W)
    assert rows.pieces(0, 3) == cp.pieces(queries[2], ref, W) and "".join(rows.pieces(1, 2)) == wide[3]
    assert (eng.sw_cut(groups, W, slot_words=2).rows[short_counting, 7] == ca.SW_CUT_SLOT) and len(eng.sw_cut(groups, W, slot_words=2).cuts(0, 2)) == 0


# ---- 7. composition ------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_querys_words_do_not_depend_on_the_batch(eng):
    groups = [x[1] for x in cp.run_groups()] + [cp.as_group(pl.classes()), cp.as_group(pl.round_edges())] + [list(g) for g in pl.nothing_counts()]
    W = 104
    together = Run(eng, groups, W)
    together.untouched()
    backwards = Run(eng, groups[::-1], W)
    backwards.untouched()
    for i, grp in enumerate(groups):
        alone = Run(eng, [grp], W)
        alone.untouched()
        at = len(groups) - 1 - i
        for k in range(1, len(grp)):
            assert np.array_equal(alone.cuts(0, k), together.cuts(i, k)) and np.array_equal(alone.cuts(0, k), backwards.cuts(at, k)), (i, k)
        assert np.array_equal(alone.rows, together.rows[together.first[i] : together.first[i + 1]]), i
        assert np.array_equal(alone.rows, backwards.rows[backwards.first[at] : backwards.first[at + 1]]), i


# ---- 8. the entry points and what they refuse ------------------------------------------------------------------------------------------------------------------------------------

def device_run(eng, run, on_stream):
    import torch

    dev = torch.device("cuda", eng.device)

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    hb, S = run.hb, len(run.hb.seq_len)
    t_in = (up(hb.win_first_seq, np.int32), up(hb.seq_len, np.int32), up(hb.seq_word_off, np.int64), up(np.concatenate([hb.bases, np.zeros(4, np.uint32)]), np.int32),
            up(run.off, np.int64))
    t_rows = torch.full((S * 8 + 16,), 99, dtype=torch.int32, device=dev)
    t_words = up(np.full(len(run.words), cp.FILL, np.uint32), np.int32)
    b = Batch(hb.n_windows, S, len(hb.bases), t_in[0].data_ptr(), t_in[1].data_ptr(), t_in[2].data_ptr(), t_in[3].data_ptr())
    cuts = SwCuts(t_words.data_ptr(), t_in[4].data_ptr(), run.W)
    torch.cuda.synchronize(dev)
    if on_stream:
        s = torch.cuda.Stream(dev)
        eng.sw_cut_device(b, C.c_void_p(t_rows.data_ptr()), cuts, C.c_void_p(s.cuda_stream))
        s.synchronize()
    else:
        eng.sw_cut_device(b, C.c_void_p(t_rows.data_ptr()), cuts)
    torch.cuda.synchronize(dev)
    rows = t_rows.cpu().numpy()
    assert (rows[S * 8 :] == 99).all(), "words behind the rows were written"
    return rows[: S * 8].reshape(-1, 8), t_words.cpu().numpy().view(np.uint32)


def test_the_device_entry_point_equals_the_host_path(eng):
    groups = [cp.as_group(pl.classes()), cp.as_group(pl.run_start(64, False)), cp.as_group(pl.round_edges()), [], [pl.round_edges()[0]]] + [list(g) for g in pl.nothing_counts()]
    for W in (64, 104):
        host = Run(eng, groups, W)
        check(eng, host, "host entry point")
        for on_stream in (False, True):
            rows, words = device_run(eng, host, on_stream)
            assert np.array_equal(rows, host.rows) and np.array_equal(words, host.words), (W, on_stream)


def test_bad_arguments_are_refused_before_anything_is_launched(eng):
    groups = [cp.as_group(pl.run_start(63, True))]
    ok = Run(eng, groups, 103)
    stages = ok.timings
    b = ok.hb.c_struct()
    rows = np.full((2, 8), 99, np.int32)
    words, off = np.full(len(ok.words), cp.FILL, np.uint32), ok.off
    p = C.c_void_p(rows.ctypes.data)
    cuts = SwCuts(_ptr(words), _ptr(off), 103)
    big = Batch(eng.max_batch_windows() + 1, b.n_seqs, b.n_words, b.win_first_seq, b.seq_len, b.seq_word_off, b.bases)
    for fn in (eng.lib.cw_sw_cut_run, lambda *a: eng.lib.cw_sw_cut_run_device(*a, None)):
        assert fn(eng.handle, C.byref(b), p, C.byref(SwCuts(_ptr(words), _ptr(off), 0))) == E_INVALID  # window == 0
        assert fn(eng.handle, C.byref(b), None, C.byref(cuts)) == E_INVALID
        assert fn(eng.handle, C.byref(b), p, None) == E_INVALID
        assert fn(eng.handle, None, p, C.byref(cuts)) == E_INVALID
        assert fn(eng.handle, C.byref(b), p, C.byref(SwCuts(None, _ptr(off), 103))) == E_INVALID
        assert fn(eng.handle, C.byref(b), p, C.byref(SwCuts(_ptr(words), None, 103))) == E_INVALID
        assert fn(eng.handle, C.byref(big), p, C.byref(cuts)) == E_INVALID
        assert fn(None, C.byref(b), p, C.byref(cuts)) == E_INVALID
        none = Batch(0, 0, 0, None, None, None, None)  # no sequence: CW_OK, nothing launched
        assert fn(eng.handle, C.byref(none), p, C.byref(cuts)) == 0
    assert (rows == 99).all() and (words == cp.FILL).all() and eng.timings() == stages, "a refused call launched something"
    again = Run(eng, groups, 103)
    assert np.array_equal(again.rows, ok.rows) and np.array_equal(again.words, ok.words)


# ---- 9. between other runs -------------------------------------------------------------------------------------------------------------------------------------------------------

def test_cut_runs_alternate_with_window_poa_and_pileup_runs_on_one_engine():
    groups = [cp.as_group(pl.classes()), cp.as_group(pl.run_start(62, False)), cp.as_group(pl.run_start(65, True)), cp.as_group(pl.round_edges())]
    prm = ca.Params(9, 4, 8, 2, 150)
    e = ca.Engine(prm)
    try:
        piles = synth_host(ca.SynthSpec.pacbio(24, 30))
        exp, _ = oracle_lib.oracle_run(prm, piles)
        got = e.run(piles)
        for w in range(piles.n_windows):
            assert got.status[w] == exp.status[w] and got.consensus(w) == exp.consensus(w), w
        before = Run(e, groups, 102)
        poa_group = pop.probe("100x10")
        assert e.poa([poa_group]).consensus(0) == pop.oracle_consensus(poa_group, 150)
        after = Run(e, groups, 102)
        assert np.array_equal(before.rows, after.rows) and np.array_equal(before.words, after.words)
        pile = e.pileup(groups)
        assert np.array_equal(pile.rows, after.rows)
        assert {"pile", "pile_clear"} <= set(e.timings()) and "cut" not in e.timings()
        again = Run(e, groups, 102)
        assert np.array_equal(before.words, again.words) and {"cut", "cut_wide", "cut_long"} <= set(again.timings) and "pile" not in again.timings
        check(e, again, "between other runs")
        got = e.run(piles)
        for w in range(piles.n_windows):
            assert got.status[w] == exp.status[w] and got.consensus(w) == exp.consensus(w), w
    finally:
        e.close()


# ---- 10. crowds, by invariants ---------------------------------------------------------------------------------------------------------------------------------------------------

CROWD_SAMPLE = {0: 97, 1: 61, 2: 29}  # every n-th pair is also compared with the reference word for word (it costs milliseconds a pair)


@pytest.mark.parametrize("cls", [0, 1, 2])
def test_a_crowd_obeys_the_invariants(eng, cls):
    """More pairs than the launch has waves (sw_op_probes.CROWDS): a wave cuts a second pair and a third from the buffers the one before left."""
    groups = [list(g) for g in sp.crowd(*pl.CROWDS[cls])]
    W = 32
    run = Run(eng, groups, W)
    print(f"class {cls}: {sum(len(g) - 1 for g in groups)} pairs, stages {run.timings}")
    path = eng.sw_path(groups)
    assert np.array_equal(run.rows, path.rows)
    run.untouched()
    n_counted = n_pairs = 0
    for g, grp in enumerate(groups):
        for k in range(1, len(grp)):
            row, c = run.rows[run.first[g] + k], run.cuts(g, k)
            n_pairs += 1
            if row[7] == ca.SW_ALIGNED and row[0] > 0:
                n_counted += 1
                cp.check_invariants(c, row)
                inner = [t for t in range(len(c)) if row[1] < t * W <= row[2]]
                assert all(row[3] <= int(c[t]) <= row[4] + 1 for t in inner)
            else:
                assert not c.any()
            if n_pairs % CROWD_SAMPLE[cls] == 0:
                assert [int(x) for x in c] == cp.cuts(grp[k], grp[0], W), (g, k)
    assert n_counted > 0.9 * n_pairs
