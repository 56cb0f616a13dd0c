"""The alignment operator's pileup run (include/consent_amd.h cw_pileup_run / cw_pileup_run_device; csrc/cw_pileup.h): every word of every column equals the
plain reference of tests/pileup_probes.py (the ops of sw_path_probes.reference walked into columns; tests/test_pileup_cpu.py holds it to its design), every row
equals Engine.sw_path's -- at the edges of a round of 64 steps, with a run starting on either side of one, in all three launch classes on one column set, with
hundreds of waves on one column set, in crowds (by invariants), beside pairs that count nothing, with a slot too short, accumulated over calls, in any batch
composition, through both entry points, between other runs of the engine -- and Engine.poa_support on top of it."""
import ctypes as C
import random

import numpy as np
import pytest

import consent_amd as ca
import oracle_lib
import pileup_probes as pl
import poa_op_probes as pop
import sw_op_probes as sp
from consent_amd.engine import Batch, Pileup, _ptr, synth_host

pytestmark = pytest.mark.gpu
E_INVALID, E_CAPACITY = -1, -4
REF_PAD, QUERY_PAD, TAIL = 2, 1, 4  # columns a reference's slot holds beyond the reference, columns of a query's slot, columns behind the last slot


@pytest.fixture(scope="module")
def eng():
    e = ca.Engine(ca.Params(*sp.PRM))
    yield e
    e.close()


class Run:
    """One cw_pileup_run over counts that held pl.FILL (or `counts`): rows, the counts as (columns, 8), the slots' offsets."""

    def __init__(self, eng, groups, flags=0, counts=None, widths=None, padded=True, expect_rc=(0,)):
        self.groups = groups
        self.hb = hb = ca.pack_piles(groups)
        S = len(hb.seq_len)
        self.first = [int(x) for x in hb.win_first_seq]
        is_ref = np.zeros(S, bool)
        is_ref[[r for g, r in enumerate(self.first[:-1]) if groups[g]]] = True
        if widths is None:
            lens = hb.seq_len.astype(np.int64)
            widths = np.where(is_ref, lens + REF_PAD, QUERY_PAD) if padded else np.where(is_ref, lens, 0)
        self.off = np.zeros(S + 1, np.uint64)
        self.off[1:] = np.cumsum(np.asarray(widths, np.int64))
        n_cols = int(self.off[-1])
        self.counts = np.full((n_cols + TAIL, 8), pl.FILL, np.uint32) if counts is None else counts
        assert self.counts.shape == (n_cols + TAIL, 8)
        self.rows = np.full((S, 8), 99, np.int32)
        b = hb.c_struct()
        pile = Pileup(_ptr(self.counts), _ptr(self.off))
        self.rc = eng.lib.cw_pileup_run(eng.handle, C.byref(b), _ptr(self.rows), C.byref(pile), flags)
        assert self.rc in expect_rc, self.rc
        self.n_cols, self.timings = n_cols, eng.timings()

    def slot(self, s):
        return self.counts[int(self.off[s]) : int(self.off[s + 1])]

    def cols(self, g):
        """The columns of group g's reference."""
        return self.slot(self.first[g])[: len(self.groups[g][0])]

    def untouched(self, filled=pl.FILL, short=()):
        """Every word the run does not own still holds the fill: a reference's slot beyond its length, every query's slot, the words behind the last slot --
        and the whole slot of the groups in `short`."""
        assert (self.counts[self.n_cols :] == filled).all(), "words behind the last slot were written"
        for g, grp in enumerate(self.groups):
            for k, seq in enumerate(grp):
                part = self.slot(self.first[g] + k)
                if k == 0 and g not in short:
                    part = part[len(seq) :]
                assert (part == filled).all(), f"group {g} member {k}: words the run does not own were written"


def as_groups(named):
    return [[ref] + list(queries) for ref, queries in named]


def check(eng, run, what, short=()):
    """Every group's columns against the reference, word for word; every row against Engine.sw_path's; nothing else written."""
    path = eng.sw_path(run.groups)
    for g, grp in enumerate(run.groups):
        if not grp or g in short:
            continue
        want, got = pl.pileup(grp[0], grp[1:]), run.cols(g)
        bad = np.argwhere(want != got)
        print(f"{what}: group {g}: {len(grp) - 1} queries on {len(grp[0])} columns, deepest {int(pl.coverage(want).max(initial=0))}, {len(bad)} words differ")
        assert len(bad) == 0, f"{what}: group {g}: column {bad[0][0]} word {bad[0][1]}: {got[bad[0][0]].tolist()}, the reference {want[bad[0][0]].tolist()}"
    keep = np.ones(len(run.rows), bool)
    for g in short:
        keep[run.first[g] : run.first[g + 1]] = False
    assert np.array_equal(run.rows[keep], path.rows[keep]), f"{what}: rows differ from cw_sw_path_run's at {np.flatnonzero((run.rows != path.rows).any(axis=1) & keep)[:5]}"
    run.untouched(short=short)
    return path


# ---- 1. round edges ------------------------------------------------------------------------------------------------------------------------------------------

def test_paths_that_end_at_the_edges_of_a_round(eng):
    groups = as_groups([pl.round_edges()])
    run = Run(eng, groups)
    check(eng, run, "round edges")
    assert [int(r[2] - r[1] + 1) for r in run.rows[1:]] == list(pl.ROUND_LENS) and (run.rows[1:, 7] == ca.SW_ALIGNED).all()
    assert {"sw_order", "pile_clear", "pile", "pile_wide", "pile_long", "total"} <= set(run.timings), run.timings
    alone = Run(eng, [[groups[0][0], q] for q in groups[0][1:]])  # each length in a group of its own: its columns hold that path and nothing else
    check(eng, alone, "round edges, a group each")
    for g, n in enumerate(pl.ROUND_LENS):
        assert int(alone.cols(g)[:, : pl.T + 1].sum()) == n and int(alone.cols(g)[:, pl.DEL :].sum()) == 2


# ---- 2. a run start at a round edge ---------------------------------------------------------------------------------------------------------------------------

def test_a_run_that_starts_on_either_side_of_a_round_edge(eng):
    named = [(p, d, pl.run_start(p, d)) for d in (False, True) for p in pl.RUN_P]
    groups = as_groups([x[2] for x in named])
    run = Run(eng, groups)
    check(eng, run, "run starts")
    for g, (p, deletion, _) in enumerate(named):
        cols = run.cols(g)
        if deletion:
            assert np.flatnonzero(cols[:, pl.DEL]).tolist() == [40 + p, 41 + p, 42 + p] and int(cols[:, pl.INS].sum()) == 0, (p, deletion)
        else:
            assert np.flatnonzero(cols[:, pl.INS]).tolist() == [40 + p - 1] and int(cols[40 + p - 1, pl.INS]) == 1 and int(cols[:, pl.DEL].sum()) == 0, (p, deletion)
        assert tuple(int(x) for x in run.rows[2 * g + 1, 5:8]) == ((0, 3, 0) if deletion else (3, 0, 0))


# ---- 3. the launch classes on one column set --------------------------------------------------------------------------------------------------------------------

def test_all_three_launch_classes_add_to_the_same_columns(eng):
    groups = as_groups([pl.classes()])
    run = Run(eng, groups)
    check(eng, run, "classes")
    assert (run.rows[1:, 7] == ca.SW_ALIGNED).all() and int(run.cols(0)[:, pl.BEGIN].sum()) == 4
    assert int(pl.coverage(run.cols(0)).max()) == 4  # a column every class adds to
    t = run.timings
    assert t["pile"] > 0 and t["pile_wide"] > 0 and t["pile_long"] > 0, t


# ---- 4. many waves on one column set ------------------------------------------------------------------------------------------------------------------------------

def test_three_hundred_queries_on_one_reference(eng):
    groups = as_groups([pl.deep()])
    run = Run(eng, groups)
    check(eng, run, "deep")
    assert int(run.cols(0)[:, pl.BEGIN].sum()) == 300 and int(pl.coverage(run.cols(0)).max()) == 300


# ---- 5. crowds, by invariants -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", [0, 1, 2])
def test_a_crowd_obeys_the_invariants(eng, cls):
    """More pairs than the launch has waves (sw_op_probes.CROWDS): a wave counts a second pair and a third from the buffers the one before left.  No reference:
    per reference the invariants of pileup_probes.check_invariants over the rows that counted, and the rows are cw_sw_path_run's."""
    groups = [list(g) for g in sp.crowd(*pl.CROWDS[cls])]
    run = Run(eng, groups)
    print(f"class {cls}: {sum(len(g) - 1 for g in groups)} pairs, stages {eng.timings()}")
    assert run.rc == 0
    path = eng.sw_path(groups)
    assert np.array_equal(run.rows, path.rows)
    run.untouched()
    n_counted = 0
    for g, grp in enumerate(groups):
        rows = [tuple(int(x) for x in r[:7]) for r in run.rows[run.first[g] + 1 : run.first[g + 1]] if r[7] == ca.SW_ALIGNED and r[0] > 0]
        n_counted += len(rows)
        pl.check_invariants(run.cols(g), rows)
    assert n_counted > 0.9 * sum(len(g) - 1 for g in groups)


# ---- 6. pairs that count nothing ------------------------------------------------------------------------------------------------------------------------------------

def test_pairs_that_count_nothing_beside_pairs_that_count(eng):
    groups = [list(g) for g in pl.nothing_counts()]
    run = Run(eng, groups)
    assert run.rc == 0 and len(run.rows) == sum(len(g) for g in groups)
    check(eng, run, "nothing counts")
    wide, poly, lone = run.first[0], run.first[1], run.first[2]
    assert [int(x) for x in run.rows[wide : wide + 4, 7]] == [ca.SW_IS_REF, ca.SW_NO_PATH, ca.SW_ALIGNED, ca.SW_ALIGNED] and run.rows[wide + 1, 0] > 0
    assert [int(x) for x in run.rows[wide + 2]] == [0, 0, -1, 0, -1, 0, 0, ca.SW_ALIGNED]  # the empty query
    assert [int(x) for x in run.rows[poly + 1]] == [0, 0, -1, 0, -1, 0, 0, ca.SW_ALIGNED]  # nothing aligns
    assert int(run.cols(0)[:, pl.BEGIN].sum()) == 1 and int(run.cols(1)[:, pl.BEGIN].sum()) == 1  # the aligned pair of each, and no other
    assert run.cols(2).shape == (90, 8) and (run.cols(2) == 0).all() and int(run.rows[lone, 7]) == ca.SW_IS_REF  # the lone reference: cleared
    empty = eng.pileup([[], []])  # no sequence at all: nothing to run
    assert empty.rc == 0 and empty.rows.shape == (0, 8) and empty.counts(0).shape == (0, 8)


# ---- 7. a slot too short ----------------------------------------------------------------------------------------------------------------------------------------------

def test_a_slot_one_column_short_stops_its_group_and_no_other(eng):
    named = [pl.run_start(63, False), pl.round_edges(), pl.run_start(64, True)]
    groups = as_groups(named)
    hb = ca.pack_piles(groups)
    first = [int(x) for x in hb.win_first_seq]
    widths = np.full(len(hb.seq_len), QUERY_PAD, np.int64)
    for g in range(3):
        widths[first[g]] = len(groups[g][0]) + REF_PAD
    widths[first[1]] = len(groups[1][0]) - 1
    run = Run(eng, groups, widths=widths)
    assert run.rc == 0  # not an error
    path = check(eng, run, "short slot", short=(1,))
    mid = slice(first[1] + 1, first[2])
    assert (run.rows[mid, 7] == ca.SW_PILE_SLOT).all() and np.array_equal(run.rows[mid, :7], path.rows[mid, :7]) and (path.rows[mid, 7] == ca.SW_ALIGNED).all()
    assert int(run.rows[first[1], 7]) == ca.SW_IS_REF and (run.slot(first[1]) == pl.FILL).all()
    again = Run(eng, groups, flags=pl.ACCUMULATE, widths=widths, counts=run.counts.copy())  # nor is anything of it counted under the flag
    assert (again.rows[mid, 7] == ca.SW_PILE_SLOT).all() and (again.slot(first[1]) == pl.FILL).all()
    assert np.array_equal(again.cols(0), 2 * run.cols(0)) and np.array_equal(again.cols(2), 2 * run.cols(2))


# ---- 8. accumulation --------------------------------------------------------------------------------------------------------------------------------------------------------

def test_queries_split_over_two_calls_add_up_to_one_call(eng):
    ref, queries = pl.deep()
    queries = list(queries[:40])
    whole = Run(eng, [[ref] + queries], padded=False)
    first = Run(eng, [[ref] + queries[:17]], padded=False)
    alone = first.counts.copy()
    both = Run(eng, [[ref] + queries[17:]], flags=pl.ACCUMULATE, counts=first.counts, padded=False)
    assert "pile_clear" not in both.timings and "pile" in both.timings and "pile_clear" in first.timings  # nothing is cleared: the launch is left out
    assert both.counts is first.counts and np.array_equal(both.counts, whole.counts)
    assert np.array_equal(np.concatenate([first.rows, both.rows[1:]]), whole.rows)
    second = Run(eng, [[ref] + queries[17:]], counts=both.counts.copy(), padded=False)  # without the flag: only its own counts
    assert np.array_equal(second.counts[:600].astype(np.int64), whole.counts[:600].astype(np.int64) - alone[:600].astype(np.int64))
    assert (second.counts[600:] == pl.FILL).all() and (whole.counts[600:] == pl.FILL).all()
    # Engine.pileup: `into` switches the flag on
    a = eng.pileup([[ref] + queries[:17]])
    b = eng.pileup([[ref] + queries[17:]], into=a)
    assert b.counts_buf is a.counts_buf and np.array_equal(b.counts(0), whole.cols(0)) and np.array_equal(b.coverage(0), pl.coverage(whole.cols(0)))
    with pytest.raises(ca.EngineError):
        eng.pileup([[ref[:-1]] + queries[:3]], into=a)  # other references: another layout


# ---- 9. composition -----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_groups_words_do_not_depend_on_the_batch(eng):
    groups = as_groups(pl.designed_groups().values()) + [list(g) for g in pl.nothing_counts()]
    order = list(range(len(groups)))
    random.Random(0x5AFF).shuffle(order)
    mixed = Run(eng, [groups[i] for i in order])
    mixed.untouched()
    for at, i in enumerate(order):
        alone = Run(eng, [groups[i]])
        alone.untouched()
        if groups[i]:
            assert np.array_equal(alone.cols(0), mixed.cols(at)), f"group {i}: its columns alone and in the batch differ"
        assert np.array_equal(alone.rows, mixed.rows[mixed.first[at] : mixed.first[at + 1]]), i


# ---- 10. the device entry point -------------------------------------------------------------------------------------------------------------------------------------------------

def device_run(eng, run, flags, on_stream, fill):
    import torch

    dev = torch.device("cuda", eng.device)

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    hb, S = run.hb, len(run.hb.seq_len)
    t_in = (up(hb.win_first_seq, np.int32), up(hb.seq_len, np.int32), up(hb.seq_word_off, np.int64), up(np.concatenate([hb.bases, np.zeros(4, np.uint32)]), np.int32),
            up(run.off, np.int64))
    t_rows = torch.full((S * 8 + 16,), 99, dtype=torch.int32, device=dev)
    t_counts = up(fill, np.int32)
    assert t_counts.data_ptr() % 16 == 0
    b = Batch(hb.n_windows, S, len(hb.bases), t_in[0].data_ptr(), t_in[1].data_ptr(), t_in[2].data_ptr(), t_in[3].data_ptr())
    pile = Pileup(t_counts.data_ptr(), t_in[4].data_ptr())
    torch.cuda.synchronize(dev)
    if on_stream:
        s = torch.cuda.Stream(dev)
        eng.pileup_device(b, C.c_void_p(t_rows.data_ptr()), pile, flags, C.c_void_p(s.cuda_stream))
        s.synchronize()
    else:
        eng.pileup_device(b, C.c_void_p(t_rows.data_ptr()), pile, flags)
    torch.cuda.synchronize(dev)
    rows = t_rows.cpu().numpy()
    assert (rows[S * 8 :] == 99).all(), "words behind the rows were written"
    misaligned = Pileup(t_counts.data_ptr() + 4, t_in[4].data_ptr())
    assert eng.lib.cw_pileup_run_device(eng.handle, C.byref(b), C.c_void_p(t_rows.data_ptr()), C.byref(misaligned), flags, None) == E_INVALID
    return rows[: S * 8].reshape(-1, 8), t_counts.cpu().numpy().view(np.uint32)


def test_the_device_entry_point_equals_the_host_path(eng):
    groups = as_groups([pl.classes(), pl.run_start(64, False), pl.round_edges()]) + [[], [pl.round_edges()[0]]]
    host = Run(eng, groups)
    for on_stream in (False, True):
        rows, counts = device_run(eng, host, 0, on_stream, np.full(host.counts.shape, pl.FILL, np.uint32))
        assert np.array_equal(rows, host.rows) and np.array_equal(counts, host.counts), on_stream
    rows, counts = device_run(eng, host, pl.ACCUMULATE, False, host.counts.copy())  # on top of the host's: twice the counts, the fill (all ones) where nothing is owned
    owned = host.counts != pl.FILL
    assert np.array_equal(rows, host.rows) and np.array_equal(counts[owned], 2 * host.counts[owned]) and (counts[~owned] == pl.FILL).all()


# ---- 11. alternation ------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_pileups_alternate_with_window_and_poa_runs_on_one_engine():
    groups = as_groups([pl.classes(), pl.run_start(62, False), pl.run_start(65, True), pl.round_edges()])
    prm = ca.Params(9, 4, 8, 2, 150)
    e = ca.Engine(prm)
    try:
        piles = synth_host(ca.SynthSpec.pacbio(24, 30))
        exp, _ = oracle_lib.oracle_run(prm, piles)
        got = e.run(piles)
        for w in range(piles.n_windows):
            assert got.status[w] == exp.status[w] and got.consensus(w) == exp.consensus(w) and np.array_equal(got.solid_kmers(w), exp.solid_kmers(w)), w
        before = Run(e, groups)
        assert {"sw_order", "pile_clear", "pile", "pile_wide", "pile_long", "total"} <= set(before.timings) and not {"sw_path", "sw_align"} & set(before.timings)
        poa_group = pop.probe("100x10")
        assert e.poa([poa_group]).consensus(0) == pop.oracle_consensus(poa_group, 150)
        after = Run(e, groups)
        assert np.array_equal(before.rows, after.rows) and np.array_equal(before.counts, after.counts)
        path = e.sw_path(groups)
        assert np.array_equal(path.rows, after.rows)
        again = Run(e, groups)
        assert np.array_equal(before.counts, again.counts)
        check(e, again, "between other runs")
    finally:
        e.close()


# ---- 12. arguments ------------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_before_anything_is_launched(eng):
    groups = as_groups([pl.run_start(63, True)])
    ok = Run(eng, groups)
    stages = ok.timings
    hb = ok.hb
    b = hb.c_struct()
    rows = np.full((2, 8), 99, np.int32)
    counts, off = np.full(ok.counts.shape, pl.FILL, np.uint32), ok.off
    p = C.c_void_p(rows.ctypes.data)
    pile = Pileup(_ptr(counts), _ptr(off))
    big = Batch(eng.max_batch_windows() + 1, b.n_seqs, b.n_words, b.win_first_seq, b.seq_len, b.seq_word_off, b.bases)
    for fn in (eng.lib.cw_pileup_run, lambda *a: eng.lib.cw_pileup_run_device(*a, None)):
        for flags in (1, 2, 4, 16, 9):  # the other runs' flags, an unknown one, the known beside an unknown one
            assert fn(eng.handle, C.byref(b), p, C.byref(pile), flags) == E_INVALID, flags
        for flags in (0, pl.ACCUMULATE):
            assert fn(eng.handle, C.byref(b), None, C.byref(pile), flags) == E_INVALID
            assert fn(eng.handle, C.byref(b), p, None, flags) == E_INVALID
            assert fn(eng.handle, None, p, C.byref(pile), flags) == E_INVALID
            assert fn(eng.handle, C.byref(b), p, C.byref(Pileup(None, _ptr(off))), flags) == E_INVALID
            assert fn(eng.handle, C.byref(b), p, C.byref(Pileup(_ptr(counts), None)), flags) == E_INVALID
            assert fn(eng.handle, C.byref(big), p, C.byref(pile), flags) == E_INVALID
    assert (rows == 99).all() and (counts == pl.FILL).all() and eng.timings() == stages, "a refused call launched something"
    again = Run(eng, groups)
    assert np.array_equal(again.rows, ok.rows) and np.array_equal(again.counts, ok.counts)
    rng = random.Random(0xCA9)  # a pair beyond a capacity: CW_E_CAPACITY from the host entry point, the other pairs counted
    stop = Run(eng, [groups[0] + [pop.rand_seq(rng, sp.QMAX + 1)]], expect_rc=(E_CAPACITY,))
    assert int(stop.rows[2, 7]) == ca.SW_STOP and np.array_equal(stop.rows[:2], ok.rows) and np.array_equal(stop.cols(0), ok.cols(0))


# ---- 13. poa_support -----------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_poa_support_counts_the_members_behind_every_consensus_base(eng):
    rng = random.Random(0x50A)
    same = pop.rand_seq(rng, 120)
    other = pop.rand_seq(rng, 90)
    at = 45
    changed = other[:at] + "ACGT".replace(other[at], "")[0] + other[at + 1 :]
    n = 7
    res, pile = eng.poa_support([[same] * n, [other] * (n - 1) + [changed]])
    assert res.consensus(0) == same and res.consensus(1) == other
    for g, cons in enumerate((same, other)):
        counts = pile.counts(g)
        assert counts.shape == (len(cons), 8) and (pile.rows[pile.index(g, 1) : pile.index(g, n) + 1, 7] == ca.SW_ALIGNED).all()
        for j, c in enumerate(cons):
            want = n - 1 if (g, j) == (1, at) else n
            assert int(counts[j, pl.code(c)]) == want, (g, j, counts[j].tolist())
        assert (pile.coverage(g) == n).all() and int(counts[:, pl.DEL :pl.INS + 1].sum()) == 0
    assert int(pile.counts(1)[at, pl.code(changed[at])]) == 1
