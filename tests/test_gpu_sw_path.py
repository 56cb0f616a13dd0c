"""The alignment operator's path run (include/consent_amd.h cw_sw_path_run / cw_sw_path_run_device; csrc/cw_sw_path.h): every row, op count and op equals the
reference of tests/sw_path_probes.py (ssw's banded pass and walk in numpy, pinned to the oracle by tests/test_sw_path_cpu.py), the row's seven numbers the
oracle's cwo_ssw -- for every band shape of the chunked fill, every launch class, ties and degenerate input, '=' / 'X' ops, the three capacities, any batch
composition, more pairs than waves, and both entry points of one engine that also runs windows, POA groups and cw_sw_run."""
import ctypes as C
import random

import numpy as np
import pytest

import consent_amd as ca
import oracle_lib
import poa_op_probes as pop
import sw_op_probes as sp
import sw_path_probes as pp
from consent_amd.engine import Batch, SwPaths, _ptr, synth_host

pytestmark = pytest.mark.gpu
E_INVALID, E_CAPACITY = -1, -4
ZERO = (0, 0, -1, 0, -1, 0, 0)
SENT = 0xABCD1234  # what the slots hold before a run


@pytest.fixture(scope="module")
def eng():
    e = ca.Engine(ca.Params(*sp.PRM))
    yield e
    e.close()


def as_groups(pairs):
    return [[r, q] for q, r in pairs]


def default_slots(groups):
    return [ca.sw_ops_bound(len(s), len(g[0])) for g in groups for s in g]


def run(eng, groups, eqx=False, slots=None):
    """cw_sw_path_run on slots filled with SENT (slots: ops per sequence, default CW_SW_OPS_BOUND); returns (SwPathRows, slots)."""
    hb = ca.pack_piles(groups)
    S = len(hb.seq_len)
    slots = default_slots(groups) if slots is None else list(slots)
    off = np.zeros(S + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray(slots, np.int64))
    ops = np.full(int(off[-1]) + 8, SENT, np.uint32)
    n_ops = np.full(max(S, 1), 77, np.uint32)
    rows = np.full((S, 8), 99, np.int32)
    b = hb.c_struct()
    paths = SwPaths(_ptr(ops), _ptr(off), _ptr(n_ops))
    rc = eng.lib.cw_sw_path_run(eng.handle, C.byref(b), _ptr(rows), C.byref(paths), pp.EQX if eqx else 0)
    assert rc in (0, E_CAPACITY), rc
    assert (ops[int(off[-1]) :] == SENT).all(), "words behind the last slot were written"
    return ca.SwPathRows(rows, hb.win_first_seq, rc, n_ops[:S], ops, off), slots


def words(ops):
    return [(n << 4) | c for n, c in ops]


def check(res, slots, groups, eqx, what, only=None):
    """Every pair of `groups` (lists: reference first) against the reference: row, n_ops, the ops, and the slot's words the path does not cover untouched.
    only: a predicate on the pair's running number choosing which pairs are compared op by op (every pair's row is compared with the oracle's)."""
    k_pair = 0
    for g, grp in enumerate(groups):
        for k, seq in enumerate(grp):
            s = res.index(g, k)
            row = tuple(int(x) for x in res.rows[s])
            slot = res.ops_buf[int(res.ops_off[s]) : int(res.ops_off[s + 1])]
            n = int(res.n_ops[s])
            if k == 0:
                assert row == ZERO + (ca.SW_IS_REF,) and n == 0 and (slot == SENT).all(), f"{what}: group {g}: the reference's row {row}, n_ops {n}"
                continue
            k_pair += 1
            oracle = sp.oracle(seq, grp[0])
            if only is not None and not only(k_pair - 1):
                assert row[7] in (ca.SW_ALIGNED, ca.SW_PATH_SLOT) and row[:7] == oracle, f"{what}: group {g} member {k}: {row}, the oracle {oracle}"
                continue
            e_row, e_n, e_ops = pp.expected(seq, grp[0], eqx, slots[s])
            print(f"{what}: group {g} member {k}: {len(seq)} x {len(grp[0])} -> {row}, {n} ops {res.cigar(g, k)[:60]}")
            assert row == e_row, f"{what}: group {g} member {k} ({len(seq)} x {len(grp[0])}): {row}, the reference {e_row}"
            assert n == e_n, f"{what}: group {g} member {k}: {n} ops, the reference {e_n}"
            if row[7] in (ca.SW_ALIGNED, ca.SW_PATH_SLOT):  # the oracle has no scratch limit: also for pairs cw_sw_run ends NO_INDELS
                assert row[:7] == oracle, f"{what}: group {g} member {k}: {row}, the oracle {oracle}"
            written = len(e_ops)
            assert [int(x) for x in slot[:written]] == words(e_ops), f"{what}: group {g} member {k}: {res.ops(g, k)[:8]} ..., the reference {e_ops[:8]} ..."
            assert (slot[written:] == SENT).all(), f"{what}: group {g} member {k}: the slot beyond the path was written"


def invariants(res, groups, g, k):
    """What holds for every reported path, whatever the reference says: run-length form, the spans, the re-scored ops."""
    q, r = groups[g][k], groups[g][0]
    score, rb, re_, qb, qe, ins, dele, status = (int(x) for x in res.row(g, k))
    ops = res.ops(g, k)
    if score <= 0:
        assert ops == []
        return
    assert status == ca.SW_ALIGNED and ops and all(a[1] != b[1] for a, b in zip(ops, ops[1:]))
    assert pp.rescore(ops, r[rb : re_ + 1], q[qb : qe + 1]) == (score, qe - qb + 1, re_ - rb + 1), (g, k)
    assert sum(n for n, c in ops if c == 1) == ins and sum(n for n, c in ops if c == 2) == dele, (g, k)


# ---- 1. band shapes: the chunked fill ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def bands(eng):
    groups = as_groups(pp.band_pairs().values())
    return groups, run(eng, groups), run(eng, groups, eqx=True)


@pytest.mark.parametrize("name", list(pp.band_pairs()))
def test_every_band_shape_equals_the_reference(bands, name):
    groups, (plain, slots), (eqx, slots_x) = bands
    g = list(pp.band_pairs()).index(name)
    assert plain.rc == 0 and eqx.rc == 0
    for res, sl, x in ((plain, slots, False), (eqx, slots_x, True)):
        one = ca.SwPathRows(res.rows[2 * g : 2 * g + 2], [0, 2], 0, res.n_ops[2 * g : 2 * g + 2], res.ops_buf, res.ops_off[2 * g : 2 * g + 3])
        check(one, sl[2 * g : 2 * g + 2], [groups[g]], x, name + (" eqx" if x else ""))
        assert int(one.row(0, 1)[7]) == ca.SW_ALIGNED and int(one.n_ops[1]) > 0


def test_the_planted_totals(bands):
    groups, (plain, _), _ = bands
    names = list(pp.band_pairs())
    for name, totals in (("planted(10)", (10, 10)), ("planted(40)", (40, 40)), ("planted(300)", (300, 300)), ("unbalanced", (0, 7)), ("deletion of 31", (0, 31)),
                         ("band wider than the matrix", (40, 0))):
        assert tuple(int(x) for x in plain.row(names.index(name), 1)[5:7]) == totals, name
    assert plain.cigar(names.index("deletion of 30"), 1) == "150M30D150M"
    assert plain.cigar(names.index("band wider than the matrix"), 1) == "30M40I30M"


# ---- 2. launch classes ---------------------------------------------------------------------------------------------------------------------------------

def test_every_launch_class_and_reference_length(eng):
    groups = as_groups(pp.class_pairs().values())
    res, slots = run(eng, groups)
    t = eng.timings()
    assert {"sw_order", "sw_path", "sw_path_wide", "sw_path_long", "total"} <= set(t), t
    check(res, slots, groups, False, "launch classes")
    res_x, slots_x = run(eng, groups, eqx=True)
    check(res_x, slots_x, groups, True, "launch classes eqx")


def test_long_queries_carry_a_path(eng):
    groups = as_groups(pp.long_pairs().values())
    for q, r in pp.long_pairs().values():  # by the rule, not by hand: every band the restated pass tries fits a wave's scratch
        assert pp.reference(q, r)[0] == pp.ALIGNED
    res, slots = run(eng, groups)
    check(res, slots, groups, False, "long pairs")
    assert all(int(res.row(g, 1)[7]) == ca.SW_ALIGNED and int(res.n_ops[2 * g + 1]) > 0 for g in range(len(groups)))
    short = as_groups([sp.embedded(5, 100, 600), sp.embedded(5, 700, 600)])
    both, slots_b = run(eng, short + groups, eqx=True)
    check(both, slots_b, short + groups, True, "long beside short")
    none_long, slots_n = run(eng, short)  # the long kernel finds nothing to do
    check(none_long, slots_n, short, False, "no long pair")


# ---- 3. ties and degenerate input --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eqx", [False, True])
def test_ties_nothing_aligns_and_degenerate_groups(eng, eqx):
    ref = pop.rand_seq(random.Random(9), 120)
    groups = as_groups(sp.tie_pairs().values()) + as_groups(sp.nothing_pairs().values()) + [[ref], [], [ref, "", ref[10:90], ""], []]
    res, slots = run(eng, groups, eqx=eqx)
    assert res.rc == 0 and len(res.rows) == sum(len(g) for g in groups)
    check(res, slots, groups, eqx, "ties and nothing")
    for g in (3, 4, 5):  # nothing aligns, empty query, empty reference
        assert tuple(res.row(g, 1)) == ZERO + (ca.SW_ALIGNED,) and int(res.n_ops[res.index(g, 1)]) == 0
    assert res.cigar(8, 2) == ("80=" if eqx else "80M") and tuple(res.row(8, 2)[:5]) == (160, 10, 89, 0, 79)
    empty = eng.sw_path([[], []])  # no sequence at all: nothing to run
    assert empty.rc == 0 and empty.rows.shape == (0, 8) and len(empty.n_ops) == 0


# ---- 4. '=' and 'X' ------------------------------------------------------------------------------------------------------------------------------------------

def test_eqx_splits_the_m_runs_by_the_bases(eng):
    pairs = list(pp.noisy_pairs().values()) + [sp.planted(10), sp.embedded(1, 641, 600)]
    groups = as_groups(pairs)
    plain, slots = run(eng, groups)
    eqx, slots_x = run(eng, groups, eqx=True)
    check(plain, slots, groups, False, "noisy")
    check(eqx, slots_x, groups, True, "noisy eqx")
    assert np.array_equal(plain.rows, eqx.rows)
    for g, (r, q) in enumerate(groups):
        m_ops, x_ops = plain.ops(g, 1), eqx.ops(g, 1)
        assert pp.merge_eqx(x_ops) == m_ops and {c for _, c in x_ops} <= {1, 2, 7, 8}, g
        _, rb, _, qb, _, _, _, _ = (int(x) for x in plain.row(g, 1))
        i, j, mismatches = qb, rb, 0
        for n, c in m_ops:  # counted directly over the M columns
            if c == 0:
                mismatches += sum(q[i + t] != r[j + t] for t in range(n))
            i, j = i + n * (c != 2), j + n * (c != 1)
        assert sum(n for n, c in x_ops if c == 8) == mismatches, g
        invariants(plain, groups, g, 1)
        invariants(eqx, groups, g, 1)


# ---- 5. capacities ---------------------------------------------------------------------------------------------------------------------------------------------

def test_no_path_path_slot_and_stop_beside_their_neighbours(eng):
    wide_q, wide_r = pp.planted_wide()
    assert pp.reference(wide_q, wide_r)[0] == pp.NO_PATH  # by the rule and the restated pass (tests/test_sw_path_cpu.py), not by the operator
    del_q, del_r = pp.one_deletion(31)
    noisy_q, noisy_r = sp.embedded(1, 640, 600)
    need = pp.expected(noisy_q, noisy_r)[1]
    assert need > 3 and pp.expected(del_q, del_r)[1] == 3
    groups = [[wide_r, wide_q], [noisy_r, noisy_q, noisy_q, noisy_q], [del_r, del_q, del_q, del_q, del_q]]
    #        ref bound   | ref, one short, exact, default  | ref, one short, exact, none, default
    slots = default_slots(groups)
    slots[3], slots[4] = need - 1, need
    slots[7], slots[8], slots[9] = 2, 3, 0
    res, slots = run(eng, groups, slots=slots)
    assert res.rc == 0  # none of the three statuses is an error
    check(res, slots, groups, False, "capacities")
    assert tuple(int(x) for x in res.row(0, 1)) == sp.oracle(wide_q, wide_r)[:5] + (0, 0, ca.SW_NO_PATH) and int(res.n_ops[1]) == 0
    assert [int(res.row(1, k)[7]) for k in (1, 2, 3)] == [ca.SW_PATH_SLOT, ca.SW_ALIGNED, ca.SW_ALIGNED] and [int(x) for x in res.n_ops[3:6]] == [need] * 3
    assert [int(res.row(2, k)[7]) for k in (1, 2, 3, 4)] == [ca.SW_PATH_SLOT, ca.SW_ALIGNED, ca.SW_PATH_SLOT, ca.SW_ALIGNED] and [int(x) for x in res.n_ops[7:11]] == [3] * 4
    assert res.ops(1, 1) == [] and res.ops(1, 2) == res.ops(1, 3) and len(res.ops(1, 2)) == need
    assert np.array_equal(res.rows[3, :7], res.rows[4, :7])  # the seven numbers stand
    # a pair beyond a capacity beside them: CW_E_CAPACITY, the other rows unaffected
    rng = random.Random(0xCA9)
    stop = [noisy_r, pop.rand_seq(rng, sp.QMAX + 1), noisy_q]
    res2, slots2 = run(eng, groups[1:] + [stop], slots=slots[2:] + [8, 8, ca.sw_ops_bound(640, 600)])
    assert res2.rc == E_CAPACITY
    assert tuple(res2.row(2, 1)) == ZERO + (ca.SW_STOP,) and int(res2.n_ops[res2.index(2, 1)]) == 0
    assert np.array_equal(res2.rows[: len(res.rows) - 2], res.rows[2:]) and np.array_equal(res2.n_ops[: len(res.rows) - 2], res.n_ops[2:])
    assert res2.ops(2, 2) == res.ops(1, 3) and (res2.ops_buf[int(res2.ops_off[res2.index(2, 1)]) : int(res2.ops_off[res2.index(2, 2)])] == SENT).all()


# ---- 6. composition ----------------------------------------------------------------------------------------------------------------------------------------------

def same(a, sa, b, sb):
    """Sequence sa of result a and sequence sb of result b: row, op count, ops."""
    na, nb = int(a.n_ops[sa]), int(b.n_ops[sb])
    oa, ob = int(a.ops_off[sa]), int(b.ops_off[sb])
    return np.array_equal(a.rows[sa], b.rows[sb]) and na == nb and np.array_equal(a.ops_buf[oa : oa + na], b.ops_buf[ob : ob + nb])


def test_a_pairs_row_and_ops_do_not_depend_on_the_batch(eng):
    pairs = sp.mixed_pairs(300)
    order = list(range(len(pairs)))
    random.Random(3).shuffle(order)
    groups = as_groups([pairs[i] for i in order])
    res, slots = run(eng, groups, eqx=True)
    check(res, slots, groups, True, "mixed", only=lambda k: order[k] % 10 == 0)  # (the pairs tests/test_sw_path_cpu.py holds the reference to the oracle for)
    for g in range(len(groups)):
        invariants(res, groups, g, 1)
    lens = sorted(range(len(pairs)), key=lambda i: len(pairs[i][0]))
    for i in lens[:3] + lens[148:152] + lens[-5:] + [i for i in range(len(pairs)) if len(pairs[i][1]) > sp.LDS_RMAX][:3]:  # every launch class, alone in its batch
        alone, _ = run(eng, as_groups([pairs[i]]), eqx=True)
        assert same(alone, 1, res, 2 * order.index(i) + 1), i


def test_one_group_of_200_queries_equals_200_groups(eng):
    rng = random.Random(0x6200)
    ref = pop.rand_seq(rng, 900)
    queries = []
    for i in range(200):
        a = rng.randrange(0, 700)
        queries.append(pop.rand_seq(rng, 10) + pop.ont_copy(rng, ref[a : a + rng.randrange(20, 200)]) + pop.rand_seq(rng, 10))
    one, slots_one = run(eng, [[ref] + queries])
    many, _ = run(eng, [[ref, q] for q in queries])
    for i in range(200):
        assert same(one, 1 + i, many, 2 * i + 1), i
        invariants(one, [[ref] + queries], 0, 1 + i)
    check(one, slots_one, [[ref] + queries], False, "one group", only=lambda k: k % 8 == 0)


# ---- 7. more pairs than waves --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", [0, 1, 2])
def test_more_pairs_than_waves_in_every_launch(eng, cls):
    """A wave that takes a second and a third pair reuses the slab, the direction scratch and the step buffer the pair before left (sw_path_probes.CROWDS:
    more pairs than the launch has waves, counted against plan_sw_path in tests/test_sw_path_cpu.py).  Every row against the oracle, every path by its
    invariants, every CROWD_SAMPLE-th pair op by op against the reference."""
    groups = [list(g) for g in sp.crowd(*pp.CROWDS[cls])]
    res, slots = run(eng, groups, eqx=cls == 1)
    print(f"class {cls}: {sum(len(g) - 1 for g in groups)} pairs, stages {eng.timings()}")
    assert res.rc == 0
    check(res, slots, groups, cls == 1, f"crowd {cls}", only=lambda k: k % pp.CROWD_SAMPLE[cls] == 0)
    for g, grp in enumerate(groups):
        for k in range(1, len(grp)):
            invariants(res, groups, g, k)


# ---- 8. entry points ---------------------------------------------------------------------------------------------------------------------------------------------------

def device_run(eng, hb, off, flags, on_stream):
    import torch

    dev = torch.device("cuda", eng.device)

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    S = len(hb.seq_len)
    t_in = (up(hb.win_first_seq, np.int32), up(hb.seq_len, np.int32), up(hb.seq_word_off, np.int64), up(np.concatenate([hb.bases, np.zeros(4, np.uint32)]), np.int32),
            up(off, np.int64))
    t_rows = torch.full((S * 8 + 16,), 99, dtype=torch.int32, device=dev)
    t_nops = torch.full((S + 16,), 77, dtype=torch.int32, device=dev)
    t_ops = torch.full((int(off[-1]) + 16,), 0x1234ABCD, dtype=torch.int32, device=dev)
    b = Batch(hb.n_windows, S, len(hb.bases), t_in[0].data_ptr(), t_in[1].data_ptr(), t_in[2].data_ptr(), t_in[3].data_ptr())
    paths = SwPaths(t_ops.data_ptr(), t_in[4].data_ptr(), t_nops.data_ptr())
    torch.cuda.synchronize(dev)
    if on_stream:
        s = torch.cuda.Stream(dev)
        eng.sw_path_device(b, C.c_void_p(t_rows.data_ptr()), paths, flags, C.c_void_p(s.cuda_stream))
        s.synchronize()
    else:
        eng.sw_path_device(b, C.c_void_p(t_rows.data_ptr()), paths, flags)
    torch.cuda.synchronize(dev)
    rows, nops, ops = t_rows.cpu().numpy(), t_nops.cpu().numpy(), t_ops.cpu().numpy()
    assert (rows[S * 8 :] == 99).all() and (nops[S:] == 77).all() and (ops[int(off[-1]) :] == 0x1234ABCD).all(), "words behind the arrays were written"
    return rows[: S * 8].reshape(-1, 8), nops[:S].view(np.uint32), ops[: int(off[-1])].view(np.uint32)


def test_both_entry_points_and_other_runs_alternate_on_one_engine():
    pairs = sp.mixed_pairs()[:40] + [sp.planted(10), pp.one_deletion(32), sp.long_pairs()["q2049xr2048"]]
    groups = as_groups(pairs) + [[], [pairs[0][1]]]
    hb = ca.pack_piles(groups)
    prm = ca.Params(9, 4, 8, 2, 150)
    e = ca.Engine(prm)
    try:
        piles = synth_host(ca.SynthSpec.pacbio(24, 30))
        exp, _ = oracle_lib.oracle_run(prm, piles)
        poa_group = pop.probe("100x10")

        def window_and_poa_runs():
            got = e.run(piles)
            for w in range(piles.n_windows):
                assert got.status[w] == exp.status[w] and got.consensus(w) == exp.consensus(w) and np.array_equal(got.solid_kmers(w), exp.solid_kmers(w)), w
            assert e.poa([poa_group]).consensus(0) == pop.oracle_consensus(poa_group, 150)

        window_and_poa_runs()
        sw_before = e.sw(hb, want_indels=True)
        host = e.sw_path(hb)  # Engine.sw_path: the default slots
        assert {"sw_order", "sw_path", "sw_path_wide", "sw_path_long", "total"} <= set(e.timings()), e.timings()
        assert not {"sw_align", "sw_align_wide", "sw_align_long"} & set(e.timings())
        sw_after = e.sw(hb, want_indels=True)
        assert np.array_equal(sw_before.rows, sw_after.rows)  # cw_sw_run's rows before and after a path run
        both = (sw_before.rows[:, 7] == ca.SW_ALIGNED) & (host.rows[:, 7] == ca.SW_ALIGNED)
        assert both.sum() >= 40 and np.array_equal(sw_before.rows[both], host.rows[both])  # where both runs say ALIGNED their rows are equal
        window_and_poa_runs()
        for on_stream in (False, True):
            rows, nops, ops = device_run(e, hb, host.ops_off, 0, on_stream)
            assert np.array_equal(rows, host.rows) and np.array_equal(nops, host.n_ops), on_stream
            for s in range(len(nops)):
                o = int(host.ops_off[s])
                assert np.array_equal(ops[o : o + int(nops[s])], host.ops_buf[o : o + int(nops[s])]), (on_stream, s)
                assert (ops[o + int(nops[s]) : int(host.ops_off[s + 1])] == 0x1234ABCD).all(), (on_stream, s)
        window_and_poa_runs()
        again = e.sw_path(hb)
        assert np.array_equal(again.rows, host.rows) and np.array_equal(again.n_ops, host.n_ops) and np.array_equal(again.ops_buf, host.ops_buf)
    finally:
        e.close()
    for g in range(len(pairs)):
        invariants(host, groups, g, 1)
    assert host.cigar(41, 1) == "150M32D150M" and host.ops(41, 1) == [(150, 0), (32, 2), (150, 0)] and host.cigar(41, 0) == ""
    for g in (0, 7, 40, 41, 42):
        q, r = pairs[g]
        e_row, e_n, e_ops = pp.expected(q, r)
        assert tuple(int(x) for x in host.row(g, 1)) == e_row and host.ops(g, 1) == list(e_ops), g


def test_bad_arguments_are_refused_before_anything_is_launched(eng):
    hb = ca.pack_piles(as_groups([sp.embedded(7, 50, 150)]))
    ok = eng.sw_path(hb)
    stages = eng.timings()
    b = hb.c_struct()
    rows = np.full((2, 8), 99, np.int32)
    ops, off, n_ops = np.full(400, SENT, np.uint32), np.array([0, 200, 400], np.uint64), np.full(2, 77, np.uint32)
    p = C.c_void_p(rows.ctypes.data)
    paths = SwPaths(_ptr(ops), _ptr(off), _ptr(n_ops))
    big = Batch(eng.max_batch_windows() + 1, b.n_seqs, b.n_words, b.win_first_seq, b.seq_len, b.seq_word_off, b.bases)
    for fn in (eng.lib.cw_sw_path_run, lambda *a: eng.lib.cw_sw_path_run_device(*a, None)):
        for flags in (1, 2, 8, 5):  # cw_sw_run's flag, the value its test pins as invalid, an unknown one, a known beside an unknown one
            assert fn(eng.handle, C.byref(b), p, C.byref(paths), flags) == E_INVALID, flags
        assert fn(eng.handle, C.byref(b), None, C.byref(paths), 0) == E_INVALID
        assert fn(eng.handle, C.byref(b), p, None, 0) == E_INVALID
        assert fn(eng.handle, None, p, C.byref(paths), 0) == E_INVALID
        for missing in range(3):
            members = [_ptr(ops), _ptr(off), _ptr(n_ops)]
            members[missing] = None
            assert fn(eng.handle, C.byref(b), p, C.byref(SwPaths(*members)), 0) == E_INVALID, missing
        assert fn(eng.handle, C.byref(big), p, C.byref(paths), 0) == E_INVALID
    assert (rows == 99).all() and (ops == SENT).all() and (n_ops == 77).all() and eng.timings() == stages, "a refused call launched something"
    again = eng.sw_path(hb)
    assert np.array_equal(again.rows, ok.rows) and again.cigar(0, 1) == ok.cigar(0, 1) != ""
