"""The re-assembly's local aligner as a batched operator (include/consent_amd.h cw_sw_run / cw_sw_run_device; csrc/cw_sw_op.h): every row equals what the
oracle's cwo_ssw (tests/sw_op_probes.py oracle) returns for that (query, reference) pair -- five numbers, seven with the indel totals, and the status -- for
every sweep instance and its edges, the long launch, the tie rules, pairs that do not align, the banded traceback's three paths, beside pairs that stop, in
any batch composition, and through both entry points of one engine that also runs windows and POA groups."""
import ctypes as C
import random

import numpy as np
import pytest

import consent_amd as ca
import oracle_lib
import poa_op_probes as pp
import sw_op_probes as sp
from consent_amd.engine import Batch, synth_host

pytestmark = pytest.mark.gpu
E_INVALID, E_CAPACITY = -1, -4
ZERO = (0, 0, -1, 0, -1, 0, 0)


@pytest.fixture(scope="module")
def eng():
    e = ca.Engine(ca.Params(*sp.PRM))
    yield e
    e.close()


def expect(query, ref, indels):
    o = sp.oracle(query, ref)
    return o if indels else o[:5] + (0, 0)


def check_rows(res, groups, indels, what, status=None):
    """Every row of `groups` (lists: reference first) against the oracle; status[(g, member)] overrides the status the scratch rule gives the pair
    (SW_NO_INDELS, with ins = del = 0, where the banded traceback's directions outgrow a wave's scratch: a long noisy pair)."""
    status = status or {}
    for g, grp in enumerate(groups):
        for k, seq in enumerate(grp):
            row = tuple(int(x) for x in res.row(g, k))
            if k == 0:
                assert row == ZERO + (ca.SW_IS_REF,), f"{what}: group {g}: the reference's row {row}"
                continue
            st = status.get((g, k), sp.expected_status(seq, grp[0]) if indels else ca.SW_ALIGNED)  # (by the header's scratch rule: sw_op_probes)
            exp = expect(seq, grp[0], indels and st == ca.SW_ALIGNED)
            print(f"{what}: group {g} member {k}: {len(seq)} x {len(grp[0])} -> {row}")
            assert row == exp + (st,), f"{what}: group {g} member {k} ({len(seq)} x {len(grp[0])}): {row}, the oracle {exp + (st,)}"


def as_groups(pairs):
    return [[r, q] for q, r in pairs]


# ---- 1. every sweep instance and its edges ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def instances(eng):
    names = list(sp.instance_pairs())
    groups = as_groups(sp.instance_pairs().values())
    return names, groups, eng.sw(groups), eng.sw(groups, want_indels=True)


@pytest.mark.parametrize("name", list(sp.instance_pairs()))
def test_every_sweep_instance_and_reference_length_equals_the_oracle(instances, name):
    names, groups, plain, full = instances
    g = names.index(name)
    assert plain.rc == 0 and full.rc == 0
    check_rows(ca.SwRows(plain.rows[2 * g : 2 * g + 2], [0, 2]), [groups[g]], False, name)
    check_rows(ca.SwRows(full.rows[2 * g : 2 * g + 2], [0, 2]), [groups[g]], True, name + " with indels")


# ---- 2. the long launch -------------------------------------------------------------------------------------------------------------------------------

def test_long_queries_alone_and_beside_short_ones(eng):
    long_groups = as_groups(list(sp.long_pairs().values()) + [sp.embedded(8, 2100, 3000)])  # the last: a reference beyond LDS in the long launch
    short_groups = as_groups([sp.embedded(5, 100, 600), sp.embedded(5, 700, 600)])
    only_long = eng.sw(long_groups, want_indels=True)
    t = eng.timings()
    assert {"sw_order", "sw_align", "sw_align_wide", "sw_align_long", "total"} <= set(t), t
    check_rows(only_long, long_groups, True, "only long pairs")
    assert [int(only_long.row(g, 1)[7]) for g in range(3)] == [ca.SW_ALIGNED, ca.SW_NO_INDELS, ca.SW_NO_INDELS]  # 2 049: the band fits; 2 500 and 9 000: it does not
    both = eng.sw(short_groups + long_groups)
    check_rows(both, short_groups + long_groups, False, "long beside short")
    none_long = eng.sw(short_groups)  # the long kernel finds nothing to do
    check_rows(none_long, short_groups, False, "no long pair")


# ---- 3. ties, nothing aligns, degenerate groups ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("indels", [False, True])
def test_tie_rules(eng, indels):
    groups = as_groups(sp.tie_pairs().values())
    check_rows(eng.sw(groups, want_indels=indels), groups, indels, "ties")


@pytest.mark.parametrize("indels", [False, True])
def test_nothing_aligns_empty_sequences_and_degenerate_groups(eng, indels):
    n = sp.nothing_pairs()
    ref = pp.rand_seq(random.Random(9), 120)
    groups = as_groups(n.values()) + [[ref], [], [ref, "", ref[10:90], ""], []]
    res = eng.sw(groups, want_indels=indels)
    assert res.rc == 0 and len(res.rows) == sum(len(g) for g in groups)
    check_rows(res, groups, indels, "nothing aligns")
    for g in range(3):
        assert tuple(res.row(g, 1)) == ZERO + (ca.SW_ALIGNED,)
    assert tuple(res.row(5, 2)[:5]) == (160, 10, 89, 0, 79)
    empty = eng.sw([[], []])  # no sequence at all: nothing to run
    assert empty.rc == 0 and empty.rows.shape == (0, 8)


# ---- 4. indel totals ---------------------------------------------------------------------------------------------------------------------------------------

def test_indel_totals_on_the_lanes_serial_and_beyond_the_scratch(eng):
    groups = as_groups([sp.planted(10), sp.planted(40), sp.planted(300), sp.unbalanced()])
    full = eng.sw(groups, want_indels=True)
    assert full.rc == 0  # CW_SW_NO_INDELS is not an error
    check_rows(full, groups, True, "planted indels", status={(2, 1): ca.SW_NO_INDELS})
    assert tuple(full.row(0, 1)[5:7]) == (10, 10) and tuple(full.row(1, 1)[5:7]) == (40, 40) and tuple(full.row(3, 1)[5:7]) == (0, 7)
    assert tuple(full.row(2, 1)[5:]) == (0, 0, ca.SW_NO_INDELS) and tuple(full.row(2, 1)[:5]) == sp.oracle(*sp.planted(300))[:5]
    plain = eng.sw(groups)
    check_rows(plain, groups, False, "planted indels, totals not asked for")
    assert (plain.rows[:, 5:7] == 0).all() and (plain.rows[1::2, 7] == ca.SW_ALIGNED).all()
    assert np.array_equal(plain.rows[:, :5], full.rows[:, :5])


# ---- 5. capacities -----------------------------------------------------------------------------------------------------------------------------------------

def test_a_pair_beyond_a_capacity_stops_alone(eng):
    rng = random.Random(0xCA9)
    ok_q, ok_r = sp.embedded(6, 300, 600)
    long_q = pp.rand_seq(rng, sp.QMAX + 1)
    long_r = pp.rand_seq(rng, sp.RMAX + 1)
    last_r = pp.rand_seq(rng, sp.RMAX)  # the longest reference that is taken
    last_q = last_r[7000:7300]
    groups = [[ok_r, ok_q, long_q, ok_q[:150]], [long_r, ok_q, ok_q[:40]], [last_r, last_q], [ok_r, ok_q]]
    hb = ca.pack_piles(groups)
    rows = np.full((len(hb.seq_len), 8), 99, np.int32)
    b = hb.c_struct()
    rc = eng.lib.cw_sw_run(eng.handle, C.byref(b), C.c_void_p(rows.ctypes.data), ca.SW_WANT_INDELS)
    assert rc == E_CAPACITY
    res = ca.SwRows(rows, hb.win_first_seq, rc)
    stops = {(0, 2): ca.SW_STOP, (1, 1): ca.SW_STOP, (1, 2): ca.SW_STOP}
    for (g, k) in stops:
        assert tuple(res.row(g, k)) == ZERO + (ca.SW_STOP,), (g, k, res.row(g, k))
    for g, k in ((0, 1), (0, 3), (2, 1), (3, 1)):
        q, r = groups[g][k], groups[g][0]
        assert tuple(res.row(g, k)) == sp.oracle(q, r) + (ca.SW_ALIGNED,), (g, k)
    assert tuple(res.row(2, 1)[:5]) == (600, 7000, 7299, 0, 299)
    assert eng.sw(groups[2:]).rc == 0


# ---- 6. composition ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed(eng):
    pairs = sp.mixed_pairs()
    out = []
    for seed in (1, 2):
        order = list(range(len(pairs)))
        random.Random(seed).shuffle(order)
        res = eng.sw(as_groups([pairs[i] for i in order]), want_indels=True)
        rows = np.zeros((len(pairs), 8), np.int32)
        rows[order] = res.rows[1::2]
        out.append((order, rows))
    return pairs, out


def test_a_pairs_row_does_not_depend_on_the_batch(eng, mixed):
    pairs, ((o1, r1), (o2, r2)) = mixed
    assert o1 != o2 and np.array_equal(r1, r2)
    for i, (q, r) in enumerate(pairs):
        assert sp.expected_status(q, r) == ca.SW_ALIGNED
        assert tuple(int(x) for x in r1[i]) == sp.oracle(q, r) + (ca.SW_ALIGNED,), (i, len(q), len(r))
    for i in range(len(pairs)):  # each alone in its batch
        alone = eng.sw(as_groups([pairs[i]]), want_indels=True)
        assert np.array_equal(alone.rows[1], r1[i]), i


@pytest.mark.parametrize("indels", [False, True])
@pytest.mark.parametrize("cls", [0, 1, 2])
def test_more_pairs_than_waves_in_every_launch(eng, cls, indels):
    """A wave that takes a second and a third pair unpacks into the buffers the pair before left -- slab, reversed prefix used for directions, direction
    scratch -- and takes places of the order beyond the grid: batches of more pairs than their launch has waves (sw_op_probes.CROWDS; the counts are checked
    against plan_sw in tests/test_sw_op_cpu.py), every row against the oracle."""
    groups = [list(g) for g in sp.crowd(*sp.CROWDS[cls])]
    n_pairs = sum(len(g) - 1 for g in groups)
    res = eng.sw(groups, want_indels=indels)
    assert res.rc == 0 and len(res.rows) == n_pairs + len(groups)
    exp = np.array([ZERO + (ca.SW_IS_REF,) if k == 0 else expect(q, g[0], indels) + (ca.SW_ALIGNED,) for g in groups for k, q in enumerate(g)], np.int32)
    bad = np.flatnonzero((res.rows != exp).any(axis=1))
    print(f"class {cls}, indels {indels}: {n_pairs} pairs, stages {eng.timings()}")
    assert len(bad) == 0, (len(bad), [(int(i), res.rows[i].tolist(), exp[i].tolist()) for i in bad[:5]])


def test_one_group_of_200_queries_equals_200_groups(eng):
    rng = random.Random(0x6200)
    ref = pp.rand_seq(rng, 900)
    queries = []
    for i in range(200):
        a = rng.randrange(0, 700)
        queries.append(pp.rand_seq(rng, 10) + pp.ont_copy(rng, ref[a : a + rng.randrange(20, 200)]) + pp.rand_seq(rng, 10))
    one = eng.sw([[ref] + queries])
    many = eng.sw([[ref, q] for q in queries])
    assert np.array_equal(one.rows[1:], many.rows[1::2])
    for i in range(0, 200, 7):
        assert tuple(int(x) for x in one.row(0, 1 + i)) == expect(queries[i], ref, False) + (ca.SW_ALIGNED,), i


# ---- 7. both entry points, one engine ----------------------------------------------------------------------------------------------------------------------

def device_run(eng, hb, flags, on_stream):
    import torch

    dev = torch.device("cuda", eng.device)

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    t_in = (up(hb.win_first_seq, np.int32), up(hb.seq_len, np.int32), up(hb.seq_word_off, np.int64), up(np.concatenate([hb.bases, np.zeros(4, np.uint32)]), np.int32))
    t_rows = torch.full((len(hb.seq_len) * 8 + 16,), 99, dtype=torch.int32, device=dev)
    b = Batch(hb.n_windows, len(hb.seq_len), len(hb.bases), t_in[0].data_ptr(), t_in[1].data_ptr(), t_in[2].data_ptr(), t_in[3].data_ptr())
    torch.cuda.synchronize(dev)
    if on_stream:
        s = torch.cuda.Stream(dev)
        eng.sw_device(b, C.c_void_p(t_rows.data_ptr()), flags, C.c_void_p(s.cuda_stream))
        s.synchronize()
    else:
        eng.sw_device(b, C.c_void_p(t_rows.data_ptr()), flags)
    torch.cuda.synchronize(dev)
    out = t_rows.cpu().numpy()
    assert (out[len(hb.seq_len) * 8 :] == 99).all(), "words behind the last row were written"
    return out[: len(hb.seq_len) * 8].reshape(-1, 8)


def test_both_entry_points_and_other_runs_alternate_on_one_engine():
    pairs = sp.mixed_pairs()[:40] + [sp.planted(10), sp.long_pairs()["q2049xr2048"]]
    groups = as_groups(pairs) + [[], [pairs[0][1]]]
    hb = ca.pack_piles(groups)
    prm = ca.Params(9, 4, 8, 2, 150)
    e = ca.Engine(prm)
    try:
        piles = synth_host(ca.SynthSpec.pacbio(24, 30))
        exp, _ = oracle_lib.oracle_run(prm, piles)
        poa_group = pp.probe("100x10")

        def window_and_poa_runs():
            got = e.run(piles)
            for w in range(piles.n_windows):
                assert got.status[w] == exp.status[w] and got.consensus(w) == exp.consensus(w) and np.array_equal(got.solid_kmers(w), exp.solid_kmers(w)), w
            assert e.poa([poa_group]).consensus(0) == pp.oracle_consensus(poa_group, 150)

        window_and_poa_runs()
        host = e.sw(hb, want_indels=True)
        assert {"sw_order", "sw_align", "sw_align_wide", "sw_align_long", "total"} <= set(e.timings()), e.timings()
        window_and_poa_runs()
        for on_stream in (False, True):
            assert np.array_equal(device_run(e, hb, ca.SW_WANT_INDELS, on_stream), host.rows), on_stream
        window_and_poa_runs()
        assert np.array_equal(e.sw(hb, want_indels=True).rows, host.rows)
    finally:
        e.close()
    check_rows(host, groups, True, "alternation")


def test_bad_arguments_are_refused_before_anything_is_launched(eng):
    hb = ca.pack_piles(as_groups([sp.embedded(7, 50, 150)]))
    ok = eng.sw(hb)
    stages = eng.timings()
    b = hb.c_struct()
    rows = np.full((2, 8), 99, np.int32)
    p = C.c_void_p(rows.ctypes.data)
    big = Batch(eng.max_batch_windows() + 1, b.n_seqs, b.n_words, b.win_first_seq, b.seq_len, b.seq_word_off, b.bases)
    for fn in (eng.lib.cw_sw_run, lambda *a: eng.lib.cw_sw_run_device(*a, None)):
        assert fn(eng.handle, C.byref(b), p, 2) == E_INVALID  # an unknown flag
        assert fn(eng.handle, C.byref(b), None, 0) == E_INVALID
        assert fn(eng.handle, None, p, 0) == E_INVALID
        assert fn(eng.handle, C.byref(big), p, 0) == E_INVALID
    assert (rows == 99).all() and eng.timings() == stages, "a refused call launched something"
    assert np.array_equal(eng.sw(hb).rows, ok.rows)


# ---- 8. the re-assembly's own inputs -------------------------------------------------------------------------------------------------------------------------

def test_window_consensuses_against_read_slices(eng):
    """Inputs shaped like alignConsensus's: a window's consensus (the oracle's own) as the query; as the reference a stand-in for the slice of the read around
    the window -- the window's template (which is that stretch of the read) between 50 random bases on either side, not a slice cut from a real read."""
    prm = ca.Params(9, 4, 8, 2, 150)
    piles = synth_host(ca.SynthSpec.ont(36, 20))
    cons, _ = oracle_lib.oracle_run(prm, piles)
    rng = random.Random(0xA11C)
    groups = []
    for w in range(piles.n_windows):
        c = cons.consensus(w)
        if c:
            groups.append([pp.rand_seq(rng, 50) + piles.pile(w)[0] + pp.rand_seq(rng, 50), c.upper()])
    assert len(groups) >= 24
    check_rows(eng.sw(groups, want_indels=True), groups, True, "re-assembly inputs")
