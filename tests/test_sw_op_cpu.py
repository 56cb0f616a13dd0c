"""The alignment operator without a GPU (include/consent_amd.h cw_sw_run / cw_sw_run_device, csrc/cw_plan.h plan_sw): the symbols exist, bad arguments are
refused before the device is touched, the plan of an alignment run holds what such a run needs -- and the probes of tests/test_gpu_sw_op.py really have the
properties those tests rely on, by the oracle (oracle/cw_oracle_c.cpp cwo_ssw)."""
import ctypes as C

import numpy as np
import pytest

import consent_amd as ca
import sw_op_probes as sp
from consent_amd import engine as en
from consent_amd.engine import _ptr

E_INVALID = -1
CUS = 256
PLAN = ["total", "order", "gref", "long_state", "dirs", "wgs0", "wgs1", "wgs_long", "dir_waves", "dir_bytes"]
GREF_BYTES, LONG_WAVE_BYTES = 16384, 16384 + 2 * 32768 + 256 * 64 * 20  # csrc/cw_sw_op.h CW_SW_GREF_BYTES, CW_SW_LONG_WAVE_BYTES


def lib():
    return ca.load_library()


def sw_plan(groups, seqs, words, flags=0, cus=CUS):
    out = np.zeros(10, np.uint64)
    rc = lib().cw_debug_sw_plan(groups, seqs, words, cus, flags, _ptr(out))
    return rc, dict(zip(PLAN, (int(x) for x in out)))


def test_the_new_symbols_and_constants_are_exported():
    l = lib()
    for name in ("cw_sw_run", "cw_sw_run_device", "cw_debug_sw_plan"):
        assert hasattr(l, name), name
    assert (ca.SW_ALIGNED, ca.SW_NO_INDELS, ca.SW_STOP, ca.SW_IS_REF, ca.SW_WANT_INDELS) == (0, 1, 2, 3, 1)
    assert en.SW_ROW == 8 and en.SW_STATUS == 7 and en.SW_QMAX == sp.QMAX == 32768 and en.SW_RMAX == sp.RMAX and sp.RMAX >= 2048
    assert hasattr(ca.Engine, "sw") and hasattr(ca.Engine, "sw_device")


def test_null_and_malformed_arguments_are_invalid_without_a_device():
    l = lib()
    hb = ca.pack_piles([["ACGTACGT", "ACGA"]])
    b = hb.c_struct()
    rows = np.full((2, 8), 77, np.int32)
    assert l.cw_sw_run(None, C.byref(b), _ptr(rows), 0) == E_INVALID  # no engine
    assert l.cw_sw_run_device(None, C.byref(b), _ptr(rows), 0, None) == E_INVALID
    assert l.cw_sw_run(None, None, _ptr(rows), 0) == E_INVALID
    assert l.cw_sw_run(None, C.byref(b), None, 1) == E_INVALID
    assert (rows == 77).all()
    out = np.zeros(10, np.uint64)
    assert l.cw_debug_sw_plan(4, 8, 8, CUS, 0, None) == E_INVALID
    assert l.cw_debug_sw_plan(4, 8, 8, 0, 0, _ptr(out)) == E_INVALID
    assert l.cw_debug_sw_plan(4, 8, 8, CUS, 2, _ptr(out)) == E_INVALID  # a flag the call does not know


def test_sw_plan_holds_what_a_run_needs():
    seqs = 100000
    rc, p = sw_plan(1000, seqs, seqs * 10)
    assert rc == 0
    assert p["order"] >= 2 * 4 * seqs, p  # a reference index and a place in the order per sequence
    assert p["dirs"] == 0 and p["dir_waves"] == 0 and p["dir_bytes"] == 0, p  # no traceback scratch unless asked for
    assert p["wgs0"] == 4 * CUS and p["wgs1"] == CUS and p["wgs_long"] == 256, p
    assert p["gref"] == p["wgs0"] * 4 * GREF_BYTES and p["long_state"] == p["wgs_long"] * LONG_WAVE_BYTES, p
    assert p["total"] == p["order"] + p["gref"] + p["long_state"] + p["dirs"], p
    rc, q = sw_plan(1000, seqs, seqs * 10, ca.SW_WANT_INDELS)
    assert rc == 0 and q["dir_bytes"] == en.SW_DIR_BYTES == 1 << 20  # the stitch's CW_ST_DIR_BYTES
    assert q["wgs0"] == 256 and q["dir_waves"] == 1024 and q["dirs"] == 1024 << 20, q  # the stitch's grid limit
    assert q["dir_waves"] >= max(4 * q["wgs0"], 4 * q["wgs1"], q["wgs_long"])  # every wave of every launch has its own
    rc, small = sw_plan(1, 3, 30, ca.SW_WANT_INDELS)
    assert rc == 0 and (small["wgs0"], small["wgs1"], small["wgs_long"], small["dir_waves"]) == (1, 1, 3, 4), small
    assert small["total"] < 8 << 20, small


@pytest.mark.parametrize("flags", [0, 1])
def test_sw_plan_is_monotone_in_pairs_and_does_not_depend_on_bases(flags):
    by_seqs = [sw_plan(max(1, s // 8), s, s * 40, flags)[1] for s in (1, 2, 5, 64, 1000, 1024, 5000, 100000, 2000000)]
    for a, b in zip(by_seqs, by_seqs[1:]):
        assert all(a[k] <= b[k] for k in PLAN), (a, b)
        assert a["order"] < b["order"] or b["order"] - 256 < a["order"]  # (parts are rounded up to 256 bytes)
    assert by_seqs[0]["total"] < by_seqs[-1]["total"]
    by_bases = [sw_plan(100, 5000, w, flags)[1] for w in (5000, 50000, 5000000)]  # a pair's buffers are its wave's, whatever the batch holds
    assert by_bases[0] == by_bases[1] == by_bases[2]
    by_groups = [sw_plan(g, 5000, 50000, flags)[1] for g in (1, 50, 5000)]
    assert by_groups[0] == by_groups[1] == by_groups[2]


# ---- the probes, by the oracle ------------------------------------------------------------------------------------------------------------------------

def test_embedded_pairs_have_interior_ends():
    """(Under CW_SSW_* -- a gap of g bases costs 2 + g, a match gains 2 -- unrelated sequences align with a positive drift, so an alignment runs on into the
    flanks for a while: the ends are interior for most pairs, not where the copy ends, and a few reach an end of the query.)"""
    interior = total = 0
    for name, (q, r) in {**sp.instance_pairs(), **sp.long_pairs()}.items():
        score, rb, re, qb, qe, _, _ = sp.oracle(q, r)
        assert score > 0 and 0 <= rb <= re < len(r) and 0 <= qb <= qe < len(q), (name, score)
        if len(q) >= 127 and len(r) >= 600:
            total += 1
            interior += qb > 0 and qe < len(q) - 1 and rb > 0 and re < len(r) - 1
            assert rb > 0 and re < len(r) - 1, (name, (rb, re, qb, qe), len(q), len(r))
    print(f"{interior} of {total} pairs have all four ends interior")
    assert 2 * interior > total, (interior, total)
    assert sorted({len(q) for q, _ in sp.instance_pairs().values()} - {200, 700}) == sp.QUERY_LENS
    assert sorted({len(r) for _, r in sp.instance_pairs().values()}) == sp.REF_LENS
    assert [len(q) for q, _ in sp.long_pairs().values()] == sp.LONG_QUERY_LENS


def _last_column(q, r, col):
    """Smith-Waterman scores of reference column `col` for every query position (include/cw_policy.h CW_SSW_*), plain Python: small inputs only."""
    m = len(q)
    H, E = [0] * m, [0] * m
    for i in range(col + 1):
        f = diag = 0
        Hn = [0] * m
        for j in range(m):
            e = max(E[j] - sp.GAP_EXT, H[j] - sp.GAP_OPEN, 0)
            h = max(diag + (sp.MATCH if q[j] == r[i] else -sp.MISMATCH), e, f, 0)
            diag, Hn[j], E[j] = H[j], h, e
            f = max(f - sp.GAP_EXT, h - sp.GAP_OPEN, 0)
        H = Hn
    return H


def test_tie_probes_have_their_ties():
    t = sp.tie_pairs()
    q, r = t["query twice in the reference"]
    first, second = r.find(q), r.rfind(q)
    assert 0 <= first < second
    o = sp.oracle(q, r)
    assert o[:5] == (2 * len(q), first, first + len(q) - 1, 0, len(q) - 1), o  # the first end wins
    q, r = t["two query positions in one column"]
    o = sp.oracle(q, r)
    col = _last_column(q, r, o[2])
    assert max(col) == o[0] and col.count(o[0]) == 2 and col.index(o[0]) == o[4], (o, col)  # two positions hold the best score; the smaller one is reported
    q, r = t["periodic reference"]
    assert len(q) == 14 and sp.oracle(q, r)[:5] == (28, 0, 13, 0, 13)


def test_nothing_aligns_probes():
    for name, (q, r) in sp.nothing_pairs().items():
        assert sp.oracle(q, r) == (0, 0, -1, 0, -1, 0, 0), name


@pytest.mark.parametrize("g", [10, 40, 300])
def test_planted_pairs_have_equal_spans_and_g_of_each(g):
    q, r = sp.planted(g)
    score, rb, re, qb, qe, ins, dele = sp.oracle(q, r)
    assert score > 0 and ins == dele == g, (g, score, ins, dele)
    r_span, q_span = re - rb + 1, qe - qb + 1
    assert r_span == q_span >= 1500, (r_span, q_span)
    # the band starts at 1 and doubles until it holds the diagonal offset g of the middle block (a narrower band cannot reach the score: it would have to
    # align 500 unrelated bases where the full alignment pays two gaps)
    bands = sp.bands_tried(0, g)
    assert bands[0] == 1 and bands[-1] == sp.final_band(0, g)
    if g == 10:  # the band's row on the lanes of a wave: 2 * band + 1 <= 64
        assert bands[-1] == 16 and all(sp.dir_fits(r_span, q_span, b) for b in bands)
    if g == 40:  # the serial path: wider than a wave
        assert bands[-1] == 64 and 2 * 64 + 1 > 64 and all(sp.dir_fits(r_span, q_span, b) for b in bands)
    if g == 300:  # the direction bytes pass the per-wave scratch before the band holds the offset: CW_SW_NO_INDELS
        assert bands[-1] == 512 and sp.dir_fits(r_span, q_span, 64) and not sp.dir_fits(r_span, q_span, 128), (r_span, q_span)


def test_the_restated_banded_pass_reaches_the_score_where_the_band_holds_the_offset():
    """sw_op_probes.banded_best / expected_status, which give the GPU tests the status the scratch rule assigns a pair."""
    code = {c: k for k, c in enumerate("ACGT")}
    for g, narrow, wide in ((10, 8, 16), (40, 32, 64)):
        q, r = sp.planted(g)
        score, rb, re, qb, qe, _, _ = sp.oracle(q, r)
        rs, qs = np.array([code[c] for c in r[rb : re + 1]]), np.array([code[c] for c in q[qb : qe + 1]])
        assert sp.banded_best(rs, qs, narrow) < score == sp.banded_best(rs, qs, wide), g
        assert sp.expected_status(q, r) == sp.ALIGNED
    assert sp.expected_status(*sp.planted(300)) == sp.NO_INDELS and sp.expected_status(*sp.unbalanced()) == sp.ALIGNED
    assert sp.dir_fits(1800, 1800, 96) and not sp.dir_fits(1800, 1800, 97)  # 3 x 193 x 1800 <= 2^20 < 3 x 195 x 1800
    assert sp.dir_fits(500, 500, 10 ** 6) and not sp.dir_fits(2009, 2019, 88)  # a band wider than the matrix stores reference span + 1 cells a row
    # long noisy pairs: 2 000 aligned bases of each with ~200 inserted and deleted ones need a band whose directions pass a wave's 1 MiB
    by_len = {len(q): sp.expected_status(q, r) for q, r in sp.long_pairs().values()}
    assert by_len == {2049: sp.ALIGNED, 2500: sp.NO_INDELS, 9000: sp.NO_INDELS}, by_len
    assert all(sp.expected_status(q, r) == sp.ALIGNED for q, r in sp.instance_pairs().values())


def test_unbalanced_pair_differs_by_seven():
    q, r = sp.unbalanced()
    score, rb, re, qb, qe, ins, dele = sp.oracle(q, r)
    assert score > 0 and (ins, dele) == (0, 7) and (re - rb + 1) - (qe - qb + 1) == 7
    assert sp.dir_fits(re - rb + 1, qe - qb + 1, 8)


def test_capacity_probes_and_mixed_pairs():
    assert sp.RMAX + 1 > en.SW_RMAX and sp.QMAX + 1 > en.SW_QMAX
    pairs = sp.mixed_pairs()
    assert len(pairs) == 300 and len(set(pairs)) == 300
    lens = [len(q) for q, _ in pairs]
    assert min(lens) <= 128 and any(128 < n <= 640 for n in lens) and any(640 < n <= 2048 for n in lens) and any(len(r) > sp.LDS_RMAX for _, r in pairs)


def test_sw_rows_maps_group_and_member():
    r = ca.SwRows(np.arange(5 * 8, dtype=np.int32).reshape(5, 8), np.array([0, 2, 2, 5], np.uint32))
    assert r.index(0, 0) == 0 and r.index(0, 1) == 1 and r.index(2, 0) == 2 and r.index(2, 2) == 4 and r.row(2, 1)[0] == 24
    for bad in ((0, 2), (1, 0), (2, 3)):
        with pytest.raises(IndexError):
            r.index(*bad)


@pytest.mark.parametrize("cls", [0, 1, 2])
def test_the_crowds_have_more_pairs_than_their_launch_has_waves(cls):
    """tests/test_gpu_sw_op.py relies on it: a wave takes a second pair only where pairs outnumber the waves of the launch."""
    ng, per, q_lo, q_hi, r_lo, r_hi, seed = sp.CROWDS[cls]
    n_seqs, pairs = ng * (per + 1), ng * per
    for cus in (64, 256, 304):
        for flags in (0, 1):
            rc, p = sw_plan(ng, n_seqs, n_seqs * 10, flags, cus)
            waves = (4 * p["wgs0"], 4 * p["wgs1"], p["wgs_long"])[cls]
            assert rc == 0 and waves == sp.waves_of(n_seqs, cls, bool(flags), cus)
            assert pairs > waves, (cls, cus, flags, pairs, waves)
    groups = sp.crowd(*sp.CROWDS[cls])
    assert len(groups) == ng and all(len(g) == per + 1 and r_lo <= len(g[0]) <= r_hi and all(q_lo <= len(q) <= q_hi for q in g[1:]) for g in groups)
    for g in groups:  # whatever band the traceback takes fits the scratch: every row is CW_SW_ALIGNED
        for q in g[1:]:
            score, rb, re, qb, qe, _, _ = sp.oracle(q, g[0])
            assert score <= 0 or sp.dir_fits(re - rb + 1, qe - qb + 1, 10 ** 6)
