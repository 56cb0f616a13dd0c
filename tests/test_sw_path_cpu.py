"""The path run without a GPU (include/consent_amd.h cw_sw_path_run / cw_sw_path_run_device, csrc/cw_plan.h plan_sw_path): the symbols and constants exist,
bad arguments are refused before the device is touched, the plan holds what such a run needs -- and the reference the GPU tests compare ops with
(tests/sw_path_probes.py: ssw's banded pass with its direction codes and the walk, in numpy) is pinned to the oracle (oracle/cw_oracle_c.cpp cwo_ssw) for every
probe used there: its indel totals are the oracle's, its ops span the alignment's ends and re-score to the alignment's score."""
import ctypes as C
import re

import numpy as np
import pytest

import consent_amd as ca
import sw_op_probes as sp
import sw_path_probes as pp
from consent_amd import engine as en
from consent_amd.engine import _ptr

E_INVALID = -1
CUS = 256
PLAN = ["total", "order", "gref", "long_state", "dirs", "steps", "wgs0", "wgs1", "wgs_long", "dir_waves", "dir_bytes", "step_bytes"]
GREF_BYTES, LONG_WAVE_BYTES = 16384, 16384 + 2 * 32768 + 256 * 64 * 20  # csrc/cw_sw_op.h CW_SW_GREF_BYTES, CW_SW_LONG_WAVE_BYTES


def lib():
    return ca.load_library()


def path_plan(groups, seqs, words, flags=0, cus=CUS):
    out = np.zeros(12, np.uint64)
    rc = lib().cw_debug_sw_path_plan(groups, seqs, words, cus, flags, _ptr(out))
    return rc, dict(zip(PLAN, (int(x) for x in out)))


def test_the_new_symbols_and_constants_are_exported():
    l = lib()
    for name in ("cw_sw_path_run", "cw_sw_path_run_device", "cw_debug_sw_path_plan"):
        assert hasattr(l, name), name
    assert (ca.SW_NO_PATH, ca.SW_PATH_OPEN, ca.SW_PATH_SLOT, ca.SW_PATH_EQX) == (4, 5, 6, 4)
    assert (pp.NO_PATH, pp.PATH_OPEN, pp.PATH_SLOT, pp.EQX) == (4, 5, 6, 4) and pp.PATH_BYTES == en.SW_PATH_BYTES == 2 << 20
    assert (en.SW_OP_M, en.SW_OP_I, en.SW_OP_D, en.SW_OP_EQ, en.SW_OP_X) == (0, 1, 2, 7, 8)
    assert ca.sw_ops_bound(300, 700) == 1000
    assert hasattr(ca.Engine, "sw_path") and hasattr(ca.Engine, "sw_path_device")
    assert (ca.SW_ALIGNED, ca.SW_NO_INDELS, ca.SW_STOP, ca.SW_IS_REF, ca.SW_WANT_INDELS) == (0, 1, 2, 3, 1)  # the existing enum is kept


def test_the_header_states_the_constants_the_tests_use():
    import os

    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "consent_amd.h")).read()
    assert re.search(r"CW_SW_NO_PATH = 4, CW_SW_PATH_OPEN = 5, CW_SW_PATH_SLOT = 6", text)
    assert re.search(r"#define CW_SW_PATH_EQX 4u", text) and re.search(r"#define CW_SW_PATH_BYTES \(2u << 20\)", text)
    assert re.search(r"#define CW_SW_OPS_BOUND\(query_len, ref_len\) \(\(query_len\) \+ \(ref_len\)\)", text)


def test_a_missing_engine_and_a_malformed_plan_request_are_invalid_without_a_device():
    """Without a device there is no engine, so both entry points end at their first check; the checks behind it (flags, NULL rows / paths / members, too many
    groups) need an engine and are tests/test_gpu_sw_path.py's.  The flag rule itself is reached here through cw_debug_sw_path_plan."""
    l = lib()
    hb = ca.pack_piles([["ACGTACGT", "ACGA"]])
    b = hb.c_struct()
    rows = np.full((2, 8), 77, np.int32)
    ops, off, n_ops = np.full(24, 77, np.uint32), np.array([0, 12, 24], np.uint64), np.full(2, 77, np.uint32)
    paths = en.SwPaths(_ptr(ops), _ptr(off), _ptr(n_ops))
    assert l.cw_sw_path_run(None, C.byref(b), _ptr(rows), C.byref(paths), 0) == E_INVALID
    assert l.cw_sw_path_run_device(None, C.byref(b), _ptr(rows), C.byref(paths), 0, None) == E_INVALID
    assert (rows == 77).all() and (ops == 77).all() and (n_ops == 77).all()
    out = np.zeros(12, np.uint64)
    assert l.cw_debug_sw_path_plan(4, 8, 8, CUS, 0, None) == E_INVALID
    assert l.cw_debug_sw_path_plan(4, 8, 8, 0, 0, _ptr(out)) == E_INVALID
    for flags in (1, 2, 8):  # cw_sw_run's flag is not this call's; the only one is CW_SW_PATH_EQX
        assert l.cw_debug_sw_path_plan(4, 8, 8, CUS, flags, _ptr(out)) == E_INVALID
    assert l.cw_debug_sw_path_plan(4, 8, 8, CUS, pp.EQX, _ptr(out)) == 0


def test_path_plan_holds_what_a_run_needs():
    seqs = 100000
    rc, p = path_plan(1000, seqs, seqs * 10)
    assert rc == 0
    assert p["order"] >= 2 * 4 * seqs, p  # a reference index and a place in the order per sequence
    assert p["dir_bytes"] == pp.PATH_BYTES and p["step_bytes"] >= sp.QMAX + sp.RMAX, p  # a step consumes a base of the query or of the reference
    assert (p["wgs0"], p["wgs1"], p["wgs_long"]) == (128, 128, 256) and p["dir_waves"] == 512 == pp.PATH_MAX_WAVES, p
    assert p["dirs"] == 512 * pp.PATH_BYTES == 1 << 30, p  # the direction scratch an indel run plans at most (tests/test_sw_op_cpu.py: 1024 << 20)
    assert p["dir_waves"] >= max(4 * p["wgs0"], 4 * p["wgs1"], p["wgs_long"])  # every wave of every launch has its own
    assert p["steps"] == p["dir_waves"] * p["step_bytes"], p
    assert p["gref"] == max(p["wgs0"], p["wgs1"]) * 4 * GREF_BYTES and p["long_state"] == p["wgs_long"] * LONG_WAVE_BYTES, p
    assert p["total"] == p["order"] + p["gref"] + p["long_state"] + p["dirs"] + p["steps"], p
    assert path_plan(1000, seqs, seqs * 10, pp.EQX)[1] == p  # the flag changes no size
    rc, small = path_plan(1, 3, 30)
    assert rc == 0 and (small["wgs0"], small["wgs1"], small["wgs_long"], small["dir_waves"]) == (1, 1, 3, 4), small
    assert small["total"] < 12 << 20, small
    rc, few_cus = path_plan(1000, seqs, seqs * 10, 0, 16)
    assert (few_cus["wgs0"], few_cus["wgs1"]) == (64, 16), few_cus


def test_path_plan_is_monotone_in_pairs_and_does_not_depend_on_bases():
    by_seqs = [path_plan(max(1, s // 8), s, s * 40)[1] for s in (1, 2, 5, 64, 1000, 1024, 5000, 100000, 2000000)]
    for a, b in zip(by_seqs, by_seqs[1:]):
        assert all(a[k] <= b[k] for k in PLAN), (a, b)
        assert a["order"] < b["order"] or b["order"] - 256 < a["order"]  # (parts are rounded up to 256 bytes)
    assert by_seqs[0]["total"] < by_seqs[-1]["total"]
    by_bases = [path_plan(100, 5000, w)[1] for w in (5000, 50000, 5000000)]
    assert by_bases[0] == by_bases[1] == by_bases[2]
    by_groups = [path_plan(g, 5000, 50000)[1] for g in (1, 50, 5000)]
    assert by_groups[0] == by_groups[1] == by_groups[2]


def test_the_alignment_plan_keeps_its_numbers():
    out = np.zeros(10, np.uint64)
    assert lib().cw_debug_sw_plan(1000, 100000, 1000000, CUS, 1, _ptr(out)) == 0
    assert [int(x) for x in out[5:]] == [256, 256, 256, 1024, 1 << 20]


# ---- the reference, by the oracle ------------------------------------------------------------------------------------------------------------------------

def check_reference(name, q, r):
    """The restated pass against the oracle for one pair; returns the reference's status."""
    status, ins, dele, ops, ops_x, bands = pp.reference(q, r)
    score, rb, re_, qb, qe, o_ins, o_del = sp.oracle(q, r)
    if status == pp.NO_PATH:
        assert (ins, dele, ops) == (0, 0, ()), name
        return status
    assert (ins, dele) == (o_ins, o_del), (name, ins, dele, o_ins, o_del)  # also for PATH_OPEN: what the walk counted, as the oracle's
    if status == pp.PATH_OPEN or score <= 0:
        assert ops == () and ops_x == (), name
        return status
    rs, qs = r[rb : re_ + 1], q[qb : qe + 1]
    for o in (ops, ops_x):
        assert all(a[1] != b[1] for a, b in zip(o, o[1:])) and all(n >= 1 for n, _ in o), name  # run-length encoded
        assert pp.rescore(o, rs, qs) == (score, len(qs), len(rs)), (name, pp.rescore(o, rs, qs), score)
        assert sum(n for n, c in o if c == pp.OP_I) == ins and sum(n for n, c in o if c == pp.OP_D) == dele, name
        assert len(o) <= ca.sw_ops_bound(len(q), len(r))
    assert pp.merge_eqx(ops_x) == list(ops) and {c for _, c in ops} <= {0, 1, 2} and {c for _, c in ops_x} <= {1, 2, 7, 8}, name
    return status


@pytest.mark.parametrize("name", list(pp.all_probes()))
def test_the_reference_equals_the_oracle_on_every_probe(name):
    q, r = pp.all_probes()[name]
    status = check_reference(name, q, r)
    print(name, len(q), len(r), "status", status, "bands", pp.reference(q, r)[5])
    # none of the probes is PATH_OPEN (the status is reached by no test); the one NO_PATH probe is made for it
    assert status == (pp.NO_PATH if name == "planted wide" else pp.ALIGNED), (name, status)


def test_the_band_probes_have_their_bands():
    bands = {name: pp.reference(q, r)[5] for name, (q, r) in pp.band_pairs().items()}
    assert [bands[f"deletion of {d}"] for d in (30, 31, 32)] == [(31,), (32,), (33,)]  # 63, 65, 67 cells a row: the edge of a chunk of 64
    assert bands["planted(10)"] == (1, 2, 4, 8, 16) and bands["planted(40)"][-1] == 64 and bands["planted(300)"][-1] == 512
    score, rb, re_, qb, qe, _, _ = sp.oracle(*sp.planted(300))
    assert pp.path_fits(re_ - rb + 1, qe - qb + 1, 512) and 1025 * 1800 + 12336 <= pp.PATH_BYTES  # rows beyond LDS share the scratch
    assert 12 * (2 * 512 + 3) > pp.ROWS_LDS >= 12 * (2 * 64 + 3)
    assert sp.expected_status(*sp.planted(300)) == sp.NO_INDELS  # what cw_sw_run says of it
    q, r = pp.planted_small()
    score, rb, re_, qb, qe, ins, dele = sp.oracle(q, r)
    assert (len(r), ins, dele) == (60, 40, 0) and bands["band wider than the matrix"] == (41,) and 2 * 41 + 1 > (re_ - rb + 1) + 1  # the stride is clipped
    assert bands["unbalanced"] == (8,)


def test_the_no_path_probe_by_the_rule():
    q, r = pp.planted_wide()
    score, rb, re_, qb, qe, ins, dele = sp.oracle(q, r)
    r_span, q_span = re_ - rb + 1, qe - qb + 1
    assert r_span == q_span == 5100 and ins == dele == 600
    status, _, _, _, _, bands = pp.reference(q, r)
    assert status == pp.NO_PATH and bands == (1, 2, 4, 8, 16, 32, 64, 128, 256)  # bands up to 128 fit and do not reach the score
    assert pp.path_fits(5100, 5100, 128) and not pp.path_fits(5100, 5100, 256) and 513 * 5100 > pp.PATH_BYTES
    assert pp.path_fits(1100, 1100, 10 ** 6) and not pp.path_fits(2034, 2034, 512) and pp.path_fits(2033, 2033, 512)  # 1025 x 2033 + 12336 <= 2^21 < 1025 x 2034 + 12336
    assert pp.expected(q, r) == (sp.oracle(q, r)[:5] + (0, 0, pp.NO_PATH), 0, ())


def test_every_long_probe_has_a_path_by_the_rule():
    for name, (q, r) in pp.long_pairs().items():
        assert pp.reference(q, r)[0] == pp.ALIGNED, name
    by_len = {len(q): sp.expected_status(q, r) for q, r in sp.long_pairs().values()}
    assert by_len[2500] == by_len[9000] == sp.NO_INDELS  # pairs cw_sw_run ends without totals


def test_expected_applies_the_slot():
    q, r = pp.one_deletion(30)
    row, n, ops = pp.expected(q, r)
    assert row[7] == pp.ALIGNED and n == len(ops) == 3 and ops == ((150, 0), (30, 2), (150, 0))
    assert pp.expected(q, r, slot=3) == (row, n, ops)
    short = pp.expected(q, r, slot=2)
    assert short == (row[:7] + (pp.PATH_SLOT,), 3, ())
    assert ca.SwPathRows(np.array([[0] * 7 + [3], list(row)], np.int32), np.array([0, 2]), 0, np.array([0, 3], np.uint32),
                         np.array([99, (150 << 4), (30 << 4) | 2, (150 << 4), 99], np.uint32), np.array([0, 1, 5], np.uint64)).cigar(0, 1) == "150M30D150M"


@pytest.mark.parametrize("cls", [0, 1, 2])
def test_the_crowds_outnumber_the_path_launches_waves_and_their_samples_hold(cls):
    ng, per, *_ = pp.CROWDS[cls]
    n_seqs, pairs = ng * (per + 1), ng * per
    for cus in (64, 256, 304):
        rc, p = path_plan(ng, n_seqs, n_seqs * 10, 0, cus)
        waves = (4 * p["wgs0"], 4 * p["wgs1"], p["wgs_long"])[cls]
        assert rc == 0 and waves == pp.waves_of(n_seqs, cls, cus) and pairs > waves, (cls, cus, pairs, waves)  # waves take a second pair
    k = 0
    for g in sp.crowd(*pp.CROWDS[cls]):
        for q in g[1:]:
            if k % pp.CROWD_SAMPLE[cls] == 0:
                assert check_reference((cls, k), q, g[0]) == pp.ALIGNED
            k += 1


def test_the_mixed_pairs_sample_holds():
    for i, (q, r) in enumerate(sp.mixed_pairs(300)[::10]):
        assert check_reference(("mixed", i), q, r) == pp.ALIGNED


# ---- the restated pass's tie rules, by the serial loop ---------------------------------------------------------------------------------------------------

def small_pairs():
    out = {name: p for name, p in pp.all_probes().items() if len(p[0]) * len(p[1]) and len(p[0]) <= 450 and len(p[1]) <= 450}
    out["planted 60 + 40"] = pp.planted_small()
    return out


@pytest.mark.parametrize("name", list(small_pairs()))
def test_the_row_at_a_time_pass_equals_the_serial_loop_cell_by_cell(name):
    """banded_dirs takes the in-row gap as a prefix maximum, as the kernel does; banded_dirs_serial is the oracle's loop, cell after cell.  Indel totals and
    a re-score cannot tell two co-optimal paths apart; equal direction codes in every cell of every band tried can."""
    q, r = small_pairs()[name]
    score, rb, re_, qb, qe, _, _ = sp.oracle(q, r)
    if score <= 0:
        return
    rs = np.array([pp.CODE[c] for c in r[rb : re_ + 1]], np.int64)
    qs = np.array([pp.CODE[c] for c in q[qb : qe + 1]], np.int64)
    bands = pp.reference(q, r)[5]
    assert bands
    for band in bands:
        fast, slow = pp.banded_dirs(rs, qs, band), pp.banded_dirs_serial(rs, qs, band)
        assert fast[0] == slow[0], (name, band)
        for a, b, what in zip(fast[1:], slow[1:], ("dir_e", "dir_f", "dir_h")):
            assert np.array_equal(a, b), (name, band, what, np.argwhere(a != b)[:4].tolist())
