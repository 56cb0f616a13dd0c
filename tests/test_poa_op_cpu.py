"""The POA operator without a GPU (include/consent_amd.h cw_poa_run / cw_poa_run_device, csrc/cw_plan.h plan_poa): the symbols exist, bad arguments
are refused before the device is touched, the plan of a POA-only run holds what such a run needs and nothing of the window path -- and the probes of
tests/test_gpu_poa_op.py are candidates: the oracle's own consensus of each fits the slot the operator reserves."""
import ctypes as C

import numpy as np
import pytest

import consent_amd as ca
import poa_op_probes as pp
from consent_amd.engine import Batch, Result, _ptr, alloc_poa_results, poa_slot_bytes

E_INVALID = -1
PLAN = ["total", "win", "solid", "segments", "arena", "tasks_members", "lists", "slab_s", "slab_m1", "slab_m2", "slab_l", "slab_g", "rows_q_h", "anchor_blocks", "fallbacks_finish"]
CUS = 256


def lib():
    return ca.load_library()


def poa_plan(groups, seqs, words, cus=CUS):
    out = np.zeros(15, np.uint64)
    rc = lib().cw_debug_poa_plan(groups, seqs, words, cus, _ptr(out))
    return rc, dict(zip(PLAN, (int(x) for x in out)))


def window_plan(windows, seqs, words, cus=CUS):
    out = np.zeros(15, np.uint64)
    l = lib()
    l.cw_debug_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]
    assert l.cw_debug_plan(9, 4, windows, seqs, words, cus, 1, 1024, _ptr(out)) == 0
    return dict(zip(PLAN, (int(x) for x in out)))


def test_the_new_symbols_are_exported():
    l = lib()
    for name in ("cw_poa_run", "cw_poa_run_device", "cw_debug_poa_plan"):
        assert hasattr(l, name), name
    assert int(poa_slot_bytes(100)) == 202  # CW_POA_SLOT_BYTES


def test_null_and_malformed_arguments_are_invalid_without_a_device():
    l = lib()
    hb = ca.pack_piles([["ACGT", "ACGA"]])
    res = alloc_poa_results(hb)
    b = hb.c_struct()
    r = Result(_ptr(res.cons), _ptr(res.cons_off), _ptr(res.cons_len), _ptr(res.status), None, None, None)
    for fn in (l.cw_poa_run, lambda *a: l.cw_poa_run_device(*a, None)):
        assert fn(None, C.byref(b), C.byref(r)) == E_INVALID  # no engine
        assert fn(None, None, C.byref(r)) == E_INVALID
        assert fn(None, C.byref(b), None) == E_INVALID
    out = np.zeros(15, np.uint64)
    assert l.cw_debug_poa_plan(0, 0, 0, CUS, _ptr(out)) == E_INVALID  # no groups
    assert l.cw_debug_poa_plan(4, 8, 8, CUS, None) == E_INVALID
    assert l.cw_debug_poa_plan(4, 8, 8, 0, _ptr(out)) == E_INVALID


def test_poa_plan_leaves_out_what_only_the_window_path_needs():
    groups, members, bases = 1024, 8, 100
    seqs, words = groups * members, groups * members * ((bases + 15) // 16)
    rc, p = poa_plan(groups, seqs, words)
    assert rc == 0
    w = window_plan(groups, seqs, words)
    assert p["solid"] == 0 and p["anchor_blocks"] == 0 and p["fallbacks_finish"] == 0, p
    assert w["solid"] > 0 and w["anchor_blocks"] > 0 and w["fallbacks_finish"] > 0, w
    assert p["total"] < w["total"], (p["total"], w["total"])
    for part in ("slab_s", "slab_m1", "slab_m2", "slab_l", "slab_g", "rows_q_h"):  # the POA stage's memory: as plan_scratch sizes it for so many windows
        assert p[part] == w[part], (part, p[part], w[part])
    assert p["arena"] >= groups * int(poa_slot_bytes(bases)), p  # every group's slot
    assert p["tasks_members"] == (groups + 1) * 32 + seqs * 8, p  # a task per group and the neutral one, a member per sequence
    parts = sum(v for k, v in p.items() if k != "total")
    assert parts <= p["total"] < parts + 64 * 256 + (1 << 20), (parts, p["total"])  # the rest is alignment and the small bookkeeping (counters, slab flags)


def test_poa_plan_grows_with_groups_and_with_members():
    words_per = (100 + 15) // 16
    by_groups = [poa_plan(g, g * 8, g * 8 * words_per)[1]["total"] for g in (1, 64, 1024, 16384, 131072)]
    assert all(a < b for a, b in zip(by_groups, by_groups[1:])), by_groups
    by_members = [poa_plan(1024, 1024 * m, 1024 * m * words_per)[1]["total"] for m in (1, 2, 8, 64, 300)]
    assert all(a < b for a, b in zip(by_members, by_members[1:])), by_members


def test_poa_plan_refuses_an_arena_beyond_32_bit_offsets():
    groups = 1024
    fits = ((1 << 32) - 1 - 32 * groups) // 32  # arena = 32 bytes a word + 32 a group
    assert poa_plan(groups, groups * 8, fits)[0] == 0
    assert poa_plan(groups, groups * 8, fits + 1)[0] == E_INVALID


@pytest.mark.parametrize("name", list(pp.SHAPES))
def test_probe_is_a_candidate_the_oracles_consensus_fits_the_slot(name):
    longest, members = pp.SHAPES[name]
    g = pp.probe(name)
    assert len(g) == members and max(len(s) for s in g) == longest and all(g)
    cons = pp.oracle_consensus(g)
    assert 0 < len(cons) <= int(poa_slot_bytes(longest)), (name, len(cons), int(poa_slot_bytes(longest)))
    assert set(cons) <= set("ACGT")


def test_the_probes_cover_every_tier_by_the_routing_rule():
    tiers = {name: pp.last_tier(m, l) for name, (l, m) in pp.SHAPES.items()}
    print(tiers)
    assert set(tiers.values()) == {"Q", "S", "M1", "M2", "L", "G", "X"}, tiers
    assert tiers["24x12"] == "Q" and tiers["1500x5"] == "G" and tiers["2500x4"] == "X"
