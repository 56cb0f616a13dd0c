"""The hand-off from the chain kernel to the POA tiers as numbers: the routed lists.  The chain kernel's flush writes, for every task it routes to a list, the
entry task index | sort class << 24 (csrc/cw_poa.h cw_list_entry); cw_sort_tier_kernel orders each list by that byte alone and leaves plain task indices.
Every probe here is a batch of one or a few windows built from the generators of tests/chain_probes.py, run on the product library and on the test-aid
library (which, with CW_KEEP_EMITTED set, keeps the lists as emitted), and read back with Engine.tier_lists():
  - each list is exactly the set of tasks that Engine.segments(w) and the routing rule (tests/poa_op_probes.py route) send there;
  - every emitted class is the plain restatement's (tests/handoff_ref.py sort_class, pinned by tests/test_handoff_class_cpu.py);
  - the classes along a sorted list never decrease, no sorted entry keeps a class byte, q_split is the number of long entries of tier Q's list;
  - the members of every task are the reference's triples in order.
A window alone and among shallow windows, in two orders, gives the same lists as sets."""
import pytest

import consent_amd as ca
import chain_probes as cp
from consent_amd import engine
from consent_amd.engine import CHAIN_ROUTE, LIST_CLS_SHIFT, LIST_IDX_MASK
from handoff_ref import COST_CLASSES, LISTS, expected_lists, sort_class, task_numbers

pytestmark = pytest.mark.gpu

STD, DEEP, SOLID1 = (9, 2, 8, 2, 20), (9, 2, 8, 2, 150), (9, 1, 8, 2, 20)


def region(length, depth):
    return cp.region_pile(1500 + length, depth, length + 7)


# name -> (parameters, piles of the batch)
BATCHES = {
    "N=1": (SOLID1, lambda: [cp.short_second_pile(801, 1)]),
    "N=2": (SOLID1, lambda: [cp.short_second_pile(802, 2)]),
    "N=63": (DEEP, lambda: [cp.clean_pile(363, 63, 120)]),
    "N=64": (DEEP, lambda: [cp.clean_pile(364, 64, 120)]),
    "N=65": (DEEP, lambda: [cp.clean_pile(365, 65, 120)]),
    "N=150": (DEEP, lambda: [cp.clean_pile(450, 150, 120)]),
    "N=65, members stop at max_msa=20": (STD, lambda: [cp.clean_pile(365, 65, 120)]),
    "max_msa=6 below N=17": ((9, 2, 8, 2, 6), lambda: [cp.max_msa_pile(1000)]),
    "first and last segment are tasks": (cp.TIE_PRM, lambda: [cp.tie_pile(100)]),
    "one member of more than 16 bases": (SOLID1, lambda: [cp.long_single_pile(804)]),
    "more than 64 queued segments": (STD, lambda: [cp.sparse_anchor_pile(950, 70, 13)]),
    "tier M2 one entry, tier L one": (cp.SWEEP_PRM, lambda: [region(256, 6), region(512, 6)]),
    "tier M2 two entries, tier L none": (cp.SWEEP_PRM, lambda: [region(256, 6), region(255, 6)]),
    "tier M1 two entries, tier M2 none": (cp.SWEEP_PRM, lambda: [region(100, 6), region(31, 6), region(110, 6)]),
}
_BUILT = {}


def built(name):
    """(parameters, piles, references): once per batch."""
    if name not in _BUILT:
        prm, make = BATCHES[name]
        piles = make()
        _BUILT[name] = (prm, piles, [cp.reference(p, prm) for p in piles])
    return _BUILT[name]


@pytest.fixture(params=("product", "aids"))
def library(request, monkeypatch):
    if request.param == "aids":
        request.getfixturevalue("aids")
        monkeypatch.setenv("CW_KEEP_EMITTED", "1")
    return request.param


def run_and_read(prm, piles, refs, which):
    """Runs the batch and checks everything a single run shows; returns {list name: set of (pile index, segment)}."""
    e = ca.Engine(ca.Params(*prm))
    try:
        assert e.lib._name == (engine.AIDS_LIB if which == "aids" else engine.lib_path())
        got = e.run(engine.pack_piles(piles))
        assert all(int(s) != ca.WIN_OVERFLOW for s in got.status), "a window stopped"
        lists, tasks = e.tier_lists()
        q_split = e.tier_q_counters()["split"]
        chain_route = e.chain_route()
        key_of, ref_tasks = {}, {}  # task index -> (pile, segment); (pile, segment) -> the reference's members
        for w, ref in enumerate(refs):
            n_segs, _, w_tasks = e.segments(w)
            assert n_segs == len(ref.segments)
            ids = [t for t in range(len(tasks)) if int(tasks[t, 0]) == w]
            assert len(ids) == len(w_tasks) == len(ref.tasks), f"window {w}: {len(ids)} records, {len(ref.tasks)} reference tasks"
            by_seg = dict(ref.tasks)
            for t, (seg, n, mx, members) in zip(ids, w_tasks):
                assert members == by_seg[seg], f"window {w} segment {seg}: members {members} against {by_seg[seg]}"  # in order, stopping at max_msa
                rn, rmx, rmean = task_numbers(by_seg[seg])
                assert (int(tasks[t, 2]), int(tasks[t, 3]) & 0xFFFF, int(tasks[t, 3]) >> 16) == (rn, rmx, rmean) == (n, mx, rmean)
                key_of[t] = (w, seg)
                ref_tasks[(w, seg)] = by_seg[seg]
    finally:
        e.close()
    want = expected_lists(ref_tasks)
    out = {}
    for name, lst in LISTS.items():
        srt, emitted = lists[name]
        assert emitted is not None if which == "aids" else emitted is None
        assert all(int(x) < len(tasks) for x in srt), f"list {name}: a sorted entry keeps a class byte or names no task: {[hex(int(x)) for x in srt]}"
        keys = [key_of[int(x)] for x in srt]
        assert len(set(keys)) == len(keys) and set(keys) == set(want[name]), f"list {name}: {sorted(keys)}, routed there: {sorted(want[name])}"
        classes = [want[name][k] for k in keys]
        assert classes == sorted(classes), f"list {name}: classes along the sorted list {classes}"
        if emitted is not None:
            assert sorted(int(x) & LIST_IDX_MASK for x in emitted) == sorted(int(x) for x in srt), f"list {name}: emitted and sorted entries differ as sets"
            for x in emitted:
                k = key_of[int(x) & LIST_IDX_MASK]
                n, mx, mean = task_numbers(ref_tasks[k])
                assert int(x) >> LIST_CLS_SHIFT == sort_class(n, mx, mean, lst) == want[name][k], f"list {name}, task {k}: emitted class {int(x) >> LIST_CLS_SHIFT}"
        out[name] = set(keys)
    assert q_split == sum(1 for c in want["Q"].values() if c < COST_CLASSES), f"q_split {q_split}, tier Q's classes {sorted(want['Q'].values())}"
    return out, chain_route


@pytest.mark.parametrize("name", BATCHES)
def test_lists_of_a_batch(name, library):
    prm, piles, refs = built(name)
    sets, chain_route = run_and_read(prm, piles, refs, library)
    sizes = {k: len(v) for k, v in sets.items()}
    if name == "first and last segment are tasks":
        assert refs[0].segments[0][0] == "task" and refs[0].segments[-1][0] == "task"
    if name == "one member of more than 16 bases":
        assert refs[0].long_single and not refs[0].tasks
    if name == "more than 64 queued segments":
        assert refs[0].early_flush and len(refs[0].tasks) > 64
        if library == "aids":
            assert chain_route & CHAIN_ROUTE["early_flush"]
    if name.startswith("max_msa") or "max_msa=20" in name:
        assert any(len(mem) == prm[4] for r in refs for _, mem in r.tasks) and prm[4] < len(piles[0])
    if name == "tier M2 one entry, tier L one":
        assert (sizes["M2"], sizes["L"], sizes["M1"]) == (1, 1, 0)
    if name == "tier M2 two entries, tier L none":
        assert (sizes["M2"], sizes["L"]) == (2, 0)
    if name.startswith("tier M1 two"):
        assert (sizes["M1"], sizes["M2"]) == (2, 0)
    if name in ("N=1", "N=2"):
        assert not any(sizes.values())
    if name == "N=63":
        assert sizes["Q"] == 1


def test_a_window_alone_and_among_shallow_windows(library):
    prm = cp.SWEEP_PRM
    deep = region(127, 40)
    shallow = [cp.clean_pile(365, 65, 120), cp.sparse_anchor_pile(950, 70, 13), region(31, 6)]
    ref_of = {id(p): cp.reference(p, prm) for p in [deep] + shallow}

    def named(piles):
        sets, _ = run_and_read(prm, piles, [ref_of[id(p)] for p in piles], library)
        return {name: {("deep" if piles[w] is deep else "shallow%d" % [id(s) for s in shallow].index(id(piles[w])), seg) for w, seg in keys} for name, keys in sets.items()}

    alone = named([deep])
    first = named([deep] + shallow)
    last = named(shallow[::-1] + [deep])
    assert first == last
    assert any(alone.values())
    for name in LISTS:
        assert {k for k in first[name] if k[0] == "deep"} == alone[name]
