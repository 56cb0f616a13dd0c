"""The plain POA reference (tests/poa_ref.py, written from the prose of include/cw_policy.h) against the oracle (oracle/cw_oracle.cpp), and the probe catalogue
of the slab tiers (tests/poa_probes.py) against the reference: every probe crosses what it is named for, by the reference's own statistics; every mutant has
another consensus; the tiers a probe says it visits are the ones the capacities of cw_poa.h send it through; and the catalogue claims every route bit the
default build can reach.  tests/test_gpu_poa_routes.py then holds the engine to the same catalogue."""
import pytest

import poa_op_probes as pp
import poa_probes as cat
import poa_ref
import tier_q_member_groups as tq
from test_gpu_poa_op import edge_groups


def test_the_references_scores_are_the_policy_headers():
    import os
    import re

    hdr = open(os.path.join(cat.ROOT, "include", "cw_policy.h")).read()
    got = tuple(int(re.search(rf"#define {n}\s+\(?(-?\d+)\)?", hdr).group(1)) for n in ("CW_POA_MATCH", "CW_POA_MISMATCH", "CW_POA_GAP"))
    assert got == (poa_ref.MATCH, poa_ref.MISMATCH, poa_ref.GAP)


@pytest.mark.parametrize("name", list(cat.PROBES))
def test_reference_equals_the_oracle_on_every_probe(name):
    cons, stats = cat.reference(name)
    assert cons == pp.oracle_consensus(cat.PROBES[name].group), name
    assert len(stats) == len(pp.aligned_members(cat.PROBES[name].group))


def test_reference_equals_the_oracle_on_the_operators_groups():
    groups = {name: pp.probe(name) for name in pp.SHAPES}
    groups.update({f"q{i}": pp.q_group(i) for i in range(200)})
    groups.update(edge_groups())
    groups.update({f"tier Q members: {k}": g for k, g in tq.STATED.items()})
    for name, g in groups.items():
        assert poa_ref.consensus(g) == pp.oracle_consensus(g), name


@pytest.mark.parametrize("name", list(cat.PROBES))
def test_probe_visits_the_tiers_it_states_and_proves_what_it_is_named_for(name):
    p = cat.PROBES[name]
    m = pp.aligned_members(p.group)
    tiers, stops, why = cat.visits(p.group)
    assert (tiers, stops) == (p.tiers, p.stops), (name, tiers, stops, why)
    for t, cause in why.items():
        assert f"{t}.{cause}" in p.has, f"{name}: tier {t} gives the task up by {cause}, which the probe does not state"
    assert not {b for b in p.has if ".rc2_" in b} - {f"{t}.{c}" for t, c in why.items()}, (name, why)
    assert not p.has & p.lacks and not p.has & set(cat.UNREACHABLE), name
    for b in p.has:
        assert b.split(".")[0] in p.tiers, f"{name}: {b} is of a tier the probe does not visit"
    _, stats = cat.reference(name)
    last, pr = stats[-1], dict(p.proves)
    print(name, "members", len(m), "longest", max(map(len, m)), "ends with", last)
    for i in pr.pop("clean", []):
        assert (stats[i].new_nodes, stats[i].new_edges) == (0, 0), f"{name}: member {i} adds {stats[i].new_nodes} nodes, {stats[i].new_edges} edges"
    for i in pr.pop("adds", []):
        assert stats[i].new_nodes > 0, f"{name}: member {i} adds no node"
    if "nodes" in pr:
        assert last.nodes == pr.pop("nodes")
    if "nodes_before_last" in pr:
        assert stats[-2].nodes <= pr.pop("nodes_before_last")
    if "edges_at_most" in pr:
        assert max(s.edges for s in stats) <= pr.pop("edges_at_most")
    if "edges_over" in pr:
        ec, nc = pr.pop("edges_over"), pr.pop("nodes_at_most")
        assert last.edges > ec and last.nodes <= nc and all(s.edges <= ec for s in stats[:-1]), (name, last)
        if "edges_before_last" in pr:
            assert stats[-2].edges == pr.pop("edges_before_last"), stats[-2]  # exactly EC edges fit
    if "max_indeg" in pr:
        want = pr.pop("max_indeg")
        assert {4, 5, 6} <= {s.max_indeg for s in stats[:-1]} and stats[-2].max_indeg >= want, [s.max_indeg for s in stats]
        assert all(len(s) <= 63 for s in m[1:]), "coded rows: members of at most 63 bases"
    if "max_far" in pr:
        assert stats[-2].max_far >= pr.pop("max_far") > cat.K["RING"]  # (before the last member: its fill meets the far row)
    if "max_far_at_most" in pr:
        assert last.max_far <= pr.pop("max_far_at_most") <= cat.K["RING"]
    if "cells_over" in pr:
        cells = pr.pop("cells_over")
        assert any((a.nodes + 1) * (len(s) + 1) > cells for a, s in zip(stats, m[1:])), name
    if "nodes_over" in pr:
        assert last.nodes > pr.pop("nodes_over")
    if "edges_first_in" in pr:
        t, nc, ec = pr.pop("edges_first_in")
        first = next(s for s in stats if s.nodes > nc or s.edges > ec)
        assert first.nodes <= nc and first.edges > ec, first
    assert not pr, f"{name}: nothing proves {sorted(pr)}"


@pytest.mark.parametrize("name", [n for n, p in cat.PROBES.items() if p.mutants])
def test_every_mutant_has_another_consensus(name):
    cons, _ = cat.reference(name)
    for what, g in cat.PROBES[name].mutants.items():
        assert poa_ref.consensus(g) != cons, f"{name}: the reference cannot tell '{what}'"
        assert poa_ref.consensus(g) == pp.oracle_consensus(g), f"{name}: '{what}'"


def test_the_ladders_hold_every_width_their_tier_takes():
    longest = {"ladder S": 65, "ladder M1": 122, "ladder M2": 301, "ladder L": 1023, "ladder G": 2047, "ladder X": 4095}
    for name, mx in longest.items():
        g = cat.PROBES[name].group
        assert len(g[0]) == mx == max(map(len, g)), name
        assert {w for w in cat.WIDTHS if w < mx} <= set(map(len, g)), (name, sorted(set(map(len, g))))
    for name in ("ladder M2", "ladder L"):
        lens = list(map(len, cat.PROBES[name].group))
        assert cat.K["GF_LC"] == 31 and 31 in lens and 32 in lens


def test_the_catalogue_claims_every_bit_the_default_build_reaches():
    claimed = set().union(*(p.has for p in cat.PROBES.values()))
    assert not set(cat.UNREACHABLE) & set(cat.NOT_PROBED)
    assert set(cat.UNREACHABLE) | set(cat.NOT_PROBED) <= cat.ALL_BITS
    missing = cat.ALL_BITS - set(cat.UNREACHABLE) - set(cat.NOT_PROBED) - claimed
    assert not missing, sorted(missing)
    assert not claimed & (set(cat.UNREACHABLE) | set(cat.NOT_PROBED))
