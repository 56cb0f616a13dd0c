"""Without a GPU: the groups of tests/test_gpu_tier_q_members.py are what they say, and the stated ones can SHOW a fault of tier Q's member window -- on the
oracle, every group differs in its consensus from what a wrong compare or a wrong count would make of it (tests/tier_q_member_groups.py MUTANTS)."""
import pytest

import poa_op_probes as pp
import tier_q_member_groups as tq


def test_the_family_is_what_it_says():
    assert len(tq.FAMILY) == 73  # 15 + 14 + 14 + 14 + 11 + 5 shapes within the estimate
    for length in tq.LENGTHS:
        for n in tq.COUNTS:
            assert (f"{length} bases x {n}" in tq.FAMILY) == (tq.est(length, n) <= pp.Q_ROUTE)
    for name, g in tq.FAMILY.items():
        length = int(name.split()[0])
        assert len(set(g)) <= 6 and all(abs(len(s) - length) <= 1 for s in g), name


def test_every_group_is_a_task_of_tier_q():
    for name, g in tq.GROUPS.items():
        mx = max(len(s) for s in g)
        assert 2 <= len(g) <= 255 and mx <= pp.Q_LC and pp.route(len(g), mx) == "Q", (name, len(g), mx)
    assert any(len(s) == 31 for g in tq.STATED.values() for s in g)
    for end in (15, 16, 17):
        g = tq.STATED[f"run ends at member {end}, one more behind it"]
        assert len(set(g[: end + 1])) == 1 and g[end + 1] != g[end]
    g = tq.STATED["run over two whole windows, one more behind it"]
    assert len(set(g[:52])) == 1 and len(set(g[52:])) == 1 and g[52] != g[51]


@pytest.mark.parametrize("name", list(tq.MUTANTS))
def test_a_fault_of_the_window_would_change_the_stated_groups_consensus(name):
    exp = pp.oracle_consensus(tq.STATED[name])
    assert tq.MUTANTS[name]
    for what, mutant in tq.MUTANTS[name].items():
        assert mutant != tq.STATED[name] and max(len(s) for s in mutant) <= pp.Q_LC
        assert pp.oracle_consensus(mutant) != exp, f"{name}: {what}, and the consensus is the same"


def test_all_but_one_stated_group_has_mutants():
    assert set(tq.STATED) - set(tq.MUTANTS) == {"repeat right after a member that added a node"}
