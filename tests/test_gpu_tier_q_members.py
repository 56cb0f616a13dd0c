"""Tier Q's member window (csrc/cw_poa_q.h PoaQWin, poaq_window, poaq_next, poaq_take): a group of the tier holds a task's members sixteen at a time in
registers -- lengths and bases as keys -- finds the members that repeat their predecessor by comparing neighbour lanes, takes a run of them in one pass and
hands an aligned member its bases from the window.  The groups are those of tests/tier_q_member_groups.py: the family (base strings of 8 .. 31 bases, members
the string or one of five variants one edit away, in runs of 1-20 equal ones, 2 .. 255 members), which walks windows, refills and runs of every length, and
the stated groups, whose vote turns on one member: a member that differs from its predecessor in the last base, the first base, the bases on either side of
the key's word boundary or in its length only, the member behind a run that ends on the window's last lane, on the next window's first and second, or that
covers two windows.  What a wrong compare or count would make of each stated group has another consensus (tests/test_tier_q_members_cpu.py shows that on the
oracle), so equal bytes here say the window decided right.  Every group goes through Engine.poa and is compared with the oracle's POA; the counters say that
tier Q ran all of them and handed none on."""
import random

import numpy as np
import pytest

import consent_amd as ca
import poa_op_probes as pp
from tier_q_member_groups import GROUPS

pytestmark = pytest.mark.gpu
N_TIER, N_OVER = 6, 18  # Engine.profile() counters: n_tier[6] from word 6 (list 0 = tier Q), n_over[6] from word 18 (0 = handed to tier S)


@pytest.fixture(scope="module")
def eng():
    e = ca.Engine(ca.Params(*pp.PRM))
    yield e
    e.close()


def counters(eng):
    c, _ = eng.profile()
    return int(c[0]), int(c[N_TIER]), int(c[N_OVER])


@pytest.fixture(scope="module")
def alone(eng):
    """Every group alone in its batch: its consensus, and (tasks, routed to tier Q, handed on by it)."""
    out = {}
    for name, g in GROUPS.items():
        res = eng.poa([g])
        assert int(res.status[0]) == ca.WIN_CONSENSUS, name
        out[name] = (res.consensus(0), counters(eng))
    return out


@pytest.mark.parametrize("name", list(GROUPS))
def test_group_alone_equals_the_oracle_and_stayed_in_tier_q(alone, name):
    got, (tasks, routed_q, handed_on) = alone[name]
    exp = pp.oracle_consensus(GROUPS[name])
    assert got == exp, f"{name}: consensus {got} differs from the oracle's {exp}"
    assert (tasks, routed_q, handed_on) == (1, 1, 0), f"{name}: tasks {tasks}, routed to tier Q {routed_q}, handed on {handed_on}"


@pytest.mark.parametrize("order", [1, 2])
def test_one_batch_of_all_groups_shuffled(eng, alone, order):
    """Waves hold tasks at different places in their windows: a group's bytes are its bytes alone."""
    names = list(GROUPS)
    random.Random(order).shuffle(names)
    assert names != list(GROUPS)
    res = eng.poa([GROUPS[n] for n in names])
    tasks, routed_q, handed_on = counters(eng)
    assert (res.status == ca.WIN_CONSENSUS).all(), [names[i] for i in np.flatnonzero(res.status != ca.WIN_CONSENSUS)]
    assert (tasks, routed_q, handed_on) == (len(names), len(names), 0), (tasks, routed_q, handed_on)
    for i, n in enumerate(names):
        assert res.consensus(i) == alone[n][0], n
