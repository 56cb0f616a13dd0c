"""GPU: tier Q's eight-lane loop (csrc/cw_poa_q.h PoaQ8: short tasks eight to a wave, on half a DPP row each) against the plain reference.

Every batch is a handful of groups through Engine.poa(); every consensus is compared byte for byte with tests/poa_ref.py, and Engine.tier_q_counters()
states which of the kernel's two loops took each task: `split` entries of tier Q's list are long (the 16-lane loop), the others short; `short_done` and
`short_handed_on` are what the eight-lane loop finished and what outgrew it (tier S redoes those: n_over[0]).  The shapes are the smallest at which the
change can go wrong: the lengths on both sides of 15 bases, the eligibility estimate at its bound and above it, fewer tasks than a wave has groups and one
more, the member window at eight members, neighbours in a wave that would change each other's result if a shift or scan crossed from lane 7 to lane 8,
and graphs that end exactly at a capacity or one beyond it -- those are built with the reference first, whose statistics state the node and edge counts."""
import os
import re

import pytest

import consent_amd as ca
import poa_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRM = (9, 4, 8, 2, 150)
N_TIER, N_OVER = 6, 18  # Engine.profile() counters: n_tier[6] from word 6, n_over[6] from word 18 (list 0 = tier Q; hand-over list 0 = tier S's)


def _num(header, name):
    txt = open(os.path.join(ROOT, "consent_amd", "csrc", header)).read()
    return int(re.search(rf"#\s*define {name} (\d+)", txt).group(1))


LC8, NC8, ROUTE8 = _num("cw_poa.h", "CW_POAQ8_LC"), _num("cw_poa.h", "CW_POAQ8_NC"), _num("cw_poa.h", "CW_POAQ8_ROUTE_NODES")
EC8, RING = 104, 8  # cw_poa_q.h: CW_POAQ8_EC under the default (column-vote) policy, the rows of the LDS ring
T = "ACGTTGCAAGCTTAC"  # the template of the built groups: 15 bases


def sub(s, i, b=None):
    """s with another base at position i (b, or the next one in ACGT)"""
    return s[:i] + (b or "ACGT"[("ACGT".index(s[i]) + 1) % 4]) + s[i + 1 :]


def estimate(group):
    """the depth-aware graph estimate the split goes by (cw_poa.h cw_poaq_is_short)"""
    return (max(len(s) for s in group) * (15 + len(group) // 5) + 9) // 10


def is_short(group):
    return max(len(s) for s in group) <= LC8 and estimate(group) <= ROUTE8


_REF = {}


def ref(group):
    """(consensus, [MemberStats]) by the plain reference, once per group"""
    key = tuple(group)
    if key not in _REF:
        _REF[key] = poa_ref.poa(list(group))
    return _REF[key]


@pytest.fixture(scope="module")
def e():
    eng = ca.Engine(ca.Params(*PRM))
    yield eng
    eng.close()


def run(e, groups, what=""):
    """The batch through the operator: every consensus is the reference's; returns (tier_q_counters, n_tier, n_over, [consensus])."""
    res = e.poa(groups)
    c, _ = e.profile()
    q = e.tier_q_counters()
    n_tier, n_over = [int(v) for v in c[N_TIER : N_TIER + 6]], [int(v) for v in c[N_OVER : N_OVER + 6]]
    print(f"{what}: {len(groups)} groups, tier Q {q}, n_tier {n_tier}, n_over {n_over}")
    got = []
    for i, g in enumerate(groups):
        assert int(res.status[i]) == ca.WIN_CONSENSUS, f"{what} group {i}: status {int(res.status[i])}"
        got.append(res.consensus(i))
        assert got[-1] == ref(g)[0], f"{what} group {i} ({len(g)} members, longest {max(map(len, g))}): {got[-1]!r} != {ref(g)[0]!r}"
    return q, n_tier, n_over, got


def check_loops(e, groups, what="", handed_on=0):
    """... and the two loops took what the rule says: the long tasks are the list's head, the short ones went through the eight-lane loop"""
    n_short = sum(1 for g in groups if is_short(g))
    q, n_tier, n_over, got = run(e, groups, what)
    assert n_tier[0] == len(groups), f"{what}: every group is tier Q's: n_tier {n_tier}"
    assert q["split"] == len(groups) - n_short, f"{what}: {q}, {n_short} short of {len(groups)}"
    assert q["short_done"] + q["short_handed_on"] == n_short and q["short_handed_on"] == handed_on, f"{what}: {q}"
    assert n_over[0] == handed_on, f"{what}: n_over {n_over}"
    return got


def copies(seq, n, at=()):
    """seq and n - 1 members like it, those at the indices `at` with one substitution each (at different places)"""
    g = [seq] * n
    for k, i in enumerate(at):
        g[i] = sub(seq, (2 + 3 * k) % len(seq))
    return g


# ---- lengths ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, 2, 7, 8, 14, 15, 16])
def test_member_lengths_on_both_sides_of_fifteen(e, length):
    """members of 1 .. 15 bases take the short loop, members of 16 the long one (the counters say which)"""
    s = (T + "G")[:length]
    groups = [copies(s, 4, at=(2,)), [s, sub(s, 0), s[: max(1, length - 1)], s, s], [s, s]]
    assert all(is_short(g) == (length <= 15) for g in groups)
    check_loops(e, groups, f"length {length}")


def test_the_eligibility_estimate_at_its_bound_and_above(e):
    """15-base members: 49 of them put the estimate at CW_POAQ8_ROUTE_NODES (short), 50 put it above (long)"""
    at, above = copies(T, 49, at=(5, 20, 40)), copies(T, 50, at=(5, 20, 40))
    assert estimate(at) == ROUTE8 and estimate(above) > ROUTE8
    check_loops(e, [at], "estimate at the bound")
    check_loops(e, [above], "estimate above the bound")
    check_loops(e, [at, above], "both")


# ---- fewer tasks than groups, the split's edges -----------------------------------------------------------------------------------------------------------
def short_task(i):
    s = T[i % 5 : 6 + (i * 3) % 10]
    return [s, sub(s, i % len(s)), s, s[:-1] if len(s) > 1 else s, s]


def long_task(i):
    s = (T + T)[i % 7 : 16 + i % 7 + (i * 5) % 9]
    return [s, sub(s, i % len(s)), s, s[:-1], s]


@pytest.mark.parametrize("n", [1, 7, 8, 9])
def test_batches_of_short_tasks_round_a_wave_of_eight(e, n):
    groups = [short_task(i) for i in range(n)]
    assert all(is_short(g) for g in groups)
    check_loops(e, groups, f"{n} short tasks")  # split == 0


def test_the_splits_edges(e):
    longs, shorts = [long_task(i) for i in range(5)], [short_task(i) for i in range(5)]
    assert not any(is_short(g) for g in longs)
    check_loops(e, longs, "long tasks only")  # split == n
    check_loops(e, shorts, "short tasks only")  # split == 0
    check_loops(e, shorts[:1], "one short task")  # the sort's early return for n < 2
    check_loops(e, longs[:1], "one long task")
    check_loops(e, [longs[0], shorts[0]], "one of each")
    check_loops(e, [shorts[0], longs[0]], "one of each, short first")


def catalogue():
    g = [short_task(i) for i in range(11)] + [long_task(i) for i in range(6)]
    g += [copies(T, 49, at=(5, 20, 40)), copies(T, 50, at=(5, 20, 40))] + window_groups() + [far_group(), fan_group()] + isolation_groups()
    return g


def test_the_catalogue_in_two_orders_against_each_group_alone(e):
    groups = catalogue()
    alone = [check_loops(e, [g], f"alone {i}")[0] for i, g in enumerate(groups)]
    mixed = [groups[i] for i in range(0, len(groups), 2)] + [groups[i] for i in range(1, len(groups), 2)]
    assert check_loops(e, groups, "catalogue") == alone
    assert check_loops(e, mixed, "catalogue, interleaved") == [alone[groups.index(g)] for g in mixed]
    assert check_loops(e, groups[::-1], "catalogue, reversed") == alone[::-1]


# ---- the member window at eight ---------------------------------------------------------------------------------------------------------------------------
def window_groups():
    g = []
    for n in (8, 9, 16, 17):  # the window is refilled behind member 8, 16: a different member on each side of every refill
        g.append([T[:13]] + [sub(T[:13], (i * 5) % 13) if i % 3 == 0 else T[:13] for i in range(1, n)])
        g.append([sub(T[:12], i % 12) for i in range(n)])
    for r in (3, 8, 9):  # a clean member (it adds nothing to the graph), then r members identical to it: a replay run, over a refill for 8 and 9
        g.append([T[:14], sub(T[:14], 4), T[:14]] + [T[:14]] * r + [sub(T[:14], 9)])
        g.append([T[:14], T[:14]] + [T[:14]] * r + [sub(T[:14], 3), T[:14]])
    g.append([T[:11], T[:11], sub(T[:11], 5), T[:11]])  # a duplicate of the first member
    return g


def test_the_member_window_at_eight_members(e):
    groups = window_groups()
    assert all(is_short(g) for g in groups)
    check_loops(e, groups, "member windows")
    for i, g in enumerate(groups):
        check_loops(e, [g], f"member window {i} alone")


# ---- lane isolation ---------------------------------------------------------------------------------------------------------------------------------------
def isolation_groups():
    """Eight different tasks for one wave (a wave claims its eight tasks in one instruction): different bases, the high scores at different columns -- the
    last columns of one task (lane 7) beside the first of the next (lane 8) --, odd and even lengths and member counts side by side.  A value that crossed from
    a group's lane 7 into its neighbour's lane 0 would be a diagonal or a running maximum from nowhere, and change that neighbour's path."""
    g = []
    for i in range(8):
        a, b = "ACGT"[i % 4], "ACGT"[(i + 1 + i // 4) % 4]
        if a == b:
            b = "ACGT"[(i + 2) % 4]
        n = 15 - (i % 3)  # 15, 14, 13: the last lane of the group holds columns 14 and 15
        s = (a * (n - 4) + b * 4) if i % 2 == 0 else (b * 4 + a * (n - 4))  # the run of matches at the task's last columns, or at its first
        members = [s, sub(s, n - 1), s[1:], sub(s, 0), s[:-1] + b, s, s[2:], s][: 5 + i % 4]
        g.append(members)
    return g


def test_eight_unlike_tasks_side_by_side_do_not_see_each_other(e):
    groups = isolation_groups()
    assert all(is_short(g) for g in groups) and len({tuple(g) for g in groups}) == 8
    alone = [check_loops(e, [g], f"isolation {i} alone")[0] for i, g in enumerate(groups)]
    assert check_loops(e, groups, "isolation") == alone
    assert check_loops(e, groups[::-1], "isolation, reversed") == alone[::-1]
    twice = groups + [list(g) for g in groups[::-1]]  # sixteen: two waves' worth, every task with other neighbours
    assert check_loops(e, twice, "isolation, twice") == alone + alone[::-1]


# ---- capacities -------------------------------------------------------------------------------------------------------------------------------------------
def node_group(nodes):
    """the template and single substitutions of it, one new node each, until the graph has `nodes` nodes"""
    g = [T]
    for i in range(1, 14):
        for b in "ACGT":
            if b != T[i] and len(T) + len(g) - 1 < nodes:
                g.append(sub(T, i, b))
    return g


# members that walk the seven full columns 3 .. 9 of edge_group()'s graph along new pairs of neighbours: no new node, new edges only (found by a search with the reference)
EDGE_WALKS = ["ACGACAATTACTTAC", "ACGCACGGGCCTTAC", "ACGCGATGCCCTTAC", "ACGAGTATCTCTTAC", "ACGGCTTTTGCTTAC", "ACGGGCAGACCTTAC", "ACGTAGGCCACTTAC", "ACGATCTCGACTTAC",
              "ACGAATTTGTCTTAC", "ACGTTAGGTCCTTAC", "ACGCATGTCCCTTAC", "ACGACGTCTACTTAC"]
EDGE_ONE_MORE = "ACGCCGTAATCTTAC"


def edge_group(one_more=False):
    g = [T] + [sub(T, i, b) for i in range(3, 10) for b in "ACGT" if b != T[i]] + EDGE_WALKS
    return g + [EDGE_ONE_MORE] if one_more else g


def far_group():
    """substitutions put a second node into columns 5 .. 9, then a member without columns 4 .. 10: an edge over more than RING ranks, read from the slab by every later fill"""
    d = T[:4] + T[11:]
    return [T] + [sub(T, i, "T" if T[i] != "T" else "A") for i in range(5, 10)] + [d, d, sub(d, 2), T, d]


def fan_group():
    """four bases in column 6 and a member without it: five in-edges at the node of column 7 (the fourth and later take the kept-row branch of the walk)"""
    return [T] + [sub(T, 6, b) for b in "ACGT" if b != T[6]] + [T[:6] + T[7:], T[:5] + "TT" + T[7:], T[:6] + T[7:], sub(T, 6, "T"), T]


def test_a_graph_of_exactly_nc8_nodes_stays_and_one_more_node_goes_to_tier_s(e):
    fits, over = node_group(NC8), node_group(NC8 + 1)
    assert ref(fits)[1][-1].nodes == NC8 and max(s.edges for s in ref(fits)[1]) <= EC8 and is_short(fits)
    assert ref(over)[1][-1].nodes == NC8 + 1 and ref(over)[1][-2].nodes == NC8 and max(s.edges for s in ref(over)[1]) <= EC8 and is_short(over)
    check_loops(e, [fits], "NC8 nodes")
    check_loops(e, [over], "NC8 + 1 nodes", handed_on=1)  # short_handed_on == 1, n_over[0] == 1, and tier S's consensus is the reference's
    check_loops(e, [fits, over, short_task(3)], "both, and a bystander", handed_on=1)


def test_a_graph_of_exactly_ec8_edges_stays_and_one_more_edge_goes_to_tier_s(e):
    fits, over = edge_group(), edge_group(one_more=True)
    assert ref(fits)[1][-1].edges == EC8 and ref(fits)[1][-1].nodes <= NC8 and is_short(fits)
    assert ref(over)[1][-1].edges == EC8 + 1 and ref(over)[1][-1].new_nodes == 0 and ref(over)[1][-1].nodes <= NC8 and is_short(over)
    check_loops(e, [fits], "EC8 edges")
    check_loops(e, [over], "EC8 + 1 edges", handed_on=1)
    check_loops(e, [over, fits, short_task(4)], "both, and a bystander", handed_on=1)


def test_rows_kept_in_the_slab(e):
    far, fan = far_group(), fan_group()
    assert max(s.max_far for s in ref(far)[1][:-1]) > RING and is_short(far), ref(far)[1]  # a predecessor beyond the ring, before the last member's fill
    assert max(s.max_indeg for s in ref(fan)[1][:-1]) >= 4 and is_short(fan), ref(fan)[1]  # a fourth in-edge, before the last member's walk
    check_loops(e, [far], "far predecessor")
    check_loops(e, [fan], "four and more in-edges")
    check_loops(e, [far, fan, far, fan, fan, far, short_task(1), far, fan], "both, nine to a wave and one over")
