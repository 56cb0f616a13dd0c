"""Groups for the tests of tier Q's member window (csrc/cw_poa_q.h PoaQWin, poaq_window): the family of runs of equal members, and stated groups built so
that ONE wrong decision of the window changes the consensus.  The consensus is a column vote, so a group can only show a fault when its vote hangs on the
member in question: every stated group is a few copies of a string `a` (the first is the template, which wins ties) and then copies of a string `x` one edit
away, as many or one more, so that the vote of the column where they differ turns on a single member.  MUTANTS lists, per stated group, what the window's
faults would make of it -- a member taken for a copy of the one before it (the compare misses their difference), a copy counted once too often or once too
rarely -- and tests/test_tier_q_members_cpu.py asserts on the oracle that each of them has another consensus.  Test infrastructure only."""
import random

import poa_op_probes as pp

LENGTHS = (8, 12, 16, 17, 24, 31)
COUNTS = (2, 15, 16, 17, 18, 31, 32, 33, 34, 48, 49, 64, 65, 100, 255)


def est(mx, n):
    """The routing rule's depth-aware estimate of the graph (csrc/cw_poa_q.h cw_poa_route): tier Q takes a task while it stays <= 60."""
    return (mx * (15 + n // 5) + 9) // 10


def sub(s, i, rng=None):
    c = "ACGT".replace(s[i], "")
    return s[:i] + (rng.choice(c) if rng else c[0]) + s[i + 1 :]


def variants(rng, s, longer):
    """Five variants of s, each one edit away: a substitution, a deleted base or (where the member may grow: `longer`) an inserted base."""
    out = []
    while len(out) < 5:
        kind = rng.choice("SDI" if longer else "SD")
        i = rng.randrange(len(s))
        v = sub(s, i, rng) if kind == "S" else s[:i] + s[i + 1 :] if kind == "D" else s[:i] + rng.choice("ACGT") + s[i:]
        if v != s and v not in out:
            out.append(v)
    return out


def run_group(length, n):
    """n members: the base string or one of its five variants, in runs of 1-20 equal ones."""
    rng = random.Random(0x7100 + 1000 * length + n)
    s = pp.rand_seq(rng, length)
    pool = [s] + variants(rng, s, longer=length < pp.Q_LC and est(length + 1, n) <= pp.Q_ROUTE)  # an inserted base must not take the task out of the tier
    g = []
    while len(g) < n:
        g += [rng.choice(pool)] * rng.randint(1, 20)
    return g[:n]


FAMILY = {f"{length} bases x {n}": run_group(length, n) for length in LENGTHS for n in COUNTS if est(length, n) <= pp.Q_ROUTE}


# ---- what a fault of the window makes of a group ------------------------------------------------------------------------------------------------

def false_repeat(g, i):
    """Member i taken for a copy of member i - 1: its path is member i - 1's, and so is that of every copy of member i that follows it (they equal member i)."""
    j = i
    while j < len(g) and g[j] == g[i]:
        j += 1
    return g[:i] + [g[i - 1]] * (j - i) + g[j:]


def one_more(g, i):
    """Member i counted once too often (a run taken one member too far, r one too large)."""
    return g[: i + 1] + [g[i]] + g[i + 1 :]


def one_less(g, i):
    """Member i not counted (r one too small)."""
    return g[:i] + g[i + 1 :]


def _stated():
    rng = random.Random(0x7157)
    a12, a16, a17, a31 = (pp.rand_seq(rng, n) for n in (12, 16, 17, 31))
    groups, mutants = {}, {}

    def vote(name, a, x, na=3, nx=4):
        """na copies of a, then nx of x: member na is the first that differs from its predecessor, and x wins the vote by the copies behind it."""
        groups[name] = [a] * na + [x] * nx
        mutants[name] = {"the first x taken for a copy of a": false_repeat(groups[name], na)}

    # keys that differ from their predecessor's in one place only: the last base, the first, the base on either side of the key's word boundary, the length alone
    for tag, a in (("16", a16), ("17", a17), ("31", a31)):  # 16: the key's first word is full; 17: one base in the second; 31: the last bits of the key
        vote(f"{tag} bases, then another last base", a, sub(a, len(a) - 1))
        vote(f"{tag} bases, then another first base", a, sub(a, 0))
        a_ = a[:-1] + "A"  # code 0: the key of the prefix is the key of the whole, only the length tells them apart
        vote(f"{tag} bases, then the proper prefix", a_, a_[:-1])
        vote(f"{tag} bases, the prefix and then the whole", a_[:-1], a_)
    for tag, a in (("17", a17), ("31", a31)):
        vote(f"{tag} bases, then another base 15", a, sub(a, 15))
        vote(f"{tag} bases, then another base 16", a, sub(a, 16))
    # a run of equal members whose last one is member `end`: on the window's last lane, on the next window's first, on its second.  One more copy of x behind it
    # than of a: x wins unless the member behind the run is taken into it; as many: a (the template) wins the tie unless a copy of either is miscounted
    x16 = sub(a16, 9)
    for end in (15, 16, 17):
        n1, n2 = f"run ends at member {end}, one more behind it", f"run ends at member {end}, as many behind it"
        groups[n1], groups[n2] = [a16] * (end + 1) + [x16] * (end + 2), [a16] * (end + 1) + [x16] * (end + 1)
        mutants[n1] = {"the member behind the run taken into it": false_repeat(groups[n1], end + 1), "the run counted once too often": one_more(groups[n1], end)}
        mutants[n2] = {"the run counted once too rarely": one_less(groups[n2], end), "the run behind it counted once too often": one_more(groups[n2], end + 1)}
    # runs that cover two whole windows (members 16 .. 47 are inside the run of a; the run of x covers two more)
    x12 = sub(a12, 7)
    n1, n2 = "run over two whole windows, one more behind it", "run over two whole windows, as many behind it"
    groups[n1], groups[n2] = [a12] * 52 + [x12] * 53, [a12] * 52 + [x12] * 52
    mutants[n1] = {"the member behind the run taken into it": false_repeat(groups[n1], 52), "the run counted once too often": one_more(groups[n1], 51)}
    mutants[n2] = {"the run counted once too rarely": one_less(groups[n2], 51), "the run behind it counted once too often": one_more(groups[n2], 52)}
    # a repeat right after a member that added a node: the first repeat of `ins` is aligned, not replayed (nothing of the result hangs on which: no mutant)
    ins = a16[:7] + ("A" if a16[7] != "A" else "C") + a16[7:]
    groups["repeat right after a member that added a node"] = [a16, a16, a16, ins, ins, ins, ins, a16]
    return groups, mutants


STATED, MUTANTS = _stated()
GROUPS = dict(FAMILY, **STATED)
