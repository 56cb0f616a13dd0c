"""Groups for the tests of the POA operator (cw_poa_run, consent_amd/csrc/cw_poa_op.h): noisy copies of one random string, a Python mirror of the
routing rule, and the oracle's consensus of every probe, computed once.  Test infrastructure only."""
import functools
import random

import oracle_lib

MAX_MSA = 1000  # the tests' engine: every member of every group here is aligned
PRM = (9, 4, 8, 2, MAX_MSA)  # (k, solid, common_kmers and min_anchors are not read by the operator)
POAX_LC = 4095  # csrc/cw_poa.h: the longest member any tier takes

# longest member x members (the issue's catalogue) -> the tier the routing rule sends the task to first and the tier that ends up aligning it.  The rule
# (route() below, csrc/cw_chain.h) sends 100 x 10 to M1, 200 x 8 to M2 and 400 x 8 to L -- a tier further than a glance at the capacities suggests: it goes by
# the expected graph, 1.7 x the longest member.  60 x 8 is added so that tier S has a probe too.
SHAPES = {"24x12": (24, 12), "60x8": (60, 8), "100x10": (100, 10), "200x8": (200, 8), "400x8": (400, 8), "900x6": (900, 6), "1500x5": (1500, 5), "2500x4": (2500, 4)}
BENCH_SHAPES = ["24x12", "100x10", "200x8", "400x8", "900x6"]  # tools/poa_bench.py's table


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def ont_copy(rng, s, rate=0.12):
    """A noisy copy: `rate` errors a base, substitutions : insertions : deletions 30 : 30 : 40 (the ONT mix of SURVEY 8d)."""
    out = []
    for c in s:
        x = rng.random()
        if x < rate * 0.4:
            continue
        if x < rate * 0.7:
            out.append(rng.choice("ACGT"))
            out.append(c)
        elif x < rate:
            out.append(rng.choice("ACGT".replace(c, "")))
        else:
            out.append(c)
    return "".join(out)


def noisy_group(seed, longest, members, rate=0.12):
    """`members` noisy copies of one random string, cut to `longest` bases: the string is an eighth longer, so most copies are cut and the longest member
    is exactly `longest`."""
    rng = random.Random(seed)
    truth = rand_seq(rng, longest + longest // 8 + 2)
    g = [ont_copy(rng, truth, rate)[:longest] for _ in range(members)]
    assert max(len(s) for s in g) == longest, (seed, longest, members)
    return g


@functools.lru_cache(maxsize=None)
def probe(name):
    longest, members = SHAPES[name]
    return noisy_group(0x90A0 + longest, longest, members)


def q_group(i):
    """A small tier-Q group: 4-12 copies of a 12-30 base string."""
    rng = random.Random(0x51000 + i)
    return noisy_group(0x52000 + i, rng.randrange(12, 31), rng.randrange(4, 13))


def aligned_members(group, max_msa=MAX_MSA):
    """What the operator aligns: the first max_msa non-empty sequences, in order."""
    return [s for s in group if s][:max_msa]


_ORACLE = {}


def oracle_consensus(group, max_msa=MAX_MSA):
    """The oracle's POA consensus of the group's aligned members ('' for none, the member for one): computed once per group."""
    key = (tuple(group), max_msa)
    if key not in _ORACLE:
        m = aligned_members(group, max_msa)
        _ORACLE[key] = "" if not m else m[0] if len(m) == 1 else oracle_lib.oracle_poa(m)
    return _ORACLE[key]


# csrc/cw_poa.h, cw_poa_q.h: the bounds the routing rule reads (the product build: tier H off, tier Q on)
Q_LC, Q_ROUTE, S_LC, S_ROUTE, M1_LC, M1_ROUTE, M2_LC, M2_ROUTE, L_LC, G_LC = 31, 60, 127, 112, 255, 208, 511, 512, 1023, 2047


def route(n, mx):
    """The routing rule of the chain kernel's flush (csrc/cw_chain.h) for a task of n members, the longest of mx bases: 'Q', 'S', 'M1', 'M2' or 'L'."""
    est, est_s = (mx * 17 + 9) // 10, (mx * (15 + n // 5) + 9) // 10
    if mx <= Q_LC and est_s <= Q_ROUTE:
        return "Q"
    if est_s <= S_ROUTE and mx <= S_LC:
        return "S"
    if max(est, est_s) <= M1_ROUTE and mx <= M1_LC:
        return "M1"
    if est <= M2_ROUTE and mx <= M2_LC:
        return "M2"
    return "L"


def last_tier(n, mx):
    """The tier whose member capacity the task needs: the routed one, or G / X for members beyond tier L's / tier G's bases."""
    return "X" if mx > G_LC else "G" if mx > L_LC else route(n, mx)
