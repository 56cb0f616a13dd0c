"""The probe catalogue of the slab POA tiers S, M1, M2, L, G and X (consent_amd/csrc/cw_poa.h poa_run and its phases, cw_poa_c.h), shared by
tests/test_poa_ref_cpu.py and tests/test_gpu_poa_routes.py.

A probe is one group for cw_poa_run, alone in its batch.  It states
  tiers    the tiers it visits, in order: the first is the one the routing rule names (poa_op_probes.route, asserted by the CPU test; a tier-Q task that
           tier Q hands on is none of this catalogue's), every later one a hand-over (rc 2) of the tier before it
  has      route bits ('tier.bit', consent_amd/engine.py POA_ROUTE / POA_RC2) the test-aid library must report, `lacks` bits it must not; beyond `lacks`, no bit
           of a tier the probe does not visit may be set
  stops    True: the group ends with status 2 and CW_WHY_POA instead of a consensus
  proves   what tests/poa_ref.py's per-member statistics must show for the probe to cross what it is named for (node and edge counts at a capacity,
           in-degrees, rank distances, which members add nothing): the CPU test re-proves every one
  mutants  groups a wrong replay or a wrong group fill would in effect align instead: the reference gives each another consensus

What the default build can and cannot reach, read from the code (UNREACHABLE, with the reason per bit; NOT_PROBED: reachable, but only by a probe too
large for a suite that runs in seconds).  The routing rule sends a task by its LONGEST member mx (est = ceil(1.7 mx), est_s = ceil(mx (15 + n / 5) / 10)):
  tier S   takes est_s <= 112, so mx <= 74: its l_cap of 127 is never met, its packed fill sees rows of 66 .. 75 columns only
  tier M1  takes max(est, est_s) <= 208, so mx <= 122: l_cap 255 never met, poa_fill_pk<2> (rows of 129 .. 256 columns) never runs
  tier M2  takes est <= 512, so mx <= 301: l_cap 511 never met, poa_fill_pk<4> sees rows of 258 .. 302 columns only
  tier L   takes the rest; members beyond 1 023 bases go on to tier G, beyond 2 047 to tier X; a group with a member beyond 4 095 gets no task at all
Test infrastructure only."""
import collections
import copy
import functools
import os
import random
import re

import poa_op_probes as pp
import poa_ref
from consent_amd.engine import POA_RC2, POA_ROUTE, POA_TIERS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constants():
    """Every tier's (nodes, edges, longest member) and the constants of the fills, out of cw_poa.h."""
    hdr = open(os.path.join(ROOT, "consent_amd", "csrc", "cw_poa.h")).read()

    def num(name):
        return int(re.search(rf"#\s*define {name} (\d+)", hdr).group(1))

    caps = {t: tuple(num(f"CW_{p}_{x}") for x in ("NC", "EC", "LC")) for t, p in (("S", "POA"), ("M1", "POAM1"), ("M2", "POAM2"), ("L", "POAL"), ("G", "POAB"), ("X", "POAX"))}
    return caps, {"GF_LC": num("CW_GF_LC"), "RING": num("CW_RING"), "PK_SPAN": num("CW_POA_PK_SPAN"), "X_MIN_SLABS": int(re.search(r"#define CW_POAX_MIN_SLABS (\d+)u", hdr).group(1))}


CAPS, K = header_constants()
NEXT = {"S": "L", "M1": "L", "M2": "L", "L": "G", "G": "X", "X": None}  # poa_hand_over: where an rc 2 sends the task
G_CELLS = (CAPS["G"][0] + 1) * 1024  # CW_POAB_HC: tier G's int32 matrix


def x_cells():
    """Tier X's matrix in int32 cells: CW_POAX_MIN_SLABS slabs of tier G (cw_plan.h big_slab_bytes) less its own graph arrays (cw_poa.h CW_POAX_GRAPH_BYTES)."""
    def graph_bytes(nc, ec, lc):
        return (nc * 29 + ec * 6 + 7 * (lc + 1) + 64 + 15) // 16 * 16

    nc, ec, lc = CAPS["G"]
    slab = (G_CELLS * 4 + graph_bytes(nc, ec, lc) + 255) // 256 * 256
    xn, _, xl = CAPS["X"]
    own = graph_bytes(xn, 2 * (xn + 1), xl) + (4 * xn + 255) // 256 * 256
    return (K["X_MIN_SLABS"] * slab - own) // 4


X_CELLS = x_cells()

Probe = collections.namedtuple("Probe", "name group tiers has lacks stops proves mutants")
PROBES = {}


def add(name, group, tiers, has, lacks=(), stops=False, proves=None, mutants=None):
    assert name not in PROBES, name
    tiers = tiers.split()
    assert tiers or stops, name
    has, lacks = set(has.split()) if isinstance(has, str) else set(has), set(lacks.split()) if isinstance(lacks, str) else set(lacks)
    for a, b in zip(tiers, tiers[1:]):
        assert NEXT[a] == b, (name, tiers)
    for bit in has | lacks:
        t, n = bit.split(".")
        assert t in POA_TIERS and (n in POA_ROUTE or n in POA_RC2), bit
    PROBES[name] = Probe(name, group, tiers, has, lacks, stops, proves or {}, mutants or {})


@functools.lru_cache(maxsize=None)
def reference(name):
    """(consensus, [MemberStats]) of probe `name` by tests/poa_ref.py, computed once."""
    return poa_ref.poa(pp.aligned_members(PROBES[name].group))


def bits(tier, names):
    return " ".join(f"{tier}.{n}" for n in names.split())


def visits(group):
    """The tiers cw_poa.h's capacities send the group through, by the reference's graph after every member: (tiers, stops, {tier: cause of its rc 2})."""
    m = pp.aligned_members(group)
    n, mx = len(m), max(len(s) for s in m)
    if mx > CAPS["X"][2]:
        return [], True, {}
    _, stats = poa_ref.poa(m)
    tier, tiers, why = pp.route(n, mx), [], {}
    if tier == "Q":  # (tier Q has capacities of its own, csrc/cw_poa_q.h: not this catalogue's)
        return ["Q"], False, {}
    while tier:
        tiers.append(tier)
        nc, ec, lc = CAPS[tier]
        cause, nodes = None, 0
        for s, st in zip(m, stats):
            cells = (nodes + 1) * (len(s) + 1)
            if len(s) > lc:
                cause = "rc2_lcap"
            elif nodes and tier == "G" and cells > G_CELLS or nodes and tier == "X" and cells > X_CELLS:
                cause = "rc2_hcap"
            elif st.nodes > nc:
                cause = "rc2_nodes"  # (poa_merge counts the fresh nodes before it adds an edge)
            elif st.edges > ec:
                cause = "rc2_edges"
            if cause:
                break
            nodes = st.nodes
        if not cause:
            return tiers, False, why
        why[tier] = cause
        tier = NEXT[tier]
    return tiers, True, why


# ---- building blocks ------------------------------------------------------------------------------------------------------------------------------

def noisy(rng, s, rate):
    return pp.ont_copy(rng, s, rate)


def cut(rng, t, n, rate=0.0):
    """A slice of t that comes out n bases long: exact (rate 0) or a noisy copy, cut or padded from t to n bases exactly."""
    a = rng.randrange(0, len(t) - n + 1)
    if rate == 0.0:
        return t[a : a + n]
    for _ in range(200):
        a = rng.randrange(0, max(1, len(t) - n - n // 8 - 1))
        c = noisy(rng, t[a : a + n + n // 8 + 2], rate)[:n]
        if len(c) == n and c != t[a : a + n]:
            return c
    raise AssertionError(n)


def sub(s, i):
    return s[:i] + "ACGT"["ACGT".index(s[i]) ^ 1] + s[i + 1 :]


WIDTHS = (8, 31, 32, 62, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 2047)


def ladder(seed, longest, rate, groups, widths=WIDTHS, near_longest=True):
    """(group, proves): the longest member first (it fixes the tier) and a noisy copy of the whole; in tiers M2 / L the runs of short members (group_runs);
    then noisy slices of the first member at every width of `widths` below `longest`, and one of longest - 1 bases."""
    rng = random.Random(seed)
    t = pp.rand_seq(rng, longest)
    g, proves = [t], {}
    if groups:
        g, proves = group_runs(rng, t)
    g.append(cut(rng, t, longest, rate))
    for w in [w for w in widths if w < longest] + ([longest - 1] if near_longest else []):
        g.append(cut(rng, t, w, rate if w > 8 else 0.0))
    return g, proves


PRIMING = 5


def group_runs(rng, t):
    """(group, proves): t, then runs of members of at most CW_GF_LC = 31 bases, each run ended by a member of 32.  A short member is aligned wherever its bases
    match in order, so even an exact slice of t adds edges the first time; every member here is therefore shown to the graph once (the priming pass: groups
    are opened and abandoned), after which it adds nothing (`clean`, proved by the reference) and the group a run opens is read to its end: runs of two,
    three, four members (gk 2, 3, 4), of five (a group of four, then a member alone), a run whose second member is new and adds to the graph (meta_ok falls,
    the group is abandoned, the rest opens another), and a run with a member repeated (the replay's branch inside a group).  s[0] has 31 bases, sep 32."""
    s = [cut(rng, t, n) for n in (31, 8, 20, 27, 15)]
    sep = cut(rng, t, 32)
    new = sub(cut(rng, t, 21), 10)
    g = [t] + (s + [sep]) * PRIMING  # more than once: a later pass settles what the edges of the pass before changed in the alignments
    clean, adds = [], []

    def run(members, dirty=()):
        for m in members + [sep]:
            (adds if m in dirty else clean).append(len(g))
            g.append(m)

    run(s[:2])
    run(s[:3])
    run(s[:4])
    run(s[:5])
    run([s[0], new, s[2], s[3]], dirty=(new,))
    run([s[0], s[1], s[1], s[2]])
    return g, {"clean": clean, "adds": adds}


def vote(tier, seed, longest, na=3, nx=4):
    """The replay's stated group (tests/tier_q_member_groups.py vote): na copies of a, then nx of x, one base different: the column's vote turns on one member."""
    rng = random.Random(seed)
    a = pp.rand_seq(rng, longest)
    x = sub(a, longest // 2)
    return [a] * na + [x] * nx


# ---- 1. a ladder per tier -------------------------------------------------------------------------------------------------------------------------
# (tier S: at most 14 members of at most 65 bases keep est_s <= 112, fewer than five of at most 74; tier M1: at most 14 of at most 122)
GROUP_BITS = "fill_group grp_2 grp_3 grp_4 grp_read grp_abandoned replay replay_grp meta_reused"


def add_ladder(name, tiers, has, lacks, *args, **kw):
    g, proves = ladder(*args, **kw)
    add(name, g, tiers, has, lacks, proves=proves)


add_ladder("ladder S", "S", bits("S", "fill_coded walk_coded fill_pk1 walk_tiles"), bits("S", "fill_pad fill_pk2 fill_group walk_runs walk_dirs rc2_nodes rc2_edges rc2_lcap"),
           0x5001, 65, 0.1, False)
add_ladder("S at 74 bases", "S", bits("S", "fill_coded fill_pk1 walk_tiles"), bits("S", "rc2_lcap rc2_nodes rc2_edges"), 0x5002, 74, 0.1, False, widths=(63, 64), near_longest=False)
add_ladder("ladder M1", "M1", bits("M1", "fill_coded walk_coded fill_pk1 walk_tiles"), bits("M1", "fill_pad fill_pk2 fill_group walk_runs walk_dirs rc2_nodes rc2_edges rc2_lcap"),
           0x5101, 122, 0.1, False)
add_ladder("ladder M2", "M2", bits("M2", "fill_pad fill_pk1 fill_pk2 fill_pk4 walk_tiles " + GROUP_BITS),
           bits("M2", "fill_coded walk_coded fill_pk8 fill_w1 walk_runs walk_dirs rc2_nodes rc2_edges rc2_lcap"), 0x5201, 301, 0.08, True)
add_ladder("ladder L", "L", bits("L", "fill_pad fill_pk1 fill_pk2 fill_pk4 fill_pk8 walk_runs " + GROUP_BITS),
           bits("L", "fill_coded fill_w1 fill_w2 fill_w4 fill_w8 fill_w16 walk_tiles walk_dirs rc2_nodes rc2_edges rc2_lcap"), 0x5301, 1023, 0.03, True)
# tier G's matrix holds (4096 + 1) x 1024 cells: a second member of 2 047 bases fits against the first member's 2 047 nodes and against nothing larger
add_ladder("ladder G", "L G", bits("G", "fill_w1 fill_w2 fill_w4 fill_w8 fill_w16 fill_w32 walk_tiles") + " L.rc2_lcap",
           bits("G", "fill_pad fill_pk1 fill_group walk_runs rc2_lcap rc2_nodes rc2_edges rc2_hcap") + " " + bits("L", "fill_pad fill_pk8 walk_runs"), 0x5401, 2047, 0.02, False,
           widths=WIDTHS + (1500,), near_longest=False)
add_ladder("ladder X", "L G X", bits("X", "fill_w1 fill_w2 fill_w4 fill_w8 fill_w16 fill_w32 fill_blocks walk_tiles") + " L.rc2_lcap G.rc2_lcap",
           bits("X", "rc2_hcap rc2_nodes rc2_edges rc2_lcap") + " " + bits("G", "fill_w1 fill_w32 walk_tiles"), 0x5501, 4095, 0.01, False, widths=WIDTHS + (2048,))

# ---- 2. replay in the slab tiers ------------------------------------------------------------------------------------------------------------------
REPLAY_SHAPES = {"S": (60, 3, 4), "M1": (110, 3, 4), "M2": (290, 3, 4), "L": (700, 3, 4), "G": (1500, 3, 4), "X": (2500, 2, 3)}
for _t, (_len, _na, _nx) in REPLAY_SHAPES.items():
    _g = vote(_t, 0x6000 + _len, _len, _na, _nx)
    _path = {"G": "L G", "X": "L G X"}.get(_t, _t)
    # a, a ... replayed; the first x is aligned (equal length, one base different) and adds a node; the second x is aligned again (its predecessor was not clean); the rest are replayed
    add(f"replay {_t}: copies, then one base different", _g, _path, bits(_t, "replay meta_reused") + {"G": " L.rc2_lcap", "X": " L.rc2_lcap G.rc2_lcap"}.get(_t, ""), bits(_t, "rc2_nodes rc2_edges"),
        proves={"clean": [i for i in range(1, len(_g)) if i != _na], "adds": [_na]},
        mutants={"the first x taken for a copy of a": [_g[0]] * (_na + 1) + [_g[-1]] * (_nx - 1), "a copy of x not counted": _g[:-1] + [_g[0]],
                 "a copy of a counted once too often": [_g[0]] + _g[:-1]})
_a = pp.rand_seq(random.Random(0x6101), 200)
_ins = _a[:90] + "ACGT"["ACGT".index(_a[90]) ^ 2] + _a[90:]
add("replay M2: a repeat right after a member that added a node", [_a, _a, _ins, _ins, _ins, _ins, _a], "M2", bits("M2", "replay meta_reused"),
    proves={"clean": [1, 3, 4, 5, 6], "adds": [2]}, mutants={"the inserted base lost with its first copy": [_a, _a, _a, _ins, _ins, _ins, _a]})

# ---- 3. coded-path rows in tiers S and M1: nodes of 4, 5 and 6 in-edges, predecessors 17 or more ranks back ---------------------------------------


def fan_group(seed, first, piece, members):
    """The first member of `first` bases; then its first `piece` (<= 63) bases with the k bases before position p left out, k = 1 .. 5 and 20 .. 22: the node at p
    gains an in-edge from k + 1 ranks back each time (where the alignment does not spread the bases in front of the gap over the skipped nodes: the
    reference's statistics say what came of it)."""
    rng = random.Random(seed)
    t = pp.rand_seq(rng, first)
    p = 40
    g = [t]
    for k in (1, 2, 3, 4, 5, 20, 21, 22)[: members - 1]:
        g.append(t[: p - k] + t[p:piece])
    return g + [g[1]]  # one more member after the last far edge: a coded fill that meets it


add("coded rows S: fan-in 6 and far predecessors", fan_group(0x7001, 60, 60, 9), "S", bits("S", "fill_coded walk_coded row_far row_fan4 row_slab"), bits("S", "fill_pk1 walk_tiles rc2_nodes"),
    proves={"max_indeg": 6, "max_far": 17})
add("coded rows M1: fan-in 6 and far predecessors", fan_group(0x7002, 120, 63, 9), "M1", bits("M1", "fill_coded walk_coded row_far row_fan4 row_slab"), bits("M1", "fill_pk1 rc2_nodes"),
    proves={"max_indeg": 6, "max_far": 17})
add("coded rows S: near predecessors only", pp.noisy_group(0x7003, 40, 4, 0.05), "S", bits("S", "fill_coded walk_coded"), bits("S", "row_far fill_pk1 walk_tiles"), proves={"max_far_at_most": 16})


# ---- 4. capacities, exact --------------------------------------------------------------------------------------------------------------------------

def grow(seed, first, others, other_len, sub_rate=None):
    """The first member and `others` more: unrelated random strings (nodes grow fastest), or -- sub_rate -- the first member with that share of its bases
    substituted and no base inserted or left out (equal lengths, columns fill up to four nodes: edges grow faster than nodes)."""
    rng = random.Random(seed)
    t = pp.rand_seq(rng, first)
    if sub_rate is None:
        return [t] + [pp.rand_seq(rng, other_len) for _ in range(others)]
    return [t] + ["".join(rng.choice("ACGT".replace(c, "")) if rng.random() < sub_rate else c for c in t) for _ in range(others)]


def pad_to(group, want_nodes, seed, cap=None):
    """(bases, variant): `group` gets one more member, an unrelated random string of so many bases (no longer than the longest member), chosen so that
    the reference's graph ends at want_nodes nodes exactly.  The search behind the constants of CAPACITY: run on the CPU, once."""
    g = poa_ref.Graph()
    for s in group:
        st = g.add(s)
    need, mx = want_nodes - st.nodes, cap or max(len(s) for s in group)
    assert need > 0, (st.nodes, want_nodes)
    for j in range(60):  # the node count grows with the member's length, near enough for a bisection; a variant that steps over want_nodes is dropped
        lo, hi = need, mx
        while lo <= hi:
            m = (lo + hi) // 2
            got = copy.deepcopy(g).add(padded(group, seed, m, j, cap)[-1]).nodes
            if got == want_nodes:
                return m, j
            lo, hi = (m + 1, hi) if got < want_nodes else (lo, m - 1)
    raise AssertionError("no member found")


def padded(group, seed, m, j, cap=None):
    return group + [pp.rand_seq(random.Random(seed * 1000 + j), cap or max(len(s) for s in group))[:m]]


# tier -> (seed, first member, other members, their length of the unrelated members that grow the nodes, {nodes wanted: pad_to's answer}, longest last member,
#          grow() arguments of the substituted members that grow the edges)
CAPACITY = {
    "S": ((0x8001, 60, 3, 50), {128: (58, 0), 129: (58, 8)}, None, (0x8104, 28, 113, 28, 0.3)),
    "M1": ((0x8002, 120, 4, 100), {256: (72, 0), 257: (75, 0)}, None, (0x8104, 56, 62, 56, 0.3)),
    "M2": ((0x8003, 290, 2, 250), {512: (215, 0), 513: (216, 0)}, None, (0x1, 120, 55, 120, 0.3)),
    "L": ((0x8004, 900, 2, 800), {1536: (464, 0), 1537: (465, 0)}, None, (0x1, 360, 61, 360, 0.3)),
    # (tier G: a first member of 2 047 bases reaches it by its length; the others stay at 1 000 bases, whose rows of 1 001 cells its matrix holds for 4 096 nodes)
    "G": ((0x8005, 2047, 12, 1000), {4096: (891, 0), 4097: (913, 1)}, 1000, (0x8105, 1000, 18, 1000, 0.45)),
}
VISITS = {"S": "S", "M1": "M1", "M2": "M2", "L": "L", "G": "L G"}
for _t, (_nodes, _found, _cap, _edges) in CAPACITY.items():
    _nc, _ec, _ = CAPS[_t]
    _base = grow(*_nodes)
    _via = " L.rc2_lcap" if _t == "G" else ""
    (_m, _j), (_m1, _j1) = _found[_nc], _found[_nc + 1]
    add(f"capacity {_t}: {_nc} nodes fit", padded(_base, _nodes[0], _m, _j, _cap), VISITS[_t], _via, bits(_t, "rc2_nodes rc2_edges rc2_hcap"), proves={"nodes": _nc, "edges_at_most": _ec})
    add(f"capacity {_t}: {_nc + 1} nodes are handed on", padded(_base, _nodes[0], _m1, _j1, _cap), VISITS[_t] + " " + NEXT[_t], f"{_t}.rc2_nodes" + _via,
        bits(_t, "rc2_edges rc2_hcap") + " " + bits(NEXT[_t], "rc2_nodes rc2_edges"), proves={"nodes": _nc + 1, "nodes_before_last": _nc, "edges_at_most": _ec})
    # members 0 .. k - 1 keep the graph inside both capacities (S, M1, M2: with exactly EC edges after member k - 1), member k takes the edges beyond EC
    add(f"capacity {_t}: edges beyond {_ec}, nodes within {_nc}", grow(*_edges), VISITS[_t] + " " + NEXT[_t], f"{_t}.rc2_edges" + (" L.rc2_nodes" if _t == "G" else ""),
        bits(_t, "rc2_nodes rc2_hcap"), proves={"edges_over": _ec, "nodes_at_most": _nc, **({"edges_before_last": _ec} if _t in ("S", "M1", "M2") else {})})

# member lengths at a tier's l_cap and one beyond (l_cap itself: the ladders of L, G and X; tiers S, M1, M2: never met, see above)
_r = random.Random(0x8301)
_t1024, _t2048, _t4096 = (pp.rand_seq(_r, n) for n in (1024, 2048, 4096))
add("1 024 bases: beyond tier L", [_t1024, cut(_r, _t1024, 1000, 0.03)], "L G", "L.rc2_lcap " + bits("G", "fill_w16 walk_tiles"), bits("L", "fill_pk8 walk_runs") + " G.rc2_lcap")
add("2 048 bases: beyond tier G", [_t2048, cut(_r, _t2048, 1000, 0.03)], "L G X", "L.rc2_lcap G.rc2_lcap " + bits("X", "fill_w16 walk_tiles"), bits("G", "fill_w16 walk_tiles") + " X.rc2_lcap")
add("4 096 bases: beyond every tier, the group stops", [_t4096, "ACGTACGT"], "", "", "", stops=True)
# tier G's matrix: (4 096 + 1) x 1 024 cells.  A third member of 2 047 bases meets a graph of more than 2 047 nodes: 2 048 cells a row do not fit
_t2047 = pp.rand_seq(_r, 2047)
add("G: the matrix beyond h_cap", [_t2047, cut(_r, _t2047, 2047, 0.02), cut(_r, _t2047, 2047, 0.02)], "L G X", "L.rc2_lcap G.rc2_hcap G.fill_w32 X.fill_w32", "G.rc2_nodes G.rc2_edges G.rc2_lcap X.rc2_hcap",
    proves={"cells_over": G_CELLS})
# tier X's matrix (X_CELLS): unrelated members of 4 095 bases until (nodes + 1) x 4 096 cells do not fit: the documented stop
add("X: the matrix beyond h_cap, the group stops", grow(0x8302, 4095, 5, 4095), "L G X", "L.rc2_lcap G.rc2_lcap X.rc2_hcap X.fill_blocks", "X.rc2_nodes X.rc2_edges", stops=True, proves={"cells_over": X_CELLS})
# one task through L, G and X: unrelated members of 900 bases grow past 1 536 nodes, past tier G's 8 192 edges (its 4 096 nodes come later) and on.  (No task
# crosses from tier S to tier X: what tier S takes has members of at most 74 bases, at most 114 of them.)
add("chain L, G, X", grow(0x8303, 900, 30, 900), "L G X", "L.rc2_nodes G.rc2_edges " + bits("X", "fill_w16 walk_tiles"), "L.rc2_lcap G.rc2_lcap G.rc2_hcap X.rc2_nodes X.rc2_hcap",
    proves={"nodes_over": CAPS["G"][0], "edges_first_in": ("G", CAPS["G"][0], CAPS["G"][1])})


# ---- 5. what no probe can reach -------------------------------------------------------------------------------------------------------------------

def _unreachable():
    """'tier.bit' -> why the default build never sets it, read from cw_poa.h (the template arguments of poa_run per tier: S <int16, PK 1, CM 2, LCAP 127>,
    M1 <int16, 1, 2, 255>, M2 <int16, 1, 0, 511>, L <int16, 2, 0, 1023>, G <int32, 0, 0>, X <int32, 0, 0, 4095, WX>)."""
    u = {}

    def no(tiers, names, why):
        for t in tiers.split():
            for n in names.split():
                assert f"{t}.{n}" not in u, (t, n)
                u[f"{t}.{n}"] = why

    no("M2 L G X", "fill_coded walk_coded row_far row_fan4 row_slab rc2_ccap", "the recorded-decision path is compiled for CM == 2 only: tiers S and M1 (CW_M2_CODES is 0)")
    no("S M1", "fill_pad", "rows of at most 64 columns take the recorded-decision path in these tiers (CW_POA_CODES); only a CW_POA_VERIFY build runs the matrix path beside it")
    no("G X", "fill_pad", "P.pad needs PK != 0")
    no("S M1 M2 L", "fill_w1", "M.pad64 is set in every slab tier (poa_slab_mem): an unpacked row of at most 64 columns is the padded fill; only -DCW_NO_PAD64 builds the masked one")
    no("S M1 M2", "fill_w2 fill_w4 fill_w8 fill_w16", "compiled for PK == 2 && LCAP > 511 only (tier L)")
    no("L", "fill_w2 fill_w4 fill_w8 fill_w16", "needs an unpacked row of more than 64 columns: n + cols > CW_POA_PK_SPAN = 2 600, against at most 1 536 nodes + 1 024 columns = 2 560; a group fill "
       "(P.grp) is packed whatever the span, and opens only while n + 32 <= 2 600")
    no("S M1 M2 L", "fill_w32", "poa_fill<32> is compiled for the int32 tiers only")
    no("S M1 M2 L G", "fill_blocks", "column blocks (j0) are tier X's")
    no("G X", "fill_pk1 fill_pk2 fill_pk4 fill_pk8", "packed fills need PK != 0")
    no("S", "fill_pk2 fill_pk4 fill_pk8", "not compiled: LCAP 127")
    no("M1", "fill_pk2", "rows of 129 .. 256 columns: the routing rule gives tier M1 tasks whose longest member has at most 122 bases (est = ceil(1.7 mx) <= CW_POAM1_ROUTE = 208)")
    no("M1", "fill_pk4 fill_pk8", "not compiled: LCAP 255")
    no("M2", "fill_pk8", "compiled for PK == 2 && LCAP > 511 only (tier L)")
    no("S M1 G X", "fill_group grp_2 grp_3 grp_4 grp_read grp_abandoned replay_grp", "poa_group_tier: PK != 0, CM == 0, int16, LCAP >= 511 -- tiers M2 and L")
    no("S M1 M2 G X", "walk_runs", "M.runs is set for tier L only")
    no("S M1 M2 G X", "walk_dirs", "d_cap is 0 (no direction words) in every tier but L")
    no("L", "walk_dirs", "M.runs is set: direction words are walked a run at a time")
    no("L", "walk_tiles", "d_cap = 1 536 x 16 pairs holds the direction words of every fill: n x nch x 2 <= 1 536 x 8 x 2")
    no("S M1 M2", "rc2_lcap", "the routing rule goes by the longest member: tier S gets mx <= 74, M1 mx <= 122, M2 mx <= 301, below their l_cap of 127, 255, 511")
    no("X", "rc2_lcap", "a group with a member beyond 4 095 bases gets no task (cw_poa_tasks_kernel: too_long); a window's pieces are shorter than twice the longest template")
    no("S M1 M2 L G X", "rc2_first", "the first member has at most l_cap bases (checked before), and l_cap < n_cap, l_cap - 1 < e_cap in every tier")
    no("S M1 M2 L", "rc2_hcap", "h_cap = (NC + 1) x (LC + 1) cells: every (n + 1) x row stride of the tier fits, the padded fill's 64 cells of slack included (rows of 64 cells against LC + 1 >= 128)")
    no("S M1", "rc2_ccap", "c_cap = NC x ((LC + 64) / 64) x 4 words: 1 024 / 4 096, against ((n + 7) / 8) x 64 <= 1 024 / 2 048 at n = NC; (n + 1) x 64 <= h_cap likewise")
    no("S M1 M2 L", "rc2_indeg", "more than 2 047 in-edges of one node need as many source nodes: beyond e_cap (S, M1, M2) or n_cap (L)")
    no("X", "rc2_indeg", "tier X's row word counts in-edges in 24 bits: the check is compiled out (WX)")
    return u


UNREACHABLE = _unreachable()
# reachable by the code, but only by a probe too large for a suite that runs in seconds (a bit listed here that IS witnessed fails the closing test all the same)
NOT_PROBED = {
    "X.rc2_nodes": "a graph of more than 65 534 nodes inside tier X's cells: more than a hundred unrelated members of 500 bases, minutes in the reference",
    "X.rc2_edges": "more than 65 534 edges: the same",
    "G.rc2_indeg": "a node with more than 2 047 in-edges: more than 2 047 members, each with an edge of its own into that node",
}
ALL_BITS = {f"{t}.{n}" for t in POA_TIERS for n in list(POA_ROUTE) + list(POA_RC2)}
