"""The reference and the probes of the cut run's and the polish's tests (cw_sw_cut_run, cw_cut_groups_device, consent_amd/csrc/cw_sw_cut.h; Engine.polish).  The
reference is plain: cuts(query, ref, W) walks the ops sw_path_probes.reference gives the pair -- the restated banded pass and walk that tests/test_sw_path_cpu.py
pins to the oracle -- and notes the query position at every window boundary by the rules of include/consent_amd.h; cut_groups(groups, W) builds the POA groups
of every (reference, window) from those pieces; polish(groups, W) joins the oracle's POA consensus over them.  tests/test_sw_cut_cpu.py holds all three to their
design.  Test infrastructure only."""
import functools
import random

import numpy as np

import pileup_probes as pl
import poa_op_probes as pop
import sw_op_probes as sp
import sw_path_probes as pp
from poa_op_probes import ont_copy, rand_seq

CUT_SLOT = 8  # CW_SW_CUT_SLOT
FILL = 0xABCDEF01  # what the tests' slots hold before a run that must not touch them


def n_windows(ref_len, W):
    return -(-ref_len // W)


def cuts(query, ref, W, ins_next=False, after_step=False):
    return list(_cuts(query, ref, W, ins_next, after_step))


@functools.lru_cache(maxsize=None)
def _cuts(query, ref, W, ins_next, after_step):
    """The T + 1 cut points of the pair.  ins_next / after_step are the two WRONG readings tests/test_sw_cut_cpu.py shows the probes to tell apart: the cut
    taken when the path arrives at the boundary, before an insertion run there (the run then falls into the next window); the cut taken after the step that
    consumes the boundary column instead of before it."""
    T = n_windows(len(ref), W)
    if not pl.counts_pair(query, ref):
        return (0,) * (T + 1)
    _, rb, re_, qb, qe, _, _ = sp.oracle(query, ref)
    out = [None] * (T + 1)
    i, j = qb, rb
    for n, c in pp.reference(query, ref)[3]:
        for _ in range(n):
            if c != pp.OP_I and j > rb and j % W == 0 and not ins_next:
                out[j // W] = i + (1 if after_step and c == pp.OP_M else 0)
            i, j = i + (c != pp.OP_D), j + (c != pp.OP_I)
            if ins_next and c != pp.OP_I and j % W == 0 and j <= re_:
                out[j // W] = i
    assert (i, j) == (qe + 1, re_ + 1), "the ops span the alignment's ends"
    for t in range(T + 1):
        if t * W <= rb:
            out[t] = qb
        elif t * W > re_:
            out[t] = qe + 1
    assert None not in out
    return tuple(out)


def pieces(query, ref, W, **wrong):
    c = cuts(query, ref, W, **wrong)
    return [query[a:b] for a, b in zip(c, c[1:])]


def check_invariants(c, row):
    """What holds for the cut points of a counted pair whatever the path is; row: (score, rb, re, qb, qe, ...)."""
    _, rb, re_, qb, qe = (int(x) for x in row[:5])
    c = [int(x) for x in c]
    assert all(a <= b for a, b in zip(c, c[1:])), "non-decreasing"
    assert c[0] == qb and c[-1] == qe + 1, "from query_begin to query_end + 1"


def spans(query, ref, c0, c1):
    """Whether the pair counts and its alignment covers columns [c0, c1)."""
    if not pl.counts_pair(query, ref):
        return False
    _, rb, re_, _, _, _, _ = sp.oracle(query, ref)
    return rb <= c0 and re_ >= c1 - 1


def cut_groups(groups, W, touching=False):
    """The output groups of cw_cut_groups_device, and grp_first: per non-empty reference and window the window's columns, then piece t of every query whose
    alignment spans the window and whose piece is not empty.  touching: the WRONG rule (every non-empty piece) the issue's first design had."""
    out, first = [], [0]
    for grp in groups:
        if grp and grp[0]:
            ref = grp[0]
            for t in range(n_windows(len(ref), W)):
                c0, c1 = t * W, min((t + 1) * W, len(ref))
                members = [pieces(q, ref, W)[t] for q in grp[1:] if touching and pl.counts_pair(q, ref) or spans(q, ref, c0, c1)]
                out.append([ref[c0:c1]] + [m for m in members if m])
        first.append(len(out))
    return out, first


def polish(groups, W, max_msa=pop.MAX_MSA, touching=False):
    """Per input group the polished reference -- the oracle's POA consensus of every window's group, joined in order -- and the windows' member counts."""
    wins, first = cut_groups(groups, W, touching)
    out = []
    for g in range(len(groups)):
        mine = wins[first[g] : first[g + 1]]
        out.append(("".join(pop.oracle_consensus(w, max_msa) for w in mine), [len(w) - 1 for w in mine]))
    return out


def edit_distance(a, b):
    """Levenshtein distance, a row at a time in numpy."""
    bb = np.frombuffer(b.encode(), np.uint8)
    ar = np.arange(len(b) + 1, dtype=np.int64)
    prev = ar.copy()
    for i, ch in enumerate(a.encode(), 1):
        cur = np.empty_like(prev)
        cur[0] = i
        cur[1:] = np.minimum(prev[:-1] + (bb != ch), prev[1:] + 1)
        prev = np.minimum.accumulate(cur - ar) + ar
    return int(prev[-1])


@functools.lru_cache(maxsize=None)
def polish_input(seed, n=1200, rate=0.10, reads=20, read_len=700):
    """(truth, [draft, reads...]): a random truth of n bases, a draft of it and `reads` noisy copies of read_len bases of it, all at `rate` ONT-mix errors."""
    rng = random.Random(seed)
    truth = rand_seq(rng, n)
    draft = ont_copy(rng, truth, rate)
    group = [draft]
    for _ in range(reads):
        a = rng.randrange(0, n - read_len + 1)
        group.append(ont_copy(rng, truth[a : a + read_len], rate))
    return truth, tuple(group)


SEED8 = dict(seed=8, n=1200, rate=0.10, reads=20, read_len=700)  # W = 100
SEED9 = dict(seed=9, n=600, rate=0.08, reads=20, read_len=350)  # W = 64: a last window shorter than W, end windows with the backbone alone
SEED7 = dict(seed=7, n=1200, rate=0.05, reads=20, read_len=700)  # W = 200: where the touching-pieces rule makes the draft worse


def run_groups():
    """(name, [reference, query], p, deletion) of the run-start probes."""
    return [(f"{'D' if d else 'I'} run at step {p}", [pl.run_start(p, d)[0]] + list(pl.run_start(p, d)[1]), p, d) for d in (False, True) for p in pl.RUN_P]


def as_group(named):
    ref, queries = named
    return [ref] + list(queries)
