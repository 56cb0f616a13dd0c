"""The reference and the probe groups of the pileup run's tests (cw_pileup_run, consent_amd/csrc/cw_pileup.h).  The reference is plain: pileup(ref, queries) walks
the ops sw_path_probes.reference gives every (query, ref) -- the restated banded pass and walk that tests/test_sw_path_cpu.py pins to the oracle -- into a numpy
[len(ref), 8] array by the rules of include/consent_amd.h.  A probe group is (reference, queries); tests/test_pileup_cpu.py holds every designed pair to its
intended ops, so that a probe that drifts fails there and not on the GPU.  Test infrastructure only."""
import functools
import random

import numpy as np

import sw_op_probes as sp
import sw_path_probes as pp
from poa_op_probes import ont_copy, rand_seq

A, C, G, T, DEL, INS, BEGIN, END, COL = range(9)  # include/consent_amd.h CW_PILE_*
PILE_SLOT, ACCUMULATE = 7, 8  # CW_SW_PILE_SLOT, CW_PILE_ACCUMULATE
FILL = 0xFFFFFFFF  # what the tests' counts hold before a run that must not touch them


def code(c):
    """A base as packed: every letter other than A, C, G is T."""
    return "ACG".find(c) if c in "ACG" else T


def counts_pair(query, ref):
    """Whether the pair contributes: cw_sw_path_run would report it ALIGNED with a positive score."""
    return pp.reference(query, ref)[0] == pp.ALIGNED and sp.oracle(query, ref)[0] > 0


def add_path(out, ops, query, rb, qb, ins_after=False, ins_bases=False):
    """One path's counts.  ins_after / ins_bases are the two WRONG readings of an insertion tests/test_pileup_cpu.py shows the probes to tell apart: the column
    after the run instead of the one before it; the inserted bases instead of the run."""
    i, j = qb, rb
    for n, c in ops:
        if c == pp.OP_M:
            for t in range(n):
                out[j + t, code(query[i + t])] += 1
            i, j = i + n, j + n
        elif c == pp.OP_D:
            out[j : j + n, DEL] += 1
            j += n
        else:
            assert c == pp.OP_I and j > rb, "a path does not begin with an insertion"
            col = j if ins_after else j - 1
            if col < len(out):
                out[col, INS] += n if ins_bases else 1
            i += n
    out[rb, BEGIN] += 1
    out[j - 1, END] += 1
    return i, j


def pileup(ref, queries, **wrong):
    """The [len(ref), 8] counts of the queries' alignments on ref."""
    out = np.zeros((len(ref), COL), np.uint32)
    for q in queries:
        if not counts_pair(q, ref):
            continue
        _, rb, re_, qb, qe, _, _ = sp.oracle(q, ref)
        i, j = add_path(out, pp.reference(q, ref)[3], q, rb, qb, **wrong)
        assert (i, j) == (qe + 1, re_ + 1), "the ops span the alignment's ends"
    return out


def coverage(counts):
    return counts[:, : DEL + 1].sum(axis=1, dtype=np.int64)


def check_invariants(counts, rows):
    """What holds for the counts of one reference whatever the paths are; rows: the (score, rb, re, qb, qe, ins, del) of the pairs that counted."""
    n = len(counts)
    cov = np.zeros(n + 1, np.int64)
    for _, rb, re_, _, _, _, _ in rows:
        cov[rb] += 1
        cov[re_ + 1] -= 1
    cov = np.cumsum(cov)[:n]
    assert np.array_equal(coverage(counts), cov), "A + C + G + T + DEL is the number of counted rows that cover the column"
    begins, ends = np.cumsum(counts[:, BEGIN].astype(np.int64)), np.cumsum(counts[:, END].astype(np.int64))
    assert np.array_equal(cov, begins - np.concatenate([[0], ends[:-1]])), "coverage is prefix(BEGIN) - prefix(END before the column)"
    assert int(counts[:, DEL].sum()) == sum(r[6] for r in rows)
    assert int(counts[:, : T + 1].sum()) == sum(r[4] - r[3] + 1 - r[5] for r in rows)
    assert int(counts[:, BEGIN].sum()) == int(counts[:, END].sum()) == len(rows)
    assert int(counts[:, INS].sum()) <= sum(r[5] for r in rows) and (counts[:, INS] <= cov).all()  # events, not bases; at most one a path and column


# ---- the probe groups: name -> (reference, [queries]) -----------------------------------------------------------------------------------------------------

ROUND_LENS = (1, 2, 63, 64, 65, 128, 129)  # pure-M paths on both sides of a round of 64 steps, and of two


@functools.lru_cache(maxsize=None)
def round_edges():
    """Exact copies of ROUND_LENS bases of a 600-base reference (sw_op_probes.embedded's): each a path of that many M steps."""
    ref = sp.embedded(1, 129, 600)[1]
    return ref, tuple(ref[200 + 3 * k : 200 + 3 * k + n] for k, n in enumerate(ROUND_LENS))


RUN_P, RUN_G, RUN_S = (62, 63, 64, 65), 3, 80


@functools.lru_cache(maxsize=None)
def run_start(p, deletion, seed=0x9117):
    """Query P + G + S against flank + P + S + flank (deletion: the three bases G in the reference instead): the run's first step is step p of the path --
    the last steps of round 0 for p = 62, 63, the first of round 1 for p = 64.  The bases around the run are chosen so that no co-optimal path moves it: G's
    ends differ from the bases a shifted run would swap them with."""
    rng = random.Random(seed + 8 * p + deletion)
    P, S = rand_seq(rng, p), rand_seq(rng, RUN_S)
    Gs = rng.choice("ACGT".replace(P[-1], "").replace(S[0], "")) + rng.choice("ACGT") + rng.choice("ACGT".replace(P[-1], "").replace(S[0], ""))
    fl, fr = rand_seq(rng, 40), rand_seq(rng, 40)
    if deletion:
        return fl + P + Gs + S + fr, (P + S,)
    return fl + P + S + fr, (P + Gs + S,)


def run_ops(p, deletion):
    return ((p, pp.OP_M), (RUN_G, pp.OP_D if deletion else pp.OP_I), (RUN_S, pp.OP_M))


CLASS_LENS = (600, 700, 2048, 2100)  # launch class 0, 1, 1 (its last length), 2


@functools.lru_cache(maxsize=None)
def classes(seed=0xC1A5):
    """One 3 000-base reference -- beyond LDS: the wave's global reference buffer -- and a query of every launch class cut from it with a few errors, on
    overlapping columns."""
    rng = random.Random(seed)
    ref = rand_seq(rng, 3000)
    out = []
    for k, n in enumerate(CLASS_LENS):
        a = 100 + 150 * k
        out.append(ont_copy(rng, ref[a : a + n + n // 8], 0.02)[:n])
        assert len(out[-1]) == n
    return ref, tuple(out)


@functools.lru_cache(maxsize=None)
def deep(n=300, seed=0xDEE9):
    """One 600-base reference and n noisy 500-base copies at 12 % errors: many waves add to one column set."""
    rng = random.Random(seed)
    ref = rand_seq(rng, 600)
    out = []
    for _ in range(n):
        a = rng.randrange(0, 60)
        out.append(ont_copy(rng, ref[a : a + 540], 0.12)[:500])
        assert len(out[-1]) == 500
    return ref, tuple(out)


@functools.lru_cache(maxsize=None)
def nothing_counts():
    """Pairs that count nothing beside pairs that count, as groups (reference first): the NO_PATH probe, an empty query and an aligned query on one reference;
    a query nothing of which aligns beside an aligned one on another (a reference that holds all four letters aligns a base of any query, so that pair needs
    a reference of its own: poly-C); a reference alone; a group of none."""
    wide_q, wide_r = pp.planted_wide()
    lone = rand_seq(random.Random(0x10E), 90)
    return ([wide_r, wide_q, "", wide_r[1000:1300]], ["C" * 500, "A" * 300, "C" * 40, ""], [lone], [])


def designed_groups():
    """The groups whose every pair is compared with the reference, word for word."""
    out = {"round edges": round_edges()}
    for p in RUN_P:
        out[f"I run at step {p}"] = run_start(p, False)
        out[f"D run at step {p}"] = run_start(p, True)
    out["classes"] = classes()
    out["deep"] = deep()
    return out


def small_groups():
    """designed_groups without the deep one: for the tests that run a group several ways."""
    return {k: v for k, v in designed_groups().items() if k != "deep"}


CROWDS = sp.CROWDS
