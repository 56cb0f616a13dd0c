"""Pairs for the tests of the alignment operator (cw_sw_run, consent_amd/csrc/cw_sw_op.h): noisy copies of a slice of a reference between unrelated flanks, the
edges of every sweep instance, ties, pairs that do not align, planted indels for the banded traceback -- and the oracle's seven numbers of every pair
(oracle/cw_oracle_c.cpp cwo_ssw), computed once.  Test infrastructure only."""
import ctypes as C
import functools
import random

import numpy as np

import oracle_lib
from poa_op_probes import ont_copy, rand_seq

PRM = (9, 4, 8, 2, 150)  # (not read by the operator)
QMAX, RMAX, LDS_RMAX = 32768, 16383, 2048  # include/consent_amd.h CW_SW_QMAX, CW_SW_RMAX; csrc/cw_stitch.h CW_ST_RMAX: the longest reference kept in LDS
MATCH, MISMATCH, GAP_OPEN, GAP_EXT = 2, 2, 3, 1  # include/cw_policy.h CW_SSW_*

# every sweep instance of st_sweep_any's ladder (1, 2, 3, 4, 5, 6, 8, 12, 16 registers a slot: up to 128, 256, 384, 512, 640, 768, 1024, 1536, 2048 positions)
# and both sides of each edge
QUERY_LENS = [1, 2, 127, 128, 129, 256, 257, 384, 385, 512, 513, 640, 641, 768, 769, 1024, 1025, 1536, 1537, 2048]
REF_LENS = [1, 63, 64, 65, 600, 2048, 2049, 6000]  # 2049: the first beyond LDS
LONG_QUERY_LENS = [2049, 2500, 9000]


@functools.lru_cache(maxsize=None)
def oracle(query, ref):
    """cwo::ssw_align(query, ref): (score, ref_begin, ref_end, query_begin, query_end, ins, del)."""
    out = np.zeros(7, np.int32)
    oracle_lib.oracle().cwo_ssw(query.encode(), len(query), ref.encode(), len(ref), C.c_void_p(out.ctypes.data))
    return tuple(int(x) for x in out)


@functools.lru_cache(maxsize=None)
def embedded(seed, qlen, rlen, rate=0.12):
    """(query, reference): the reference is random; the query, of exactly qlen bases, is a noisy copy of a slice from the middle of the reference between two
    unrelated random flanks, so that the alignment begins and ends inside both (most of the time: tests/test_sw_op_cpu.py counts)."""
    rng = random.Random(seed * 1000003 + qlen * 131 + rlen)
    ref = rand_seq(rng, rlen)
    span = max(1, min(rlen, qlen) * 3 // 5)
    r0 = (rlen - span) // 2
    core = ont_copy(rng, ref[r0 : r0 + span], rate)[: max(1, qlen * 4 // 5)] or ref[r0]
    left = (qlen - len(core)) // 2
    query = rand_seq(rng, left) + core + rand_seq(rng, qlen - len(core) - left)
    assert len(query) == qlen and len(ref) == rlen
    return query, ref


def instance_pairs():
    """name -> (query, reference): every query length against a 600-base reference, every reference length against a 200-base and a 700-base query
    (the 128-register and the wide kernel)."""
    out = {f"q{m}xr600": embedded(1, m, 600) for m in QUERY_LENS}
    for n in REF_LENS:
        out[f"q200xr{n}"] = embedded(2, 200, n)
        out[f"q700xr{n}"] = embedded(3, 700, n)
    return out


def long_pairs():
    return {f"q{m}xr2048": embedded(4, m, 2048) for m in LONG_QUERY_LENS}


def tie_pairs():
    rng = random.Random(0x71E5)
    q = rand_seq(rng, 40)
    twice = rand_seq(rng, 100) + q + rand_seq(rng, 77) + q + rand_seq(rng, 90)  # the first end wins
    # the best score of a column reached at two query positions: the query holds the reference's only letters twice, far apart
    unit = "ACGTTGCA"
    two_rows = ("T" * 20 + unit + "T" * 20 + unit + "T" * 20, "GGGG" + unit + "GGGG")
    return {"query twice in the reference": (q, twice), "two query positions in one column": two_rows, "periodic reference": ("ACGT" * 3 + "AC", "ACGT" * 100)}


def nothing_pairs():
    return {"poly-A against poly-C": ("A" * 300, "C" * 500), "empty query": ("", rand_seq(random.Random(1), 80)), "empty reference": (rand_seq(random.Random(2), 80), "")}


@functools.lru_cache(maxsize=None)
def planted(g, seed=0x1DE1):
    """reference = P + G1 + M + S, query = P + M + G2 + S: random 500-base P, M, S and unrelated random G1, G2 of g bases each.  The aligned spans have equal
    length, so the traceback's band starts at 1 and has to double until it holds a diagonal offset of g."""
    rng = random.Random(seed + g)
    P, M, S, G1, G2 = (rand_seq(rng, n) for n in (500, 500, 500, g, g))
    return P + M + G2 + S, P + G1 + M + S


@functools.lru_cache(maxsize=None)
def unbalanced(seed=0x0BA1):
    """One deletion of 7 reference bases: the spans differ by 7 and the band starts at 8."""
    rng = random.Random(seed)
    P, S, D = rand_seq(rng, 300), rand_seq(rng, 300), rand_seq(rng, 7)
    return P + S, rand_seq(rng, 40) + P + D + S + rand_seq(rng, 40)


DIR_BYTES = 1 << 20  # include/consent_amd.h CW_SW_DIR_BYTES
ALIGNED, NO_INDELS = 0, 1  # CW_SW_ALIGNED, CW_SW_NO_INDELS


def dir_fits(ref_span, query_span, band):
    """The scratch rule as include/consent_amd.h states it: direction bytes of a band, and the three rows once they outgrow 4096 bytes."""
    dirs = 3 * min(2 * band + 1, ref_span + 1) * query_span
    rows = 12 * min(2 * band + 3, ref_span + 3)
    return dirs + (0 if rows <= 4096 else (rows + 15) // 16 * 16) <= DIR_BYTES


def banded_best(ref, read, band):
    """The best score of ssw's banded pass (oracle/cw_oracle.cpp ssw_banded_indels, one band) over code arrays: its rows h_b / e_b / h_c with their index
    rules and zeroed edge cells, a row at a time in numpy -- the in-row gap as an exclusive prefix maximum, exact because open >= ext and no cell is
    negative."""
    ref_len, read_len = len(ref), len(read)
    width = 2 * band + 3
    h_b, e_b = np.zeros(width, np.int64), np.zeros(width, np.int64)
    best = 0
    for i in range(read_len):
        beg, end = max(0, i - band), min(ref_len - 1, i + band)
        if end < beg:
            continue
        edge = min(end + 1, width - 1)
        h_b[0] = e_b[0] = h_b[edge] = e_b[edge] = 0
        xp = max(i - 1 - band, 0)
        t = np.arange(end - beg + 1)
        e_i = beg + t - xp + 1
        if i == 0:
            e_new = np.full(len(t), -GAP_EXT, np.int64)
        else:
            e_new = np.maximum(h_b[e_i] - GAP_OPEN, e_b[e_i] - GAP_EXT)
        e1 = np.maximum(e_new, 0)
        diag = h_b[e_i - 1] + np.where(ref[beg : end + 1] == read[i], MATCH, -MISMATCH)
        hq = np.maximum(e1, diag)
        inc = np.maximum.accumulate(hq - GAP_OPEN + (t + 1) * GAP_EXT)
        ex = np.concatenate([[-(1 << 40)], inc[:-1]])
        f = np.maximum(ex, -GAP_EXT) - t * GAP_EXT
        hc = np.maximum(np.maximum(e1, np.maximum(f, 0)), diag)
        e_b[1 : len(t) + 1] = e_new
        h_b[1 : len(t) + 1] = hc
        best = max(best, int(hc.max()))
    return best


@functools.lru_cache(maxsize=None)
def expected_status(query, ref):
    """The status of the pair's row under CW_SW_WANT_INDELS by the header's rule: the band starts at |reference span - query span| + 1 and doubles until the
    banded score reaches the alignment's (or the band passes both spans together); the first band that does not fit the wave's scratch is NO_INDELS."""
    score, rb, re, qb, qe, _, _ = oracle(query, ref)
    if score <= 0:
        return ALIGNED
    r_span, q_span = re - rb + 1, qe - qb + 1
    band = abs(r_span - q_span) + 1
    if not dir_fits(r_span, q_span, band):
        return NO_INDELS
    if dir_fits(r_span, q_span, 2 * (r_span + q_span) + 2):  # whatever band it takes
        return ALIGNED
    code = {c: k for k, c in enumerate("ACGT")}
    r = np.array([code[c] for c in ref[rb : re + 1]], np.int64)
    q = np.array([code[c] for c in query[qb : qe + 1]], np.int64)
    while True:
        if not dir_fits(r_span, q_span, band):
            return NO_INDELS
        if banded_best(r, q, band) >= score or band > r_span + q_span:
            return ALIGNED
        band *= 2


def final_band(span_diff, offset):
    """The band the traceback ends with when the alignment needs a diagonal offset of `offset`: it starts at span_diff + 1 and doubles."""
    b = span_diff + 1
    while b < offset:
        b *= 2
    return b


def bands_tried(span_diff, offset):
    b, out = span_diff + 1, []
    while True:
        out.append(b)
        if b >= offset:
            return out
        b *= 2


def mixed_pairs(n=300, seed=0xC0DE):
    """n pairs of mixed shapes: mostly short queries, some of every register class, references on both sides of the LDS limit."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        x = rng.random()
        m = rng.randrange(1, 130) if x < 0.5 else rng.randrange(130, 641) if x < 0.85 else rng.randrange(641, 1300) if x < 0.97 else rng.randrange(1300, 2049)
        r = rng.choice([150, 600, 600, 600, 900, 2048, 2100]) if x < 0.97 else 600
        out.append(embedded(100 + i, m, r))
    return out


@functools.lru_cache(maxsize=None)
def crowd(n_groups, per_group, q_lo, q_hi, r_lo, r_hi, seed):
    """Groups of one random reference (r_lo .. r_hi bases) and per_group queries (q_lo .. q_hi bases) each: a noisy copy of a stretch of the reference between
    random flanks, cut or padded to its length.  For batches of more pairs than a launch has waves: a wave then takes a second pair and a third."""
    rng = random.Random(seed)
    groups = []
    for _ in range(n_groups):
        ref = rand_seq(rng, rng.randrange(r_lo, r_hi + 1))
        grp = [ref]
        for _ in range(per_group):
            m = rng.randrange(q_lo, q_hi + 1)
            span = max(1, min(len(ref), m) * 3 // 5)
            a = rng.randrange(0, len(ref) - span + 1)
            core = ont_copy(rng, ref[a : a + span])[: max(1, m * 4 // 5)] or ref[a]
            left = (m - len(core)) // 2
            grp.append(rand_seq(rng, left) + core + rand_seq(rng, m - len(core) - left))
        groups.append(tuple(grp))
    return tuple(groups)


def waves_of(n_seqs, cls, indels, cus):
    """Waves of the launch of query class `cls` (0: up to 640 bases, 1: up to 2 048, 2: beyond) for a batch of n_seqs sequences on `cus` compute units:
    csrc/cw_plan.h plan_sw, which tests/test_sw_op_cpu.py pins through cw_debug_sw_plan."""
    if cls == 2:
        return min(n_seqs, 256)
    by_seqs = (n_seqs + 3) // 4
    most = cus * 4 if cls == 0 else cus
    if indels:
        most = min(most, 256)
    return 4 * max(1, min(by_seqs, most))


# (groups, members, query lengths, reference lengths, seed) per launch class: each has more pairs than its launch has waves on a device of up to 304 compute
# units, with and without the indel totals
CROWDS = {0: (260, 20, 10, 60, 100, 150, 0xC0), 1: (1, 1300, 641, 700, 120, 150, 0xC1), 2: (1, 300, 2049, 2100, 80, 100, 0xC2)}
