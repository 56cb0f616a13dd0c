"""The plain reference and the probes of the span runs (include/consent_amd.h cw_sw_span_run, cw_sw_path_span_run, cw_pileup_span_run, cw_sw_cut_span_run,
cw_seed_spans; consent_amd/csrc/cw_sw_op.h sw_unpack_from).  span_expected(query, ref, lo, hi) is built from the plain references the four runs already have
-- sw_op_probes.oracle, sw_path_probes.reference, pileup_probes.pileup, the cut rule of sw_cut_probes -- on ref[lo:hi], shifted by lo; seed_spans is
cw_seed_spans' rule in Python integers.  Test infrastructure only."""
import functools
import random

import numpy as np

import pileup_probes as pl
import seed_probes as sdp
import sw_cut_probes as cp
import sw_op_probes as sp
import sw_path_probes as pp
from poa_op_probes import ont_copy, rand_seq

STOP = 2  # CW_SW_STOP
PAD, PAD_SHIFTS = 64, (4, 3, 2)  # CW_SPAN_PAD and the candidates for CW_SPAN_PAD_SHIFT, smallest pad first
INT32_MAX = (1 << 31) - 1


def clamp_span(lo, hi, n):
    lo, hi = min(lo, n), min(hi, n)
    return (lo, hi) if hi > lo else (0, 0)


class Expected:
    """What the four span runs owe one pair: .row (the path run's eight numbers), .plain_row (cw_sw_span_run's under CW_SW_WANT_INDELS), .ops / .ops_eqx,
    .counts ([len(ref), 8], absolute columns), and .cuts(W)."""

    def __init__(self, query, ref, lo, hi):
        n = len(ref)
        self.query, self.n = query, n
        self.lo, self.hi = clamp_span(lo, hi, n)
        self.sub = ref[self.lo : self.hi]
        self.counts = np.zeros((n, pl.COL), np.uint32)
        self.ops, self.ops_eqx = (), ()
        self.counted = False
        if len(query) > sp.QMAX or len(self.sub) > sp.RMAX or n > INT32_MAX:
            self.row = self.plain_row = (0, 0, -1, 0, -1, 0, 0, STOP)
            return
        if not self.sub or not query:
            self.row = self.plain_row = (0, 0, -1, 0, -1, 0, 0, pp.ALIGNED)
            return
        seven = sp.oracle(query, self.sub)
        shift = self.lo if seven[0] > 0 else 0
        five = (seven[0], seven[1] + shift, seven[2] + shift, seven[3], seven[4])
        status, ins, dele, ops, ops_x, _ = pp.reference(query, self.sub)
        self.row = five + (ins, dele, status)
        st = sp.expected_status(query, self.sub)
        self.plain_row = five + ((seven[5], seven[6]) if st == sp.ALIGNED else (0, 0)) + (st,)
        self.ops, self.ops_eqx = ops, ops_x
        self.counted = pl.counts_pair(query, self.sub)
        if self.counted:
            self.counts[self.lo : self.hi] = pl.pileup(self.sub, [query])

    def cuts(self, W):
        """The T + 1 words on the WHOLE reference: sw_cut_probes' rule with the absolute ends and columns."""
        T = cp.n_windows(self.n, W)
        if not self.counted:
            return [0] * (T + 1)
        _, rb, re_, qb, qe = self.row[:5]
        out = [None] * (T + 1)
        i, j = qb, rb
        for k, c in self.ops:
            for _ in range(k):
                if c != pp.OP_I and j > rb and j % W == 0:
                    out[j // W] = i
                i, j = i + (c != pp.OP_D), j + (c != pp.OP_I)
        assert (i, j) == (qe + 1, re_ + 1)
        for t in range(T + 1):
            if t * W <= rb:
                out[t] = qb
            elif t * W > re_:
                out[t] = qe + 1
        assert None not in out
        return out


@functools.lru_cache(maxsize=None)
def span_expected(query, ref, lo, hi):
    return Expected(query, ref, lo, hi)


def seed_spans(seq_len, ref_len, row, min_hits, pad=PAD, pad_shift=4):
    """cw_seed_spans' rule for one sequence: row is (STATUS, HITS, DIAG, OTHER)."""
    m, n = int(seq_len), int(ref_len)
    status, hits, diag = int(row[0]), int(row[1]), int(row[2])
    if status not in (sdp.FWD, sdp.REV) or hits < min_hits:
        return 0, 0
    P = pad + (m >> pad_shift)
    clamp = lambda v: max(0, min(n, v))
    return clamp(diag - P), clamp(diag + sdp.SPAN + m + P)


# the rows cw_seed_spans is held to, here and on the GPU
SEED_CASES = [  # (m, n, (STATUS, HITS, DIAG, OTHER), min_hits, pad, pad_shift)
    (500, 3000, (sdp.FWD, 100, 1000, 3), 14, 64, 4),
    (500, 3000, (sdp.REV, 100, -300, 3), 14, 64, 4),      # a negative DIAG: the read overhangs the start
    (500, 3000, (sdp.FWD, 100, -2000, 3), 14, 64, 4),     # so far off that hi clamps at 0 too
    (500, 3000, (sdp.FWD, 100, 2800, 3), 14, 64, 4),      # DIAG + ... > n
    (500, 3000, (sdp.FWD, 100, 5000, 3), 14, 64, 4),      # lo > n
    (500, 3000, (sdp.FWD, 13, 1000, 3), 14, 64, 4),       # min_hits - 1
    (500, 3000, (sdp.FWD, 14, 1000, 3), 14, 64, 4),       # min_hits
    (3000, 3000, (sdp.IS_REF, 0, 0, 0), 14, 64, 4),
    (5, 3000, (sdp.NONE, 0, 0, 0), 0, 64, 4),
    (32768, 16383, (sdp.FWD, 999, -100, 0), 14, 64, 31),  # pad_shift = 31: m >> 31 = 0
    (32768, 16383, (sdp.FWD, 999, 100, 0), 14, 0xFFFFFFFF, 0),  # a pad beyond 32 bits of sum: 64-bit arithmetic
    (700, 2 ** 31 - 1, (sdp.REV, 50, 2 ** 31 - 900, 0), 14, 64, 4),
]


# ---- the pad: planted reads and where their seeds place them -----------------------------------------------------------------------------------------------------

# (draft_and_reads arguments, tile): seed_probes.CONTIG as Engine.polish(seeded=True) sees it (one tile) and as polish_reads(tile=1000 or 1100) places it, and the planted
# reads of tests/test_seed_cpu.py (300 to 5 000 bases at 10 - 12 %) under Engine.place's default tile
PAD_INPUTS = ((sdp.CONTIG, 8192), (sdp.CONTIG, 1000), (sdp.CONTIG, 1100),
              (dict(seed=0x5D20, n=1200, reads=12, lo=300, hi=700), 8192), (dict(seed=0x5D20, n=6000, reads=12, lo=300, hi=5000), 8192),
              (dict(seed=0x5D20, n=16000, reads=10, lo=1000, hi=5000), 8192))


@functools.lru_cache(maxsize=None)
def placed_reads(i):
    """Per placed read of PAD_INPUTS[i]: (the read oriented as placed, its draft, its position)."""
    spec, tile = PAD_INPUTS[i]
    draft, reads, _, _ = sdp.draft_and_reads(**spec)
    out = []
    for q, p in zip(reads, sdp.place(draft, list(reads), tile, 0)):
        if p is not None:
            out.append((sdp.revcomp(q) if p[0] == sdp.REV else q, draft, p[1]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pad_mismatches(pad_shift):
    """(reads, those whose spanned alignment differs from the unspanned one) over all PAD_INPUTS.  Compared are the oracle's seven numbers with lo added back.
    Equal numbers make the path equal too: sw_path_probes.reference is a function of the aligned slices ref[rb : re + 1], query[qb : qe + 1] and the score."""
    total, bad = 0, []
    for i in range(len(PAD_INPUTS)):
        for r, (q, draft, pos) in enumerate(placed_reads(i)):
            lo, hi = seed_spans(len(q), len(draft), (sdp.FWD, 1 << 20, pos, 0), 0, PAD, pad_shift)
            full = sp.oracle(q, draft)
            part = sp.oracle(q, draft[lo:hi])
            part = (part[0], part[1] + lo, part[2] + lo) + part[3:] if part[0] > 0 else part
            total += 1
            if part != full:
                bad.append((i, r))
    return total, tuple(bad)


# ---- the GPU probes ----------------------------------------------------------------------------------------------------------------------------------------------

QUERY_LENS = (100, 700, 2100)  # one per launch class
REF_LENS = (600, 2049, 16401)  # the last beyond CW_SW_RMAX: valid only under the span entry points; none a multiple of 16: each ends in a partial word
ALIGNED_LO = 400  # a span that begins on a window boundary of the GPU test's cut run (W = 100): its cut words are the sliced reference's, moved


@functools.lru_cache(maxsize=None)
def ref_of(n, seed=0x59A9):
    return rand_seq(random.Random(seed + n), n)


@functools.lru_cache(maxsize=None)
def query_on(n, m, at, seed=0):
    """A query of exactly m bases: a noisy copy of a stretch of ref_of(n) that begins near column `at`, between short random flanks."""
    rng = random.Random(0x9E7 + 7919 * n + 31 * m + at + seed)
    ref = ref_of(n)
    span = max(1, min(n - at, m * 4 // 5))
    core = ont_copy(rng, ref[at : at + span], 0.10)[: max(1, m * 9 // 10)] or ref[at]
    left = (m - len(core)) // 2
    q = rand_seq(rng, left) + core + rand_seq(rng, m - len(core) - left)
    assert len(q) == m
    return q


def identity_cases():
    """(name, query, ref, lo, hi): every query class on every reference length with lo % 16 and hi % 16 in {0, 1, 15}; hi = n with n % 16 != 0; span lengths
    2 048 and 2 049 (the LDS / global switch) and 16 383 (the capacity)."""
    out = []
    for n in REF_LENS:
        for qi, m in enumerate(QUERY_LENS):
            base = (n // 3) & ~15
            length = min(n - base - 16, max(320, m + 160)) & ~15
            for lo_r in (0, 1, 15):
                for hi_r in (0, 1, 15):
                    lo, hi = base + lo_r, base + length + hi_r
                    if (lo_r, hi_r) in ((0, 0), (1, 15), (15, 1)) or (n == 600 and m == 100):  # the full cross on the smallest, a diagonal of it elsewhere
                        out.append((f"n{n} m{m} lo%16={lo_r} hi%16={hi_r}", query_on(n, m, base + 20, qi), ref_of(n), lo, hi))
            out.append((f"n{n} m{m} hi=n", query_on(n, m, max(0, n - m - 40), 7), ref_of(n), max(0, n - m - 203), n))
    for qi, m in enumerate(QUERY_LENS):  # spans from a window boundary: the cut words compare with the cut run on the slice
        out.append((f"n2049 m{m} lo on a boundary", query_on(2049, m, ALIGNED_LO + 30, 20 + qi), ref_of(2049), ALIGNED_LO, ALIGNED_LO + max(320, m + 160) + 7))
    n = REF_LENS[-1]
    for length in (2048, 2049, 16383):
        for m in (100, 700):
            lo = 7
            out.append((f"n{n} m{m} span {length}", query_on(n, m, lo + length - m - 30, 11), ref_of(n), lo, lo + length))
    return out
