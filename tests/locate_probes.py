"""The plain reference of the locate run (include/consent_amd.h cw_locate_run_device) and of Engine.locate / Engine.polish_reads(index=True), and the probes the
GPU tests run: Python strings, Counter and dict only -- no GPU, no oracle.  The row is seed_probes.seed_of's with the reference allowed any length."""
import functools
import random

import seed_probes as sd
import strand_probes as st
from poa_op_probes import rand_seq
from seed_probes import DIAG, FWD, HITS, NONE, OTHER, REV, ROW, SHIFT, SPAN, STATUS, revcomp  # noqa: F401

K_DEFAULT = 15  # CW_LOCATE_K
RMAX = (1 << 28) - 1  # CW_LOCATE_RMAX
MIN_HITS = 4  # Engine.locate's default: twice the chance level test_locate_cpu.py measures at k = 15
LDS_SLOTS = 4096  # cw_locate.h CW_LOC_SLOTS: the sparse table of the LDS route,
LDS_CAP = LDS_SLOTS // 2  # and the distinct (orientation, bin) pairs it takes: a read with more goes the dense route


def locate_of(q, ref, k):
    """(STATUS, HITS, DIAG, OTHER) of a read on a reference of any length: seed_of's four lines without its capacity."""
    if not (k <= len(q) <= st.QMAX and k <= len(ref) <= RMAX):
        return NONE, 0, 0, 0
    best = [max((w, -b) for b, w in enumerate(ws)) for ws in sd.windows(q, ref, k)]
    o = REV if best[REV][0] > best[FWD][0] else FWD
    return o, best[o][0], (-best[o][1] << SHIFT) - len(q), best[1 - o][0]


def expected(ref, reads, k):
    """Per read, in order: its row.  There is no reference row."""
    return [locate_of(q, ref, k or K_DEFAULT) for q in reads]


def distinct_pairs(q, ref, k):
    """The distinct (orientation, bin) pairs the read's hits fall into: what its sparse histogram has to hold."""
    pos, m = sd.unique_positions(ref, k), len(q)
    return len({(o, (pos[qo[i : i + k]] - i + m) >> SHIFT) for o, qo in enumerate((q, revcomp(q))) for i in range(m - k + 1) if qo[i : i + k] in pos})


def locate(reference, reads, k, min_hits=MIN_HITS):
    """Per read (strand, position, hits, other) -- position is DIAG on the whole reference -- or None below min_hits or without a vote."""
    out = []
    for q in reads:
        row = locate_of(q, reference, k or K_DEFAULT)
        out.append((row[STATUS], row[DIAG], row[HITS], row[OTHER]) if row[STATUS] in (FWD, REV) and row[HITS] >= min_hits else None)
    return out


def polish_groups(reference, reads, tile, k, min_hits=MIN_HITS):
    """seed_probes.polish_groups with the placements of locate(): per tile the tile and, in the order of the reads, every placed read -- turned when REV -- whose
    footprint [position, position + m + SPAN) meets the tile."""
    placed = locate(reference, reads, k, min_hits)
    groups = []
    for a, t in sd.tiles_of(reference, tile):
        grp = [t]
        for q, p in zip(reads, placed):
            if p is not None and p[1] < a + len(t) and p[1] + len(q) + SPAN > a:
                grp.append(revcomp(q) if p[0] == REV else q)
        groups.append(grp)
    return groups


def seeded_group(reference, reads, k, min_hits=MIN_HITS):
    """What Engine.polish_reads(index=True, seeded=True) hands to Engine.polish: ONE group, the contig and the placed reads, oriented, and per sequence the
    span of cw_seed_spans' rule about its position (the reference's own entry is not read)."""
    placed = locate(reference, reads, k, min_hits)
    group, spans, n = [reference], [(0, 0)], len(reference)
    for q, p in zip(reads, placed):
        if p is None:
            continue
        m = len(q)
        pad = 64 + (m >> 4)  # CW_SPAN_PAD + (m >> CW_SPAN_PAD_SHIFT)
        group.append(revcomp(q) if p[0] == REV else q)
        spans.append((min(max(p[1] - pad, 0), n), min(max(p[1] + SPAN + m + pad, 0), n)))
    return group, spans


# ---- the probes ------------------------------------------------------------------------------------------------------------------------------------------------------

DRAFT = (0x10CA7E, 70000, 24, 300, 5000)  # seed_probes.draft_and_reads: a reference beyond CW_SW_RMAX, 65 535 and 1 023 bins


@functools.lru_cache(maxsize=None)
def far_reads(k):
    """(draft, reads, names) past every 16-bit and 10-bit field: the draft of DRAFT with a 60-base stretch copied 40 000 bases on and a 60-base
    reverse-complement palindrome planted; its planted and unrelated reads; exact slices whose d + m is 65 535, 65 536, 65 599 and 65 600 and whose position
    is 65 535 and 65 536; reads that overhang both ends; a read of the twice-present stretch; the palindrome."""
    draft, reads, _, other = sd.draft_and_reads(*DRAFT)
    rng = random.Random(0xFA2 + k)
    half = rand_seq(rng, 30)
    pal = half + revcomp(half)
    draft = draft[:30000] + pal + draft[30060:]
    draft = draft[:50000] + draft[10000:10060] + draft[50060:]
    m = 200
    out = list(reads) + list(other)
    names = ["planted"] * len(reads) + ["unrelated"] * len(other)
    for s in (65535, 65536, 65599, 65600):  # d + m = s for an exact slice at d = s - m
        out.append(draft[s - m : s])
        names.append(f"d + m = {s}")
    for a in (65535, 65536):
        out.append(draft[a : a + m])
        names.append(f"position {a}")
    out += [rand_seq(rng, 30) + draft[:50], draft[-50:] + rand_seq(rng, 30), revcomp(rand_seq(rng, 30) + draft[:50]), revcomp(draft[-50:] + rand_seq(rng, 30))]
    names += ["over the start", "over the end", "over the start, turned", "over the end, turned"]
    out.append(draft[10000:10060])
    names.append("present twice")
    out.append(pal)
    names.append("its own reverse complement")
    return draft, tuple(out), tuple(names)


DENSE = dict(seed=0xDE45E, n=1000000, m=16000, k=11)  # a random read of m bases on a random reference of n: more distinct pairs than LDS_CAP


@functools.lru_cache(maxsize=None)
def dense_reads():
    """(reference, reads): a random reference of 1 000 000 bases; a random read of 16 000 bases, whose chance hits at k = 11 fall into more than LDS_CAP
    distinct pairs; a planted one of 16 000 bases, turned; a few short reads, planted and random."""
    rng = random.Random(DENSE["seed"])
    ref = rand_seq(rng, DENSE["n"])
    m = DENSE["m"]
    reads = [rand_seq(rng, m), revcomp(sd.ont_copy(rng, ref[600000 : 600000 + m], 0.11)), ref[999800:], rand_seq(rng, 300), sd.ont_copy(rng, ref[123456:124456], 0.1), rand_seq(rng, 10)]
    return ref, tuple(reads)


CONTIG = dict(seed=0x10C0471, n=20000, reads=40, lo=300, hi=700)  # Engine.polish_reads(index=True)
