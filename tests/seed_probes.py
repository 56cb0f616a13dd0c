"""The plain reference of the seed run (include/consent_amd.h cw_seed_run) and of Engine.place / Engine.polish_reads, and the probe catalogue the GPU tests
run: Python strings, Counter and dict only -- no GPU, no oracle.  A k-mer here is a substring; N is T, as the packing has it."""
import functools
import random
from collections import Counter

import strand_probes as st
from poa_op_probes import ont_copy, rand_seq
from strand_probes import FWD, IS_REF, KS, NONE, REV, revcomp  # noqa: F401

SHIFT = 6  # CW_SEED_SHIFT: a bin is 64 diagonals, a window two neighbouring bins
STATUS, HITS, DIAG, OTHER, ROW = 0, 1, 2, 3, 4  # CW_SEED_*
SPAN = 2 << SHIFT  # the diagonals of a window
MIN_HITS = 14  # Engine.place's default: twice the chance level test_seed_cpu.py measures at k = 11


@functools.lru_cache(maxsize=64)
def unique_positions(ref, k):
    """U with P: the k-mers that occur at exactly one position of ref, and that position."""
    count = Counter(ref[j : j + k] for j in range(len(ref) - k + 1))
    return {ref[j : j + k]: j for j in range(len(ref) - k + 1) if count[ref[j : j + k]] == 1}


def windows(q, ref, k):
    """Per orientation the window scores w[0 .. B): positions of q (as given, reverse-complemented) whose k-mer is in U, counted by the bin of their diagonal."""
    pos, n, m = unique_positions(ref, k), len(ref), len(q)
    out = []
    for qo in (q, revcomp(q)):
        c = Counter((pos[qo[i : i + k]] - i + m) >> SHIFT for i in range(m - k + 1) if qo[i : i + k] in pos)
        out.append([c[b] + c[b + 1] for b in range(((n + m) >> SHIFT) + 1)])
    return out


def seed_of(q, ref, k):
    """(STATUS, HITS, DIAG, OTHER) of a query: the best window of both orientations, ties forward, then to the lowest bin."""
    if not st.votable(q, ref, k):
        return NONE, 0, 0, 0
    best = [max((w, -b) for b, w in enumerate(ws)) for ws in windows(q, ref, k)]
    o = REV if best[REV][0] > best[FWD][0] else FWD
    return o, best[o][0], (-best[o][1] << SHIFT) - len(q), best[1 - o][0]


def expected(groups, k):
    """Per sequence of the batch, in order: its row; a group's first sequence is its reference."""
    k = k or st.K_DEFAULT
    return [(IS_REF, 0, 0, 0) if i == 0 else seed_of(s, grp[0], k) for grp in groups for i, s in enumerate(grp)]


# ---- placement and the polish of a contig ------------------------------------------------------------------------------------------------------------------------

def tiles_of(reference, tile):
    return [(a, reference[a : a + tile]) for a in range(0, len(reference), tile)]


def place(reference, reads, tile, k, min_hits=MIN_HITS):
    """Per read (strand, position, hits, other) of its best tile -- the most hits, ties to the lowest tile -- or None below min_hits."""
    out = []
    for q in reads:
        rows = [(a, seed_of(q, t, k or st.K_DEFAULT)) for a, t in tiles_of(reference, tile)]
        a, row = max(rows, key=lambda x: (x[1][HITS] if x[1][STATUS] in (FWD, REV) else -1, -x[0]))
        out.append((row[STATUS], a + row[DIAG], row[HITS], row[OTHER]) if row[STATUS] in (FWD, REV) and row[HITS] >= min_hits else None)
    return out


def polish_groups(reference, reads, tile, k, min_hits=MIN_HITS):
    """The groups Engine.polish_reads hands to Engine.polish: per tile the tile and, in the order of the reads, every placed read -- turned when REV -- whose
    footprint [position, position + m + SPAN) meets the tile."""
    placed = place(reference, reads, tile, k, min_hits)
    groups = []
    for a, t in tiles_of(reference, tile):
        grp = [t]
        for q, p in zip(reads, placed):
            if p is not None and p[1] < a + len(t) and p[1] + len(q) + SPAN > a:
                grp.append(revcomp(q) if p[0] == REV else q)
        groups.append(grp)
    return groups


# ---- the catalogue -------------------------------------------------------------------------------------------------------------------------------------------------

PLANTED_SUMS = (63, 64, 127, 128, 129)  # d + m of the planted diagonals: both sides of two bin edges
PLANTED_M = 40


@functools.lru_cache(maxsize=None)
def seed_groups(k):
    """What the strand catalogue has no reason to hold, seven groups: a repeat, a homopolymer, a tie between bins, a tie between strands, planted diagonals
    at the bin edges, overhangs, queries longer than their reference."""
    rng = random.Random(0x5EED + k)
    r = lambda n: rand_seq(rng, n)
    x, half = r(60), r(40)
    ref = r(600)
    m = PLANTED_M
    planted = [ref[s - m : s - m + m] for s in PLANTED_SUMS]  # exact slices at a = s - m: diagonal a, d + m = s
    a = 127 - m  # a deletion in the read moves its second half from diagonal a to a + 1: d + m = 127 and 128, two bins, one window
    straddle = ref[a : a + 20] + ref[a + 21 : a + 41]
    small = r(100)
    while True:  # two halves of a query on two far diagonals with as many hits each -- drawn again while a chance hit (k = 8 has some) breaks the tie
        y, z = r(60), r(60)
        halves = [r(200) + z + r(300) + y + r(200), y + z]
        ws = windows(halves[1], halves[0], k)
        if sorted(ws[FWD])[-4:] == [60 - k + 1] * 4 and max(ws[REV]) < 60 - k + 1:
            break
    return (
        [r(300) + x + r(100) + x + r(300), x, revcomp(x)],  # a stretch present twice: none of its k-mers seeds
        ["A" * 200, "A" * 77, "T" * 77],  # a homopolymer reference: one k-mer, everywhere
        halves,  # the lower of the two bins
        [r(150) + half + revcomp(half) + r(150), half + revcomp(half)],  # the query is its own reverse complement: the same histogram twice, forward
        [ref] + planted + [straddle, revcomp(straddle)],
        [ref, r(30) + ref[:50], ref[-50:] + r(30), revcomp(r(30) + ref[:50])],  # overhanging the start (negative DIAG) and the end
        [small, r(200) + small + r(200), revcomp(r(150) + small)],  # queries longer than their reference
    )


def catalogue(k):
    """strand_probes.catalogue(k) whole, and the seed groups."""
    return dict(st.catalogue(k), seeds=list(seed_groups(k)))


# ---- planted reads ---------------------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def draft_and_reads(seed, n, reads, lo, hi, rate_lo=0.10, rate_hi=0.12):
    """(draft, [read...], [(planted start, turned)...], [unrelated read...]): a random draft of n bases; reads are ont_copy, at a rate drawn from rate_lo ..
    rate_hi, of slices of lo .. hi bases of it that begin at the planted start, every second one reverse-complemented; and as many random reads of the same
    lengths, which belong nowhere."""
    rng = random.Random(seed)
    draft = rand_seq(rng, n)
    out, where, other = [], [], []
    for i in range(reads):
        m = rng.randrange(lo, min(hi, n) + 1)
        a = rng.randrange(0, n - m + 1)
        q = ont_copy(rng, draft[a : a + m], rng.uniform(rate_lo, rate_hi))
        out.append(revcomp(q) if i % 2 else q)
        where.append((a, bool(i % 2)))
        other.append(rand_seq(rng, m))
    return draft, tuple(out), tuple(where), tuple(other)


CONTIG = dict(seed=0xC0471, n=3000, reads=24, lo=300, hi=700)  # Engine.place / polish_reads on the GPU: tile 1 000 (narrow class) and 2 100 (wide)
