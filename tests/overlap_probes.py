"""The plain reference of the overlap run (include/consent_amd.h cw_overlap_*) and of Engine.overlaps / overlaps_paf, and the probes the GPU tests run: Python
strings, a dict of lists and a Counter only -- no GPU, no oracle.  Written from the header's definition, not from the kernels."""
import functools
import random
from collections import Counter

from poa_op_probes import rand_seq
from strand_probes import QMAX, revcomp

K_DEFAULT, SAMPLE_DEFAULT, MAX_OCC_DEFAULT = 15, 3, 512  # CW_OVL_K, CW_OVL_SAMPLE, CW_OVL_MAX_OCC
MIN_HITS = 2  # CW_OVL_MIN_HITS: twice the chance level test_overlap_cpu.py measures
MIN_K = 15  # the k the default min_hits is measured for
MIN_OVERLAP = 2000  # L of test_overlap_cpu.py: every planted overlap of at least L bases is found at the defaults
END_SLACK = 143  # CW_OVL_END_SLACK: the measured distance of an end from the truth, plus one bin
SHIFT = 6
TARGET, STRAND, HITS, DIAG, Q_START, Q_END, T_START, T_END, ROW = range(9)
FWD, REV = 0, 1
OK, NONE, SLOT, DENSE, BAD_INDEX = range(5)
LDS_CAP = 1024  # cw_overlap.h CW_OVL_CAP: the distinct (t, o, b) keys the LDS route takes
DENSE_CAP = 1 << 17  # CW_OVL_DENSE_CAP: beyond it CW_OVL_DENSE
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def code(s):
    v = 0
    for ch in s:
        v = (v << 2) | _CODE.get(ch, 3)
    return v


def occurrences(read, k, sample):
    """(c, i, s) of every sampled position of one read."""
    out = []
    for i in range(len(read) - k + 1):
        w = read[i : i + k]
        K, R = code(w), code(revcomp(w))
        if K == R:
            continue
        c = min(K, R)
        if sample == 0 or (((c * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - sample)) == 0:
            out.append((c, i, int(K > R)))
    return out


def indexed(read, k):
    return k <= len(read) <= QMAX


class Index:
    """Every sampled occurrence of every indexed read: c -> [(read, position, strand)], and per read its own occurrences."""

    def __init__(self, reads, k=0, sample=SAMPLE_DEFAULT):
        self.reads, self.k, self.sample = list(reads), k or K_DEFAULT, sample
        self.own = [occurrences(r, self.k, sample) if indexed(r, self.k) else [] for r in self.reads]
        self.post = {}
        for t, occ in enumerate(self.own):
            for c, p, s in occ:
                self.post.setdefault(c, []).append((t, p, s))
        self.n_entries = sum(len(o) for o in self.own)


def votes(ix, q, max_occ=0):
    """The Counter c[t, o, b] of query q."""
    max_occ, k, m = max_occ or MAX_OCC_DEFAULT, ix.k, len(ix.reads[q])
    c = Counter()
    for key, i, sq in ix.own[q]:
        entries = ix.post[key]
        if len(entries) > max_occ:
            continue
        for t, p, st in entries:
            if t == q:
                continue
            o = sq ^ st
            c[t, o, ((p + k + i) if o else (p - i + m)) >> SHIFT] += 1
    return c


def coordinates(diag, o, m, n, k):
    c0 = min(max(diag + 64, -(m - k)), n - k)
    a, z = max(0, -c0), min(m, n - c0)
    return ((m - z, m - 1 - a) if o else (a, z - 1)) + (a + c0, z + c0 - 1)


def rows_of(ix, q, max_occ=0, min_hits=MIN_HITS):
    """(status, rows) of query q without a slot: the candidates in row order."""
    m = len(ix.reads[q])
    if not indexed(ix.reads[q], ix.k):
        return NONE, []
    c = votes(ix, q, max_occ)
    if len(c) > DENSE_CAP:
        return DENSE, []
    best = {}
    for (t, o, b), n in c.items():
        for bb in (b, b - 1):
            if bb >= 0:
                cand = (c[t, o, bb] + c[t, o, bb + 1], -bb)
                if cand > best.get((t, o), (0, 0)):
                    best[t, o] = cand
    rows = []
    for (t, o), (w, nb) in sorted(best.items(), key=lambda x: (-x[1][0], x[0][0], x[0][1])):
        if w >= min_hits:
            diag = (-nb << SHIFT) - m
            rows.append((t, o, w, diag) + coordinates(diag, o, m, len(ix.reads[t]), ix.k))
    return OK, rows


def expected(reads, k=0, sample=SAMPLE_DEFAULT, max_occ=0, min_hits=MIN_HITS, first=0, count=None, slots=None, ix=None):
    """Per query first .. first + count - 1: (status, n_rows, rows written).  slots[j], when given, is the rows query j's slot holds."""
    ix = ix or Index(reads, k, sample)
    count = len(ix.reads) - first if count is None else count
    out = []
    for j in range(count):
        status, rows = rows_of(ix, first + j, max_occ, min_hits)
        if slots is not None and len(rows) > slots[j]:
            out.append((SLOT, len(rows), []))
        else:
            out.append((status, len(rows), rows))
    return out


def distinct_keys(ix, q, max_occ=0):
    return len(votes(ix, q, max_occ))


def paf_lines(reads, names, per_query):
    """The PAF lines of Engine.overlaps_paf for per_query = the rows of every query in order."""
    out = []
    for q, rows in enumerate(per_query):
        for t, o, hits, _, qs, qe, ts, te in rows:
            out.append("\t".join(str(x) for x in (names[q], len(reads[q]), qs, qe + 1, "-" if o else "+", names[t], len(reads[t]), ts, te + 1, hits,
                                                   max(qe + 1 - qs, te + 1 - ts), 255)))
    return out


# ---- planted read sets ---------------------------------------------------------------------------------------------------------------------------------------------

def ont_copy_map(rng, s, rate):
    """poa_op_probes.ont_copy with where every input base went: (copy, at) with at[j] the copy's length before input base j, at[len(s)] its whole length."""
    out, at = [], []
    for ch in s:
        at.append(len(out))
        x = rng.random()
        if x < rate * 0.4:
            continue
        if x < rate * 0.7:
            out.append(rng.choice("ACGT"))
            out.append(ch)
        elif x < rate:
            out.append(rng.choice("ACGT".replace(ch, "")))
        else:
            out.append(ch)
    at.append(len(out))
    return "".join(out), at


@functools.lru_cache(maxsize=None)
def planted(seed, n, reads, lo, hi, rate_lo=0.10, rate_hi=0.12):
    """(genome, reads, where): noisy copies (the ONT mix at rate_lo .. rate_hi) of slices of lo .. hi bases of a random genome of n bases, every second one
    turned; where[r] = (start, slice length, turned, at) with `at` the map of ont_copy_map."""
    rng = random.Random(seed)
    genome = rand_seq(rng, n)
    out, where = [], []
    for i in range(reads):
        m = rng.randrange(lo, min(hi, n) + 1)
        a = rng.randrange(0, n - m + 1)
        q, at = ont_copy_map(rng, genome[a : a + m], rng.uniform(rate_lo, rate_hi))
        out.append(revcomp(q) if i % 2 else q)
        where.append((a, m, bool(i % 2), tuple(at)))
    return genome, tuple(out), tuple(where)


SET = (0x0E71A9, 30000, 120, 1500, 5000)  # the measured set: test_overlap_cpu.py, and Engine.overlaps on the GPU
SMALL = (0x5A11, 6000, 40, 800, 2000)  # the end-to-end set


def gap_and_overlap(wa, wb):
    """(bases between the two true intervals, bases they share)."""
    lo, hi = max(wa[0], wb[0]), min(wa[0] + wa[1], wb[0] + wb[1])
    return max(0, lo - hi), max(0, hi - lo)


def true_ends(w, read_len, g0, g1):
    """The inclusive ends, on the read as given, of the genome's [g0, g1) in the read of where-entry w."""
    a, _, turned, at = w
    s, e = at[g0 - a], at[g1 - a]
    return (read_len - e, read_len - 1 - s) if turned else (s, e - 1)


@functools.lru_cache(maxsize=None)
def planted_index(which, k=0, sample=SAMPLE_DEFAULT):
    return Index(planted(*which)[1], k, sample)


# ---- the probes ------------------------------------------------------------------------------------------------------------------------------------------------------

PALINDROME8 = "ACGTACGT"  # its own reverse complement: K == R at k = 8
PLANTED_SUMS = (63, 64, 127, 128, 129)  # d + m of the planted diagonals
assert revcomp(PALINDROME8) == PALINDROME8


@functools.lru_cache(maxsize=None)
def family(k):
    """Reads of 24 to 600 bases: slices of a 1 500-base genome, exact and noisy, every third one turned; the palindrome planted in two of them; a read twice; a
    target that holds a stretch and its reverse complement; equal hits on three targets; reads shorter than k and empty ones.  Returns (reads, notes)."""
    rng = random.Random(0x0FA3 + k)
    r = lambda n: rand_seq(rng, n)
    genome = r(700) + PALINDROME8 + r(792)
    reads, notes = [], {}
    for i in range(18):
        m = rng.randrange(24, 601)
        a = rng.randrange(0, len(genome) - m + 1)
        q = genome[a : a + m] if i % 2 else ont_copy_map(rng, genome[a : a + m], 0.08)[0]
        reads.append(revcomp(q) if i % 3 == 2 else q)
    reads.append(genome[650:800])  # the palindrome, exact, in two more reads
    reads.append(revcomp(genome[690:760]))
    notes["twice"] = (len(reads), len(reads) + 1)
    reads += [genome[100:400], genome[100:400]]
    stretch = r(120)
    notes["both"] = (len(reads), len(reads) + 1)
    reads += [stretch, r(80) + stretch + r(60) + revcomp(stretch) + r(40)]
    shared = r(90)
    notes["ties"] = (len(reads), (len(reads) + 1, len(reads) + 2, len(reads) + 3))
    reads += [shared, r(50) + shared + r(50), revcomp(r(50) + shared + r(50)), r(20) + shared + r(70)]
    notes["short"] = (len(reads), len(reads) + 1, len(reads) + 2)
    reads += ["", genome[5 : 5 + k - 1], "ACG"]
    return tuple(reads), notes


@functools.lru_cache(maxsize=None)
def geometry(k):
    """A 600-base target (read 0); exact 40-base slices on the planted diagonals; reads that overhang both ends, as given and turned; reads that share only the
    target's last and first 20 bases; 24 bases on a read of 30 (the clamp of c0 at n - k); two halves of a query on two far diagonals with as many hits each (the lower bin)."""
    rng = random.Random(0x6E0 + k)
    r = lambda n: rand_seq(rng, n)
    ref = r(600)
    m = 40
    reads = [ref] + [ref[s - m : s] for s in PLANTED_SUMS]
    reads += [r(30) + ref[:50], ref[-50:] + r(30), revcomp(r(30) + ref[:50]), revcomp(ref[-50:] + r(30))]
    reads += [ref[-20:] + r(150), r(150) + ref[:20], revcomp(ref[-20:] + r(150))]
    tiny = r(30)
    reads += [tiny, tiny[5:25] + r(4)]  # m + n - k < 64: DIAG + 64 lies beyond n - k
    while True:  # drawn again while a chance hit (k = 8 has some) breaks the tie of the two bins or stands beside them
        y, z = r(60), r(60)
        halves = [r(200) + z + r(300) + y + r(200), y + z]
        c = votes(Index(halves, k, 0), 1)
        full = sorted(b for (t, o, b), n in c.items() if o == 0 and n >= 60 - k)
        if len(full) == 2 and c[0, 0, full[0]] == c[0, 0, full[1]] and not any(c[0, 0, b + d] for b in full for d in (-1, 1)):
            break
    reads += halves
    return tuple(reads)


@functools.lru_cache(maxsize=None)
def occurrence_edges():
    """k = 11, sample = 0, max_occ = 3: an 11-mer planted in three reads votes, another planted in four does not.  Returns (reads, x reads, y reads)."""
    rng = random.Random(0x0CC)
    while True:
        x, y = rand_seq(rng, 11), rand_seq(rng, 11)
        reads = [rand_seq(rng, 30) + (x if i < 3 else y) + rand_seq(rng, 30) for i in range(7)]
        ix = Index(reads, 11, 0)
        if sorted(len(v) for v in ix.post.values() if len(v) > 1) == [3, 4]:  # no chance repeat
            return tuple(reads), (0, 1, 2), (3, 4, 5, 6)


LONG = QMAX + 1


@functools.lru_cache(maxsize=None)
def too_long():
    """One read of CW_SW_QMAX + 1 bases among slices of it: CW_OVL_NONE, and no target either."""
    rng = random.Random(0x70010)
    big = rand_seq(rng, LONG)
    return (big[100:400], big, big[200:500], revcomp(big[30000:30300]), big[150:350])


DENSE_SET = dict(seed=0xDE45E0, m=16000, reads=300, n=300, k=8, min_hits=3)


@functools.lru_cache(maxsize=None)
def dense_reads():
    """One random query of 16 000 bases against 300 random reads of 300 bases at k = 8, sample = 0: its chance hits fall into more distinct keys than LDS_CAP."""
    rng = random.Random(DENSE_SET["seed"])
    return tuple([rand_seq(rng, DENSE_SET["m"])] + [rand_seq(rng, DENSE_SET["n"]) for _ in range(DENSE_SET["reads"])])
