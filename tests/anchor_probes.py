"""The probe catalogue of the index kernel's anchor phase (consent_amd/csrc/cw_index.h from idx_template_table to idx_hand_over), shared by
tests/test_anchor_ref_cpu.py and tests/test_gpu_anchor_block.py.  The reference for what that phase writes -- the window's anchor block -- is
tests/anchor_ref.py.

A probe is one window, alone in its batch, aimed at one edge.  It carries prm = (k, solid, common_kmers, min_anchors, max_msa), an optional `configure`
(cw_configure's template length: the engine of the long templates), its designed numbers (asserted from the reference alone, on the CPU) and its route:
the anchor-phase bits of INDEX_ROUTE (consent_amd/engine.py), written down by hand from these rules of cw_index.h --
  wide         more than 1024 template k-mers (nk0): the arrays per template k-mer are twice as long and the room behind them is 92416 bytes, not 107776
  tfit         need(nk0) <= room, need(rows) = rows * Np * 2 + rows * Nw * 8 + 2 N + 16: a matrix row per template k-mer, filled by the support pass
  pg           not tfit and need(A) > room: the matrix in global memory (else a row per anchor in LDS)
  hit_list     not tfit and N <= 1024: the support pass writes its hits to a list
  second_pass  hit_list, but a hit at position >= 2048 or more than CW_IDX_HIT_CAP = 524288 hits: the rows are filled by a second pass over the pile.  A hit
               is a (sequence, position) whose k-mer is a template k-mer, repeated ones included (hits() below counts them so)
  bucket_walk  some lookup of the support pass left its home bucket ((key * 2654435761 mod 2^32) >> 22, four entries a bucket, overflow into the next):
               five or more template k-mers homed in one bucket (the template's own k-mers are looked up too, and one of the five is elsewhere), or a
               pile k-mer that is no template k-mer homed in a full bucket (bucket_walk() below)
  use_bits     N <= 2048 and matrix + A * Nw * 8 + 2 N <= room
-- and the count-phase bits, which this catalogue does not aim at but writes down by hand as well, one of eight sets (S_BYTES .. HASH_P below) by the rules
of tests/index_probes.py: every probe stays on k = 9 with solid <= 15 or on the hash table, away from the walk export whose re-walk depends on the key
distribution; big_ex has a second cause that the count probes do not reach: more than 524288 occurrences beyond a key's fifteenth, the list
idx_count_nibbles keeps of them.  chain_probes.index_arithmetic does the sums for the anchor phase and count_route() restates the count phase's rules; the
CPU test compares both with what is written here.

Sizes (room 107776; Np = N rounded up to twice an odd number, Nw = ceil(N / 64)):
  N = 100   Np 102, Nw 2: need(488) = 107576 fits, need(489) = 107796 does not; with A = 488 the bitsets end at 99552 + 7808 + 200 = 107560 <= room, but
            the masks' arrays (+ 33 A + 508) do not fit: dirty sequences without masks
  N = 38    wide room 92416: Np 38, Nw 1: need(1099) = 92408 fits, need(1100) = 92492 does not
  N = 2048  no matrix in LDS (pg): A * 32 * 8 + 4096 <= 107776 iff A <= 405
  254 rows  need A >= 254 anchors and, in the block, 255 * Ap bytes on what the nk0 - A template k-mers that are no anchors leave free, 2 Np + 8 Nw + 12
            each.  On tfit nk0 * (2 Np + 8 Nw) must fit the room as well: N = 46 (Np 46, Nw 1), nk0 = 1024: need(1024) = 102508 fits, and with A = 300 the
            724 other k-mers leave 724 * 112 = 81088 >= 255 * 304 = 77520.  With a row per anchor in LDS (N = 60, nk0 = 925) and on pg (N = 200) the
            template has 330 anchors
The largest probe is `hits 524288` / `hits 524289` (1024 sequences of 512 template k-mers): its reference takes 0.7 s on one CPU core and the score identity
over its 130 816 pairs 0.15 s (measured); `N=2048 A=405 / 406` take 0.55 s and 0.18 s, no probe takes longer.
Every probe but `nk0=2049` ends not stopped; that one stops on CW_WHY_TEMPLATE, a documented stop, and has no block."""
import collections
import random

import numpy as np

from anchor_ref import block_reference
from chain_probes import anchors, block_moved, distinct, swapped
from consent_amd.engine import INDEX_ROUTE
from index_probes import pack, rand_seq, str2num

ANCHOR_BITS = ("wide", "tfit", "pg", "hit_list", "use_bits", "second_pass", "bucket_walk")
HIT_CAP = 524288  # CW_IDX_HIT_CAP
TAIL_UNIT = "ACGTT"

_LUT = np.zeros(256, np.uint64)
for _i, _ch in enumerate(b"ACGT"):
    _LUT[_ch] = _i
_KEYS = {}


def keys_of(seq, k):
    """The k-mers of a string as integers in str2num order, one per position."""
    if (seq, k) not in _KEYS:
        c = _LUT[np.frombuffer(seq.encode(), np.uint8)]
        n = len(c) - k + 1
        v = np.zeros(max(n, 0), np.uint64)
        for j in range(k if n > 0 else 0):
            v = (v << np.uint64(2)) | c[j : j + n]
        _KEYS[(seq, k)] = v
    return _KEYS[(seq, k)]


def hits(pile, k):
    """(hits, the largest hit position in a support pass over the pile): every (sequence, position) whose k-mer is a template k-mer, the template's own included."""
    tk = np.unique(keys_of(pile[0], k))
    n, far = 0, -1
    for seq, mult in collections.Counter(pile).items():
        at = np.nonzero(np.isin(keys_of(seq, k), tk))[0]
        n += len(at) * mult
        far = max(far, int(at.max()) if len(at) else -1)
    return n, far


def home(keys):
    return ((keys.astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)


def bucket_homes(pile, k):
    """(template k-mers homed per bucket, entries per bucket once overflow has moved on): linear probing over buckets, whose occupancy no insertion order changes."""
    homed = np.bincount(home(np.unique(keys_of(pile[0], k))).astype(np.int64), minlength=1024)
    occ, carry = np.zeros(1024, np.int64), 0
    for _ in range(2):  # (the table is a ring: the second round starts with what the first carried past the end)
        for b in range(1024):
            occ[b] = min(4, homed[b] + carry)
            carry = homed[b] + carry - occ[b]
    return homed, occ


def bucket_walk(pile, k):
    homed, occ = bucket_homes(pile, k)
    if homed.max() > 4:
        return True
    tk = np.unique(keys_of(pile[0], k))
    for seq in set(pile):
        ks = keys_of(seq, k)
        other = ks[~np.isin(ks, tk)]
        if len(other) and (occ[home(other).astype(np.int64)] == 4).any():
            return True
    return False


def count_route(pile, prm):
    """The count-phase bits of the window's route, by the rules tests/index_probes.py writes down (and tests/test_gpu_index_counts.py holds the kernel to)."""
    k, solid = prm[0], prm[1]
    N = len(pile)
    names = ["staged"] * (N <= 192 and sum((len(s) + 15) // 16 for s in pile) <= 5628)
    counts = collections.Counter()
    for seq, mult in collections.Counter(pile).items():
        u, c = np.unique(keys_of(seq, k), return_counts=True)
        for key, n in zip(u.tolist(), c.tolist()):
            counts[key] += n * mult
    if k > 9:
        assert sum(1 for c in counts.values() if c >= solid) <= 16384  # (no probe sorts its solid set in global memory)
        return names + ["hashed"] + ["hash_passes"] * (sum(counts.values()) > 8192)
    assert k == 9 and solid <= 15
    if N <= 200 and N >= 64 and max(counts.values(), default=0) <= 255:
        return names + ["bytes_done"]
    assert sum(1 for c in counts.values() if c >= 15) <= 1024  # (no probe has more saturated keys than the exact table in LDS holds)
    # idx_count_nibbles lists every occurrence beyond a key's fifteenth in the work-group's global scratch, 2 * CW_EXG_SLOTS = 524288 entries: a pile with more
    # of them is counted again with the exact table in global memory (big_ex) -- the two piles of 2048 sequences
    late = sum(max(c - 15, 0) for c in counts.values())
    return names + ["nibbles", "export_masks"] + ["big_ex"] * (late > 524288)


# ---- pile builders ------------------------------------------------------------------------------------------------------------------------
def tail_of(n):
    return (TAIL_UNIT * (n // 5 + 1))[:n]


def proper(seed, length, k):
    """`length` bases whose k-mers are all different and which a tandem-repeat tail can follow without continuing into it."""
    rng = random.Random(seed)
    while True:
        t = distinct(rng, length, k)
        if t[-1] != "T":
            return t


def copies(seed, n_kmers, k, n, tail=0, changed=(), extra=()):
    """A template of n_kmers different k-mers (and `tail` bases of a tandem repeat behind it, whose k-mers are repeated: template k-mers that are no anchors),
    n sequences in all: exact copies, then one sequence change(template proper) + tail for every entry of `changed`, then the strings of `extra`.  With a
    tail the template proper is n_kmers bases: the k - 1 k-mers across its end into the tail are different from all others too."""
    t = proper(seed, n_kmers + (0 if tail else k - 1), k)
    end = tail_of(tail)
    return [t + end] * (n - len(changed) - len(extra)) + [c(t) + end for c in changed] + list(extra)


def far_hit(seed, n_kmers, k, n, tail, at):
    """copies(), and one sequence that holds the template's first k-mer at position `at` behind unrelated bases and ends there.  The first seed from `seed` on
    whose template fills no bucket of its table is taken: then no k-mer of the unrelated bases can walk, and the pile's route has no bucket_walk by chance."""
    for s in range(seed, seed + 256):
        pile = copies(s, n_kmers, k, n - 1, tail)
        if bucket_homes(pile, k)[1].max() < 4:
            break
    else:
        raise AssertionError("no seed leaves every bucket with room")
    rng, tk = random.Random(s + 1), keys_of(pile[0], k)
    while True:  # (unrelated: the filler and its k-mers into the template's first k-mer hold no template k-mer, so the hit at `at` is the sequence's only one)
        far = rand_seq(rng, at) + pile[0][:k]
        if np.isin(keys_of(far, k), tk).sum() == 1:
            return pile + [far]


def near_miss_pile(seed, k):
    """Six copies of a template of 150 k-mers and two sequences made of near misses: every fifth template k-mer with its first base changed -- the same last ten
    bases, so for k > 10 the same 20-bit fingerprint in the template table -- strung together."""
    t = proper(seed, 150 + k - 1, k)
    rng, tk = random.Random(seed), keys_of(t, k)
    while True:  # (the k-mers across two near misses are chance: none of them may be a template k-mer)
        # (the changed first base is also not the base that would continue the near miss in front of it into the template's next k-mer)
        miss = [rng.choice([c for c in "ACGT" if c != t[i] and c != t[i - 5 + k]]) + t[i + 1 : i + k] for i in range(0, 150, 5)]
        out = ["".join(miss[:15]), "".join(miss[15:])]
        if not any(np.isin(keys_of(s, k), tk).any() for s in out):
            return [t] * 6 + out


def crowded_pile(seed, k):
    """A template of 1000 k-mers in the table's 1024 buckets, the first seed from `seed` on that homes five or more of them in one bucket, five copies, and one
    sequence that ends in a k-mer which is no template k-mer and is homed in that bucket."""
    for s in range(seed, seed + 64):
        t = proper(s, 1000 + k - 1, k)
        homed, _ = bucket_homes([t], k)
        if homed.max() >= 5:
            break
    else:
        raise AssertionError("no seed crowds a bucket")
    full, rng, tk = int(homed.argmax()), random.Random(s), set(keys_of(t, k).tolist())
    while True:
        w = rand_seq(rng, k)
        if str2num(w) not in tk and int(home(np.array([str2num(w)], np.uint64))[0]) == full:
            return [t] * 5 + [t[:40] + w]


def repeats_pile(seed):
    """Which k-mers are anchors: D[40:49] is twice in the template; T[250:259] is twice in sequence 1 only, at 250 and 259 (two rounds of 256 k-mers of the
    wave that scans it); T[2:11] twice in sequence 2 only, at 2 and 11 (two lanes' groups of four)."""
    d = proper(seed, 320, 9)
    t = d[:100] + d[40:49] + d[100:]
    return [t, t[:259] + t[250:259] + t[259:], t[:11] + t[2:11] + t[11:]] + [t] * 6


def support_pile(seed, n, common=8):
    """Three stretches of 30 bases: the k-mers that start in the first are held by exactly sup - 1 sequences, all others by sup or more (sup = min(common, n // 2))."""
    t = proper(seed, 90, 9)
    sup = min(common, n // 2)
    return [t] * (sup - 1) + [t[30:]] + [t[60:]] * (n - sup)


def short_pile(seed):
    """Sequences shorter than k and one of exactly k bases, which holds one anchor."""
    t = proper(seed, 80, 9)
    return [t, t, "ACGT", t[10:19], t, "ACGTACGT", t[20:70]]


# what puts a sequence out of order, by the block it moves (template proper of 200 bases or more):
FORWARD = lambda t: block_moved(t, 150, 80, 20)  # a block earlier: its 12 k-mers are bad forward, the 70 between bad backward
BACKWARD = lambda t: block_moved(t, 80, 150, 20)  # a block later: the other way round
TIE = lambda t: swapped(t, 40, 100, 20)  # two blocks exchanged: as many bad either way, forward it is
NEAR = lambda t: swapped(t, 40, 80, 20)
DIRECTIONS = (FORWARD, FORWARD, BACKWARD, BACKWARD, TIE)


def bad_counts(P32, s):
    """(anchors that set no new record in sequence s scanned forward, the same scanned backward)."""
    pos = P32[P32[:, s] >= 0, s].astype(np.int64)
    rev = -pos[::-1]
    return int((pos[1:] <= np.maximum.accumulate(pos)[:-1]).sum()), int((rev[1:] <= np.maximum.accumulate(rev)[:-1]).sum())


def directions_pile(seed, n_kmers, n, tail=0):
    """Exact copies and five sequences out of order: two forward, two backward, and one in which two blocks of equal length change places -- as many bad
    anchors either way unless a k-mer across a cut happens to be a template k-mer: the first seed from `seed` on with the exact tie is taken (the CPU test
    asserts it again)."""
    for s in range(seed, seed + 64):
        pile = copies(s, n_kmers, 9, n, tail=tail, changed=DIRECTIONS)
        fwd, bwd = bad_counts(anchors(pile, 9, 8)[1], n - 1)
        if fwd == bwd > 0:
            return pile
    raise AssertionError("no seed gives the tie")


def rows_pile(seed, extra_block, n, tail, n_kmers=330, blocks=21, first=50, back=40):
    """n_rows on its edge: `blocks` dirty sequences each move their own block of 20 bases (12 k-mers, next to each other in the template from `first` on) `back`
    bases earlier, and one more a block of extra_block bases: 12 * blocks + (extra_block - 8) anchors are bad somewhere.  The clean copies and the tail give
    the block room for the rows: 254 rows of Ap bytes on what a template k-mer that is no anchor leaves free, 2 Np + 8 Nw + 12 bytes."""
    last = first + 12 * blocks
    moves = [lambda t, x=first + 12 * j: block_moved(t, x, x - back, 20) for j in range(blocks)] + [lambda t: block_moved(t, last, last - back, extra_block)]
    return copies(seed, n_kmers, 9, n, tail=tail, changed=moves)


# ---- the catalogue ------------------------------------------------------------------------------------------------------------------------
class Probe:
    def __init__(self, name, prm, route, count, build, configure=None, stop=None, **designed):
        self.name, self.prm, self.build, self.configure, self.stop, self.designed = name, prm, build, configure, stop, designed
        self.anchor_route, self.count_route = sorted(route.split()), sorted(count.split())
        self._pile = self._hb = self._ref = self._route = None

    @property
    def pile(self):
        if self._pile is None:
            self._pile = self.build()
        return self._pile

    @property
    def hb(self):
        if self._hb is None:
            self._hb = pack(self.pile)
        return self._hb

    @property
    def ref(self):
        if self._ref is None:
            self._ref = block_reference(self.pile, self.prm)
        return self._ref

    @property
    def route(self):
        """The window's whole route on the test-aid library, as written in the catalogue: the anchor-phase bits and the count phase's (a stopped window has
        neither: cw_setup_kernel stops it and the index kernel passes it by)."""
        return sum(INDEX_ROUTE[n] for n in self.anchor_route + self.count_route)

    def __repr__(self):
        return self.name


def arithmetic_route(probe):
    """The anchor-phase bits by the sums of chain_probes.index_arithmetic and the counts of this module, from the reference's numbers."""
    r, k = probe.ref, probe.prm[0]
    names = [n for n in ("wide", "tfit", "pg", "hit_list", "use_bits") if r.arith[n]]
    n_hits, far = hits(probe.pile, k)
    names += ["second_pass"] * (r.arith["hit_list"] and (far >= 2048 or n_hits > HIT_CAP))
    names += ["bucket_walk"] * bucket_walk(probe.pile, k)
    return sorted(names)


# the count-phase bits of a probe, written down by hand like the anchor-phase bits (rules: tests/index_probes.py; count_route() above restates them and
# the CPU test compares): S = staged (at most 192 sequences and 5628 packed words)
S_BYTES, BYTES = "staged bytes_done", "bytes_done"  # k = 9, 64 .. 200 sequences, no k-mer more than 255 times
S_NIB, NIB, NIB_BIG = "staged nibbles export_masks", "nibbles export_masks", "nibbles export_masks big_ex"  # k = 9 otherwise; big_ex: more than 524288 late occurrences
S_HASH, S_HASH_P, HASH_P = "staged hashed", "staged hashed hash_passes", "hashed hash_passes"  # k > 9; more than 8192 k-mers in the pile


def catalogue():
    P = []
    std, k12 = (9, 2, 8, 2, 20), (12, 2, 8, 2, 20)
    LONG = 2048 + 12 - 1  # the longest template cw_configure takes at k = 12

    def add(name, prm, route, count, build, **kw):
        P.append(Probe(name, prm, route, count, build, **kw))

    # ---- where the matrix lies
    add("tfit N=100 nk0=488", std, "tfit use_bits", S_BYTES, lambda: copies(2000, 488, 9, 100), N=100, A=488, nk0=488, flags=1)
    add("tfit N=100 nk0=489", std, "pg hit_list use_bits", S_BYTES, lambda: copies(2001, 489, 9, 100), N=100, A=489, nk0=489, flags=1)
    add("rows in LDS A=488", std, "hit_list use_bits", S_NIB, lambda: copies(2002, 488, 9, 100, tail=40), N=100, A=488, nk0=520, flags=1)  # (the tail's k-mers: 600 times each)
    add("rows in global memory A=489", std, "pg hit_list use_bits", S_NIB, lambda: copies(2003, 489, 9, 100, tail=40), N=100, A=489, nk0=521, flags=1)
    for nk0, route in ((1024, "tfit use_bits bucket_walk"), (1025, "wide tfit use_bits bucket_walk"), (2048, "wide tfit use_bits bucket_walk")):
        add(f"nk0={nk0} k=12", k12, route, S_HASH, lambda n=nk0: copies(2100 + n, n, 12, 3), configure=LONG, N=3, A=nk0, nk0=nk0, flags=1)
    add("nk0=2049 k=12", k12, "", "", lambda: copies(2149, 2049, 12, 3), configure=LONG, stop="template", N=3, nk0=2049)
    add("wide tfit nk0=1099", k12, "wide tfit use_bits bucket_walk", S_HASH_P, lambda: copies(2150, 1099, 12, 38), configure=LONG, N=38, A=1099, nk0=1099, flags=1)
    add("wide nk0=1100", k12, "wide pg hit_list use_bits bucket_walk", S_HASH_P, lambda: copies(2151, 1100, 12, 38), configure=LONG, N=38, A=1100, nk0=1100, flags=1)
    # ---- how it is filled
    add("hit list N=1024", std, "pg hit_list use_bits", NIB, lambda: copies(2200, 60, 9, 1024), N=1024, A=60, flags=1)
    add("no hit list N=1025", std, "pg use_bits", NIB, lambda: copies(2201, 60, 9, 1025), N=1025, A=60, flags=1)
    # (a hit at 2047 / 2048 behind as many unrelated bases, none of which homes in a full bucket of the template table: far_hit sees to it, so that the two
    # probes differ in second_pass alone)
    add("hit at 2047 from the list", std, "hit_list use_bits", S_NIB, lambda: far_hit(2210, 488, 9, 100, 40, 2047), N=100, A=488, far=2047, flags=1)
    add("hit at 2048 second pass", std, "hit_list second_pass use_bits", S_NIB, lambda: far_hit(2211, 488, 9, 100, 40, 2048), N=100, A=488, far=2048, flags=1)
    add("hit at 2047 tfit", std, "tfit use_bits", S_NIB, lambda: far_hit(2212, 100, 9, 6, 0, 2047), N=6, A=100, far=2047, flags=1)
    add("hit at 2048 tfit", std, "tfit use_bits", S_NIB, lambda: far_hit(2213, 100, 9, 6, 0, 2048), N=6, A=100, far=2048, flags=1)
    add("hits 524288", std, "pg hit_list use_bits", NIB, lambda: copies(2220, 512, 9, 1024), N=1024, A=512, hits=HIT_CAP, flags=1)
    # (one more: the last copy ends in the template's first k-mer once more -- twice in that sequence, so no anchor any more, and a hit twice)
    add("hits 524289", std, "pg hit_list second_pass use_bits", NIB, lambda: (lambda p: p[:-1] + [p[0] + p[0][:9]])(copies(2220, 512, 9, 1024)), N=1024, A=511, hits=HIT_CAP + 1, flags=1)
    for k in (10, 11, 12, 16):
        add(f"near misses k={k}", (k, 2, 8, 2, 20), "tfit use_bits", S_HASH, lambda k=k: near_miss_pile(2300 + k, k), N=8, A=150, near_misses=30 if k > 10 else 0, flags=1)
    add("crowded bucket k=9", std, "tfit use_bits bucket_walk", S_NIB, lambda: crowded_pile(2400, 9), N=6, crowded=True, flags=1)
    add("crowded bucket k=12", k12, "tfit use_bits bucket_walk", S_HASH, lambda: crowded_pile(2401, 12), N=6, crowded=True, flags=1)
    # ---- which k-mers are anchors
    add("repeated k-mers", std, "tfit use_bits", S_NIB, lambda: repeats_pile(2500), N=9, flags=1,
        no_anchor=lambda p: [p[0][40:49], p[0][250:259], p[0][2:11]], anchor=lambda p: [p[0][39:48], p[0][249:258], p[0][251:260], p[0][1:10], p[0][3:12]])
    for n in (11, 17, 20):  # sup = 5 = N // 2, 8 = N // 2 = common_kmers at an odd N, 8 = common_kmers < N // 2
        add(f"support N={n}", std, "tfit use_bits", S_NIB, lambda n=n: support_pile(2510 + n, n), N=n, A=52, sup=min(8, n // 2), flags=1,
            no_anchor=lambda p: [p[0][29:38]], anchor=lambda p: [p[0][30:39]])
    add("short sequences", std, "tfit use_bits", S_NIB, lambda: short_pile(2530), N=7, A=72, flags=1)
    add("N=1", (9, 1, 8, 2, 20), "tfit use_bits", S_NIB, lambda: copies(2531, 72, 9, 1), N=1, A=72, flags=1)
    # ---- classification, masks and rows, each on every placement of the matrix it can reach: scan_seq, idx_presence and the rows read it through M.row() /
    # M.rd().  `place`: tfit, lds (a row per anchor in LDS) or pg, asserted from the arithmetic
    TFIT, LDS, PG = ("tfit use_bits", "tfit"), ("hit_list use_bits", "lds"), ("pg hit_list use_bits", "pg")
    # forward, backward and a tie; without a tail the block has no room for rows: one-word masks only
    add("directions tfit masks", std, TFIT[0], S_NIB, lambda: directions_pile(2600, 200, 11), N=11, n_dirty=5, flags=3, directions=(3, 2), place="tfit")
    add("directions tfit rows", std, TFIT[0], S_NIB, lambda: directions_pile(2601, 200, 11, tail=300), N=11, n_dirty=5, flags=7, directions=(3, 2), place="tfit")
    add("directions rows in LDS", std, LDS[0], S_NIB, lambda: directions_pile(2602, 300, 110, tail=200), N=110, n_dirty=5, flags=7, directions=(3, 2), place="lds")
    add("directions pg", std, PG[0], NIB, lambda: directions_pile(2603, 200, 400, tail=60), N=400, n_dirty=5, flags=7, directions=(3, 2), place="pg")
    # masks of 1 .. 4 words and rows made of them; 256 dirty sequences: no masks.  N = nd + 8; (anchors, tail) per placement: tfit needs few template k-mers,
    # a row per anchor in LDS a tail long enough for need(nk0) > room, pg enough anchors for need(A) > room -- fewer of both the deeper the pile
    ladder = {64: ((100, 60), (100, 600), (700, 200)), 128: ((100, 60), (100, 300), (400, 100)), 192: ((100, 60), (100, 200), (300, 60)), 255: ((100, 60), (100, 120), (220, 60))}
    for nd in (64, 65, 128, 129, 192, 193, 255, 256):
        for (route, place), (a, tail) in zip((TFIT, LDS, PG), ladder[nd & ~1 if nd < 255 else 255]):
            count = S_NIB if nd + 8 <= 192 and (nd + 8) * ((a + tail + 15) // 16) <= 5628 else NIB
            if (nd, place) == (65, "pg"):
                route += " bucket_walk"  # (this template's 892 k-mers home five in one bucket; its neighbour's do not)
            add(f"{nd} dirty sequences {place}", std, route, count, lambda nd=nd, a=a, tail=tail: copies(2700 + nd, a, 9, nd + 8, tail=tail, changed=[NEAR] * nd),
                N=nd + 8, n_dirty=nd, W=(nd + 63) // 64, flags=1 if nd == 256 else 7 if nd <= 64 else 5, place=place)
    # masks of two words that fit, and no room in the block for rows: no masks at all.  On tfit and pg every template k-mer is an anchor; with a row per anchor in
    # LDS there are 35 that are none (need(260) > room), whose 15.7 KB are less than the 84 rows of 240 bytes that a swap across 100 bases makes
    add("65 dirty sequences without room for rows tfit", std, TFIT[0], S_BYTES, lambda: copies(2765, 100, 9, 73, changed=[NEAR] * 65), N=73, n_dirty=65, W=2, flags=1, masks=True, place="tfit")
    add("65 dirty sequences without room for rows lds", std, LDS[0], NIB, lambda: copies(2766, 225, 9, 200, tail=43, changed=[lambda t: swapped(t, 40, 140, 20)] * 65),
        N=200, A=225, nk0=260, n_dirty=65, W=2, flags=1, masks=True, place="lds")
    add("65 dirty sequences without room for rows pg", std, PG[0], NIB, lambda: copies(2767, 200, 9, 300, changed=[NEAR] * 65), N=300, n_dirty=65, W=2, flags=1, masks=True, place="pg")
    # beyond 1024 sequences: the dirty index lives in the `clean` byte, one-word masks or none.  A matrix row is 2348 bytes: tfit holds 44 of them
    small = lambda t: swapped(t, 4, 24, 10)
    for nd in (64, 65):
        add(f"N=1100 {nd} dirty sequences tfit", std, "tfit use_bits", NIB, lambda nd=nd: copies(2810 + nd, 44, 9, 1100, changed=[small] * nd), N=1100, A=44, nk0=44, n_dirty=nd,
            flags=7 if nd == 64 else 1, place="tfit")  # (room for rows all the same: the block is sized for 1100 dirty sequences, and their list is 2 KB shorter)
        add(f"N=1100 {nd} dirty sequences lds", std, "use_bits", NIB, lambda nd=nd: copies(2820 + nd, 40, 9, 1100, tail=20, changed=[small] * nd), N=1100, A=40, nk0=52, n_dirty=nd,
            flags=7 if nd == 64 else 1, place="lds")
        add(f"N=1100 {nd} dirty sequences pg", std, "pg use_bits", NIB, lambda nd=nd: copies(2800 + nd, 60, 9, 1100, tail=60, changed=[lambda t: swapped(t, 10, 40, 12)] * nd),
            N=1100, n_dirty=nd, flags=7 if nd == 64 else 1, place="pg")
    # n_rows on its edge (the module docstring has the sums of the three placements); on tfit 300 anchors of 1024 template k-mers at 46 sequences
    add("254 rows tfit", std, TFIT[0], S_NIB, lambda: rows_pile(2900, 22, 46, 732, 300, 20, 31, 30), N=46, A=300, nk0=1024, n_dirty=21, rows=254, flags=7, place="tfit")
    add("255 rows tfit", std, TFIT[0], S_NIB, lambda: rows_pile(2900, 23, 46, 732, 300, 20, 31, 30), N=46, A=300, nk0=1024, n_dirty=21, rows=255, flags=3, place="tfit")
    add("254 rows lds", std, LDS[0], S_NIB, lambda: rows_pile(2900, 10, 60, 603), N=60, n_dirty=22, rows=254, flags=7, place="lds")
    add("255 rows lds", std, LDS[0], S_NIB, lambda: rows_pile(2900, 11, 60, 603), N=60, n_dirty=22, rows=255, flags=3, place="lds")
    add("254 rows pg", std, PG[0], NIB, lambda: rows_pile(2900, 10, 200, 200), N=200, n_dirty=22, rows=254, flags=7, place="pg")
    add("255 rows pg", std, PG[0], NIB, lambda: rows_pile(2900, 11, 200, 200), N=200, n_dirty=22, rows=255, flags=3, place="pg")
    # the bitsets fit and the masks' arrays behind them do not (+ 33 A + 508): dirty sequences without masks
    add("bitsets fit, masks do not tfit", std, TFIT[0], S_BYTES, lambda: copies(2910, 488, 9, 100, changed=[NEAR] * 4), N=100, A=488, nk0=488, n_dirty=4, flags=1, masks=False, place="tfit")
    add("bitsets fit, masks do not lds", std, LDS[0], S_NIB, lambda: copies(2911, 488, 9, 100, tail=40, changed=[NEAR] * 4), N=100, A=488, nk0=520, n_dirty=4, flags=1, masks=False, place="lds")
    add("bitsets fit, masks do not pg", std, "pg use_bits", NIB_BIG, lambda: copies(2912, 405, 9, 2048, changed=[NEAR] * 4), N=2048, A=405, n_dirty=4, flags=1, masks=False, place="pg")
    # rows of anchors beyond 1024: the row numbering's second round
    add("dirty beyond anchor 1024 tfit", k12, "wide tfit use_bits bucket_walk", S_HASH, lambda: copies(2920, 1300, 12, 4, tail=520, changed=[lambda t: block_moved(t, 1200, 1100, 20)]),
        configure=LONG, N=4, n_dirty=1, flags=7, rows_beyond=1024, place="tfit")
    add("dirty beyond anchor 1024 lds", k12, "wide hit_list use_bits bucket_walk", S_HASH_P, lambda: copies(2921, 1050, 12, 22, tail=758, changed=[lambda t: block_moved(t, 1030, 930, 20)]),
        configure=LONG, N=22, A=1050, n_dirty=1, flags=7, rows_beyond=1024, place="lds")
    add("dirty beyond anchor 1024 pg", k12, "wide pg hit_list use_bits bucket_walk", S_HASH_P, lambda: copies(2922, 1100, 12, 38, tail=150, changed=[lambda t: block_moved(t, 1060, 960, 20)]),
        configure=LONG, N=38, A=1100, n_dirty=1, flags=7, rows_beyond=1024, place="pg")
    # ---- no bitsets
    add("N=2049", std, "pg", NIB, lambda: copies(3000, 64, 9, 2049, changed=[lambda t: swapped(t, 10, 40, 12)] * 3), N=2049, n_dirty=0, flags=0)
    add("N=2048 A=405", std, "pg use_bits", NIB_BIG, lambda: copies(3001, 405, 9, 2048), N=2048, A=405, flags=1)
    add("N=2048 A=406", std, "pg", NIB_BIG, lambda: copies(3002, 406, 9, 2048), N=2048, A=406, flags=0)
    return P


PROBES = catalogue()


def check_designed(probe):
    """The probe is what the catalogue says it is, from the reference alone: a probe that misses its edge fails here, on the CPU."""
    d, r, k = probe.designed, probe.ref, probe.prm[0]
    pile = probe.pile
    got = {"N": r.N, "A": r.A, "nk0": r.nk0, "n_dirty": r.n_dirty, "flags": r.flags, "W": r.arith["W"], "sup": r.sup}
    for name, value in got.items():
        if name in d:
            assert value == d[name], (probe, name, value, d[name])
    if "hits" in d or "far" in d:
        n_hits, far = hits(pile, k)
        assert d.get("hits", n_hits) == n_hits and d.get("far", far) == far, (probe, n_hits, far)
    if "rows" in d:  # the anchors that are bad somewhere, whether the block carries rows for them or not
        assert int(r.isbad.any(axis=1).sum()) == d["rows"] and r.n_rows == (d["rows"] if d["rows"] <= 254 else 0), (probe, int(r.isbad.any(axis=1).sum()), r.n_rows)
    if "rows_beyond" in d:
        assert r.has_delta and (np.nonzero(r.rowid != 0xFF)[0] >= d["rows_beyond"]).any() and r.A > 1024, probe
    if "directions" in d:
        went = [r.direction[int(s)] for s in r.dirty]
        assert (went.count("forward"), went.count("backward")) == d["directions"], (probe, went)
        fwd, bwd = bad_counts(r.P32, r.N - 1)  # the last sequence: as many bad anchors backward as forward, and forward it goes
        assert fwd == bwd == len(r.bad[r.N - 1]) and r.direction[r.N - 1] == "forward", (probe, fwd, bwd)
    keys = set(r.ckey.tolist())
    for w in d.get("no_anchor", lambda p: [])(pile):
        assert str2num(w) not in keys, (probe, w)
    for w in d.get("anchor", lambda p: [])(pile):
        assert str2num(w) in keys, (probe, w)
    if "near_misses" in d:
        tk = keys_of(pile[0], k)
        low, whole = set((tk & np.uint64(0xFFFFF)).tolist()), set(tk.tolist())
        missed = [int(x) for s in pile[6:] for x in keys_of(s, k) if int(x) not in whole and (int(x) & 0xFFFFF) in low]
        assert (len(missed) >= 30) if d["near_misses"] else True, (probe, len(missed))
        assert not (r.P32[:, 6:] >= 0).any(), probe  # none of them is in the matrix
    if "place" in d:
        assert ("tfit" if r.arith["tfit"] else "pg" if r.arith["pg"] else "lds") == d["place"], (probe, r.arith)
    if "masks" in d:  # whether the masks' arrays fit behind the bitsets (and there are 1 .. 255 dirty sequences of at most four words)
        assert r.arith["masks"] == d["masks"], (probe, r.arith)
    if d.get("crowded"):
        homed, occ = bucket_homes(pile, k)
        full = int(homed.argmax())
        last = keys_of(pile[-1], k)[-1:]
        assert homed[full] >= 5 and int(home(last)[0]) == full and int(last[0]) not in set(keys_of(pile[0], k).tolist()), (probe, homed.max())
