"""The probe catalogue of the finish kernel (consent_amd/csrc/cw_finish.h: weightConsensus and the local de-Bruijn polish), shared by
tests/test_finish_ref_cpu.py and tests/test_gpu_finish.py, and what every probe is compared with.

The reference of a probe is built without cwo_run's finish, from the pile's own strings (tests/test_chain_ref_cpu.py assert_oracle_agrees does the same):
  raw       the concatenation of oracle_poa(pieces(pile, members)) over the segments of chain_probes.reference(pile, prm) (the template for a window
            without a chain)
  counts    every k-mer of the pile, index_probes.reference_counts(hb, k, 1): plain numpy
  weighted  oracle_weight_polish(raw, counts, k, solid, polish=False)
  polished  oracle_weight_polish(raw, counts, k, solid): the scalar restatement of correctionMSA.cpp:6-27, correctionDBG.cpp and DBG.cpp that
            tests/test_oracle_units.py pins with hand-derived answers
  link_calls, nbr_calls   oracle_run's statistics: every frame of the recursive link, every getNeighbours call made inside it
and beside it walk(): the same polish once more in plain Python over the weighted string, which must spell `polished` and count the same frames and
calls (the CPU test holds the two together) and says what the oracle's statistics do not: whether the head or the tail was extended, whether a link
succeeded, whether a zone k-mer below the solidity threshold was met, whether any table lookup beyond weightConsensus happened at all.

A probe is one window, alone in its batch.  Its route is written down by hand -- the FINISH_ROUTE bits (consent_amd/engine.py) it must set in the test-aid
library -- from these constants, read out of cw_finish.h (FIN below; nothing is restated):
  table     `staged` n_solid <= CW_FIN_SKEYS; `compact` above that up to CW_FIN_K16_MAX when k <= 9 and the bitmap is in LDS; else `global`
  counts    `cnt16` with the staged table while no count exceeds 65535; else `cnt_global`
  bitmap    `vis_lds` up to 32 * CW_FIN_VIS_WORDS solid k-mers, `vis_global` beyond
  pass      `first_pass`; `second_pass` when the raw consensus is longer than CW_FIN_CB or the polish outgrows it (up to CW_FIN_CB_BIG)
  walk      `find4` (staged and any lookup beyond weightConsensus), `count_scan`, `head`, `tail`, `linked`: what walk() saw
A consensus shorter than k is not polished: its route is its pass alone.

Two kinds of pile.  The designed pile: a truth T whose k-mers are all different, the template t' = T with substitutions, T itself `copies` times, then
ballast; prm = (k, copies, 2, 2, 1): with max_msa = 1 every segment's only member is the template's piece, so raw is t' letter for letter, its k-mers
across a substitution occur once and are weak, T's occur `copies` times and are solid: the polish has to put T's letters back by a link (a substitution in
the middle), by the head or the tail extension (one near an end).  Variants of T (`alleles`: T with one more substitution, as often as T) fork the graph
next to a weak region: two solid successors with equal counts, told apart by generation order only.  The noisy pile is index_probes.noisy_pile, a shallow
core under (k, 2, 8, 2, 12).  Ballast grows n_solid without touching the members: unrelated random sequences behind the core, each `solid` times, the last
one cut at the base that brings n_solid to the designed number exactly."""
import os
import random
import re
import sys
from collections import Counter

import consent_amd as ca
import oracle_lib
from chain_probes import distinct, pieces, reference
from consent_amd.engine import FINISH_ROUTE
from index_probes import noisy_pile, pack, poly_a_pile, reference_counts, str2num

__all__ = ["PROBES", "FIN", "walk", "route_from_constants"]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZONE, MAX_BRANCHES, MAX_ANCHORS = 3, 50, 5  # include/cw_policy.h CW_DBG_ZONE, CW_DBG_MAX_BRANCHES, CW_DBG_MAX_ANCHORS (tests/test_finish_ref_cpu.py holds them to the header)


def header_constants():
    """CW_FIN_CB, CW_FIN_SKEYS, CW_FIN_VIS_WORDS, CW_FIN_K16_MAX, CW_FIN_CB_BIG and the launch geometry, out of cw_finish.h."""
    hdr = open(os.path.join(ROOT, "consent_amd", "csrc", "cw_finish.h")).read()
    out = {}
    for name in ("CW_FIN_WAVES", "CW_FIN_WGS_PER_CU", "CW_FIN_CB", "CW_FIN_CB_BIG", "CW_FIN_VIS_WORDS", "CW_FIN_SKEYS", "CW_FIN_FRAMES"):
        out[name[7:]] = int(re.search(rf"#define {name} (\d+)", hdr).group(1))
    expr = re.search(r"#define CW_FIN_K16_MAX (\(.*?\)) /\*", hdr).group(1)  # an integer expression over the others
    out["K16_MAX"] = eval(re.sub(r"CW_FIN_(\w+)", lambda m: str(out[m.group(1)]), expr).replace("/", "//"), {})
    return out


FIN = header_constants()


# ---- the polish once more, in plain Python --------------------------------------------------------------------------------------------------
class Walk:
    pass


def walk(read, counts, k, solid):
    """polishCorrection over the weighted string `read` with the pile's counts {key: occurrences}: a Walk with .string and what was met on the way."""
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))
    w = Walk()
    w.link_calls = w.nbr_calls = 0
    w.head = w.tail = w.linked = w.scan = w.lookups = False
    w.weak_zone_kmers, w.ties, w.pair_ties, w.longest = [], [], 0, len(read)
    cnt = lambda word: counts.get(str2num(word.upper()), 0)

    def neighbours(kmer, left):
        w.lookups = True
        kmer = kmer.upper()
        cands = [c + kmer[:-1] for c in "TGCA"] if left else [kmer[1:] + c for c in "ACGT"]  # generation order (DBG.cpp:29-44)
        out = sorted((c for c in cands if cnt(c) >= solid), key=lambda c: -cnt(c))  # stable
        w.ties += [(x, y) for x, y in zip(out, out[1:]) if cnt(x) == cnt(y)]  # (winner, loser) by generation order alone
        return out

    visited = set()

    def link(dst, branches, dist, cur, max_len):
        w.link_calls += 1
        if branches[0] > MAX_BRANCHES or dist > max_len:
            return None
        src = cur[-k:]
        found = src == dst
        path = cur
        nb = neighbours(src, 0)
        w.nbr_calls += 1
        it = 0
        while not found and len(nb) == 1 and it < len(nb) and dist <= max_len:
            cand = nb[it]
            seen = cand in visited
            found = cand == dst
            if not found and not seen:
                visited.add(cand)
                path += cand[-1]
                dist += 1
                nb = neighbours(path[-k:], 0)
                w.nbr_calls += 1
                it = 0
            elif found:
                path += cand[-1]
            else:
                it += 1
        while not found and len(nb) > 1 and it < len(nb) and dist <= max_len:
            cand = nb[it]
            seen = cand in visited
            found = cand == dst
            if not found and not seen:
                visited.add(cand)
                branches[0] += 1
                got = link(dst, branches, dist + 1, path + cand[-1], max_len)
                if got is not None:
                    return got
                it += 1
            elif found:
                path += cand[-1]
            else:
                it += 1
        return path if found else None

    up = str.isupper
    i = 0
    while i < len(read) and not up(read[i]):
        i += 1
    if 0 < i < len(read) and len(read) - i >= k:
        ext_len, dist = i, 0
        nb = neighbours(read[i : i + k], 1)
        while len(nb) == 1 and dist < ext_len:
            read = read[: i - 1 - dist] + nb[0][0] + read[i - dist :]
            dist += 1
            w.head = True
            nb = neighbours(nb[0], 1)
        i = dist

    def next_src(beg, m):
        run, j = 0, beg
        while j < len(read) and (up(read[j]) or run < m):
            run = run + 1 if up(read[j]) else 0
            j += 1
        return j - 1 if run >= m else -1

    def next_dst(beg, m):
        run, j = 0, beg
        while j < len(read) and run < m:
            run = run + 1 if up(read[j]) else 0
            j += 1
        return j - 1 if run >= m else -1

    m = k + ZONE
    t_src_beg = t_dst_beg = t_dst_end = 0
    while i < len(read):
        src_end = next_src(i, m)
        dst_end = next_dst(src_end + 1, m)
        if src_end == -1 or dst_end == -1:
            break
        w.lookups = True
        src_beg, dst_beg = src_end - m + 1, dst_end - m + 1
        ks = [read[src_beg + q : src_beg + q + k] for q in range(ZONE + 1)]
        kd = [read[dst_beg + q : dst_beg + q + k] for q in range(ZONE + 1)]
        weak = [x for x in ks + kd if cnt(x) < solid]
        if weak:
            w.scan = True
            w.weak_zone_kmers += weak
        pairs = [(a, d) for a in range(ZONE + 1) if ks.count(ks[a]) == 1 for d in range(ZONE + 1) if kd.count(kd[d]) == 1]
        pairs.sort(key=lambda p: -(cnt(ks[p[0]]) + cnt(kd[p[1]])))  # stable: the lowest pair index wins a tie
        sums = [cnt(ks[a]) + cnt(kd[d]) for a, d in pairs]
        w.pair_ties += sum(1 for x, y in zip(sums, sums[1:]) if x == y)
        region = None
        for a, d in pairs[:MAX_ANCHORS]:
            if region is not None:
                break
            t_src_beg, t_dst_beg = src_beg + a, dst_beg + d
            t_dst_end = t_dst_beg + k - 1
            if ks[a] != kd[d]:
                gap = t_dst_beg - (t_src_beg + k - 1) - 1
                max_size = int(((15.0 / 100.0 * 2.0) * float(gap) + float(gap)) + float(k))
                region = link(kd[d].upper(), [0], 0, ks[a].upper(), max_size)
        if region is not None:
            w.linked = True
            r = read[t_src_beg : t_dst_end + 1]
            b = read.find(r)
            read = read[:b] + region + read[b + len(r) :]
            w.longest = max(w.longest, len(read), len(region) + 1)  # (the path buffer holds one character more than the path)
            i = b
        else:
            i = t_dst_beg if t_dst_beg > i else dst_beg

    i = len(read) - 1
    while i > 0 and not up(read[i]):
        i -= 1
    if 0 < i < len(read) - 1 and i + 1 >= k:
        ext_len, dist = len(read) - 1 - i, 0
        nb = neighbours(read[i + 1 - k : i + 1], 0)
        while nb and dist < ext_len:
            read = read[: i + 1 + dist] + nb[0][-1] + read[i + 2 + dist :]
            dist += 1
            w.tail = True
            nb = neighbours(nb[0], 0)
    w.string = read
    return w


def route_from_constants(k, n_solid, max_count, raw_len, w):
    """The FINISH_ROUTE names of a window by the header's constants and what walk() met."""
    names = ["second_pass" if max(raw_len, w.longest) > FIN["CB"] else "first_pass"]
    if raw_len < k:
        return sorted(names)
    vis_glb = n_solid > 32 * FIN["VIS_WORDS"]
    staged = n_solid <= FIN["SKEYS"]
    compact = not staged and n_solid <= FIN["K16_MAX"] and k <= 9 and not vis_glb
    names += ["staged" if staged else "compact" if compact else "global", "cnt16" if staged and max_count <= 0xFFFF else "cnt_global", "vis_global" if vis_glb else "vis_lds"]
    names += ["find4"] * (staged and w.lookups) + ["count_scan"] * w.scan + ["head"] * w.head + ["tail"] * w.tail + ["linked"] * w.linked
    return sorted(names)


# ---- the reference of one probe -----------------------------------------------------------------------------------------------------------
class Ref:
    pass


def build_ref(pile, prm, hb):
    k, solid = prm[:2]
    r = Ref()
    ch = reference(pile, prm)
    r.has_chain = ch.has_chain
    keys, cnts, _ = reference_counts(hb, k, 1)
    r.counts = dict(zip(keys.tolist(), cnts.tolist()))
    r.n_solid = int((cnts >= solid).sum())
    r.max_count = int(cnts.max()) if len(cnts) else 0
    r.raw = "".join(oracle_lib.oracle_poa(pieces(pile, mem)) for _, mem in ch.segments if mem) if ch.has_chain else pile[0]
    if ch.has_chain and len(r.raw) >= k:
        r.weighted = oracle_lib.oracle_weight_polish(r.raw, r.counts, k, solid, polish=False)
        r.polished = oracle_lib.oracle_weight_polish(r.raw, r.counts, k, solid)
        r.walk = walk(r.weighted, r.counts, k, solid)
    else:  # the template as it is, or a consensus the polish skips
        r.weighted = r.polished = r.raw
        r.walk = walk("", {}, k, solid)
        r.walk.string = r.raw
    r.oracle, st = oracle_lib.oracle_run(ca.Params(*prm), hb)
    r.link_calls, r.nbr_calls = st["link_calls"], st["nbr_calls"]
    return r


# ---- pile builders ------------------------------------------------------------------------------------------------------------------------
def other(c, step=1):
    return "ACGT"[("ACGT".index(c) + step) % 4]


def distinct_over(rng, n, k, letters):
    while True:
        s = "".join(rng.choice(letters) for _ in range(n))
        if len({s[i : i + k] for i in range(n - k + 1)}) == n - k + 1:
            return s


def designed_core(seed, k, length, errors, copies=2, alleles=(), run=None, letters="ACGT", frag=None, extra=()):
    """[t', T x copies, every allele x copies].  errors: positions where t' differs from T (the next letter of `letters`); alleles: (position, step) -- T
    with the letter at `position` moved `step` letters on; run = (position, letter, n): T holds exactly n of `letter` there; frag = (first, k-mers): the
    copies are that stretch of T only; extra: sequences put behind."""
    rng = random.Random(seed)
    while True:
        T = distinct_over(rng, length, k, letters)
        if run:
            at, ch, n = run
            T = T[:at] + ch * n + T[at + n :]
            if T[at - 1] == ch or T[at + n] == ch or len({T[i : i + k] for i in range(length - k + 1)}) != length - k + 1:
                continue
        break
    nxt = lambda c, step=1: letters[(letters.index(c) + step) % len(letters)]
    t1 = "".join(nxt(c) if i in errors else c for i, c in enumerate(T))
    F = T if frag is None else T[frag[0] : frag[0] + frag[1] + k - 1]
    pile = [t1] + [F] * copies
    for at, step in alleles:
        pile += [T[:at] + nxt(T[at], step) + T[at + 1 :]] * copies
    return pile + list(extra)


def with_ballast(core, k, solid, target, seed, letters="ACGT", length=300):
    """core + unrelated sequences of `length` bases, each `solid` times, until the pile has exactly `target` solid k-mers: the last one is cut where it gets there."""
    cnt = Counter(s[i : i + k] for s in core for i in range(len(s) - k + 1))
    n = sum(1 for v in cnt.values() if v >= solid)
    assert n <= target, (n, target)
    rng = random.Random(seed)
    pile = list(core)
    while n < target:
        b = "".join(rng.choice(letters) for _ in range(length))
        cut = length
        for i in range(length - k + 1):
            word = b[i : i + k]
            if cnt[word] < solid:
                n += 1
            cnt[word] += solid
            if n == target:
                cut = i + k
                break
        pile += [b[:cut]] * solid
    return pile


def noisy_core(seed=11, n=12, length=300, rate=0.12):
    return noisy_pile(seed, n, length, rate)


def poly_a_behind(core, total):
    """The poly-A pile of index_probes.py (A x 9 exactly `total` times) behind a core that holds no A x 9 itself."""
    assert not any("A" * 9 in s for s in core)
    return core + poly_a_pile(4100, total)


# ---- the catalogue ------------------------------------------------------------------------------------------------------------------------
class Probe:
    def __init__(self, name, prm, route, build, configure=None, **designed):
        self.name, self.prm, self.build, self.configure, self.designed = name, prm, build, configure, designed
        self.route_names = sorted(route.split())
        self._pile = self._hb = self._ref = None

    @property
    def route(self):
        return sum(FINISH_ROUTE[n] for n in self.route_names)

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
            self._ref = build_ref(self.pile, self.prm, self.hb)
        return self._ref

    def __repr__(self):
        return self.name


def n_solid_of(pile, k, solid):
    cnt = Counter(s[i : i + k] for s in pile for i in range(len(s) - k + 1))
    return sum(1 for v in cnt.values() if v >= solid)


def small_pile(seed, k, length, errors, frag, want):
    """A designed pile whose copies are a stretch of `want` k-mers of T only: the first seed from `seed` on with exactly that many solid k-mers (a substituted
    letter can spell one of them again)."""
    for s in range(seed, seed + 64):
        pile = designed_core(s, k, length, errors, frag=frag)
        if n_solid_of(pile, k, 2) == want:
            return pile
    raise AssertionError("no seed gives the designed solid set")


def long_flank_pile(seed, k, flank, deletions, every=200, tlen=300):
    """A template T of `tlen` bases between two flanks only the other sequences have: S = X + T + Y three times (solid = 3), and in front of them, as the two
    members beside the template (max_msa = 3), S' = S with every `every`-th flank base substituted or deleted: the consensus spells S', longer than the
    first pass's buffers when the flanks are long enough, and the polish puts S's letters back -- a deleted base back in makes the string one longer."""
    rng = random.Random(seed)
    T = distinct(rng, tlen, k)
    X, Y = ("".join(rng.choice("ACGT") for _ in range(flank)) for _ in range(2))
    S = X + T + Y
    hit = lambda i: i % every == every // 2 and not flank <= i < flank + tlen
    S1 = "".join(("" if deletions else other(c)) if hit(i) else c for i, c in enumerate(S))
    return [T, S1, S1, S, S, S]


CORE_ERRORS = {3, 60, 100, 146}  # of the 150-base designed core: one near each end (head, tail), two in the middle (links)
NOISY = (9, 2, 8, 2, 12)
LONG = (8, 3, 2, 2, 3)


def catalogue():
    P = []
    D = lambda k: (k, 2, 2, 2, 1)
    FIRST = "first_pass vis_lds "
    STAGED = FIRST + "staged cnt16 find4 "
    COMPACT = FIRST + "compact cnt_global "
    GLOBAL = FIRST + "global cnt_global "
    ALL = "head linked tail"

    def add(name, prm, route, build, **designed):
        P.append(Probe(name, prm, route, build, **designed))

    core = lambda seed=1, k=9, **kw: designed_core(seed, k, 150, CORE_ERRORS, **kw)
    # ---- the staged table: fin_find4's pivots (every 64th key), buckets, four-key groups and padding
    add("staged n_solid=1 k=2", D(2), STAGED + "tail", lambda: small_pile(21, 2, 7, {5}, (3, 1), 1), n_solid=1, links=0, nbrs=0)
    for n in (3, 4, 5):  # (k = 3, 2: the stretch of n solid k-mers is long enough for the tail extension to find a successor among them)
        add(f"staged n_solid={n} k=3", D(3), STAGED + "tail", lambda n=n: small_pile(30 + n, 3, 14, {n + 5}, (2, n), n), n_solid=n, links=0, nbrs=0)
    for n in (63, 64, 65, 128):
        add(f"staged n_solid={n}", D(9), STAGED + ALL, lambda n=n: designed_core(10 + n, 9, n + 8, {2, (n + 8) // 2, n + 5}), n_solid=n, links=1, nbrs=21, changed=True)
    for n in (1020, 1021, 1022, 1023, 1024):
        add(f"staged n_solid={n}", D(9), STAGED + ALL, lambda n=n: with_ballast(core(), 9, 2, n, 5), n_solid=n, changed=True)
    add("staged k=16, T x16 solid and on the path", D(16), STAGED + "linked", lambda: designed_core(50, 16, 160, {80}, run=(72, "T", 16), extra=["G" + "T" * 16 + "G"]), n_solid=145, holds="T" * 16, changed=True)
    add("staged k=9, A x9 solid and on the path", D(9), STAGED + "linked", lambda: designed_core(51, 9, 150, {75}, run=(70, "A", 9)), n_solid=142, holds="A" * 9, changed=True)
    for k, length, errors, walk_bits in ((5, 44, {20}, "linked"), (7, 100, {2, 50, 97}, ALL), (8, 120, {2, 60, 117}, ALL), (12, 150, {3, 70, 146}, ALL), (16, 160, {3, 80, 156}, ALL)):
        add(f"staged k={k}", D(k), STAGED + walk_bits, lambda k=k, length=length, errors=errors: designed_core(40 + k, k, length, errors), n_solid=length - k + 1, changed=True)
    add("staged noisy", NOISY, STAGED + "linked", lambda: noisy_core(11), n_solid=347, links=10, nbrs=44, changed=True)
    # ---- the compact table: its bounds, the four 16-bit ranges, one of them empty, k = 8 (one range) and 7
    for n in (1025, 2000, 3839, 3840):
        add(f"compact n_solid={n}", D(9), COMPACT + ALL, lambda n=n: with_ballast(core(), 9, 2, n, 5), n_solid=n, changed=True, **({"ranges": (True, True, True, True)} if n == 2000 else {}))
    add("compact noisy n_solid=2000", NOISY, COMPACT + "linked", lambda: with_ballast(noisy_core(12), 9, 2, 2000, 0), n_solid=2000, changed=True)
    add("compact, no key in the second range", D(9), COMPACT + ALL, lambda: with_ballast(core(52, letters="AGT"), 9, 2, 1100, 7, letters="AGT"), n_solid=1100, changed=True, ranges=(True, False, True, True))
    add("compact k=8", D(8), COMPACT + ALL, lambda: with_ballast(core(68, 8), 8, 2, 1100, 8), n_solid=1100, changed=True, ranges=(True, False, False, False))
    add("compact k=7", D(7), COMPACT + "linked tail", lambda: with_ballast(designed_core(67, 7, 100, {3, 60, 96}), 7, 2, 1100, 8), n_solid=1100, changed=True, ranges=(True, False, False, False))
    # ---- the global table: one past the compact table's bound, and every k beyond 9
    for n in (3841, 4100):
        add(f"global n_solid={n}", D(9), GLOBAL + ALL, lambda n=n: with_ballast(core(), 9, 2, n, 5), n_solid=n, changed=True)
    add("global noisy n_solid=4100", NOISY, GLOBAL + "linked", lambda: with_ballast(noisy_core(12), 9, 2, 4100, 0), n_solid=4100, changed=True)
    for k in (10, 12):
        for n in (1025, 1300):
            add(f"global k={k} n_solid={n}", D(k), GLOBAL + ALL, lambda k=k, n=n: with_ballast(core(60 + k, k), k, 2, n, 8), n_solid=n, changed=True)
    # ---- counts beyond 16 bits: A x9 65535 / 65536 times behind a core whose link forks into it
    for total, counts in ((65535, "cnt16"), (65536, "cnt_global")):
        add(f"poly-A {total}", D(9), FIRST + f"staged find4 linked {counts}", lambda t=total: poly_a_behind(designed_core(70, 9, 150, {73}, run=(70, "A", 8)), t), max_count=total, changed=True,
            **({"truncation": True} if total == 65536 else {}))
    # ---- ties: an allele of T as often as T, next to the weak region; on each table road
    for step, who in ((1, "the truth's letter first"), (3, "the allele's letter first")):
        add(f"tie, {who}", D(9), STAGED + "linked", lambda step=step: designed_core(1, 9, 150, {60}, alleles=((61, step),)), n_solid=151, tie=True, changed=True)
    add("tie on the compact table", D(9), COMPACT + "linked", lambda: with_ballast(designed_core(1, 9, 150, {60}, alleles=((61, 3),)), 9, 2, 1100, 5), n_solid=1100, tie=True, changed=True)
    add("tie on the global table", D(9), GLOBAL + "linked", lambda: with_ballast(designed_core(1, 9, 150, {60}, alleles=((61, 3),)), 9, 2, 4100, 5), n_solid=4100, tie=True, changed=True)
    # ---- the visited bitmap: 32 * CW_FIN_VIS_WORDS solid k-mers in LDS, one more in the wave's global slot
    for n in (32768, 32769):
        add(f"bitmap k=9 n_solid={n}", D(9), ("first_pass global cnt_global head tail " + ("vis_lds" if n == 32768 else "vis_global")), lambda n=n: with_ballast(core(), 9, 2, n, 9), n_solid=n)
    for n in (32768, 32769, 33000):
        add(f"bitmap k=12 n_solid={n}", D(12), ("first_pass global cnt_global " + ALL + (" vis_lds" if n == 32768 else " vis_global")), lambda n=n: with_ballast(core(72, 12), 12, 2, n, 9), n_solid=n, changed=True)
    # ---- head, tail and nothing
    add("weak at its first and last characters", D(9), STAGED + "head tail", lambda: designed_core(80, 9, 150, {0, 149}), n_solid=142)
    add("shorter than k + 3", D(9), STAGED.replace("find4 ", ""), lambda: designed_core(81, 9, 11, {5}), n_solid=3, raw_len=11)
    add("a template shorter than k", D(9), "first_pass", lambda: ["ACGTACG", "ACGTACG", "ACGTACG"], n_solid=0, raw_len=7, template=True)
    add("all weak", (9, 5, 2, 2, 1), STAGED.replace("find4 ", ""), lambda: designed_core(82, 9, 150, set()), n_solid=0)
    add("all solid", D(9), STAGED.replace("find4 ", ""), lambda: designed_core(83, 9, 150, set()), n_solid=142)
    # ---- buffers: CW_FIN_CB characters in the first pass
    SECOND = "second_pass vis_lds compact cnt_global linked"
    add("raw consensus of 3300 characters", LONG, SECOND, lambda: long_flank_pile(2, 8, 1500, False), raw_len=3300, polished_len=3300, changed=True)
    add("the polish fills the buffer: 3062 to 3072", LONG, SECOND.replace("second", "first"), lambda: long_flank_pile(2, 8, 1388, True), raw_len=3062, polished_len=3072, changed=True)
    add("the polish outgrows the buffer: 3066 to 3076", LONG, SECOND, lambda: long_flank_pile(2, 8, 1390, True), raw_len=3066, polished_len=3076, changed=True)
    add("a full buffer outgrown: 3072 to 3082", LONG, SECOND, lambda: long_flank_pile(2, 8, 1393, True), raw_len=3072, polished_len=3082, changed=True)
    return P


PROBES = catalogue()
BY_NAME = {p.name: p for p in PROBES}


def check_designed(probe):
    """The probe is what the catalogue says it is, from the reference alone: a probe that misses its edge fails here, on the CPU."""
    d, r = probe.designed, probe.ref
    for name, got in (("n_solid", r.n_solid), ("max_count", r.max_count), ("raw_len", len(r.raw)), ("polished_len", len(r.polished)), ("links", r.link_calls), ("nbrs", r.nbr_calls)):
        if name in d:
            assert got == d[name], (probe, name, got, d[name])
    assert r.has_chain != bool(d.get("template")), probe
    if "holds" in d:  # a k-mer the pile makes solid and the polished consensus spells
        assert r.counts.get(str2num(d["holds"]), 0) >= probe.prm[1] and d["holds"] in r.polished, probe
    if d.get("changed"):  # a link succeeded and changed the string
        assert r.walk.linked and r.link_calls > 0 and r.polished.upper() != r.weighted.upper(), probe
    if "ranges" in d:  # which of the compact table's four ranges (bits 17:16 of the key) hold a solid key
        have = {key >> 16 for key, c in r.counts.items() if c >= probe.prm[1]}
        assert tuple(h in have for h in range(4)) == d["ranges"] and have <= {0, 1, 2, 3}, (probe, have)
