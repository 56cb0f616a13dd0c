"""The probe catalogue of the index kernel's count paths, shared by tests/test_index_counts_cpu.py and tests/test_gpu_index_counts.py, the numpy
reference for a window's k-mer counts, and the helper the tests that name a path use to ask the test-aid library which way a window went.

A probe is one window aimed at one edge of cw_index_kernel's count phase (consent_amd/csrc/cw_index.h).  It carries
  prm       (k, solid, common_kmers, min_anchors, max_msa)
  route     the INDEX_ROUTE bits (consent_amd/engine.py) the window must take, written down by hand from the constants of cw_index.h:
              staged       N <= CW_IDX_STAGE_N = 192 sequences and at most CW_IDX_STAGE_WORDS = 5628 packed words
              bytes_done   N <= 200, solid <= 127, 4^k / 4 words a multiple of 4096 (k = 7, 8, 9), k = 9 only from CW_IDX_BYTES_MIN_N = 64 sequences on, and
                           no count past 255; otherwise nibbles
              export_masks on the nibble path: solid <= 15 and 4^k / 8 words a multiple of 4096 (k = 8, 9); otherwise export_walk
              rewalk       a thread of the walk holds more than CW_EXP_SLOTS = 8 solid keys in its 4^k / 8 / 1024 words, or a count >= 2^14
              big_ex       more than CW_EX_SLOTS = 1024 keys reach fifteen occurrences
              hashed       k > 9; hash_passes: more than 8192 k-mers in the pile; hash_gsort: more than 16384 solid keys
              tfit         nk0 * Np * 2 + nk0 * ceil(N / 64) * 8 + 2 N + 16 <= 107776 bytes (nk0 template k-mers, Np = N rounded up to twice an odd number)
              use_bits     N <= 2048 and the presence bitsets fit
            every probe keeps its template short enough for tfit, so none has hit_list, pg or wide: tests/test_gpu_parity.py and
            tests/test_gpu_batch_invariance.py hold those bits
  designed  the numbers the probe was built to have, asserted from the numpy side on the CPU: n_seqs, kmers (the pile's k-mer count), markers
            ({k-mer: occurrences}), distinct_solid (number of solid keys) or distinct_solid_min, and for a probe that exports by the walk
            per_thread = (keys a thread owns, the most solid keys any thread may hold | the fewest the fullest thread must hold): what `rewalk` goes by
Every probe ends not stopped: none of these edges is a documented stop."""
import contextlib
import random

import numpy as np

import consent_amd as ca
from consent_amd import engine
from consent_amd.engine import INDEX_ROUTE, HostBatch, route_names


# ---- the reference: plain numpy -----------------------------------------------------------------------------------------------------------
def pile_codes(hb, w=0):
    """Window w of a HostBatch unpacked: one array of 2-bit codes per sequence."""
    out = []
    shifts = (30 - 2 * np.arange(16, dtype=np.uint32))[None, :]
    for s in range(int(hb.win_first_seq[w]), int(hb.win_first_seq[w + 1])):
        n, o = int(hb.seq_len[s]), int(hb.seq_word_off[s])
        words = hb.bases[o : o + (n + 15) // 16].astype(np.uint32)
        out.append(((words[:, None] >> shifts) & 3).reshape(-1)[:n].astype(np.uint64))
    return out


def reference_counts(hb, k, solid, w=0):
    """(keys, counts, pile k-mer count): every k-mer of every sequence of length >= k, template included, as an integer in str2num order (first base
    most significant); np.unique; counts >= solid kept.  Ascending by key."""
    keys = []
    for c in pile_codes(hb, w):
        n = len(c) - k + 1
        if n <= 0:
            continue
        v = np.zeros(n, np.uint64)
        for j in range(k):
            v = (v << np.uint64(2)) | c[j : j + n]
        keys.append(v)
    allk = np.concatenate(keys) if keys else np.zeros(0, np.uint64)
    u, cnt = np.unique(allk, return_counts=True)
    m = cnt >= solid
    return u[m], cnt[m].astype(np.int64), len(allk)


def str2num(s):
    v = 0
    for ch in s:
        v = v * 4 + "ACGT".index(ch)
    return v


def pack(pile):
    """One window of ACGT strings (template first) as a HostBatch, sequences front to back: packed here, not by the library under test."""
    lens = np.array([len(s) for s in pile], np.uint32)
    nw = (lens.astype(np.int64) + 15) // 16
    offs = np.concatenate([[0], np.cumsum(nw)[:-1]]).astype(np.uint64)
    bases = np.zeros(max(int(nw.sum()), 1), np.uint32)
    lut = np.zeros(256, np.uint32)
    for i, ch in enumerate(b"ACGT"):
        lut[ch] = i
    for s, o, n in zip(pile, offs, nw):
        c = np.zeros(int(n) * 16, np.uint32)
        c[: len(s)] = lut[np.frombuffer(s.encode(), np.uint8)]
        bases[int(o) : int(o) + int(n)] = (c.reshape(-1, 16) << (30 - 2 * np.arange(16, dtype=np.uint32))[None, :]).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    return HostBatch(np.array([0, len(pile)], np.uint32), lens, offs, bases)


# ---- pile builders ------------------------------------------------------------------------------------------------------------------------
def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def mutate(rng, s, rate):  # as in test_gpu_parity.py
    out = []
    for c in s:
        x = rng.random()
        if x < rate * 0.3:
            continue
        if x < rate * 0.6:
            out.append(rng.choice("ACGT"))
        out.append(rng.choice("ACGT") if x < rate else c)
    return "".join(out)


def substitute(rng, s, rate):
    """Substitutions only: the length, and with it the pile's k-mer count, stays what it was designed to be."""
    return "".join(rng.choice("ACGT") if rng.random() < rate else c for c in s)


def count_of(pile, kmer):
    n = 0
    for s in pile:
        i = s.find(kmer)
        while i >= 0:
            n += 1
            i = s.find(kmer, i + 1)
    return n


def noisy_pile(seed, n_seqs, length, rate=0.1):
    rng = random.Random(seed)
    truth = rand_seq(rng, length)
    return [truth] + [mutate(rng, truth, rate) for _ in range(n_seqs - 1)]


def planted_pile(seed, n_seqs, length, plan, rate=0.1):
    """A noisy pile in whose support sequences each marker of `plan` ({k-mer: occurrences}) is inserted exactly that often.  An insertion can make a
    second copy of a marker by chance: the first seed from `seed` on that gives the designed numbers is taken (the CPU test asserts them again)."""
    for attempt in range(64):
        rng = random.Random(seed + 1000 * attempt)
        pile = noisy_pile(rng.randrange(1 << 30), n_seqs, length, rate)
        cuts = [[] for _ in pile]
        for marker, occ in plan.items():
            for _ in range(occ):
                cuts[rng.randrange(1, n_seqs)].append(marker)
        for s in range(1, n_seqs):
            seq, ms = pile[s], cuts[s]
            rng.shuffle(ms)
            pos = sorted(rng.sample(range(12, len(seq) - 12), len(ms)))
            out, last = [], 0
            for p, m in zip(pos, ms):
                out += [seq[last:p], m]
                last = p
            pile[s] = "".join(out + [seq[last:]])
        if all(count_of(pile, m) == occ for m, occ in plan.items()):
            return pile
    raise AssertionError("no seed gives the planted counts")


def markers(seed, k, n):
    rng = random.Random(seed)
    return [rand_seq(rng, k) for _ in range(n)]


def de_bruijn_pile(k, piece):
    """Every k-mer over ACGT at least once: the de Bruijn sequence B(4, k), cut into pieces that overlap by k - 1 bases."""
    a, seq = [0] * (4 * k), []

    def db(t, p):
        if t > k:
            if k % p == 0:
                seq.extend(a[1 : p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, 4):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    s = "".join("ACGT"[c] for c in seq)
    s += s[: k - 1]
    return [s[i : i + piece + k - 1] for i in range(0, len(s) - k + 1, piece)]


def poly_a_pile(seed, total):
    """Sequences of 30 unique bases, a run of A's and 30 more unique bases, the same flanks in all of them: a run of r A's holds r - 8 copies of A^9, and
    the runs are cut so that the pile holds exactly `total`.  The template's run is 30 long (a short template: tfit); the others' at most 190 (250 bases)."""
    rng = random.Random(seed)
    while True:
        head, tail = rand_seq(rng, 30), rand_seq(rng, 30)
        if "AAAA" not in head + tail and head[-1] != "A" and tail[0] != "A":
            break
    rest = total - 22
    runs = [190] * (rest // 182) + ([rest % 182 + 8] if rest % 182 else [])
    return [head + "A" * 30 + tail] + [head + "A" * r + tail for r in runs]


def exact_kmers_pile(seed, k, kmers, per=136):
    """A noisy pile (substitutions only) of exactly `kmers` k-mers: sequences of `per` k-mers each and a last, shorter one."""
    rng = random.Random(seed)
    truth = rand_seq(rng, per + k - 1)
    pile = [truth] + [substitute(rng, truth, 0.08) for _ in range(kmers // per - 1)]
    if kmers % per:
        pile.append(substitute(rng, truth[: kmers % per + k - 1], 0.08))
    return pile


def distinct_kmers_pile(seed, k, distinct, length=250):
    """Unrelated random sequences holding exactly `distinct` different k-mers: whole sequences, then the last one cut base by base."""
    rng = random.Random(seed)
    seen, pile = set(), []
    while len(seen) < distinct:
        s = rand_seq(rng, length)
        cut = length
        for i in range(length - k + 1):
            seen.add(s[i : i + k])
            if len(seen) == distinct:
                cut = i + k
                break
        pile.append(s[:cut])
    return pile


def several_truths_pile(seed, n_truths, copies, length, tpl_len):
    """`copies` exact copies of each of `n_truths` unrelated sequences behind a short template: every k-mer of every truth occurs `copies` times or more."""
    rng = random.Random(seed)
    truths = [rand_seq(rng, length) for _ in range(n_truths)]
    return [truths[0][:tpl_len]] + [t for t in truths for _ in range(copies)]


# ---- the catalogue ------------------------------------------------------------------------------------------------------------------------
class Probe:
    def __init__(self, name, prm, route, build, **designed):
        self.name, self.prm, self.build, self.designed = name, prm, build, designed
        self.route = 0
        for n in route.split():
            self.route |= INDEX_ROUTE[n]
        self._hb = None

    @property
    def hb(self):
        if self._hb is None:
            self._hb = pack(self.build())
        return self._hb

    def __repr__(self):
        return self.name


def catalogue():
    P = []
    tail = "tfit use_bits"  # every probe: a short template and at most a few hundred sequences

    def add(name, prm, route, build, **designed):
        P.append(Probe(name, prm, route + " " + tail, build, **designed))

    # small k: 4^k / 4 words of byte counters are no multiple of 4096, so the byte path declines; no masks below k = 8.  Twelve sequences of 120 bases
    for k in (2, 3, 4):
        for solid in (1, 4):
            add(f"k={k} solid={solid}", (k, solid, 8, 2, 12), "staged nibbles export_walk", lambda k=k: noisy_pile(200 + k, 12, 120), n_seqs=12, per_thread=(8, 8, None))
    add("k=5 walk export", (5, 2, 8, 2, 12), "staged nibbles export_walk", lambda: noisy_pile(205, 30, 150), n_seqs=30, per_thread=(8, 8, None))
    # k = 6: 512 words, a thread owns one word of eight keys; all 4096 keys present fills every thread's CW_EXP_SLOTS = 8 slots and not one more
    add("k=6 every key, eight per thread", (6, 1, 8, 2, 12), "staged nibbles export_walk", lambda: de_bruijn_pile(6, 300), n_seqs=14, kmers=4096, distinct_solid=4096, per_thread=(8, 8, 8))
    # k = 7: 2048 words, two per thread, sixteen keys: 210 unrelated sequences (N > 200: no byte path) hold three keys in four -- more than eight a thread
    add("k=7 more than eight keys per thread", (7, 1, 8, 2, 12), "nibbles export_walk rewalk",
        lambda: [rand_seq(random.Random(7000 + i), 120) for i in range(210)], n_seqs=210, kmers=210 * 114, distinct_solid_min=9 * 1024, per_thread=(16, None, 9))
    # CW_IDX_BYTES_MIN_N = 64: k = 9 counts in nibbles below it, k = 7 and 8 in bytes on both sides
    for n in (63, 64):
        for k in (7, 8, 9):
            route = "staged nibbles export_masks" if (k == 9 and n == 63) else "staged bytes_done"
            add(f"k={k} N={n}", (k, 4, 8, 2, 20), route, lambda k=k, n=n: noisy_pile(6300 + k, n, 120), n_seqs=n)
    # CW_IDX_STAGE_N = 192 and the byte path's N <= 200, k = 9
    for n, route in ((192, "staged bytes_done"), (193, "bytes_done"), (200, "bytes_done"), (201, "nibbles export_masks")):
        add(f"k=9 N={n}", (9, 4, 8, 2, 20), route, lambda n=n: noisy_pile(1900 + n, n, 120), n_seqs=n)
    # solid thresholds at k = 9, 150 sequences: keys planted at solid - 1, solid and solid + 1 occurrences.  `past 255`: one more key planted 300 times sends
    # the window from the byte counters to the nibbles, where solid <= 15 exports by masks and solid >= 16 by the walk.  The 300 copies are followed by
    # random bases: the sixteen k-mers `marker[2:] + xy` are neighbours in the key space and occur ~19 times each, so with solid 16 or 17 one thread of the
    # walk (256 keys at k = 9) holds more than eight solid keys and walks again; solid 128 leaves two solid keys in all
    for solid, past255, route, per in ((15, True, "staged nibbles export_masks", None), (16, True, "staged nibbles export_walk rewalk", (256, None, 9)),
                                       (17, True, "staged nibbles export_walk rewalk", (256, None, 9)), (16, False, "staged bytes_done", None),
                                       (127, False, "staged bytes_done", None), (128, False, "staged nibbles export_walk", (256, 8, None))):
        m = markers(900 + solid, 9, 4)
        plan = {m[0]: solid - 1, m[1]: solid, m[2]: solid + 1}
        if past255:
            plan[m[3]] = 300
        add(f"k=9 solid={solid}{' past 255' if past255 else ''}", (9, solid, 8, 2, 20), route, lambda s=solid, plan=plan: planted_pile(1500 + s, 150, 200, plan), n_seqs=150, markers=plan,
            **({"per_thread": per} if per else {}))
    # "exactly 15 occurrences leave no entry" in the exact table; the sixteenth does
    m = markers(77, 9, 3)
    plan = {m[0]: 15, m[1]: 16, m[2]: 300}
    add("k=9 fifteen and sixteen occurrences in nibbles", (9, 4, 8, 2, 20), "staged nibbles export_masks", lambda plan=plan: planted_pile(1515, 150, 200, plan), n_seqs=150, markers=plan)
    # poly-A: A^9 exactly 2^14 - 1 / 2^14 times (a count that no longer packs beside its key: the walk's `wide` re-walk) and 2^16 - 1 / 2^16 times (the
    # finish kernel cannot stage the counts as 16-bit).  91 sequences are staged and tried in bytes first; 361 are neither
    for total, n, route in ((16383, 91, "staged nibbles export_walk"), (16384, 91, "staged nibbles export_walk rewalk"),
                            (65535, 361, "nibbles export_walk rewalk"), (65536, 361, "nibbles export_walk rewalk")):
        add(f"poly-A {total}", (9, 16, 8, 2, 6), route, lambda t=total: poly_a_pile(4100, t), n_seqs=n, markers={"A" * 9: total}, per_thread=(256, 8, None))
    # more than CW_EX_SLOTS = 1024 keys at fifteen occurrences or more: 51 copies of four unrelated 300-base sequences, ~1130 different 7-mers
    add("k=7 more saturated keys than the LDS exact table", (7, 4, 8, 2, 6), "nibbles big_ex export_walk", lambda: several_truths_pile(5100, 4, 51, 300, 150),
        n_seqs=205, kmers=144 + 204 * 294, distinct_solid_min=1100, per_thread=(16, 8, None))
    # the hash table: one pass up to 8192 k-mers, two from 8193 on
    for k in (10, 12, 14, 15, 16):
        for kmers, route in ((8192, "staged hashed"), (8193, "staged hashed hash_passes")):
            add(f"k={k} {kmers} k-mers", (k, 3, 8, 2, 12), route, lambda k=k, kmers=kmers: exact_kmers_pile(8100 + k, k, kmers), n_seqs=61, kmers=kmers)
    # the sort of the hashed solid set: 16384 keys in LDS, 16385 in the work-group's global table (three passes either way)
    for distinct, route in ((16384, "staged hashed hash_passes"), (16385, "staged hashed hash_passes hash_gsort")):
        add(f"k=13 solid=1 {distinct} keys", (13, 1, 8, 2, 12), route, lambda d=distinct: distinct_kmers_pile(1300, 13, d), distinct_solid=distinct)
    return P


PROBES = catalogue()


def check_designed(probe, keys, counts, n_kmers):
    """The probe is what the catalogue says it is (numpy side only): a probe that misses its edge fails here, on the CPU."""
    d = probe.designed
    hb = probe.hb
    if "n_seqs" in d:
        assert len(hb.seq_len) == d["n_seqs"], (probe, len(hb.seq_len))
    if "kmers" in d:
        assert n_kmers == d["kmers"], (probe, n_kmers)
    by_key = dict(zip((int(x) for x in keys), (int(x) for x in counts)))
    for kmer, occ in d.get("markers", {}).items():
        assert by_key.get(str2num(kmer), 0) == (occ if occ >= probe.prm[1] else 0), (probe, kmer, occ, by_key.get(str2num(kmer), 0))
        assert count_of(hb.pile(0), kmer) == occ, (probe, kmer, occ)
    if "distinct_solid" in d:
        assert len(keys) == d["distinct_solid"], (probe, len(keys))
    if "distinct_solid_min" in d:
        assert len(keys) >= d["distinct_solid_min"], (probe, len(keys))
    assert ("per_thread" in d) == bool(probe.route & INDEX_ROUTE["export_walk"]), probe
    if "per_thread" in d:
        owns, at_most, at_least = d["per_thread"]
        fullest = int(np.bincount((keys // np.uint64(owns)).astype(np.int64)).max())
        assert (at_most is None or fullest <= at_most) and (at_least is None or fullest >= at_least), (probe, fullest)
        counted_wide = bool(len(counts) and counts.max() >= 1 << 14)
        assert bool(probe.route & INDEX_ROUTE["rewalk"]) == ((at_least or 0) > 8 or counted_wide), probe  # CW_EXP_SLOTS = 8


# ---- asking the test-aid library for a route ----------------------------------------------------------------------------------------------
@contextlib.contextmanager
def aids_engine(*prm, configure=None):
    """An Engine of the -DCW_TEST_AIDS library (the only build that writes the route witness), for tests whose other engines are the product's:
    what the `aids` fixture of conftest.py does, for the length of a `with`."""
    prev = engine.use_library(engine.AIDS_LIB)
    e = None
    try:
        e = ca.Engine(ca.Params(*prm))
        if configure:
            e.configure(configure)
        yield e
    finally:
        if e is not None:
            e.close()
        engine._LIB = prev


def route_alone(e, hb, w=0):
    """Window w of hb run alone on e (a test-aid engine): (results, route bits of that window)."""
    one = hb.slice(w, w + 1)
    res = e.run(one)
    return res, e.index_route()


def assert_route(route, has="", lacks="", what=""):
    for n in has.split():
        assert route & INDEX_ROUTE[n], f"{what}: route {route_names(route)} lacks {n}"
    for n in lacks.split():
        assert not route & INDEX_ROUTE[n], f"{what}: route {route_names(route)} has {n}"
