"""The probe catalogue of the chain kernel (consent_amd/csrc/cw_chain.h: anchor chaining and segmentation), shared by tests/test_chain_ref_cpu.py and
tests/test_gpu_chain.py, and the plain Python / numpy reference for what that kernel writes: which anchors form a window's chain and how every
sequence is cut into segments.  The reference works from the pile's strings alone -- no call into the library or the oracle (oracle/cw_oracle.cpp
A4a-A4c, which it restates; the CPU test holds the two together).

The reference (reference(pile, prm)):
  anchors   template k-mers, in template order, repeated in no sequence of the pile, held by at least sup = min(common_kmers, N // 2) sequences;
            P[a][s] = position of anchor a in sequence s, -1 when absent
  chain     score(a, b) = #{s : P[a][s] != -1, P[b][s] != -1, P[a][s] < P[b][s]}; a link iff score >= sup; a = A-1 .. 0: the longer chain wins, then
            the higher score, then the smallest successor (tie="largest": the largest); the start is the longest, then best scored, then largest
            index; an anchor without a link starts no chain
  segments  m + 1 of them; members (sequence, start, length) among the first max_msa sequences with a non-empty piece; classes as the kernel tells
            them apart: `empty`, `by_anchor` (an inner segment, all pieces equally long and no longer than k), `single` (one member), `task`
  sequences clean or dirty (the positions of the anchors a sequence holds are not strictly increasing in anchor order); rows = anchors that are "bad"
            in some dirty sequence in its chosen direction (forward unless the backward scan has strictly fewer bad anchors; cw_index.h
            idx_classify_sequences)
  early stop far_step: some step of the recurrence had to look at successors beyond a + 64 under the kernel's rule (the best link among a+1 .. a+64
            does not beat smax[a + 65], the longest chain from any later anchor); far_link: a link of the chain goes beyond a + 64

A probe is one window, alone in its batch, aimed at one edge.  It carries prm = (k, solid, common_kmers, min_anchors, max_msa), its designed numbers
(asserted from the reference on the CPU) and its route: the CHAIN_ROUTE bits (consent_amd/engine.py) it must set in the test-aid library, and the
four counters of the product's profile -- written down by hand from these constants of cw_chain.h and cw_index.h:

  slab      CW_CH_SLAB = 20480 bytes of LDS per wave (CW_CH_SLAB_LONG = 32768 in an engine configured for templates beyond 1024 + k - 1 bases:
            `long_slab`), of which the last CW_CH_LIST_BYTES = 1792 are phase D's queue: 18688 (30976) usable
  DP arrays 12 bytes per anchor: off_csc = (8 A + 5) & ~3, off_var = (off_csc + 4 A + 7) & ~7; room = usable - off_var
  presence  A * Nw * 8 bytes, Nw = ceil(N / 64); `pres_lds` iff the index kernel made bitsets (use_bits: N <= 2048) and they fit the room
  rows      row ids Ap = (A + 15) & ~15 bytes and n_rows * Ap bytes of rows behind the presence bits: `rows_lds` iff all of it fits the room,
            `rows_far` iff only presence + Ap does
  fast      pres_lds, Nw <= 4 and (no dirty sequence, or rows_lds, or rows_far); everything else is in place (counter `slow`)
  in place  use_bits: rows in the block (`inplace_rows`), else one-word masks (`inplace_masks`), else `inplace_all_dirty` (also what a pile
            without dirty sequences takes: the loop over none of them); no bitsets: `inplace_matrix`
  index     the index kernel keeps matrix, presence bits, dirty list, masks and row numbering in the 139776 - 32000 = 107776 bytes of LDS between its
            template arrays and the staged pile (92416 for a template of more than 1024 k-mers): the matrix of nk0 template k-mers x Np u16 (Np = N
            rounded up to twice an odd number) when that, nk0 * Nw * 8 of presence and 2 N + 16 fit (tfit), else of the A anchors, else in global memory;
            behind it A * Nw * 8 of presence and 2 N of dirty list (use_bits iff N <= 2048 and these fit), then 32 A of masks, A row ids and 254 x 2 of
            row anchors, which must fit too for masks to exist;
            masks exist for 1 .. 255 dirty sequences, W = ceil(n_dirty / 64) words (at most 4; 1 beyond 1024 sequences); rows exist (counter `fix`,
            `rows` = their number) iff masks exist, 1 <= rows <= CW_AB_ROWS_MAX = 254 and the window's anchor block holds them: it is sized for an
            anchor per template k-mer, every sequence dirty and no rows (block_bytes below restates cw_ab_bytes), so the rows live on what the
            k-mers that are no anchors leave free; the chain kernel sees masks (counter `masks`) iff W = 1
  key       `wide_key` unless A * N < 2^21 and A < 2047
  flush     `early_flush`: rounds of 64 segments queue their tasks and long single pieces, and a round that would take the queue past 64 entries
            empties it first; `long_single`: a one-member segment of more than 16 bases (and not by_anchor)
arithmetic(ref, slab) below does these sums for the CPU test, which compares them with what is written in the catalogue; the index kernel's share of them
(`index` above, and where its matrix lies: tfit, pg, hit_list, wide) is index_arithmetic, which tests/anchor_ref.py and tests/anchor_probes.py use too.

Arithmetic of the probes whose placement is close (room = 18688 - off_var):
  dirty rows in LDS     A 200: off_var 2408, room 16280; presence 1600 + ids 208 + 55 rows x 208 = 13248: fits; block 32528 of 34672 bytes (332 template k-mers)
  dirty rows far        A 418: off_var 5024, room 13664; presence 3344 + ids 432 = 3776 fits, + 82 rows x 432 = 39200 does not; block 96144 of 99840
  presence in the block A 498, Nw 4: off_var 5984, room 12704 < presence 15936
  N = 257               A 112, Nw 5: presence 4480 fits 17336, but Nw > 4: in place
  A = 2046 / 2047       long slab: off_var 24560 / 24576 of 30976; presence 16368 / 16376 > room: in the block, in place; 2047 is the first wide key
Every probe ends not stopped."""
import random

import numpy as np

from consent_amd.engine import CHAIN_ROUTE, ab_layout, ab_np
from index_probes import mutate, pack, rand_seq, substitute

__all__ = ["PROBES", "reference", "arithmetic", "pack"]

# cw_chain.h's CW_CH_SLAB, CW_CH_SLAB_LONG, CW_CH_LIST_BYTES and CW_CH_TILE_STRIDE (tests/test_chain_ref_cpu.py holds them to the header)
CH_SLAB, CH_SLAB_LONG, CH_LIST_BYTES, CH_TILE_STRIDE = 20480, 32768, 1792, 66


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
class Ref:
    pass


def anchors(pile, k, common):
    """(sup, P): P[a][s], int32, -1 = absent; anchors in template order."""
    N = len(pile)
    sup = min(common, N // 2)
    where, repeated = {}, set()
    for s, r in enumerate(pile):
        seen = set()
        for i in range(len(r) - k + 1):
            w = r[i : i + k]
            if w in seen:
                repeated.add(w)
            seen.add(w)
            where.setdefault(w, []).append((s, i))
    tpl = [pile[0][i : i + k] for i in range(len(pile[0]) - k + 1)]
    tpl = [w for w in tpl if w not in repeated and len(where[w]) >= sup]
    P = np.full((len(tpl), N), -1, np.int32)
    for a, w in enumerate(tpl):
        for s, i in where[w]:
            P[a, s] = i
    return sup, P


def chain_of(P, sup, tie="smallest"):
    """(chain, far_step): the recurrence over all successors, plain; far_step says whether the kernel's early stop would have had to go on."""
    A = len(P)
    ln, sc, nx = np.zeros(A, np.int64), np.zeros(A, np.int64), np.full(A, -1, np.int64)
    smax = np.full(A + 1, -1, np.int64)
    held = P >= 0
    far_step = False
    for a in range(A - 1, -1, -1):
        if a + 1 < A:
            score = (held[a] & held[a + 1 :] & (P[a] < P[a + 1 :])).sum(axis=1)
            link = score >= sup
            if link.any():
                b = np.nonzero(link)[0]
                L, S = ln[a + 1 :][b], sc[a + 1 :][b] + score[b]
                b, S = b[L == L.max()], S[L == L.max()]
                b = b[S == S.max()]
                ln[a], sc[a], nx[a] = L.max() + 1, S.max(), a + 1 + (b.max() if tie == "largest" else b.min())
            if a + 65 < A:  # the kernel looks at a+1 .. a+64 first and goes on unless their best link is longer than anything from a+65 on
                near = link[:64]
                if not near.any() or not smax[a + 65] < ln[a + 1 : a + 65][near].max():
                    far_step = True
        smax[a] = max(smax[a + 1], ln[a])
    start, top = -1, (0, 0)
    for a in range(A - 1, -1, -1):
        if (ln[a], sc[a]) > top:
            top, start = (ln[a], sc[a]), a
    chain = []
    while start != -1:
        chain.append(int(start))
        start = nx[start]
    return chain, far_step


def classify(P, detail=False):
    """(dirty sequences, number of correction rows); detail: also {dirty sequence: "forward" | "backward"} and {dirty sequence: its bad anchors, ascending}.
    An anchor is bad in a dirty sequence when it sets no new record in the sequence's direction: forward unless the backward scan has strictly fewer bad
    anchors."""
    dirty, bad_anchors, direction, bad = [], set(), {}, {}
    for s in range(P.shape[1]):
        a_of = np.nonzero(P[:, s] >= 0)[0]
        pos = P[a_of, s].astype(np.int64)
        if len(pos) < 2:
            continue
        fwd = np.concatenate([[False], pos[1:] <= np.maximum.accumulate(pos)[:-1]])
        if not fwd.any():
            continue
        dirty.append(s)
        rev = -pos[::-1]
        bwd = np.concatenate([[False], rev[1:] <= np.maximum.accumulate(rev)[:-1]])[::-1]
        back = bwd.sum() < fwd.sum()
        direction[s] = "backward" if back else "forward"
        bad[s] = [int(a) for a in a_of[bwd if back else fwd]]
        bad_anchors.update(bad[s])
    return (dirty, len(bad_anchors), direction, bad) if detail else (dirty, len(bad_anchors))


def segments_of(pile, P, chain, k, max_msa):
    """[(class, members)], members = [(sequence, start, length)]."""
    m, out = len(chain), []
    for seg in range(m + 1 if m else 0):
        mem = []
        for s in range(len(pile)):
            if len(mem) >= max_msa:
                break
            if seg == 0:
                p1, p2 = 0, int(P[chain[0], s])
            elif seg == m:
                p1, p2 = int(P[chain[-1], s]), len(pile[s])
            else:
                p1, p2 = int(P[chain[seg - 1], s]), int(P[chain[seg], s])
            if p1 < 0 or p2 < 0 or p1 >= p2:
                continue
            mem.append((s, p1, p2 - p1))
        lens = {l for _, _, l in mem}
        cls = "empty" if not mem else "by_anchor" if 0 < seg < m and len(lens) == 1 and max(lens) <= k else "single" if len(mem) == 1 else "task"
        out.append((cls, mem))
    return out


def reference(pile, prm, tie="smallest"):
    k, _, common, min_anchors, max_msa = prm
    r = Ref()
    r.N = len(pile)
    r.sup, r.P = anchors(pile, k, common)
    r.A = len(r.P)
    r.template_kmers = max(len(pile[0]) - k + 1, 0)
    r.chain, r.far_step = chain_of(r.P, r.sup, tie)
    r.far_link = any(b > a + 64 for a, b in zip(r.chain, r.chain[1:]))
    r.skips = any(b > a + 1 for a, b in zip(r.chain, r.chain[1:]))
    r.dirty, r.rows = classify(r.P)
    r.has_chain = len(r.chain) >= max(min_anchors, 1)
    r.segments = segments_of(pile, r.P, r.chain, k, max_msa) if r.has_chain else []
    r.tasks = [(i, mem) for i, (cls, mem) in enumerate(r.segments) if cls == "task"]
    r.n_members = sum(len(mem) for _, mem in r.tasks)
    r.max_piece = max((l for _, mem in r.segments for _, _, l in mem), default=0)
    r.long_single = any(cls == "single" and mem[0][2] > 16 for cls, mem in r.segments)
    # phase D's queue: 64 segments a round, tasks and long single pieces wait for the whole wave; a round that would overfill the 64 entries empties them first
    r.early_flush, waiting = False, 0
    for r0 in range(0, len(r.segments), 64):
        new = sum(1 for cls, mem in r.segments[r0 : r0 + 64] if cls == "task" or (cls == "single" and mem[0][2] > 16))
        if waiting + new > 64:
            r.early_flush, waiting = True, 0
        waiting += new
    return r


def pieces(pile, members):
    return [pile[s][st : st + l] for s, st, l in members]


def block_bytes(A, N, n_dirty, n_rows):
    """cw_ab_bytes of cw_index.h: header, keys, presence, dirty list, one-word masks, and with rows the row ids and rows, then the matrix; all 16-byte aligned."""
    return ab_layout(A, N, n_dirty, n_rows)[-1]  # (consent_amd/engine.py restates cw_ab_carve; tests/test_anchor_ref_cpu.py holds it to the library's)


def slab_fits(A, slab=CH_SLAB):
    """cw_chain.h ch_fits: the DP arrays and what lies behind them, and phase D's tile of 65 rows with its 64 sequence lengths over csc, end in front of the queue."""
    off_csc = (8 * A + 5) & ~3
    return ((off_csc + 4 * A + 7) & ~7) <= slab - CH_LIST_BYTES and off_csc + 65 * CH_TILE_STRIDE * 2 + 4 + 256 <= slab - CH_LIST_BYTES


def index_room(nk0):
    """The index kernel's LDS between its template arrays and the staged pile: narrow layout, and wide for a template of more than 1024 k-mers."""
    return 139776 - (47360 if nk0 > 1024 else 32000)


def matrix_need(rows, N):
    """cw_index.h idx_matrix_need: matrix, presence bits and dirty list of `rows` rows."""
    return rows * ab_np(N) * 2 + rows * ((N + 63) // 64) * 8 + 2 * N + 16


def index_arithmetic(A, N, nd, nk0, rows):
    """What the index kernel's anchor phase decides for a window of A anchors among nk0 template k-mers, N sequences, nd dirty ones and `rows` anchors bad
    somewhere, by the sums of `index` in the module docstring: a dict of wide, tfit, pg, hit_list (idx_hit_list: the support pass writes the list),
    use_bits, n_dirty (what the block says: 0 without bitsets), W, masks (they exist), masks_count (the presence bits go by them: one word, or rows made of
    wider ones), one_word (the chain kernel sees them: the header's flag 2), fix (rows exist: flag 4), n_rows."""
    Nw, Np, lds = (N + 63) // 64, ab_np(N), index_room(nk0)
    tfit = matrix_need(nk0, N) <= lds
    pg = not tfit and matrix_need(A, N) > lds
    matrix = ((nk0 * Np + 3) & ~3) * 2 if tfit else ((A * Np + 3) & ~3) * 2 if not pg else 0
    lists_end = matrix + A * Nw * 8 + 2 * N
    use_bits = N <= 2048 and lists_end <= lds
    if not use_bits:
        nd = 0  # no classification without bitsets: the block says no dirty sequence
    W = max(1, (nd + 63) // 64)
    masks = 0 < nd <= 255 and W <= (4 if N <= 1024 else 1) and ((((lists_end + 7) & ~7) + 33 * A + 1) & ~1) + 508 <= lds
    fix = masks and 1 <= rows <= 254 and block_bytes(A, N, nd, rows) <= block_bytes(nk0, N, N, 0)
    return dict(wide=nk0 > 1024, tfit=tfit, pg=pg, hit_list=not tfit and N <= 1024, use_bits=use_bits, n_dirty=nd, W=W, masks=masks,
                masks_count=masks and (W == 1 or fix), one_word=masks and W == 1, fix=fix, n_rows=rows if fix else 0)


def arithmetic(ref, slab=CH_SLAB):
    """(route names, (fix, rows, masks, slow)) by the sums of the module docstring, from the reference's numbers."""
    A, N = ref.A, ref.N
    Nw = (N + 63) // 64
    ia = index_arithmetic(A, N, len(ref.dirty), ref.template_kmers, ref.rows)
    use_bits, nd, fix, n_rows, one_word = ia["use_bits"], ia["n_dirty"], ia["fix"], ia["n_rows"], ia["one_word"]
    off_csc = (8 * A + 5) & ~3
    room = slab - CH_LIST_BYTES - ((off_csc + 4 * A + 7) & ~7)
    Ap = (A + 15) & ~15
    pres = A * Nw * 8
    pres_lds = use_bits and pres <= room
    rows_lds = pres_lds and n_rows > 0 and pres + Ap + n_rows * Ap <= room
    rows_far = pres_lds and n_rows > 0 and not rows_lds and pres + Ap <= room
    fast = pres_lds and Nw <= 4 and (nd == 0 or rows_lds or rows_far)
    names = []
    if fast:
        names += ["fast"] + ["rows_lds"] * rows_lds + ["rows_far"] * rows_far
    elif A >= 2:  # (a lone anchor scores no pair)
        names.append("inplace_matrix" if not use_bits else "inplace_rows" if n_rows else "inplace_masks" if one_word else "inplace_all_dirty")
    names += ["pres_lds"] * pres_lds + ["wide_key"] * (not (A * N < 1 << 21 and A < 2047)) + ["far_scan"] * ref.far_step
    names += ["early_flush"] * ref.early_flush + ["long_single"] * ref.long_single + ["long_slab"] * (slab == CH_SLAB_LONG)
    return sorted(names), (int(fix), n_rows, int(one_word), int(not fast)), nd


# ---- pile builders ------------------------------------------------------------------------------------------------------------------------
def distinct(rng, n, k):
    """n random bases whose k-mers are all different."""
    while True:
        s = rand_seq(rng, n)
        if len({s[i : i + k] for i in range(n - k + 1)}) == n - k + 1:
            return s


def swapped(s, a, b, n):  # the stretches s[a:a+n] and s[b:b+n] exchanged
    return s[:a] + s[b : b + n] + s[a + n : b] + s[a : a + n] + s[b + n :]


def block_moved(s, a, b, n):  # the stretch s[a:a+n] taken out and put in again at b
    rest = s[:a] + s[a + n :]
    return rest[:b] + s[a : a + n] + rest[b:]


def clean_pile(seed, n, length, rate=0.02):
    rng = random.Random(seed)
    t = distinct(rng, length, 9)
    return [t] + [substitute(rng, t, rate) for _ in range(n - 1)]


def copies_pile(seed, n_anchors, k, copies):
    return [distinct(random.Random(seed), n_anchors + k - 1, k)] * copies


def short_second_pile(seed, n):
    """A template of 80 bases and n - 1 copies of its first 50: behind them the template alone supports an anchor."""
    t = distinct(random.Random(seed), 80, 9)
    return [t] + [t[:50]] * (n - 1)


def long_single_pile(seed):
    """N = 2, and in the part only the template holds a stretch of 26 bases twice: its 18 k-mers are repeated, no anchors, so the template's piece between
    the anchors around each copy is 19 bases long -- one member, more than the 16 bases a single lane writes."""
    rng = random.Random(seed)
    t, rep = distinct(rng, 60, 9), distinct(rng, 26, 9)
    tpl = t + rep + "ACGT" + rep + distinct(rng, 30, 9)
    return [tpl, tpl[:50]]


def gap_pile(seed, n_each, rate):
    """Half of the support holds the template's first and last third, the other half its middle: the chain links the thirds across ~100 anchors."""
    rng = random.Random(seed)
    t = rand_seq(rng, 300)
    sub = (lambda s: substitute(rng, s, rate)) if rate else (lambda s: s)
    return [t] + [sub(t[:100]) + sub(t[200:]) for _ in range(n_each[0])] + [sub(t[95:205]) for _ in range(n_each[1])]


def tie_pile(seed):
    r = random.Random(seed)
    t = rand_seq(r, 120)
    return [t] + [mutate(r, t[r.randrange(0, 30) : 120 - r.randrange(0, 30)], 0.12) for _ in range(r.randrange(3, 9))]


def max_msa_pile(seed):
    """Sequences 1-4 cover the first 60 bases only: behind them the first six sequences that hold a piece are not the pile's first six."""
    rng = random.Random(seed)
    t = distinct(rng, 150, 9)
    return [t] + [t[:60]] * 4 + [substitute(rng, t, 0.05) for _ in range(12)]


def dirty_pile(seed, length, n_clean, n_dirty, change, rate=0.03, tail=0):
    """n_clean noisy copies of a template and n_dirty of `change`(template), which puts stretches of it out of order.  `tail`: so many bases of a tandem
    repeat behind every sequence -- their k-mers are repeated, template k-mers that are no anchors: the room in the window's anchor block that the
    correction rows need (see `index` in the module docstring)."""
    rng = random.Random(seed)
    while True:
        t = distinct(rng, length, 9)
        if t[-1] != "T":  # (the k-mers across the end of the template proper must not continue the repeat)
            break
    end = ("ACGTT" * (tail // 5 + 1))[:tail]
    return [t + end] + [substitute(rng, t, rate) + end for _ in range(n_clean)] + [substitute(rng, change(t), rate) + end for _ in range(n_dirty)]


def sparse_anchor_pile(seed, periods, n):
    """Every support sequence differs from the template at every tenth base: the nine template k-mers that cover such a base are in the template alone, the
    tenth is an anchor, so the chain's anchors are ten bases apart and every segment between two of them -- longer than k -- is a POA task."""
    rng = random.Random(seed)
    while True:  # (4^9 k-mers are few: a changed k-mer must not be a template k-mer from elsewhere, which would be an anchor out of order)
        t = distinct(rng, 10 * periods + 9, 9)
        other = "".join("ACGT"[("ACGT".index(c) + 1) % 4] if i % 10 == 9 else c for i, c in enumerate(t))
        at = {t[i : i + 9]: i for i in range(len(t) - 8)}
        if all(at.get(other[i : i + 9], i) == i for i in range(len(t) - 8)):
            return [t] + [other] * (n - 1)


def deep_pile(seed, n):
    """n - 1 exact pieces of a 70-base template with ragged ends: beyond 2048 sequences the index kernel makes no presence bitsets."""
    rng = random.Random(seed)
    t = distinct(rng, 70, 7)
    return [t] + [t[rng.randrange(0, 12) : 70 - rng.randrange(0, 12)] for _ in range(n - 1)]


def region_pile(seed, depth, mid_len):
    """Two stretches every sequence shares around one variable region, as in tests/test_gpu_tier_q.py -- the region a tandem repeat of five bases, so that
    none of its k-mers is an anchor whatever its length: one POA task whose longest member (the template's) is mid_len - 7 bases, from the last k-mer
    that holds a base of the left stretch to the first that holds one of the right.  (A substitution inside the region can spell one of those two
    k-mers a second time, which takes it out of the anchors: the substitutions avoid the two bases next to the region, and the first seed from `seed`
    on whose task has the designed length is taken -- by the reference; the CPU test asserts it again.)"""
    unit = "ACGTT"
    mid = (unit * (mid_len // 5 + 1))[:mid_len]
    for attempt in range(64):
        rng = random.Random(seed + 10000 * attempt)
        while True:  # the k-mers across the region's two ends must not continue the repeat: they are the chain's anchors next to the region
            left, right = distinct(rng, 40, 9), distinct(rng, 40, 9)
            if left[-1] != unit[-1] and right[0] != unit[mid_len % 5]:
                break
        letters = [c for c in "ACGT" if c not in (left[-1], right[0])]
        pile = [left + mid + right]
        for _ in range(depth - 1):  # the others: substitutions and a deletion of up to three bases, both away from the region's ends
            m = mid[:9] + "".join(rng.choice(letters) if rng.random() < 0.03 else c for c in mid[9:-9]) + mid[-9:]
            cut = rng.randrange(0, 4)
            at = rng.randrange(9, mid_len - 9 - cut)
            pile.append(left + m[:at] + m[at + cut :] + right)
        if max((l for _, mem in reference(pile, SWEEP_PRM).tasks for _, _, l in mem), default=0) == mid_len - 7:
            return pile
    raise AssertionError("no seed gives the designed region")


# ---- the catalogue ------------------------------------------------------------------------------------------------------------------------
class Probe:
    def __init__(self, name, prm, route, counters, build, configure=None, use_bits=True, **designed):
        self.name, self.prm, self.build, self.configure, self.use_bits, self.designed = name, prm, build, configure, use_bits, designed
        self._route, self._counters = route, counters  # counters: (fix, rows, masks, slow), prof[50 .. 53]
        self._pile = self._hb = self._ref = None

    @property
    def route_names(self):
        return sorted(self._route.split()) if self._route is not None else arithmetic(self.ref, self.slab)[0]

    @property
    def route(self):
        return sum(CHAIN_ROUTE[n] for n in self.route_names)

    @property
    def counters(self):
        return self._counters if self._counters is not None else arithmetic(self.ref, self.slab)[1]

    @property
    def n_dirty(self):
        """What the block's header says (prof[43]): the reference's dirty sequences -- none without bitsets, where nothing classifies them."""
        return len(self.ref.dirty) if self.use_bits else 0

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
            self._ref = reference(self.pile, self.prm)
        return self._ref

    @property
    def slab(self):
        return CH_SLAB_LONG if self.configure else CH_SLAB

    def __repr__(self):
        return self.name


TIE_PRM = (7, 2, 3, 2, 5)
TIE_SEEDS = range(100, 164)
SWEEP_PRM = (9, 4, 8, 2, 150)
SWEEP_LENGTHS = (31, 32, 63, 64, 127, 128, 255, 256, 511, 512)  # CW_POAQ_LC, CW_POAH_LC, CW_POA_LC, CW_POAM1_LC, CW_POAM2_LC and one past each
SWEEP_DEPTHS = (6, 40)


def catalogue():
    P = []
    FAST, NONE = "fast pres_lds", (0, 0, 0, 0)
    SLOW = (0, 0, 0, 1)

    def add(name, prm, route, counters, build, **kw):
        P.append(Probe(name, prm, route, counters, build, **kw))

    std = (9, 2, 8, 2, 20)
    # presence words 1 .. 4 of the fast path and phase D's chunks of 64 sequences; 257 sequences are five words: in place, presence in LDS
    for n in (3, 64, 65, 128, 129, 192, 193, 256):
        add(f"clean N={n}", std, FAST, NONE, lambda n=n: clean_pile(300 + n, n, 120), N=n, A=112 if n != 65 else 111, n_dirty=0, chain=112 if n != 65 else 111)  # (N = 65: a substitution spells one template k-mer twice)
    add("clean N=257", std, "pres_lds inplace_all_dirty", SLOW, lambda: clean_pile(557, 257, 120), N=257, A=112, n_dirty=0, chain=112)
    # presence does not fit behind the DP arrays: in place, bits read from the block
    add("presence in the block", std, "inplace_all_dirty", SLOW, lambda: clean_pile(704, 200, 510, 0.01), N=200, A=498, n_dirty=0, chain=498)
    # the smallest piles
    solid1 = (9, 1, 8, 2, 20)
    add("N=1", solid1, FAST, NONE, lambda: short_second_pile(801, 1), N=1, A=72, n_dirty=0, chain=72, tasks=0)
    add("N=2", solid1, FAST, NONE, lambda: short_second_pile(802, 2), N=2, A=72, n_dirty=0, chain=72)
    add("N=3", solid1, FAST, NONE, lambda: short_second_pile(803, 3), N=3, A=72, n_dirty=0, chain=72)
    add("N=2 long single piece", solid1, FAST + " long_single", NONE, lambda: long_single_pile(804), N=2, n_dirty=0, long_single=True)
    # anchor counts around the 64-lane window and smax
    for a in (1, 2, 64, 65, 66, 128, 129):
        add(f"A={a}", std, FAST, NONE, lambda a=a: copies_pile(900 + a, a, 9, 5), N=5, A=a, n_dirty=0, chain=a if a > 1 else 0, tasks=1 if a > 1 else 0)
    # the early stop fails: a link across ~100 anchors
    add("gap", std, FAST + " far_scan", NONE, lambda: gap_pile(5, (6, 6), 0), N=13, n_dirty=0, far_step=True, far_link=True)
    add("gap noisy", std, FAST + " far_scan", NONE, lambda: gap_pile(8, (6, 6), 0.02), N=13, n_dirty=0, far_step=True, far_link=True)
    add("gap N=260", std, "pres_lds inplace_all_dirty far_scan", SLOW, lambda: gap_pile(7, (130, 129), 0), N=260, n_dirty=0, far_step=True, far_link=True)
    # more than 64 segments waiting for the whole wave: 71 tasks in a row, the second round of 64 segments finds the queue full
    add("more tasks than the queue holds", std, FAST + " early_flush", NONE, lambda: sparse_anchor_pile(950, 70, 13), N=13, A=71, n_dirty=0, chain=71, tasks=71, early_flush=True)
    # ties: 64 tiny noisy piles (the CPU test asserts how many of them end with a chain and how many chains skip an anchor).  Random piles aimed at no
    # placement: at k = 7 two in five have a dirty sequence or two -- with rows in LDS, or scored in place from one-word masks where the block has no room
    # for rows -- so their routes and counters are not written here but taken from arithmetic(); all have their presence bits in LDS
    for seed in TIE_SEEDS:
        add(f"tie {seed}", TIE_PRM, None, None, lambda seed=seed: tie_pile(seed))
    add("max_msa", (9, 2, 8, 2, 6), FAST, NONE, lambda: max_msa_pile(1000), N=17, n_dirty=0, cut_differs=True)
    # dirty sequences, each placement of the correction rows
    sw20 = lambda t: swapped(t, 40, 100, 20)
    # (every probe with rows has a tail of a tandem repeat behind its sequences: the rows live on the block room of template k-mers that are no anchors)
    add("dirty rows in LDS", std, FAST + " rows_lds", (1, 55, 1, 0), lambda: dirty_pile(1100, 200, 34, 5, sw20, tail=140), N=40, A=200, n_dirty=5, rows=55)
    add("dirty rows far", std, FAST + " rows_far", (1, 82, 1, 0), lambda: dirty_pile(1101, 420, 53, 6, lambda t: block_moved(t, 80, 300, 90), tail=280), N=60, A=418, n_dirty=6, rows=82)
    add("dirty rows in place", std, "pres_lds inplace_rows", (1, 44, 1, 1), lambda: dirty_pile(1102, 200, 254, 5, sw20, tail=30), N=260, A=200, n_dirty=5, rows=44)
    add("dirty masks without rows", (9, 2, 8, 2, 30), "pres_lds inplace_masks", (0, 0, 1, 1), lambda: dirty_pile(1103, 620, 13, 6, lambda t: t[310:] + t[:310], 0.02), N=20, A=611, n_dirty=6, rows_min=255)
    add("every dirty sequence", std, "pres_lds inplace_all_dirty", SLOW, lambda: dirty_pile(1104, 150, 9, 260, lambda t: swapped(t, 40, 90, 20)), N=270, A=133, n_dirty=260)
    near = lambda t: swapped(t, 40, 80, 20)
    for nd, a, rows in ((65, 150, 37), (129, 149, 36), (193, 150, 41)):
        add(f"masks of {(nd + 63) // 64} words", std, FAST + " rows_lds", (1, rows, 0, 0), lambda nd=nd: dirty_pile(1200 + nd, 150, 10, nd, near, 0.01, tail=60), N=11 + nd, A=a, n_dirty=nd, rows=rows, chain=a)
    # no presence bitsets
    add("N=2049", (7, 4, 8, 2, 20), "inplace_matrix", SLOW, lambda: deep_pile(1300, 2049), use_bits=False, N=2049, A=64, n_dirty=0, chain=64)
    # the fused 32-bit key and the 64-bit key, on the long instance
    for a in (2046, 2047):
        add(f"A={a} k=12", (12, 2, 8, 2, 20), "inplace_all_dirty long_slab" + (" wide_key" if a == 2047 else ""), SLOW, lambda a=a: copies_pile(1400, a, 12, 3), configure=2048 + 12 - 1,  # (the longest template cw_configure takes at k = 12)
            N=3, A=a, n_dirty=0, chain=a, tasks=1)
    # the routing rule's bounds: one region whose longest member crosses each of them, shallow and deep
    for depth in SWEEP_DEPTHS:
        for length in SWEEP_LENGTHS:
            add(f"region {length} depth {depth}", SWEEP_PRM, FAST, NONE, lambda d=depth, l=length: region_pile(1500 + l, d, l + 7), N=depth, n_dirty=0, longest_task=length)
    return P


PROBES = catalogue()


def check_designed(probe):
    """The probe is what the catalogue says it is, from the reference alone."""
    d, r = probe.designed, probe.ref
    for name, got in (("N", r.N), ("A", r.A), ("n_dirty", len(r.dirty)), ("chain", len(r.chain)), ("tasks", len(r.tasks)), ("rows", r.rows),
                      ("far_step", r.far_step), ("far_link", r.far_link), ("early_flush", r.early_flush), ("long_single", r.long_single)):
        if name in d:
            assert got == d[name], (probe, name, got, d[name])
    if "tasks_min" in d:
        assert len(r.tasks) >= d["tasks_min"], (probe, len(r.tasks))
    if "rows_min" in d:
        assert r.rows >= d["rows_min"], (probe, r.rows)
    if "longest_task" in d:
        assert [max(l for _, _, l in mem) for _, mem in r.tasks if max(l for _, _, l in mem) > 20] == [d["longest_task"]], (probe, [max(l for _, _, l in mem) for _, mem in r.tasks])
    if d.get("cut_differs"):  # in most segments the members are not the pile's first max_msa sequences
        n = sum(1 for cls, mem in r.segments if mem and [s for s, _, _ in mem] != list(range(len(mem))))
        assert n * 2 > len(r.segments), (probe, n, len(r.segments))
    assert r.has_chain or not r.chain or len(r.chain) < probe.prm[3]
