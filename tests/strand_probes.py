"""The plain reference of the strand vote and the packed reverse complement (include/consent_amd.h cw_strand_run, cw_revcomp), and the probe catalogue the GPU
tests run: Python strings and sets only -- no GPU, no oracle.  A k-mer here is a substring; N is T, as the packing has it."""
import functools
import random

from poa_op_probes import ont_copy, rand_seq

FWD, REV, IS_REF, NONE = 0, 1, 2, 3  # CW_STRAND_*
K_DEFAULT, KMIN, KMAX = 11, 8, 15  # CW_STRAND_K, CW_STRAND_KMIN, CW_STRAND_KMAX
QMAX, RMAX, LDS_RMAX = 32768, 16383, 2048  # CW_SW_QMAX, CW_SW_RMAX; CW_ST_RMAX: the longest reference of the narrow launch class
KS = (8, 11, 15)  # the k the GPU tests run
CHUNK = 32  # cw_strand.h CW_STR_CHUNK: the queries of one unit of work behind a narrow table
_COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def votes(q, ref, k):
    """(forward hits, reverse hits): the positions of q whose k-mer is in the SET of ref's k-mers, and those whose k-mer's reverse complement is."""
    K = {ref[j : j + k] for j in range(len(ref) - k + 1)}
    fwd = rev = 0
    for i in range(len(q) - k + 1):
        w = q[i : i + k]
        fwd += w in K
        rev += revcomp(w) in K
    return fwd, rev


def votable(q, ref, k):
    return k <= len(q) <= QMAX and k <= len(ref) <= RMAX


def strand_of(q, ref, k):
    """(strand, forward hits, reverse hits) of a query: NONE with 0, 0 where no vote is possible, ties forward."""
    if not votable(q, ref, k):
        return NONE, 0, 0
    f, r = votes(q, ref, k)
    return (REV if r > f else FWD), f, r


def expected(groups, k):
    """Per sequence of the batch, in order: (strand, forward, reverse); a group's first sequence is its reference."""
    k = k or K_DEFAULT
    out = []
    for grp in groups:
        for i, s in enumerate(grp):
            out.append((IS_REF, 0, 0) if i == 0 else strand_of(s, grp[0], k))
    return out


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------------------------------------------

EDGE_LENS = (15, 16, 17, 31, 32, 33, 63, 64, 65, 640, 641)


def _kinds(rng, ref, n):
    """Three queries of n bases about `ref`: a noisy copy of a slice, the reverse complement of one, a random one (a slice is what the reference has)."""
    def piece():
        a = rng.randrange(0, max(1, len(ref) - n + 1))
        return ref[a : a + n]
    noisy = ont_copy(rng, piece() + rand_seq(rng, n), 0.05)[:n]
    return [noisy, revcomp(ont_copy(rng, piece() + rand_seq(rng, n), 0.05)[:n]), rand_seq(rng, n)]


@functools.lru_cache(maxsize=None)
def edge_groups(k):
    """Edges of k and of the packed words: a random 600-base reference and a 16-base one (one word), queries of k - 1, k, k + 1 and EDGE_LENS bases -- noisy
    copies of a slice, reverse complements of one, random ones -- an empty query, and a group of one sequence."""
    rng = random.Random(0x57A0 + k)
    ref = rand_seq(rng, 600)
    word = rand_seq(rng, 16)
    lens = (k - 1, k, k + 1) + EDGE_LENS
    g0 = [ref] + [q for n in lens for q in _kinds(rng, ref, n)] + [""]
    g1 = [word] + [q for n in lens for q in _kinds(rng, word, n)] + ["", word, revcomp(word)]
    return [g0, g1, [rand_seq(rng, 40)]]


@functools.lru_cache(maxsize=None)
def boundary_groups(k):
    """Class boundary and capacities: references of k - 1, k, 2 048, 2 049, 16 383 and 16 384 bases, each with a copy, a reverse complement and a random query of
    300 bases -- and on the 2 049-base one a query of 32 768 bases, which is voted, and one of 32 769, which is not."""
    rng = random.Random(0xB0DA + k)
    out = []
    for n in (k - 1, k, LDS_RMAX, LDS_RMAX + 1, RMAX, RMAX + 1):
        ref = rand_seq(rng, n)
        a = rng.randrange(0, max(1, n - 300 + 1))
        piece = (ref[a : a + 300] + rand_seq(rng, 300))[:300]  # (a reference shorter than 300 bases: all of it, then random bases)
        out.append([ref, piece, revcomp(piece), rand_seq(rng, 300)])
    long_q = rand_seq(rng, QMAX + 1)
    out[3] += [revcomp(out[3][0]) + long_q[: QMAX - LDS_RMAX - 1], long_q]
    return out


def set_groups(k):
    """Set semantics and ties: poly-A against poly-A and poly-T, a query that is its own reverse complement, and -- at k = 8 only, where 16 376 positions share
    65 536 possible k-mers -- a reference of 16 383 random bases: a table near its densest, with many duplicate k-mers."""
    rng = random.Random(0x5E75 + k)
    own = "ACGT" * 25
    out = [["A" * 200, "A" * 77, "T" * 77, own], [rand_seq(rng, 300) + own + rand_seq(rng, 300), own, "ACGT" * 4]]
    if k == 8:
        ref = rand_seq(rng, RMAX)
        out.append([ref, ref[5000:5300], revcomp(ref[9000:9300]), rand_seq(rng, 300)])
    return out


@functools.lru_cache(maxsize=None)
def spread_group():
    """One group of a 500-base reference and 300 short queries (40 to 120 bases): several chunks of CHUNK queries and a remainder."""
    rng = random.Random(0x5B4EAD)
    ref = rand_seq(rng, 500)
    qs = []
    for i in range(300):
        n = rng.randrange(40, 121)
        a = rng.randrange(0, len(ref) - n + 1)
        q = ont_copy(rng, ref[a : a + n + 20], 0.06)[:n] if i % 7 else rand_seq(rng, n)
        qs.append(revcomp(q) if i % 3 == 1 else q)
    assert 300 % CHUNK != 0 and 300 > 3 * CHUNK
    return [ref] + qs


def catalogue(k):
    """Every probe group of the tests at this k, by name."""
    return {"edges": edge_groups(k), "boundary": boundary_groups(k), "sets": set_groups(k), "spread": [spread_group()]}


# every length of up to 70 bases, around 512 -- and around the 1 024 bases (64 words) beyond which the work-group shares a sequence's words, and a long one
REVCOMP_LENS = tuple(range(0, 71)) + (511, 512, 513, 1023, 1024, 1025, 1041, 5003)


@functools.lru_cache(maxsize=None)
def revcomp_strings():
    rng = random.Random(0x2EC0)
    return tuple(rand_seq(rng, n) for n in REVCOMP_LENS)


def mixed_strands(group):
    """A group with its odd-numbered reads (members 1, 3, ..) reverse-complemented, and the strand value planted on every read."""
    out = [group[0]] + [revcomp(q) if m % 2 else q for m, q in enumerate(group[1:], 1)]
    return out, [REV if m % 2 else FWD for m in range(1, len(group))]
