"""The plain reference of the pile extraction: getAlignmentWindowsSequences (alignmentWindows.cpp:87-149, the prose of include/consent_amd.h) restated over
Python strings and ints, with the reference's unsigned wrap written out where a value becomes a length or a count, the reverse complement by string reversal,
and a note for every overlap saying which way it went.  No ctypes, no oracle.  Test infrastructure only.

Oracle-row overlaps as tests/oracle_lib.py takes them: [q_len, q_start, q_end, strand, t_len, t_start, t_end, t_id], ends inclusive.

Notes of one overlap (a frozenset):
  no_span      the window neither begins nor ends inside the overlap's query span (:117, first half)
  t_gate       t_start + shift > t_end (:117, second half)
  dead         the arm of :119-123 (the overlap strictly inside the window) -- the span test excludes it: never seen
  left         :124-127, the overlap begins inside the window
  right        :128-130, the overlap ends inside the window
  inside       none of the three: the window lies inside the overlap
  throw_tbeg   :133 substr would throw (the slice begins beyond the target read): no member
  throw_shift  :138 substr would throw (the shift is longer than the slice): no member
  short        :141 the piece has fewer than k bases: no member
  clamp0       a target coordinate below 0 was clamped to 0
  clamp_end    a target coordinate beyond t_len - 1 was clamped to it
  substr_clamp the slice of :133 was cut by the read's end
"""
import numpy as np

U32 = 2 ** 32
U64 = 2 ** 64
_COMP = str.maketrans("ACGT", "TGCA")

ARMS = ("inside", "left", "right")
OUTCOMES = ("no_span", "t_gate", "throw_tbeg", "throw_shift", "short")
CLAMPS = ("clamp0", "clamp_end", "substr_clamp")
NOTES = ARMS + OUTCOMES + CLAMPS

# A kernel wrong in one decision, as a switch of the reference (tests/extract_probes.py MUTANT_CAUGHT_BY names the probe that catches each)
MUTANTS = ("span_ge_begin", "span_le_end", "gate_lt", "no_clamp0", "no_clamp_end", "keep_gt_k", "minus_unclamped_slice", "shift_before_revcomp")


class Throw(Exception):
    pass


def revcomp(s):
    return s[::-1].translate(_COMP)


def substr(s, pos, count):
    """std::string::substr(pos, count): throws for pos > size, clamps count at the end."""
    if pos > len(s):
        raise Throw
    return s[pos : pos + count]


def piece(al, target, q_beg, end, k, mut=()):
    """(piece or None, notes) of one overlap for the window [q_beg, end]."""
    _, q_start, q_end, strand, t_len, t_start, t_end_al, _ = (int(x) for x in al)
    notes = set()
    t_beg, t_end = t_start, t_end_al
    length = (end - q_beg + 1) % U32
    shift = q_beg - q_start if q_beg > q_start else 0                                    # :110-114
    begins = q_end >= q_beg if "span_ge_begin" in mut else q_end > q_beg
    ends = q_start <= end if "span_le_end" in mut else q_start < end
    if not ((q_start <= q_beg and begins) or (end <= q_end and ends)):                   # :117
        return None, frozenset({"no_span"})
    gate = (t_start + shift) % U32
    if not (gate < t_end_al if "gate_lt" in mut else gate <= t_end_al):
        return None, frozenset({"t_gate"})

    def at_least_0(v):
        if v < 0 and "no_clamp0" not in mut:
            notes.add("clamp0")
            return 0
        return v

    def at_most_last(v):
        if v > t_len - 1 and "no_clamp_end" not in mut:
            notes.add("clamp_end")
            return t_len - 1
        return v

    if q_beg < q_start and q_end < end:                                                  # :119-123
        notes.add("dead")
        shift = 0
        t_beg = at_least_0(t_start - (q_start - q_beg)) % U32
        t_end = at_most_last(t_end_al + (end - q_end)) % U32
        length = (t_end - t_beg + 1) % U32
    elif q_beg < q_start:                                                                # :124-127
        notes.add("left")
        shift = 0
        t_beg = at_least_0(t_start - (q_start - q_beg)) % U32
        length = min(length, at_most_last(t_beg + length - 1) - t_beg + 1) % U32
    elif q_end < end:                                                                    # :128-130
        notes.add("right")
        t_end = at_most_last(t_end_al + (end - q_end)) % U32
        length = min(length, t_end - at_least_0(t_end - length + 1) + 1) % U32
    else:
        notes.add("inside")
    count = (t_end - t_beg + 1) % U32
    try:
        seq = substr(target, t_beg, count)                                               # :133
    except Throw:
        return None, frozenset(notes | {"throw_tbeg"})
    if len(seq) < count:
        notes.add("substr_clamp")
        if strand and "minus_unclamped_slice" in mut:  # the '-' piece counted from the end of the slice as asked for, not as cut
            seq = seq + "A" * min(count - len(seq), 1 << 16)
    try:
        if strand and "shift_before_revcomp" in mut:
            seq = revcomp(substr(seq, shift, length))
        else:
            if strand:
                seq = revcomp(seq)                                                       # :134-136
            seq = substr(seq, shift, length)                                             # :138
    except Throw:
        return None, frozenset(notes | {"throw_shift"})
    if len(seq) > k if "keep_gt_k" in mut else len(seq) >= k:                            # :141
        return seq, frozenset(notes)
    return None, frozenset(notes | {"short"})


def window_pile(ovls, tpl, targets, q_beg, q_end, k, mut=()):
    """(pile, notes): the pile as a list of strings, template first, and one frozenset of notes per overlap ([] for a window beyond its template)."""
    length = (q_end - q_beg + 1) % U32
    if (q_beg + length - 1) % U32 >= len(tpl):                                           # :95-97
        return [], []
    pile, notes = [substr(tpl, q_beg, length)], []                                       # :100
    for al in ovls:
        p, n = piece(al, targets[int(al[7])], q_beg, q_end, k, mut)
        notes.append(n)
        if p is not None:
            pile.append(p)
    return pile, notes


_CODE = np.full(256, 3, np.uint32)
for _i, _c in enumerate("ACG"):
    _CODE[ord(_c)] = _i


def pack_words(s):
    """The 2-bit words of one sequence: A=0 C=1 G=2 anything else 3, sixteen bases a word, the first base in the top bits, zero padding."""
    codes = _CODE[np.frombuffer(s.encode("latin-1"), np.uint8)]
    padded = np.zeros((len(s) + 15) // 16 * 16, np.uint32)
    padded[: len(s)] = codes
    return (padded.reshape(-1, 16) << (30 - 2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)


def layout(piles):
    """A list of piles as one batch: (win_first_seq[n + 1] u32, seq_len u32, seq_word_off u64, words u32), sequences and words front to back."""
    wfs, lens, offs, words = [0], [], [], []
    n_words = 0
    for p in piles:
        for s in p:
            lens.append(len(s))
            offs.append(n_words)
            w = pack_words(s)
            words.append(w)
            n_words += len(w)
        wfs.append(len(lens))
    return (np.array(wfs, np.uint32), np.array(lens, np.uint32), np.array(offs, np.uint64),
            np.concatenate(words).astype(np.uint32) if words else np.zeros(0, np.uint32))
