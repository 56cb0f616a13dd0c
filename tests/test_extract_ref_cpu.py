"""CPU: the plain restatement of the pile extraction (tests/extract_ref.py) against the oracle (cwo_window_pile) and the reference's own alignmentWindows.cpp
(oracle/_ref, or the digests of its answers under tests/golden/) on every probe of tests/extract_probes.py and on the random overlaps of
tests/test_gpu_extract.py; every hand-written note against the reference's; the catalogue's cover of the notes; the arm that is never entered; and the
subtly wrong kernels (extract_ref.MUTANTS), each caught by a named probe.  Strings and integers: every comparison is exact."""
import random

import numpy as np
import pytest

import consent_amd as ca
import extract_probes as pb
import extract_ref as xr
import oracle_lib
from extract_probes import BY_NAME, CATALOGUE, ref_of


def compiled_inputs(rows, tpl, targets, q_beg, q_end):
    """A job as the compiled reference can take it.  getAlignmentWindowsSequences reads its template's name from the first overlap (alignments.begin()->qName,
    :95), so it cannot be called with none -- its driver never does.  A job without overlaps goes to it with one overlap of the template's first base alone
    (q 0..0), which no window of two or more bases spans: the template by itself, which is what a pile without overlaps is."""
    if rows:
        return rows, tpl, targets, q_beg, q_end
    assert q_end > q_beg
    return [[len(tpl), 0, 0, 0, 1, 0, 0, 0]], tpl, ["A"], q_beg, q_end


def compiled_reference(p):
    """The piles of a probe's jobs by the reference's own code (or the digest of them)."""
    assert not p.reference_throws
    jobs = [compiled_inputs(*p.job_inputs(j)) for j in range(len(p.jobs))]
    return oracle_lib.ref_answer(["extract_probe", p.name, p.reads, p.ovl, p.jobs, p.k],
                                 lambda r: [oracle_lib.window_pile(r.ref_window_pile, *inp, p.k) for inp in jobs])


@pytest.mark.parametrize("name", list(BY_NAME))
def test_probe(name):
    """The reference against the oracle and the compiled reference, and the probe's hand-written notes against the reference's."""
    p, ref = BY_NAME[name], ref_of(name)
    piles = [pile for pile, _ in ref]
    assert piles == [oracle_lib.window_pile(oracle_lib.oracle().cwo_window_pile, *p.job_inputs(j), p.k) for j in range(len(p.jobs))]
    if not p.reference_throws:  # (a C++ exception has no way out through ctypes)
        assert piles == compiled_reference(p)
        for j in range(len(p.jobs)):  # the stand-in overlap of compiled_inputs changes no pile
            assert xr.window_pile(*compiled_inputs(*p.job_inputs(j)), p.k)[0] == piles[j]
    for j, notes in p.notes.items():
        assert [set(n) for n in ref[j][1]] == [set(n) for n in notes], (j, ref[j][1], notes)
    assert p.kind == "launch" or set(p.notes) == set(range(len(p.jobs)))  # every job's notes are written down


def test_only_the_two_throw_probes_stay_away_from_the_compiled_reference():
    """A condition, not a measurement: test_probe hands every probe to the compiled reference but the two whose overlap lies beyond its read."""
    assert len(BY_NAME) == len(CATALOGUE)  # (test_probe goes by name)
    flagged = [p for p in CATALOGUE if p.reference_throws]
    assert [p.name for p in flagged] == ["t_start beyond the read: the reference throws (+)", "shift beyond the cut slice: the reference throws (-)"]
    for p, note in zip(flagged, ("throw_tbeg", "throw_shift")):
        (pile, notes), = ref_of(p.name)
        assert len(pile) == 1 and note in notes[0]
        (_, _, t_read, t_start, t_end, _), = p.ovl
        assert t_end >= len(p.reads[t_read])  # a coordinate beyond the read
    for p in CATALOGUE:
        if not p.reference_throws:
            assert not any(n & {"throw_tbeg", "throw_shift"} for _, notes in ref_of(p.name) for n in notes), p.name


def test_reference_equals_oracle_and_compiled_reference_on_random_overlaps():
    """The random piles of tests/test_gpu_extract.py."""
    from test_gpu_extract import build_case

    for seed, k in ((1, 9), (3, 15), (4, 7)):
        _, _, _, exp_in = build_case(seed)
        got = [xr.window_pile(fixed, tpl, targets, qb, qe, k)[0] for fixed, tpl, targets, qb, qe in exp_in]
        assert got == [oracle_lib.window_pile(oracle_lib.oracle().cwo_window_pile, fixed, tpl, targets, qb, qe, k) for fixed, tpl, targets, qb, qe in exp_in]
        assert got == oracle_lib.ref_answer(["extract_random", seed, k, [list(x) for x in exp_in]],
                                            lambda r: [oracle_lib.window_pile(r.ref_window_pile, fixed, tpl, targets, qb, qe, k) for fixed, tpl, targets, qb, qe in exp_in])
        assert sum(len(p) > 1 for p in got) > len(got) // 2


def test_the_layout_is_pack_piles():
    piles = [pile for name in ("inside: a piece of 17 bases (+)", "129 overlaps", "an empty pile between two full ones (-)", "inside: a window of 1025 bases (-)")
             for pile, _ in ref_of(name)]
    piles.append(["ACGTN", "GNRYCA-", "A" * 16, "T" * 33])  # anything but A, C, G packs as T (3)
    wfs, lens, offs, words = xr.layout(piles)
    hb = ca.pack_piles(piles)
    assert np.array_equal(wfs, hb.win_first_seq) and np.array_equal(lens, hb.seq_len) and np.array_equal(offs, hb.seq_word_off) and np.array_equal(words, hb.bases)
    assert wfs.dtype == np.uint32 and lens.dtype == np.uint32 and offs.dtype == np.uint64 and words.dtype == np.uint32
    assert xr.pack_words("C").tolist() == [1 << 30] and xr.pack_words("A" * 15 + "T" + "G").tolist() == [3, 2 << 30]


def test_the_catalogue_covers_every_note_on_both_strands():
    seen = {0: set(), 1: set()}
    hand = {0: set(), 1: set()}
    for p in CATALOGUE:
        for j, (_, notes) in enumerate(ref_of(p.name)):
            first = p.jobs[j][3]
            for i, n in enumerate(notes):
                seen[p.ovl[first + i][5]] |= n
                if j in p.notes:
                    hand[p.ovl[first + i][5]] |= p.notes[j][i]
    assert seen[0] | seen[1] == set(xr.NOTES) == hand[0] | hand[1]  # (`dead` is no note of xr.NOTES: it is never seen, below)
    for strand in (0, 1):
        assert set(xr.ARMS) | set(xr.CLAMPS) | {"no_span", "short"} <= seen[strand], strand


def test_the_dead_arm_is_never_entered_and_a_throw_needs_a_coordinate_beyond_the_read():
    """Every (q_start, q_end) around a 12-base window, with every target span of a 40-base read and some beyond it."""
    q_beg, end, t_len = 10, 21, 40
    tgt = pb.rand_seq("sweep/target", t_len)
    spans = [(ts, te) for ts in (0, 1, 5, 20, 38, 39, 40, 41, 60) for te in (0, 4, 12, 25, 38, 39, 40, 41, 70) if ts <= te]
    arms = set()
    for q_start in range(0, 36):
        for q_end in range(q_start, 36):
            # the arithmetic: the arm needs q_beg < q_start and q_end < end; the span test needs q_start <= q_beg or end <= q_end
            assert not ((q_beg < q_start and q_end < end) and ((q_start <= q_beg and q_end > q_beg) or (end <= q_end and q_start < end)))
            for ts, te in spans:
                for strand in (0, 1):
                    _, n = xr.piece([40, q_start, q_end, strand, t_len, ts, te, 0], tgt, q_beg, end, 3)
                    assert "dead" not in n
                    arms |= n
                    if n & {"throw_tbeg", "throw_shift"}:
                        assert ts >= t_len or te >= t_len, (q_start, q_end, ts, te)
                    if q_beg < q_start and q_end < end:
                        assert n == {"no_span"}
    assert set(xr.NOTES) <= arms


@pytest.mark.parametrize("mutant", list(pb.MUTANT_CAUGHT_BY))
def test_mutant_is_caught(mutant):
    """A kernel wrong in this one decision would fail the named probe: its pile differs from the reference's."""
    p = BY_NAME[pb.MUTANT_CAUGHT_BY[mutant]]
    good = [pile for pile, _ in ref_of(p.name)]
    bad = [xr.window_pile(*p.job_inputs(j), p.k, mut=(mutant,))[0] for j in range(len(p.jobs))]
    assert bad != good


def test_the_clamp_at_the_reads_last_base_changes_no_pile():
    """The one switch of extract_ref.MUTANTS that no probe can catch (tests/extract_probes.py EQUIVALENT_MUTANTS says why): leaving out the clamp at t_len - 1
    changes no pile of the catalogue and none of 20 000 random overlaps with target coordinates up to 60 beyond the read -- but it is seen in the notes."""
    assert set(pb.MUTANT_CAUGHT_BY) | set(pb.EQUIVALENT_MUTANTS) == set(xr.MUTANTS) and not set(pb.MUTANT_CAUGHT_BY) & set(pb.EQUIVALENT_MUTANTS)
    for p in CATALOGUE:
        if len(p.jobs) < 100:
            for j, (pile, _) in enumerate(ref_of(p.name)):
                assert xr.window_pile(*p.job_inputs(j), p.k, mut=("no_clamp_end",))[0] == pile, p.name
    rng = random.Random(11)
    noted = 0
    for _ in range(20000):
        t_len = rng.randrange(1, 90)
        tgt = pb.rand_seq(rng.random(), t_len)
        q_beg = rng.randrange(0, 40)
        end = q_beg + rng.randrange(1, 40)
        q_start = rng.randrange(0, 80)
        ts = rng.randrange(0, t_len + 60)
        al = [100, q_start, q_start + rng.randrange(0, 60), rng.randrange(2), t_len, ts, ts + rng.randrange(0, 80), 0]
        k = rng.choice([1, 9])
        good, bad = xr.piece(al, tgt, q_beg, end, k), xr.piece(al, tgt, q_beg, end, k, mut=("no_clamp_end",))
        assert good[0] == bad[0], al
        noted += "clamp_end" in good[1]
        assert "clamp_end" not in bad[1]
    assert noted > 1000
