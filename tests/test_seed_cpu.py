"""The seed run without a GPU (include/consent_amd.h cw_seed_run / cw_seed_run_device; Engine.seeds, place, polish_reads): the symbols, constants and the plan
exist, a missing engine and missing arguments are refused before the device is touched -- and the reference the GPU tests compare with (tests/seed_probes.py)
is held to its design: on planted reads it finds the strand and the start and leaves the other orientation far behind, its probes are the edges they are named
for, and the chance level that Engine.place's default min_hits doubles is measured here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import consent_amd as ca
import seed_probes as sp
import strand_probes as st
from consent_amd import engine as en
from consent_amd.engine import _ptr

E_INVALID = -1
KS = (8, 11, 15)
# (draft_and_reads arguments): drafts of 1 200 to 16 000 bases, reads of 300 to 5 000
PLANTED = (dict(seed=0x5D20, n=1200, reads=12, lo=300, hi=700), dict(seed=0x5D20, n=6000, reads=12, lo=300, hi=5000), dict(seed=0x5D20, n=16000, reads=10, lo=1000, hi=5000))
LONG = dict(seed=0x5D04, n=16000, reads=4, lo=12000, hi=12000)
TILE = 8192  # Engine.place's default


def header():
    return open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "consent_amd.h")).read()


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_header_declares_the_functions_the_struct_and_the_constants():
    text = header()
    assert re.search(r"int cw_seed_run_device\(cw_engine\* e, const cw_batch\* groups, const cw_seeds\* out, void\* hip_stream\);", text)
    assert re.search(r"int cw_seed_run\(cw_engine\* e, const cw_batch\* groups, const cw_seeds\* out\);", text)
    assert re.search(r"typedef struct cw_seeds \{\s*int32_t\*\s+rows;[^}]*uint8_t\*\s+strand;[^}]*uint32_t\s+k;[^}]*\} cw_seeds;", text)
    assert re.search(r"enum \{ CW_SEED_STATUS, CW_SEED_HITS, CW_SEED_DIAG, CW_SEED_OTHER, CW_SEED_ROW = 4 \};", text)
    assert re.search(r"#define CW_SEED_SHIFT\s+6u", text)
    assert "cw_seed_run / cw_seed_run_device" in text.split("#ifndef CONSENT_AMD_H")[0]  # the head comment's list of entry points
    assert "SHARE words" in text.split("typedef struct cw_batch")[0]  # what Engine.place relies on is stated where the layout is


def test_the_library_exports_them_and_the_binding_names_them():
    l = ca.load_library()
    for name in ("cw_seed_run", "cw_seed_run_device", "cw_debug_seed_plan"):
        assert hasattr(l, name), name
    assert (ca.SEED_STATUS, ca.SEED_HITS, ca.SEED_DIAG, ca.SEED_OTHER, ca.SEED_ROW) == (sp.STATUS, sp.HITS, sp.DIAG, sp.OTHER, sp.ROW) == (0, 1, 2, 3, 4)
    assert ca.SEED_SHIFT == sp.SHIFT == 6 and ca.SEED_SPAN == sp.SPAN == 128 and ca.SEED_MIN_HITS == sp.MIN_HITS
    assert [f[0] for f in ca.Seeds._fields_] == ["rows", "strand", "k"] and C.sizeof(ca.Seeds) == 24
    for name in ("seeds", "seed_device", "place", "polish_reads"):
        assert hasattr(ca.Engine, name), name
    assert ca.Polished("ACGT", []).placements == [] and ca.Placement(1, -5, 70, 2) == ca.Placement(1, -5, 70, 2) != ca.Placement(0, -5, 70, 2)
    assert issubclass(ca.SeedRows, ca.SwRows)
    assert en._revcomp("AACGTN") == "AACGTT" and all(en._revcomp(s) == st.revcomp(s) for s in st.revcomp_strings())


def test_null_arguments_are_refused_without_a_device():
    """Without a device there is no engine, so every entry point ends at its first check; nothing is written."""
    l = ca.load_library()
    hb = ca.pack_piles([["ACGTACGTACGTACGT", "ACGTACGTACGT"]])
    b = hb.c_struct()
    rows, strand = np.full(8, 77, np.int32), np.full(2, 77, np.uint8)
    for k in (0, 7, 11, 16):
        out = en.Seeds(_ptr(rows), _ptr(strand), k)
        assert l.cw_seed_run(None, C.byref(b), C.byref(out)) == E_INVALID
        assert l.cw_seed_run_device(None, C.byref(b), C.byref(out), None) == E_INVALID
    assert l.cw_seed_run(None, None, None) == E_INVALID and l.cw_seed_run_device(None, None, None, None) == E_INVALID
    assert (rows == 77).all() and (strand == 77).all()


def test_the_seed_plan_is_the_strand_plan_with_six_narrow_work_groups_a_cu():
    l = ca.load_library()
    out, ref = np.zeros(5, np.uint64), np.zeros(5, np.uint64)
    assert l.cw_debug_seed_plan(4, 8, 256, None) == E_INVALID and l.cw_debug_seed_plan(4, 8, 0, _ptr(out)) == E_INVALID
    for groups, seqs, cus in ((1, 1, 256), (1, 16385, 256), (4096, 69632, 256), (3, 301, 8), (65536, 1 << 22, 304)):
        assert l.cw_debug_seed_plan(groups, seqs, cus, _ptr(out)) == 0 and l.cw_debug_strand_plan(groups, seqs, cus, _ptr(ref)) == 0
        assert out[:3].tolist() == ref[:3].tolist() and int(out[4]) == int(ref[4])  # the same counters, units and wide grid
        assert int(out[3]) == max(1, min(groups + seqs // st.CHUNK, 6 * cus))  # 25 KB of LDS a work-group: six a CU


# ---- the reference: its edges --------------------------------------------------------------------------------------------------------------------------------------

def test_only_k_mers_at_one_position_seed():
    assert sp.unique_positions("ACGTACGTACG", 4) == {}  # ACGT, CGTA, GTAC, TACG: each twice
    assert sp.unique_positions("AAAACGTT", 4) == {"AAAA": 0, "AAAC": 1, "AACG": 2, "ACGT": 3, "CGTT": 4}
    for k in KS:
        twice, poly, halves, own = sp.seed_groups(k)[:4]
        m = len(twice[1])
        # present twice: no seed in the orientation that has it (the other one's k-mers are random: k = 8 finds a chance hit or two)
        assert not any(sp.windows(twice[1], twice[0], k)[sp.FWD]) and not any(sp.windows(twice[2], twice[0], k)[sp.REV]) and m == 60
        assert st.votes(twice[1], twice[0], k)[0] == m - k + 1  # (the strand vote, a set, counts them all)
        assert sp.seed_of(poly[1], poly[0], k) == (sp.FWD, 0, -77, 0) and sp.seed_of(poly[2], poly[0], k) == (sp.FWD, 0, -77, 0)  # though the strand vote counts 67
        assert st.votes(poly[1], poly[0], 11) == (67, 0)


def test_ties_go_forward_and_then_to_the_lowest_bin():
    for k in KS:
        _, _, halves, own = sp.seed_groups(k)[:4]
        ws = sp.windows(halves[1], halves[0], k)[sp.FWD]
        top = max(ws)
        at = [b for b, w in enumerate(ws) if w == top]
        assert top == 60 - k + 1 and len(at) >= 2 and at[-1] - at[0] > 2, (k, top, at)  # two far windows hold as many hits
        row = sp.seed_of(halves[1], halves[0], k)
        assert row[:3] == (sp.FWD, top, (at[0] << sp.SHIFT) - 120)
        wf, wr = sp.windows(own[1], own[0], k)
        assert own[1] == sp.revcomp(own[1]) and wf == wr and max(wf) == 80 - k + 1
        assert sp.seed_of(own[1], own[0], k)[0] == sp.FWD and sp.seed_of(own[1], own[0], k)[1] == sp.seed_of(own[1], own[0], k)[3]


def test_planted_diagonals_fall_on_both_sides_of_the_bin_edges():
    for k in KS:
        grp = sp.seed_groups(k)[4]
        m = sp.PLANTED_M
        for s, q in zip(sp.PLANTED_SUMS, grp[1:]):
            status, hits, diag, other = sp.seed_of(q, grp[0], k)
            lone = s >> sp.SHIFT  # the one bin of the hits: the window that holds it and begins lowest is the bin before (bin 0: itself)
            assert (status, hits) == (sp.FWD, m - k + 1) and diag == (max(lone - 1, 0) << sp.SHIFT) - m, (k, s, diag)
            assert diag <= s - m < diag + sp.SPAN  # (the planted diagonal s - m lies in the window)
        straddle, turned = grp[-2], grp[-1]
        half = 20 - k + 1  # a half's k-mers; those across the deleted base are nowhere
        assert sp.windows(straddle, grp[0], k)[sp.FWD][:3] == [half, 2 * half, half]  # the halves in bins 1 and 2: only window 1 holds both
        assert sp.seed_of(straddle, grp[0], k)[:3] == (sp.FWD, 2 * half, 64 - 40) and sp.seed_of(turned, grp[0], k)[:3] == (sp.REV, 2 * half, 64 - 40)


def test_reads_may_overhang_the_reference_and_be_longer_than_it():
    for k in KS:
        over, longer = sp.seed_groups(k)[5:7]
        start, end, turned = (sp.seed_of(q, over[0], k) for q in over[1:])
        assert start[:3] == (sp.FWD, 50 - k + 1, -80) and turned[:3] == (sp.REV, 50 - k + 1, -80)  # diagonal -30: d + m = 50, bin 0
        assert end[0] == sp.FWD and end[1] == 50 - k + 1 and end[2] <= 550 < end[2] + sp.SPAN
        big, rev = (sp.seed_of(q, longer[0], k) for q in longer[1:])
        assert big[:2] == (sp.FWD, 100 - k + 1) and big[2] <= -200 < big[2] + sp.SPAN and big[2] < 0
        assert rev[:2] == (sp.REV, 100 - k + 1) and rev[2] <= -150 < rev[2] + sp.SPAN  # turned, the read is 150 bases and then the reference
    assert sp.seed_of("ACGT", "ACGT" * 10, 8) == (sp.NONE, 0, 0, 0) and sp.seed_of("A" * 20, "A" * (st.RMAX + 1), 8) == (sp.NONE, 0, 0, 0)
    assert sp.seed_of("C" * 20, "A" * 20 + "ACGTTGCA", 8) == (sp.FWD, 0, -20, 0)  # no hit at all
    # (k = 11: the query is the reference's first 11-mer, and its reverse complement the second: a hit each, the tie goes forward)
    assert sp.expected([["ACGTACGTACGT", "ACGTACGTACG", ""], ["AC"]], 0) == [(sp.IS_REF, 0, 0, 0), (sp.FWD, 1, -11, 1), (sp.NONE, 0, 0, 0), (sp.IS_REF, 0, 0, 0)]


# ---- the reference: planted reads ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_planted_reads_are_found_with_their_strand_and_start(k):
    """Reads are ont_copy at 10 - 12 % of slices of a draft, every second one turned: the strand is right, the planted start lies in the window, and the
    window holds at least four times what the other orientation finds.  (The start inside the window is what these inputs have, not a theorem: a read's
    diagonal climbs by 12 per 1 000 bases, and of 1 020 reads made this way over 30 other seeds, 6 -- all longer than 3 400 bases, their start diagonal high in
    its bin -- begin 3 to 12 diagonals below their window.  DIAG is the densest window)"""
    least, most_other = 1 << 30, 0
    for spec in PLANTED:
        draft, reads, where, _ = sp.draft_and_reads(**spec)
        for q, (a, turned) in zip(reads, where):
            status, hits, diag, other = sp.seed_of(q, draft, k)
            least, most_other = min(least, hits), max(most_other, other)
            assert status == (sp.REV if turned else sp.FWD), (spec, a, status)
            assert diag <= a < diag + sp.SPAN, (spec, len(q), a, diag)
            assert hits >= 4 * other and (k < st.K_DEFAULT or hits >= sp.MIN_HITS), (spec, a, hits, other)  # (and the default threshold where it applies)
    print(f"k = {k}: planted reads of 300 to 5 000 bases: at least {least} hits, the other orientation at most {most_other}")


@pytest.mark.parametrize("k", KS)
def test_long_reads_drift_out_of_the_window_but_not_off_their_strand(k):
    """12 000 bases at 10 - 12 % lose 1.2 % more bases than they gain: the diagonal drifts by more than a window, DIAG is the densest part and not the start."""
    draft, reads, where, _ = sp.draft_and_reads(**LONG)
    for q, (a, turned) in zip(reads, where):
        status, hits, diag, other = sp.seed_of(q, draft, k)
        print(f"k = {k}: 12 000-base read planted at {a}: window at {diag}, {hits} hits against {other}")
        assert status == (sp.REV if turned else sp.FWD) and hits >= 4 * other and hits >= 2 * sp.MIN_HITS


def test_the_chance_level_behind_min_hits():
    """Unrelated pairs: the random reads of the planted inputs (300 to 5 000 bases) against every tile of Engine.place's default 8 192 bases of the drafts, and
    one pair at the capacities (32 768 random bases against 16 383).  The largest HITS over them at the default k = 11, doubled, is the default min_hits; a
    random k-mer is four times rarer with every base of k, so the level holds for every k from 11 up, and below 11 Engine.place asks for a min_hits."""
    import random

    rng = random.Random(0xC4A2CE)
    pairs = [(sp.rand_seq(rng, st.QMAX), sp.rand_seq(rng, st.RMAX))]
    for spec in PLANTED:
        draft, _, _, other = sp.draft_and_reads(**spec)
        pairs += [(q, tile) for _, tile in sp.tiles_of(draft, TILE) for q in other]
    worst = {k: max(sp.seed_of(q, tile, k)[sp.HITS] for q, tile in pairs) for k in KS}
    for k in KS:
        print(f"k = {k}: the largest HITS of {len(pairs)} unrelated pairs is {worst[k]}")
    assert worst[15] <= worst[11] <= worst[8]
    assert 2 * worst[st.K_DEFAULT] == sp.MIN_HITS == ca.SEED_MIN_HITS and ca.SEED_MIN_K == st.K_DEFAULT


def test_the_reference_places_reads_over_tiles_and_builds_the_polish_groups():
    draft, reads, where, other = sp.draft_and_reads(**sp.CONTIG)
    for tile in (1000, 2100):
        bag = list(reads) + [other[0]]
        placed = sp.place(draft, bag, tile, 0)
        assert placed[-1] is None and all(p is not None for p in placed[:-1])  # the unrelated read is nowhere
        for q, (a, turned), p in zip(reads, where, placed):
            assert p[0] == (sp.REV if turned else sp.FWD) and p[1] <= a + len(q) and a < p[1] + len(q) + sp.SPAN  # (the best tile's window is on the read)
        groups = sp.polish_groups(draft, bag, tile, 0)
        assert [g[0] for g in groups] == [t for _, t in sp.tiles_of(draft, tile)] and "".join(g[0] for g in groups) == draft
        used = {q for g in groups for q in g[1:]}
        assert all((sp.revcomp(q) if turned else q) in used for q, (_, turned) in zip(reads, where)) and other[0] not in used
        assert max(len(g) for g in groups) < len(bag) + 1  # no tile takes every read: the bag is sorted onto its regions
