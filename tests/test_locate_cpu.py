"""The locate run without a GPU (include/consent_amd.h cw_locate_*; Engine.locate_index, locate_rows, locate, polish_reads(index=True)): the symbols, constants
and the plan exist, the table's size is what the header says, a missing engine is refused before the device is touched -- and the reference the GPU tests compare
with (tests/locate_probes.py) agrees with the seed run's on every reference the seed run takes, finds its planted reads, and the chance level that
Engine.locate's default min_hits doubles is measured here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import consent_amd as ca
import locate_probes as lp
import seed_probes as sd
import strand_probes as st
from consent_amd import engine as en
from consent_amd.engine import _ptr

E_INVALID = -1
KS = (8, 11, 15)


def header():
    return open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "consent_amd.h")).read()


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_header_declares_the_functions_the_struct_and_the_constants():
    text = header()
    assert "uint64_t cw_locate_table_words(uint64_t ref_len);" in text
    assert "int cw_locate_build_device(cw_engine* e, const cw_locate_ref* ref, void* hip_stream);" in text
    assert "int cw_locate_run_device(cw_engine* e, const cw_locate_ref* ref, const cw_batch* reads, const cw_seeds* out, void* hip_stream);" in text
    assert "int cw_locate_run(cw_engine* e, const uint32_t* ref_bases, uint64_t ref_len, uint32_t k, const cw_batch* reads, const cw_seeds* out);" in text
    assert re.search(r"typedef struct cw_locate_ref \{\s*const uint32_t\*\s+bases;[^}]*uint64_t\s+len;[^}]*uint32_t\*\s+table;[^}]*uint32_t\s+k;[^}]*\} cw_locate_ref;", text)
    assert re.search(r"#define CW_LOCATE_K\s+15u", text) and re.search(r"#define CW_LOCATE_RMAX\s+\(\(1u << 28\) - 1u\)", text)
    assert "cw_locate_build_device, cw_locate_run_device / cw_locate_run" in text.split("#ifndef CONSENT_AMD_H")[0]  # the head comment's list of entry points
    assert "unique in its TILE" in text  # the difference from the tiled seed run is stated


def test_the_library_exports_them_and_the_binding_names_them():
    l = ca.load_library()
    for name in ("cw_locate_table_words", "cw_locate_build_device", "cw_locate_run_device", "cw_locate_run", "cw_debug_locate_plan", "cw_debug_locate_routes"):
        assert hasattr(l, name), name
    assert (ca.LOCATE_K, ca.LOCATE_RMAX) == (lp.K_DEFAULT, lp.RMAX) == (15, (1 << 28) - 1)
    assert ca.LOCATE_MIN_HITS == lp.MIN_HITS and ca.LOCATE_MIN_K == lp.K_DEFAULT
    assert [f[0] for f in ca.LocateRef._fields_] == ["bases", "len", "table", "k"] and C.sizeof(ca.LocateRef) == 32
    for name in ("locate_index", "locate_rows", "locate_device", "locate_routes", "locate"):
        assert hasattr(ca.Engine, name), name
    import inspect

    assert inspect.signature(ca.Engine.polish_reads).parameters["index"].default is False
    assert inspect.signature(ca.Engine.locate).parameters["min_hits"].default is None


def test_a_missing_engine_is_refused_without_a_device():
    l = ca.load_library()
    hb = ca.pack_piles([["ACGTACGTACGTACGTACGT"]])
    b = hb.c_struct()
    rows, strand, table = np.full(4, 77, np.int32), np.full(1, 77, np.uint8), np.full(1024, 77, np.uint32)
    ref = en.LocateRef(_ptr(hb.bases), 20, _ptr(table), 0)
    out = en.Seeds(_ptr(rows), _ptr(strand), 0)
    assert l.cw_locate_build_device(None, C.byref(ref), None) == E_INVALID
    assert l.cw_locate_run_device(None, C.byref(ref), C.byref(b), C.byref(out), None) == E_INVALID
    assert l.cw_locate_run(None, _ptr(hb.bases), 20, 0, C.byref(b), C.byref(out)) == E_INVALID
    assert l.cw_debug_locate_routes(None, _ptr(table)) == E_INVALID
    assert (rows == 77).all() and (strand == 77).all() and (table == 77).all()


def test_the_table_is_a_power_of_two_of_at_least_twice_the_positions():
    words = ca.load_library().cw_locate_table_words
    assert words(0) == words(1) == 1024 == words(512) and words(513) == 2048  # the floor, and the first size above it
    for p in (1 << 12, 1 << 16, 1 << 20, 1 << 27):
        assert words(p - 1) == 2 * p and words(p) == 2 * p and words(p + 1) == 4 * p, p
    assert words(lp.RMAX) == 1 << 29 and words(lp.RMAX + 1) == 0 and words(1 << 40) == 0
    for n in (0, 1, 777, 70000, 1000000, 4600000, lp.RMAX):
        w = words(n)
        assert w & (w - 1) == 0 and w >= 2 * n and w >= 1024 and (w == 1024 or w < 4 * n), n


def test_the_locate_plan_is_its_arithmetic():
    l = ca.load_library()
    out = np.zeros(6, np.uint64)
    assert l.cw_debug_locate_plan(8, 256, None) == E_INVALID and l.cw_debug_locate_plan(8, 0, _ptr(out)) == E_INVALID
    up = lambda v: (v + 255) // 256 * 256
    dense_words = (1 << 17) + (1 << 16)  # a dense table: 4 x CW_SW_QMAX keys, and their 16-bit counts two to a word
    assert 4 * st.QMAX == 1 << 17
    for seqs, cus in ((1, 256), (63, 256), (64, 256), (65, 256), (1535, 256), (1536, 256), (1537, 256), (17250, 256), (5, 8), (1 << 22, 304)):
        assert l.cw_debug_locate_plan(seqs, cus, _ptr(out)) == 0
        wgs, dense = max(1, min(seqs, 6 * cus)), max(1, min(seqs, 64))  # 24 KB of LDS a work-group: six a CU; at most 64 dense tables
        parts = [up(8 * 4), up(4 * seqs), up(4 * dense_words * dense)]
        assert out.tolist() == [sum(parts)] + parts + [wgs, dense], (seqs, cus)


# ---- the reference -------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_the_reference_is_the_seed_runs_wherever_the_seed_run_takes_the_reference(k):
    checked = beyond = 0
    for name, groups in sd.catalogue(k).items():
        for grp in groups:
            for q in grp[1:]:
                if len(grp[0]) <= st.RMAX:
                    assert lp.locate_of(q, grp[0], k) == sd.seed_of(q, grp[0], k), (name, len(grp[0]), len(q))
                    checked += 1
                else:  # the seed run's capacity: no row there, a row here
                    assert sd.seed_of(q, grp[0], k) == (sd.NONE, 0, 0, 0) and (lp.locate_of(q, grp[0], k)[0] == sd.NONE) == (not k <= len(q) <= st.QMAX)
                    beyond += 1
    assert checked > 300 and beyond == 3
    assert lp.locate_of("ACGT", "ACGT" * 10, 8) == (lp.NONE, 0, 0, 0) and lp.locate_of("C" * 20, "A" * 20 + "ACGTTGCA", 8) == (lp.FWD, 0, -20, 0)
    assert lp.expected("ACGTACGTACGT", ["ACGTACGTACG" + "ACGT"], 0) == [(lp.NONE, 0, 0, 0)]  # k = 0 is 15 here, not the seed run's 11
    assert lp.distinct_pairs("AAAACCCCGG", "AAAACCCCGG", 8) == 1 and lp.distinct_pairs("C" * 20, "A" * 28, 8) == 0


def test_the_far_probes_are_the_edges_they_are_named_for():
    for k in (11, 15):
        draft, reads, names = lp.far_reads(k)
        rows = dict(zip(names[48:], lp.expected(draft, reads[48:], k)))
        assert len(draft) == 70000 > 65536 > st.RMAX and ((len(draft) + 300) >> lp.SHIFT) > 1023
        near = lambda hits, most: most - 8 <= hits <= most  # (of a 70 000-base draft's 11-mers a few in a hundred occur twice and seed nothing)
        assert [s >> lp.SHIFT for s in (65535, 65536, 65599, 65600)] == [1023, 1024, 1024, 1025]  # the bins on both sides of ten bits
        for s in (65535, 65536, 65599, 65600):  # an exact slice: every hit on the diagonal s - 200, in the one bin s >> 6
            row = rows[f"d + m = {s}"]
            assert row[0] == lp.FWD and near(row[1], 200 - k + 1) and row[2] <= s - 200 < row[2] + lp.SPAN, (k, s, row)
        for a in (65535, 65536):
            row = rows[f"position {a}"]
            assert row[0] == lp.FWD and near(row[1], 200 - k + 1) and row[2] <= a < row[2] + lp.SPAN, (k, a, row)
        assert rows["over the start"][0] == lp.FWD and near(rows["over the start"][1], 50 - k + 1) and rows["over the start"][2] == -80  # d + m = 50: bin 0
        assert rows["over the start, turned"][0] == lp.REV and rows["over the start, turned"][1:3] == rows["over the start"][1:3]
        assert rows["over the end"][0] == lp.FWD and near(rows["over the end"][1], 50 - k + 1) and rows["over the end"][2] <= 69950 < rows["over the end"][2] + lp.SPAN
        assert rows["over the end, turned"][0] == lp.REV and near(rows["over the end, turned"][1], 50 - k + 1)
        twice = reads[names.index("present twice")]
        assert draft.count(twice) == 2 and draft.find(twice) + 40000 == draft.rfind(twice) and not any(sd.windows(twice, draft, k)[lp.FWD])
        assert any(sd.windows(twice, draft[8192:16384], k)[lp.FWD])  # a tile that holds it once seeds: Engine.place finds it, Engine.locate does not
        own = reads[names.index("its own reverse complement")]
        assert own == lp.revcomp(own) and rows["its own reverse complement"][0] == lp.FWD
        assert rows["its own reverse complement"][1] == rows["its own reverse complement"][3] and near(rows["its own reverse complement"][1], 60 - k + 1)


def test_the_chance_level_behind_min_hits_and_the_planted_reads():
    """The measurement behind LOCATE_MIN_HITS: the 24 unrelated random reads of 300 to 5 000 bases against the 70 000-base draft, the largest reference this file
    builds.  The largest HITS over them at the default k = 15, doubled, is the default min_hits; the planted reads' smallest HITS stands beside it.  Every
    planted read's strand is right and its start lies in its window.  For longer references the figure is an extrapolation: chance hits grow with
    n m / 4^k."""
    draft, reads, where, other = sd.draft_and_reads(*lp.DRAFT)
    chance, least, cross = {}, {}, {}
    for k in (11, 15):
        chance[k] = max(lp.locate_of(q, draft, k)[lp.HITS] for q in other)
        rows = [lp.locate_of(q, draft, k) for q in reads]
        least[k], cross[k] = min(r[lp.HITS] for r in rows), max(r[lp.OTHER] for r in rows)
        for row, (a, turned) in zip(rows, where):
            assert row[0] == (lp.REV if turned else lp.FWD) and row[2] <= a < row[2] + lp.SPAN, (k, a, row)
        print(f"k = {k}: planted reads' smallest HITS {least[k]}, largest other-orientation HITS {cross[k]}, chance maximum {chance[k]}")
    assert chance[15] <= chance[11]
    assert 2 * chance[lp.K_DEFAULT] == lp.MIN_HITS == ca.LOCATE_MIN_HITS and ca.LOCATE_MIN_K == lp.K_DEFAULT == ca.LOCATE_K
    assert least[15] >= 10 * lp.MIN_HITS and least[15] >= 4 * cross[15]
    placed = lp.locate(draft, list(reads) + list(other), 0)
    assert None not in placed[:24] and placed[24:] == [None] * 24


def test_the_reference_builds_the_polish_groups_of_a_contig():
    draft, reads, where, other = sd.draft_and_reads(**lp.CONTIG)
    bag = list(reads) + [other[0]]
    placed = lp.locate(draft, bag, 0)
    assert placed[-1] is None and None not in placed[:-1] and {p[0] for p in placed[:-1]} == {lp.FWD, lp.REV}
    groups = lp.polish_groups(draft, bag, 5000, 0)
    assert "".join(g[0] for g in groups) == draft and len(groups) == 4 and sum(len(g) - 1 for g in groups) >= len(reads)
    group, spans = lp.seeded_group(draft, bag, 0)
    assert group[0] == draft and len(group) == len(reads) + 1 == len(spans)
    for q, (a, turned), (lo, hi) in zip(reads, where, spans[1:]):
        assert lo <= a and a + len(q) <= hi + 64 and hi - lo <= len(q) + lp.SPAN + 2 * (64 + (len(q) >> 4))
