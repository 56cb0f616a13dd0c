"""Both strands without a GPU (include/consent_amd.h cw_strand_run / cw_strand_run_device / cw_revcomp / cw_revcomp_device): the symbols and constants exist, a
missing engine and missing arguments are refused before the device is touched -- and the reference the GPU tests compare with (tests/strand_probes.py) is held to
its design: the reverse complement is an involution and packs with zero tail bits, the plan is what a run needs, and the polish inputs the GPU tests mix the
strands of are decisive at every k they could be voted with."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import consent_amd as ca
import strand_probes as st
import sw_cut_probes as cp
from consent_amd import engine as en
from consent_amd.engine import _ptr

E_INVALID = -1
NEW_FUNCTIONS = ("cw_strand_run", "cw_strand_run_device", "cw_revcomp", "cw_revcomp_device")


def header():
    return open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "consent_amd.h")).read()


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_header_declares_the_four_functions_the_struct_and_the_constants():
    text = header()
    assert re.search(r"int cw_strand_run_device\(cw_engine\* e, const cw_batch\* groups, const cw_strands\* out, void\* hip_stream\);", text)
    assert re.search(r"int cw_strand_run\(cw_engine\* e, const cw_batch\* groups, const cw_strands\* out\);", text)
    assert re.search(r"int cw_revcomp_device\(cw_engine\* e, const cw_batch\* groups, const uint8_t\* strand, uint32_t\* bases_out, void\* hip_stream\);", text)
    assert re.search(r"int cw_revcomp\(cw_engine\* e, const cw_batch\* groups, const uint8_t\* strand, uint32_t\* bases_out\);", text)
    assert re.search(r"typedef struct cw_strands \{\s*uint8_t\*\s+strand;[^}]*uint32_t\*\s+hits;[^}]*uint32_t\s+k;[^}]*\} cw_strands;", text)
    assert re.search(r"enum \{ CW_STRAND_FWD = 0, CW_STRAND_REV = 1, CW_STRAND_IS_REF = 2, CW_STRAND_NONE = 3 \};", text)
    for name, value in (("CW_STRAND_K", 11), ("CW_STRAND_KMIN", 8), ("CW_STRAND_KMAX", 15)):
        assert re.search(rf"#define {name}\s+{value}u", text), name
    for name in ("cw_strand_run / cw_strand_run_device", "cw_revcomp / cw_revcomp_device"):  # the head comment's list of entry points
        assert name in text.split("#ifndef CONSENT_AMD_H")[0], name


def test_the_library_exports_them_and_the_binding_names_them():
    l = ca.load_library()
    for name in NEW_FUNCTIONS:
        assert hasattr(l, name), name
    assert (ca.STRAND_FWD, ca.STRAND_REV, ca.STRAND_IS_REF, ca.STRAND_NONE) == (st.FWD, st.REV, st.IS_REF, st.NONE) == (0, 1, 2, 3)
    assert (ca.STRAND_K, ca.STRAND_KMIN, ca.STRAND_KMAX) == (st.K_DEFAULT, st.KMIN, st.KMAX) == (11, 8, 15)
    assert [f[0] for f in ca.Strands._fields_] == ["strand", "hits", "k"] and C.sizeof(ca.Strands) == 24
    for name in ("strands", "strand_device", "revcomp", "revcomp_device", "orient", "polish"):
        assert hasattr(ca.Engine, name), name
    assert ca.Polished("ACGT", []).strands == []


def test_null_arguments_are_refused_without_a_device():
    """Without a device there is no engine, so every entry point ends at its first check; nothing is written."""
    l = ca.load_library()
    hb = ca.pack_piles([["ACGTACGTACGTACGT", "ACGTACGTACGT"]])
    b = hb.c_struct()
    strand, hits, words = np.full(2, 77, np.uint8), np.full(4, 77, np.uint32), np.full(len(hb.bases), 77, np.uint32)
    for k in (0, 7, 11, 16):
        out = en.Strands(_ptr(strand), _ptr(hits), k)
        assert l.cw_strand_run(None, C.byref(b), C.byref(out)) == E_INVALID
        assert l.cw_strand_run_device(None, C.byref(b), C.byref(out), None) == E_INVALID
    assert l.cw_strand_run(None, None, None) == E_INVALID and l.cw_strand_run_device(None, None, None, None) == E_INVALID
    assert l.cw_revcomp(None, C.byref(b), _ptr(strand), _ptr(words)) == E_INVALID
    assert l.cw_revcomp_device(None, C.byref(b), None, _ptr(words), None) == E_INVALID
    assert l.cw_revcomp(None, None, None, None) == E_INVALID and l.cw_revcomp_device(None, None, None, None, None) == E_INVALID
    assert (strand == 77).all() and (hits == 77).all() and (words == 77).all()


def test_the_strand_plan_is_two_counters_and_a_word_a_group():
    l = ca.load_library()
    out = np.zeros(5, np.uint64)
    assert l.cw_debug_strand_plan(4, 8, 256, None) == E_INVALID and l.cw_debug_strand_plan(4, 8, 0, _ptr(out)) == E_INVALID
    for groups, seqs, cus in ((1, 1, 256), (1, 16385, 256), (4096, 69632, 256), (3, 301, 8), (65536, 1 << 22, 304)):
        assert l.cw_debug_strand_plan(groups, seqs, cus, _ptr(out)) == 0
        total, ctr, units, wgs, wgs_wide = (int(v) for v in out)
        assert ctr == 256 and units >= 4 * (groups + 1) and total == ctr + units and total % 256 == 0
        assert 1 <= wgs <= min(groups + seqs // st.CHUNK, 8 * cus) and wgs == max(1, min(groups + seqs // st.CHUNK, 8 * cus))  # no more work-groups than units, eight a CU
        assert wgs_wide == max(1, min(groups + seqs // 256, cus))


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_revcomp_is_an_involution_and_complements_from_the_other_end():
    assert st.revcomp("AACGT") == "ACGTT" and st.revcomp("") == ""
    for s in st.revcomp_strings():
        r = st.revcomp(s)
        assert len(r) == len(s) and st.revcomp(r) == s
        assert all("ACGT".index(r[j]) == 3 - "ACGT".index(s[len(s) - 1 - j]) for j in range(len(s)))


def test_packed_reverse_complements_have_zero_tail_bits():
    strings = [st.revcomp(s) for s in st.revcomp_strings()]
    hb = ca.pack_piles([strings])
    assert hb.pile(0) == strings
    for s, n in enumerate(hb.seq_len):
        n = int(n)
        if n % 16:
            last = int(hb.bases[int(hb.seq_word_off[s]) + (n - 1) // 16])
            assert last & ((1 << (32 - 2 * (n % 16))) - 1) == 0, n


def test_the_votes_count_positions_against_a_set_and_ties_go_forward():
    assert st.votes("A" * 77, "A" * 200, 11) == (67, 0) and st.votes("T" * 77, "A" * 200, 11) == (0, 67)
    own = "ACGT" * 25
    f, r = st.votes(own, "GG" + own + "CC", 11)
    assert f == r == len(own) - 10 and st.strand_of(own, "GG" + own + "CC", 11)[0] == st.FWD
    assert st.strand_of("ACGT", "ACGT" * 10, 8) == (st.NONE, 0, 0) and st.strand_of("ACGT" * 10, "ACGTACG", 8) == (st.NONE, 0, 0)
    assert st.strand_of("C" * 20, "A" * 20, 8) == (st.FWD, 0, 0)  # both zero: forward
    assert st.strand_of("A" * (st.QMAX + 1), "A" * 20, 8)[0] == st.NONE and st.strand_of("A" * 20, "A" * (st.RMAX + 1), 8)[0] == st.NONE
    assert st.expected([["ACGTACGTACGT", "ACGTACGTACG", ""], ["AC"]], 0)[0] == (st.IS_REF, 0, 0)
    for q in ("ACGGTTACGATTACA", "TTTTTTTTTTTTGGG"):  # the reverse hits are the forward hits of the reverse-complemented query
        ref = "GG" + q + "AC" + st.revcomp(q)[:12]
        assert st.votes(q, ref, 8)[1] == st.votes(st.revcomp(q), ref, 8)[0]


@pytest.mark.parametrize("seed", ["SEED8", "SEED9"])
def test_the_polish_inputs_are_decisive_at_every_k(seed):
    """Every read as given has more forward than reverse hits against the draft, every read reverse-complemented the opposite: a vote that is right decides them."""
    grp = cp.polish_input(**getattr(cp, seed))[1]
    for k in (8, 9, 11, 13, 15):
        given = [st.votes(q, grp[0], k) for q in grp[1:]]
        turned = [st.votes(st.revcomp(q), grp[0], k) for q in grp[1:]]
        print(f"{seed}, k = {k}: as given at least {min(f for f, _ in given)} forward against at most {max(r for _, r in given)} reverse")
        assert all(f > r for f, r in given), (seed, k)
        assert all(r > f for f, r in turned), (seed, k)
        assert [(r, f) for f, r in given] == turned
