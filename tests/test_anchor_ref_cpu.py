"""The anchor block's reference (tests/anchor_ref.py) and probe catalogue (tests/anchor_probes.py) on the CPU: the Python restatement of the block's layout
against the library's (cw_debug_ab_layout, host arithmetic), every probe's designed numbers and route arithmetic from the reference alone -- a probe that
misses its edge fails here, before tests/test_gpu_anchor_block.py runs it -- and the score identity applied to the reference's own block over all pairs
of every probe, which is where the reference tests itself: its presence bits, masks and correction rows are derived from the classification, the plain
score from the positions alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import anchor_probes
from anchor_probes import ANCHOR_BITS, HIT_CAP, PROBES, arithmetic_route, check_designed
from anchor_ref import assert_score_identity
from chain_probes import index_room, matrix_need
from consent_amd import engine
from consent_amd.engine import AB_PARTS, INDEX_ROUTE, ab_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_probe_names_are_unique():
    assert len({p.name for p in PROBES}) == len(PROBES)


@pytest.mark.parametrize("path", ["product", "aids"])
def test_layout_restatement_is_the_librarys(path):
    """consent_amd/engine.py ab_layout against cw_debug_ab_layout, in both builds: anchor counts around the 16-byte granules, sequence counts around the
    presence words and the matrix's row padding, with and without dirty sequences and rows -- n_rows = 0 included, where P starts at rowid."""
    lib = engine._load(engine.lib_path() if path == "product" else engine.AIDS_LIB)
    assert hasattr(lib, "cw_debug_ab_layout") and hasattr(lib, "cw_debug_anchor_block"), path
    out = np.zeros(9, np.uint64)
    for A in (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 33, 488, 1024, 1025, 2047, 2048):
        for N in (1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 100, 128, 129, 1024, 1025, 2048, 2049, 5000):
            for n_dirty in (0, 1, 7, 8, 9, 64, 255, N):
                for n_rows in (0, 1, 2, 254):
                    assert lib.cw_debug_ab_layout(A, N, n_dirty, n_rows, C.c_void_p(out.ctypes.data)) == 0
                    assert tuple(int(x) for x in out) == ab_layout(A, N, n_dirty, n_rows), (A, N, n_dirty, n_rows)
                    if n_rows == 0:
                        assert out[AB_PARTS.index("P")] == out[AB_PARTS.index("rowid")]
    assert lib.cw_debug_ab_layout(1, 1, 0, 0, None) == -1  # CW_E_INVALID
    n = C.c_uint64()
    assert lib.cw_debug_anchor_block(None, 0, None, 0, C.byref(n)) == -1  # without an engine


def test_constants_are_the_kernels():
    hdr = open(os.path.join(ROOT, "consent_amd", "csrc", "cw_index.h")).read()
    assert f"#define CW_IDX_HIT_CAP (CW_EXG_SLOTS * 2u)" in hdr and int(re.search(r"#define CW_EXG_SLOTS (\d+)", hdr).group(1)) * 2 == HIT_CAP
    assert "return x * 2654435761u;" in hdr and "#define CW_TH_HOME(key) (cw_hash32(key) >> (32 - 10))" in hdr
    assert set(ANCHOR_BITS) <= set(INDEX_ROUTE)
    stage_off = int(re.search(r"#define CW_IDX_STAGE_OFF (\d+)", hdr).group(1))
    assert index_room(1024) == stage_off - int(re.search(r"IdxTplOff<1024>::P == (\d+)u", hdr).group(1))
    assert index_room(1025) == stage_off - int(re.search(r"IdxTplOff<2048>::P == (\d+)u", hdr).group(1))


def test_sizes_of_the_module_docstring():
    """The edges the catalogue's docstring names, recomputed."""
    assert (matrix_need(488, 100), matrix_need(489, 100)) == (107576, 107796) and index_room(488) == 107776
    assert (matrix_need(1099, 38), matrix_need(1100, 38)) == (92408, 92492) and index_room(1100) == 92416
    assert 405 * 32 * 8 + 2 * 2048 <= 107776 < 406 * 32 * 8 + 2 * 2048
    assert matrix_need(1024, 46) == 102508 <= index_room(1024) and (1024 - 300) * (2 * 46 + 8 + 12) == 81088 >= 255 * 304 == 77520


@pytest.mark.parametrize("probe", PROBES, ids=repr)
def test_probe_has_its_designed_numbers_and_route(probe):
    check_designed(probe)
    if probe.stop:
        assert probe.ref.nk0 > 2048 and probe.route == 0 and not probe.anchor_route and not probe.count_route  # CW_TMAX: the one documented stop of the catalogue, in cw_setup_kernel -- no route at all
        return
    assert probe.anchor_route == arithmetic_route(probe), f"{probe}: the catalogue says {probe.anchor_route}, the constants' arithmetic {arithmetic_route(probe)}"
    restated = sorted(anchor_probes.count_route(probe.pile, probe.prm))
    assert probe.count_route == restated, f"{probe}: the catalogue says {probe.count_route} for the count phase, the restated rules {restated}"


@pytest.mark.parametrize("probe", [p for p in PROBES if not p.stop], ids=repr)
def test_score_identity_of_the_references_own_block(probe):
    assert_score_identity(probe.ref, probe.ref.P32, probe)


def test_every_anchor_phase_bit_has_a_probe_and_the_new_ones_both_ways():
    routes = [set(p.anchor_route) for p in PROBES if not p.stop]
    assert set().union(*routes) == set(ANCHOR_BITS)
    for bit in ("second_pass", "bucket_walk"):
        assert any(bit in r for r in routes) and any(bit not in r for r in routes)
    for bit in ANCHOR_BITS:  # (and every bit is seen clear somewhere)
        assert any(bit not in r for r in routes), bit
