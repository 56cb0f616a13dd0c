"""The reference of tests/chain_probes.py -- which anchors form a window's chain and where every sequence is cut, in plain Python / numpy -- against the
oracle's statistics (oracle/cw_oracle.cpp A4a-A4c) over the chain kernel's probe catalogue, and the catalogue's designed numbers and routes asserted
from the reference: a probe that misses its edge fails here, on the CPU, before tests/test_gpu_chain.py runs it."""
import ctypes as C
import os
import re
import subprocess

import pytest

import consent_amd as ca
import oracle_lib
import chain_probes
from chain_probes import PROBES, SWEEP_DEPTHS, SWEEP_LENGTHS, TIE_PRM, arithmetic, check_designed, pieces, reference
from index_probes import reference_counts
from consent_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIES = [p for p in PROBES if p.name.startswith("tie ")]


def assert_oracle_agrees(probe, ref, lib=None):
    """The oracle's statistics are the reference's -- and, since two chains that tie have the same statistics, its consensus is what the oracle's own POA and
    polish make of the reference's segments: a different chain or cut spells a different string in a noisy pile."""
    exp, st = oracle_lib.oracle_run(ca.Params(*probe.prm), probe.hb, lib=lib)
    want = {"tpl_anchors": ref.A, "chain_len": len(ref.chain), "segments": len(ref.segments), "poa_segments": sum(1 for _, mem in ref.segments if mem),
            "max_seg_len": ref.max_piece}
    assert {n: st[n] for n in want} == want, probe
    assert int(exp.status[0]) == (ca.WIN_CONSENSUS if ref.has_chain else ca.WIN_TEMPLATE), probe
    if ref.has_chain:
        k, solid = probe.prm[:2]
        raw = "".join(oracle_lib.oracle_poa(pieces(probe.pile, mem)) for _, mem in ref.segments if mem)
        keys, counts, _ = reference_counts(probe.hb, k, 1)
        assert exp.consensus(0) == oracle_lib.oracle_weight_polish(raw, dict(zip(keys.tolist(), counts.tolist())), k, solid), probe


def test_probe_names_are_unique():
    assert len({p.name for p in PROBES}) == len(PROBES)


@pytest.mark.parametrize("probe", PROBES, ids=repr)
def test_oracle_statistics_are_the_references(probe):
    assert_oracle_agrees(probe, probe.ref)


@pytest.mark.parametrize("probe", PROBES, ids=repr)
def test_probe_has_its_designed_numbers_and_route(probe):
    check_designed(probe)
    names, counters, n_dirty = arithmetic(probe.ref, probe.slab)
    assert probe.route_names == names, f"{probe}: the catalogue says {probe.route_names}, the constants' arithmetic {names}"
    assert all(c is None or c == a for c, a in zip(probe.counters, counters)), (probe, probe.counters, counters)
    assert probe.n_dirty == n_dirty and probe.use_bits == (probe.ref.N <= 2048)  # (no probe is too large for bitsets in the index kernel's LDS)
    assert "fast" in names or counters[3] == 1


def test_every_route_bit_has_a_probe():
    seen = set()
    for p in PROBES:
        seen.update(p.route_names)
    assert seen == set(engine.CHAIN_ROUTE)


def test_the_tie_set_has_chains_that_skip_anchors():
    """The 64 tiny piles are there for the tie rules: by the reference alone, at least 56 end with a chain and at least 48 of those chains skip an anchor."""
    assert len(TIES) == 64 and all(p.prm == TIE_PRM for p in TIES)
    assert sum(p.ref.has_chain for p in TIES) >= 56
    assert sum(p.ref.has_chain and p.ref.skips for p in TIES) >= 48
    assert all("pres_lds" in p.route_names for p in TIES)


def test_the_sweep_crosses_every_bound_of_the_routing_rule():
    hdr = "".join(open(os.path.join(ROOT, "consent_amd", "csrc", f)).read() for f in ("cw_poa.h", "cw_poa_q.h"))
    bounds = [int(re.search(rf"#define {n} (\d+)", hdr).group(1)) for n in ("CW_POAQ_LC", "CW_POAH_LC", "CW_POA_LC", "CW_POAM1_LC", "CW_POAM2_LC")]
    assert sorted(SWEEP_LENGTHS) == sorted(bounds + [b + 1 for b in bounds])
    for depth in SWEEP_DEPTHS:
        got = sorted(max(l for _, mem in p.ref.tasks for _, _, l in mem) for p in PROBES if p.name.startswith("region ") and p.name.endswith(f" depth {depth}"))
        assert got == sorted(SWEEP_LENGTHS), (depth, got)


def test_reference_follows_the_tie_policy(tmp_path):
    """A -DCW_CHAIN_TIE=1 build of the oracle (the largest successor on equal length and score) against the reference's tie="largest": the agreement under
    the default is no accident of piles without ties -- the two rules give different chains in some of the piles."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "policy", f"OUT={tmp_path}", "POLICY=-DCW_CHAIN_TIE=1"])
    lib = C.CDLL(str(tmp_path / "liboracle.so"))
    differ = 0
    for p in TIES:
        other = reference(p.pile, p.prm, tie="largest")
        assert_oracle_agrees(p, other, lib)
        differ += other.chain != p.ref.chain
    assert differ >= 1, differ  # (one pile is enough to tell the two rules apart; three of the 64 do)


def test_route_table_is_the_kernels():
    """consent_amd/engine.py CHAIN_ROUTE names the bits of csrc/cw_chain.h's CwChRoute, and CHAIN_ROUTE_SLOT is CW_PS_CHAIN_ROUTE."""
    hdr = open(os.path.join(ROOT, "consent_amd", "csrc", "cw_chain.h")).read()
    bits = {m.group(1).lower(): 1 << int(m.group(2)) for m in re.finditer(r"CW_CR_(\w+) = 1u << (\d+)", hdr)}
    assert bits == engine.CHAIN_ROUTE
    dev = open(os.path.join(ROOT, "consent_amd", "csrc", "cw_device.h")).read()
    assert int(re.search(r"CW_PS_CHAIN_ROUTE = (\d+)", dev).group(1)) == engine.CHAIN_ROUTE_SLOT


def test_slab_constants_are_the_kernels():
    """The slab sizes, the queue's bytes and the tile's row stride that tests/chain_probes.py does its sums with are csrc/cw_chain.h's, and its fit test gives the
    anchor counts that header's static_asserts pin: 1230 on the 20 KB slab (1231 does not fit), CW_TMAX on the long one."""
    hdr = open(os.path.join(ROOT, "consent_amd", "csrc", "cw_chain.h")).read()
    define = lambda n: int(re.search(rf"#define {n} (\d+)", hdr).group(1))
    assert chain_probes.CH_SLAB == define("CW_CH_SLAB") and chain_probes.CH_SLAB_LONG == define("CW_CH_SLAB_LONG")
    assert chain_probes.CH_LIST_BYTES == define("CW_CH_LIST_BYTES") and chain_probes.CH_TILE_STRIDE == define("CW_CH_TILE_STRIDE")
    tmax = int(re.search(r"#define CW_TMAX (\d+)", open(os.path.join(ROOT, "consent_amd", "csrc", "cw_index.h")).read()).group(1))
    assert chain_probes.slab_fits(1230) and not chain_probes.slab_fits(1231)
    assert chain_probes.slab_fits(tmax, chain_probes.CH_SLAB_LONG)


def test_segments_entry_point_is_in_both_builds_and_refuses_without_an_engine():
    """cw_debug_segments (csrc/cw_private.h) is host code of the product library and of the test-aid library alike; without an engine it is invalid."""
    n = C.c_uint32()
    for path in (engine.lib_path(), engine.AIDS_LIB):
        lib = engine._load(path)
        assert hasattr(lib, "cw_debug_segments"), path
        assert lib.cw_debug_segments(None, 0, C.byref(n), None, 0, None, 0, C.byref(n), None, 0, C.byref(n)) == -1  # CW_E_INVALID
