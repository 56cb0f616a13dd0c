"""The oracle's k-mer counts as numbers (cwo_counts), over the probe catalogue of the index kernel's count paths (tests/index_probes.py), against plain
numpy -- for the checker build of the oracle and for the tuned one (-DCWO_FAST: flat count tables, f_cnt / touched), which has its own count code.
The catalogue's designed numbers are asserted here too: a probe that misses its edge fails on the CPU, before tests/test_gpu_index_counts.py runs it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import consent_amd as ca
import oracle_lib
from consent_amd import engine
from index_probes import PROBES, check_designed, reference_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def oracles(tmp_path_factory):
    out = tmp_path_factory.mktemp("oracle_fast")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "policy", f"OUT={out}", "POLICY=-DCWO_FAST"])
    return {"plain": oracle_lib.oracle(), "tuned": C.CDLL(str(out / "liboracle.so"))}


_REF = {}


def reference(probe):
    if probe.name not in _REF:
        _REF[probe.name] = reference_counts(probe.hb, probe.prm[0], probe.prm[1])
    return _REF[probe.name]


def test_probe_names_are_unique():
    assert len({p.name for p in PROBES}) == len(PROBES)


@pytest.mark.parametrize("probe", PROBES, ids=repr)
def test_probe_has_its_designed_numbers(probe):
    check_designed(probe, *reference(probe))


@pytest.mark.parametrize("build", ["plain", "tuned"])
@pytest.mark.parametrize("probe", PROBES, ids=repr)
def test_oracle_counts_are_numpys(probe, build, oracles):
    keys, counts, _ = reference(probe)
    got_k, got_c = oracle_lib.oracle_counts(ca.Params(*probe.prm), probe.hb, 0, lib=oracles[build])
    assert np.array_equal(got_k, keys), f"{probe}: the oracle's solid keys differ from numpy's ({len(got_k)} against {len(keys)})"
    assert np.array_equal(got_c.astype(np.int64), counts), f"{probe}: counts differ at keys {keys[got_c.astype(np.int64) != counts][:8]}"


def test_route_table_is_the_kernels():
    """consent_amd/engine.py INDEX_ROUTE names the bits of csrc/cw_index.h's CwIdxRoute, and INDEX_ROUTE_SLOT is CW_PS_IDX_ROUTE."""
    hdr = open(os.path.join(ROOT, "consent_amd", "csrc", "cw_index.h")).read()
    bits = {m.group(1).lower(): 1 << int(m.group(2)) for m in re.finditer(r"CW_IR_(\w+) = 1u << (\d+)", hdr)}
    assert bits == engine.INDEX_ROUTE
    dev = open(os.path.join(ROOT, "consent_amd", "csrc", "cw_device.h")).read()
    assert int(re.search(r"CW_PS_IDX_ROUTE = (\d+)", dev).group(1)) == engine.INDEX_ROUTE_SLOT
