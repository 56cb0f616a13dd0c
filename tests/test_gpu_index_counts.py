"""The index kernel's k-mer counts as numbers.  Every other GPU test compares status, consensus and the solid key SET; the counts behind the set
(solid_cnt: five producers in cw_index.h) only order neighbours and anchor pairs in the finish kernel, so a wrong count that stays at or above the
threshold shows nowhere.  Here every probe of tests/index_probes.py -- one window, alone in its batch, aimed at one edge of the count paths -- is run on
the product library and on the test-aid library; each run is compared with the oracle (status, consensus, solid set) and its count table
(Engine.solid_table) with plain numpy, keys and counts exactly; on the test-aid library the route witness (Engine.index_route) must be the
probe's hand-written route, so that a probe cannot end up testing another path."""
import os

import numpy as np
import pytest

import consent_amd as ca
import oracle_lib
from consent_amd import engine
from consent_amd.engine import route_names
from index_probes import PROBES, reference_counts

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)


@pytest.fixture(scope="module")
def engines():
    cache = {}  # at most four engines alive, as in test_gpu_parity.py

    def get(which, prm):
        key = (which, prm)
        if key in cache:
            cache[key] = cache.pop(key)
        else:
            while len(cache) >= 4:
                cache.pop(next(iter(cache))).close()
            cache[key] = ca.Engine(ca.Params(*prm))
        want = engine.AIDS_LIB if which == "aids" else engine.lib_path()
        assert cache[key].lib._name == want, (cache[key].lib._name, want)
        return cache[key]

    yield get
    for e in cache.values():
        e.close()


_EXP = {}


def expected(probe):
    """The oracle's window and numpy's counts, once per probe."""
    if probe.name not in _EXP:
        exp, _ = oracle_lib.oracle_run(ca.Params(*probe.prm), probe.hb, threads=THREADS)
        _EXP[probe.name] = (exp, reference_counts(probe.hb, probe.prm[0], probe.prm[1]))
    return _EXP[probe.name]


def run_and_compare(e, probe):
    exp, (keys, counts, _) = expected(probe)
    got = e.run(probe.hb)
    assert int(got.status[0]) != ca.WIN_OVERFLOW, f"{probe}: stopped, why {int(e.win_info(1)[0, 15])}"
    assert int(got.status[0]) == int(exp.status[0]), f"{probe}: status {got.status[0]} != {exp.status[0]}"
    assert got.consensus(0) == exp.consensus(0), f"{probe}: consensus differs from the oracle's"
    assert np.array_equal(got.solid_kmers(0), exp.solid_kmers(0)), f"{probe}: solid set differs from the oracle's"
    tk, tc = e.solid_table(0)
    assert np.array_equal(tk.astype(np.uint64), keys), f"{probe}: keys of the count table differ from numpy's ({len(tk)} against {len(keys)})"
    bad = np.nonzero(tc.astype(np.int64) != counts)[0]
    assert len(bad) == 0, f"{probe}: {len(bad)} counts differ, first at key {int(keys[bad[0]])}: {int(tc[bad[0]])} against {int(counts[bad[0]])}"


@pytest.mark.parametrize("probe", PROBES, ids=repr)
def test_counts_on_the_product_library(probe, engines):
    run_and_compare(engines("product", probe.prm), probe)


@pytest.mark.parametrize("probe", PROBES, ids=repr)
def test_counts_and_route_on_the_test_aid_library(probe, engines, aids):
    e = engines("aids", probe.prm)
    run_and_compare(e, probe)
    route = e.index_route()
    assert route == probe.route, f"{probe}: went {route_names(route)}, designed for {route_names(probe.route)}"


def test_the_product_library_writes_no_route(engines):
    e = engines("product", PROBES[0].prm)
    e.run(PROBES[0].hb)
    assert e.index_route() == 0
