"""The index kernel's anchor block as bytes.  The second half of cw_index_kernel -- anchors, position matrix, classification, masks, correction rows, presence
bits, hand-over -- writes one thing, the window's anchor block, and every other GPU test sees it only through what cw_chain_kernel makes of it: a wrong
position in a row off the chain, a presence bit for an anchor held out of order, a correction row off by one for a pair the chain never links, a pad left
over from the work-group's previous window change no consensus of today's probes.  Here every probe of tests/anchor_probes.py -- one window, alone in its
batch, aimed at one edge of that phase -- is run on the product library and on the test-aid library; each run is compared with the oracle (status,
consensus: that locates a failure), its block (Engine.anchor_block) with the plain reference of tests/anchor_ref.py field by field and byte for byte, the
pair scores rebuilt from the block as the chain kernel reads them with the plain score over all pairs, and on the test-aid library the route witness with
the probe's hand-written route.  Then the probes that share an engine go into one batch among more shallow windows than the device has compute units, in
two orders, so that a work-group of the index kernel runs several windows over the same LDS: every block must be what it was alone."""
import os

import numpy as np
import pytest
import torch

import consent_amd as ca
import oracle_lib
from anchor_probes import ANCHOR_BITS, PROBES
from anchor_ref import assert_same_block, assert_score_identity, canonical
from consent_amd import engine
from consent_amd.engine import INDEX_ROUTE, EngineError, route_names, synth_host
from consent_amd.engine import concat_batches as concat

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
WHY_TEMPLATE = 4  # cw_device.h CW_WHY_TEMPLATE
ANCHOR_MASK = sum(INDEX_ROUTE[n] for n in ANCHOR_BITS)


@pytest.fixture(scope="module")
def engines():
    cache = {}  # at most four engines alive, as in test_gpu_index_counts.py; the long templates get their configured engine

    def get(which, prm, configure=None):
        key = (which, prm, configure)
        if key in cache:
            cache[key] = cache.pop(key)
        else:
            while len(cache) >= 4:
                cache.pop(next(iter(cache))).close()
            cache[key] = ca.Engine(ca.Params(*prm))
            if configure:
                cache[key].configure(configure)
        want = engine.AIDS_LIB if which == "aids" else engine.lib_path()
        assert cache[key].lib._name == want, (cache[key].lib._name, want)
        return cache[key]

    yield get
    for e in cache.values():
        e.close()


_EXP, _WITNESSED = {}, {}


def expected(probe):
    """The oracle's window, once per probe."""
    if probe.name not in _EXP:
        _EXP[probe.name] = oracle_lib.oracle_run(ca.Params(*probe.prm), probe.hb, threads=THREADS)[0]
    return _EXP[probe.name]


def run_and_compare(e, probe):
    got = e.run(probe.hb)
    if probe.stop:  # the one documented stop: cw_setup_kernel refuses the template, and there is no block to read
        assert int(got.status[0]) == ca.WIN_OVERFLOW and int(e.win_info(1)[0, 15]) == WHY_TEMPLATE, f"{probe}: status {got.status[0]}, why {int(e.win_info(1)[0, 15])}"
        with pytest.raises(EngineError, match=r"\(-1\)"):  # CW_E_INVALID
            e.anchor_block(0)
        return e.index_route()
    exp = expected(probe)
    assert int(got.status[0]) != ca.WIN_OVERFLOW, f"{probe}: stopped, why {int(e.win_info(1)[0, 15])}"
    assert int(got.status[0]) == int(exp.status[0]), f"{probe}: status {got.status[0]} != {exp.status[0]}"
    assert got.consensus(0) == exp.consensus(0), f"{probe}: consensus differs from the oracle's"
    route = e.index_route()
    block = e.anchor_block(0)
    assert_same_block(block, probe.ref, probe)
    assert_score_identity(block, probe.ref.P32, probe)
    return route


@pytest.mark.parametrize("probe", PROBES, ids=repr)
def test_block_on_the_product_library(probe, engines):
    assert run_and_compare(engines("product", probe.prm, probe.configure), probe) == 0  # no witness in the product's kernel


@pytest.mark.parametrize("probe", PROBES, ids=repr)
def test_block_and_route_on_the_test_aid_library(probe, engines, aids):
    route = run_and_compare(engines("aids", probe.prm, probe.configure), probe)
    _WITNESSED[probe.name] = route
    assert route == probe.route, f"{probe}: went {route_names(route)}, designed for {route_names(probe.route)}"


def fillers(n):
    """Shallow windows (depth 4-8), as tests/test_gpu_batch_invariance.py has them."""
    return concat([synth_host(ca.SynthSpec.pacbio(n // 5 + 1, d, first_window=70000 + 1000 * d, window_len=500)) for d in (4, 5, 6, 7, 8)])


def groups():
    out = {}
    for p in PROBES:
        if not p.stop:
            out.setdefault((p.prm, p.configure), []).append(p)
    return out


@pytest.mark.parametrize("key", list(groups()), ids=lambda k: f"k={k[0][0]} solid={k[0][1]} configure={k[1]}")
def test_blocks_do_not_depend_on_the_batch(key, engines):
    """Batch composition: the group's probes among shallow fillers, more windows than compute units, in two orders of the probes."""
    prm, configure = key
    probes = groups()[key]
    e = engines("product", prm, configure)
    alone = {}
    for p in probes:
        e.run(p.hb)
        alone[p.name] = canonical(e.anchor_block(0))
    fill = fillers(n=torch.cuda.get_device_properties(0).multi_processor_count + 300)
    step = fill.n_windows // (len(probes) + 1)
    for order in (probes, probes[::-1]):
        parts, at, pos = [], {}, 0
        for i, p in enumerate(order):
            parts += [fill.slice(i * step, (i + 1) * step), p.hb]
            pos += step
            at[p.name] = pos
            pos += 1
        parts.append(fill.slice(len(order) * step, fill.n_windows))
        got = e.run(concat(parts))
        for p in order:
            w = at[p.name]
            assert int(got.status[w]) != ca.WIN_OVERFLOW, f"{p} at window {w}: stopped, why {int(e.win_info(w + 1)[w, 15])}"
            block = e.anchor_block(w)
            assert_same_block(block, p.ref, f"{p} at window {w} of {len(parts)} parts")
            now = canonical(block)
            assert sorted(now) == sorted(alone[p.name]) and all(np.array_equal(now[f], alone[p.name][f]) for f in now), f"{p} at window {w}: not the block it was alone"


def test_every_anchor_phase_bit_was_witnessed_and_the_new_ones_both_ways(engines, aids):
    for p in PROBES:  # (run on its own, this test witnesses the routes itself)
        if p.name not in _WITNESSED:
            e = engines("aids", p.prm, p.configure)
            e.run(p.hb)
            _WITNESSED[p.name] = e.index_route()
    seen = [r & ANCHOR_MASK for r in _WITNESSED.values()]
    union = 0
    for r in seen:
        union |= r
    assert union == ANCHOR_MASK, f"no probe went {route_names(ANCHOR_MASK & ~union)}"
    for bit in ("second_pass", "bucket_walk"):
        assert any(r & INDEX_ROUTE[bit] for r in seen) and any(not r & INDEX_ROUTE[bit] for r in seen if r), bit
