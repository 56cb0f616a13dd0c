"""Tier X (cw_poa.h cw_poa_x_kernel): the POA tasks that outgrow tier G -- graphs of more than 4 096 nodes, members of more than 2 047 bases --
are aligned on one wave in tier G's slab pool instead of stopping their window (status 2, CW_WHY_POA).  Every probe here stopped before tier X
existed; now each one is routed to tier X (Engine.tier_x_counters), corrected, and equal to the oracle, whose POA has no size caps.  What still
stops in tier X stops the same way in every batch: the pool it uses is the one every plan has."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import consent_amd as ca
import oracle_lib
from consent_amd.engine import alloc_results, synth_host
from test_gpu_batch_invariance import THREADS, Run, fillers, insert, rand_seq, run_at, run_device, same_run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHY_POA = 8  # cw_device.h CW_WHY_POA
PRM_A = (9, 2, 8, 2, 150)


def probe_a(seed, members=24):
    """A graph of more than 4 096 nodes: the batch-invariance catalogue's tier-G construction (shared 60-base head and tail, random middles)
    with `members` sequences instead of 8, and the other members' middles 1 300-1 500 bases long: random pieces of the catalogue's 520-640
    bases fill every column of the graph with all four bases and stop adding nodes near 3 000 (measured), wider ones do not."""
    rng = random.Random(seed)
    head, tail = rand_seq(rng, 60), rand_seq(rng, 60)
    tpl = head + rand_seq(rng, rng.randrange(520, 640)) + tail
    return ca.pack_piles([[tpl] + [head + rand_seq(rng, rng.randrange(1300, 1501)) + tail for _ in range(members - 1)]])


def probe_b(seed, members=8, mid_len=2100, tpl_mid=1936):
    """Members of more than 2 047 bases: a template of head + 1 936 + tail bases (cw_configure(2056)) and members whose random middles are
    about 2 100 bases (middles that share k-mers would give the chain anchors there, and short pieces)."""
    rng = random.Random(seed)
    head, tail = rand_seq(rng, 60), rand_seq(rng, 60)
    pile = [head + rand_seq(rng, tpl_mid) + tail]
    pile += [head + rand_seq(rng, rng.randrange(mid_len - 20, mid_len + 21)) + tail for _ in range(members - 1)]
    return ca.pack_piles([pile])


def engine(prm, conf=None):
    e = ca.Engine(ca.Params(*prm))
    if conf:
        e.configure(conf)
    return e


PROBES = {  # name -> (params, cw_configure argument, one-window batch)
    "a: graph over 4096 nodes": (PRM_A, None, probe_a(0x7A01)),
    "b: members over 2047 bases": (PRM_A, 2056, probe_b(0x7B01)),
    "b with 3000-base middles": (PRM_A, 2056, probe_b(0x7B04, members=12, mid_len=3000)),  # ~80 MB of cells: more than a four-slab pool holds
    "a at k 8": ((8, 2, 8, 2, 150), None, probe_a(0x7A02)),
    "a at max_msa 20": ((9, 2, 8, 2, 20), None, probe_a(0x7A03)),
    "b at max_msa 20": ((9, 2, 8, 2, 20), 2056, probe_b(0x7B03)),
}


def oracle_equal(prm, hb, r, what):
    exp, _ = oracle_lib.oracle_run(ca.Params(*prm), hb, threads=THREADS)
    assert r.status == int(exp.status[0]), f"{what}: status {r.status}, oracle {int(exp.status[0])}"
    assert r.cons == exp.consensus(0), f"{what}: consensus differs from the oracle"
    assert np.array_equal(r.solid, exp.solid_kmers(0)), f"{what}: solid set differs from the oracle"


@pytest.fixture(scope="module")
def alone():
    """Every probe alone on a fresh engine: routed to tier X, corrected, equal to the oracle."""
    out = {}
    for name, (prm, conf, hb) in PROBES.items():
        e = engine(prm, conf)
        try:
            (r,) = run_at(e, hb, [0])
            x = e.tier_x_counters()
        finally:
            e.close()
        print(f"{name}: {r!r}, tier X {x}")
        out[name] = (r, x)
    return out


@pytest.mark.parametrize("name", list(PROBES))
def test_probe_that_stopped_is_routed_to_tier_x_and_equals_the_oracle(alone, name):
    prm, conf, hb = PROBES[name]
    r, x = alone[name]
    assert x["routed"] >= 1 and x["done"] == x["routed"] and x["stopped"] == 0, f"{name}: tier X {x}"
    assert r.status != ca.WIN_OVERFLOW, f"{name}: {r!r}"
    oracle_equal(prm, hb, r, name)


def test_probe_a_and_b_are_a_function_of_the_window(alone):
    """Among 2 000 shallow fillers, inside a 16 384-window depth-150 batch, and through cw_run_device and cw_submit + cw_wait: the outcome of
    the window alone."""
    fill = fillers()
    bench = synth_host(ca.SynthSpec.pacbio(16384, 150))
    for name in ("a: graph over 4096 nodes", "b: members over 2047 bases"):
        prm, conf, hb = PROBES[name]
        ref = alone[name][0]
        e = engine(prm, conf)
        try:
            for pos in (0, fill.n_windows // 2, fill.n_windows):
                (r,) = run_at(e, insert(fill, hb, pos), [pos])
                same_run(r, ref, f"{name} at {pos} of {fill.n_windows} shallow windows")
                assert e.tier_x_counters()["done"] >= 1
            at = bench.n_windows // 2
            (r,) = run_at(e, insert(bench, hb, at), [at])
            same_run(r, ref, f"{name} inside the 16 384-window batch")
            assert e.tier_x_counters()["done"] >= 1
            mixed = insert(fill.slice(0, 600), hb, 300)
            res = run_device(e, mixed)
            same_run(Run(res, e.win_info(mixed.n_windows), 300), ref, f"{name}, cw_run_device")
            res = alloc_results(mixed, True, prm[1], prm[0])
            t, keep = e.submit(mixed, res)
            e.wait(t)
            same_run(Run(res, e.win_info(mixed.n_windows), 300), ref, f"{name}, cw_submit + cw_wait")
            del keep
        finally:
            e.close()


def test_the_bench_batch_sends_nothing_to_tier_x():
    """bench.py's batch: 16 384 synthetic PacBio-profile windows at depth 150, k 9, solid 4, 8 common k-mers, 2 anchors, maxMSA 150."""
    e = engine((9, 4, 8, 2, 150))
    try:
        e.run(synth_host(ca.SynthSpec.pacbio(16384, 150)))
        assert e.tier_x_counters() == {"routed": 0, "done": 0, "stopped": 0, "max_cells": 0}
    finally:
        e.close()


def test_a_small_pool_still_stops_the_same_way_everywhere(aids, monkeypatch, alone):
    """CW_BIG_SLOTS=4 (test-aid build): tier G's pool is four slabs, ~68 MB.  Probe (a) fits and is corrected as with the full pool; probe (b)
    with 3 000-base middles, whose last alignment needs more cells than that, stops with (2, CW_WHY_POA) -- alone and among shallow fillers alike."""
    monkeypatch.setenv("CW_BIG_SLOTS", "4")
    fill = fillers()
    prm, conf, hb = PROBES["a: graph over 4096 nodes"]
    e = engine(prm, conf)
    try:
        (r,) = run_at(e, hb, [0])
        same_run(r, alone["a: graph over 4096 nodes"][0], "probe (a), 68 MB pool")
        assert e.tier_x_counters()["done"] >= 1
    finally:
        e.close()
    prm, conf, hb = PROBES["b with 3000-base middles"]
    e = engine(prm, conf)
    try:
        (r,) = run_at(e, hb, [0])
        x = e.tier_x_counters()
        assert (r.status, r.why) == (ca.WIN_OVERFLOW, WHY_POA), f"probe (b) alone, 68 MB pool: {r!r}, tier X {x}"
        assert x["stopped"] >= 1 and x["max_cells"] * 4 > 64_000_000, x  # it asked for more than the four slabs hold next to the graph arrays
        (r2,) = run_at(e, insert(fill, hb, 1000), [1000])
        same_run(r2, r, "probe (b) among shallow fillers, 68 MB pool")
    finally:
        e.close()


POLICY_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import consent_amd as ca
import oracle_lib
from test_gpu_poa_tier_x import PRM_A, probe_a, probe_b
same, routed = True, 0
# under the affine model probe (b) with a 600-base template middle and 2 080-base member middles: 18.7 M cells in three layers, inside tier X
b_args = dict(mid_len=2080, tpl_mid=600) if sys.argv[2] == "affine" else {}
probes = [(probe_a(0x7A11, 12), None), (probe_b(0x7B11, 8, **b_args), 2056)]
for hb, conf in probes:
    eng = ca.Engine(ca.Params(*PRM_A))
    if conf:
        eng.configure(conf)
    got = eng.run(hb)
    x = eng.tier_x_counters()
    eng.close()
    exp, _ = oracle_lib.oracle_run(ca.Params(*PRM_A), hb, threads=min(16, os.cpu_count() or 1))
    print("probe", x, int(got.status[0]), len(got.consensus(0)), file=sys.stderr)
    routed += x["done"] > 0
    same = same and int(got.status[0]) != 2 and int(got.status[0]) == int(exp.status[0]) and got.consensus(0) == exp.consensus(0)
    same = same and np.array_equal(got.solid_kmers(0), exp.solid_kmers(0))
print("RESULT", int(same), routed)
"""


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("policy, tag", [(["-DCW_POA_GAP_MODEL=1"], "affine"), (["-DCW_POA_CONSENSUS=1", "-DCW_POA_MODE=2"], "hb-ov")], ids=["affine", "heaviest-bundle-overlap"])
def test_tier_x_under_other_policies(tmp_path, policy, tag):
    """The engine and the oracle built once more under a policy of include/cw_policy.h (as test_gpu_policy.py does): probes (a) and (b), sized to
    fit tier X under the affine model's three layers, are routed to tier X and agree with the oracle."""
    from consent_amd import _build

    alt_lib = str(tmp_path / "libconsent_amd_policy.so")
    subprocess.check_call([_build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", *policy, *_build.SRC, "-o", alt_lib])
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "policy", f"OUT={tmp_path}", "POLICY=" + " ".join(policy)])
    env = dict(os.environ, CONSENT_AMD_LIB=alt_lib, CW_ORACLE_LIB=str(tmp_path / "liboracle.so"))
    out = subprocess.run([sys.executable, "-c", POLICY_CHILD, ROOT, tag], capture_output=True, text=True, env=env, timeout=1200)
    assert out.returncode == 0, out.stderr[-2000:]
    _, same, routed = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")][-1].split()
    assert routed == "2", out.stderr[-2000:]
    assert same == "1", out.stderr[-2000:]
