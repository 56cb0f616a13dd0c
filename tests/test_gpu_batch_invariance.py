"""Batch-composition invariance (include/consent_amd.h: a window's result does not depend on the batch it comes in).

The engine sizes its scratch from batch totals and hands out per-window slices in window order (cw_plan.h plan_scratch,
cw_index.h cw_setup_kernel), so whether a window fits could depend on the windows beside it.  Here a catalogue of probe windows, each
aimed at one code path, is run alone and in other batches -- among copies of itself, among shallow fillers (low mean depth), inside the
bench batch, on an engine that has just run something larger, through the device-buffer path -- and every run must give the same
status, consensus (case included), solid set and, for a stopped window, the same reason; every window that does not stop equals the
oracle.  Then one regression test per dependence that was found in the planning, and a short mixed-batch fuzz pass."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import consent_amd as ca
import oracle_lib
from consent_amd.engine import Batch, Result, alloc_results, synth_host
from consent_amd.engine import concat_batches as concat
from index_probes import aids_engine, assert_route, route_alone

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = min(16, os.cpu_count() or 1)
WHY_TEMPLATE, WHY_MATRIX, WHY_TASKS, WHY_ARENA = 4, 5, 7, 14  # cw_device.h CW_WHY_*
CW_MAX_BATCH_WINDOWS = 131072


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def mutate(rng, s, rate):  # as in test_gpu_parity.py
    out = []
    for c in s:
        x = rng.random()
        if x < rate * 0.3:
            continue
        if x < rate * 0.6:
            out.append(rng.choice("ACGT"))
        out.append(rng.choice("ACGT") if x < rate else c)
    return "".join(out)


def insert(fill, probe, pos):
    """`probe` (a one-window HostBatch) at window position `pos` of `fill`."""
    parts = [fill.slice(0, pos), probe, fill.slice(pos, fill.n_windows)]
    return concat([p for p in parts if p.n_windows])


def synth_pile(n_windows, depth, first, window_len=500):
    return synth_host(ca.SynthSpec.pacbio(n_windows, depth, first_window=first, window_len=window_len))


def byte_counter_pile(rng, occ):
    """A pile in which one 9-mer occurs `occ` times in all (test_gpu_parity.py test_byte_counters_hand_over_exactly_at_256_occurrences)."""
    truth, depth = rand_seq(rng, 420), 130
    per = [occ // depth + (1 if s < occ % depth else 0) for s in range(depth)]
    pile = []
    for s in range(depth):
        seq = mutate(rng, truth, 0.1)
        cuts = sorted(rng.sample(range(20, len(seq) - 20), per[s])) if per[s] else []
        out, last = [], 0
        for c in cuts:
            out += [seq[last:c], "ACGTTGCAA"]
            last = c
        out.append(seq[last:])
        pile.append("".join(out))
    return pile


# ---- the probe catalogue --------------------------------------------------------------------------------------------------------
# group -> (params, cw_configure argument or None, {probe name: (one-window HostBatch, why code it is documented to stop with or None)})
def catalogue():
    rng = random.Random(0xB47C)
    groups = {}
    p = {}
    p["pacbio depth 30"] = (synth_pile(1, 30, 4242), None)
    p["pacbio depth 150"] = (synth_pile(1, 150, 4343), None)
    truth = rand_seq(rng, 520)
    # the matrix of ~480 anchors x ~3000 sequences outgrows LDS and a 1024-row fallback slot: it needs the global slot at full size;
    # errors this rare keep the pile's saturated k-mers inside the counter table (test_gpu_parity.py, very deep piles)
    p["deep pile, global matrix fallback"] = (ca.pack_piles([[truth[:500]] + [mutate(rng, truth[:500], 0.004) for _ in range(3000)]]), None)
    t300 = rand_seq(rng, 320)
    for n in (1024, 1025):  # cw_index.h: the hit list holds the sequence in ten bits (hl = N <= 1024)
        p[f"pile of {n} sequences"] = (ca.pack_piles([[t300[:300]] + [mutate(rng, t300[:300], 0.01) for _ in range(n - 1)]]), None)
    for occ in (256, 257):  # the byte counters of phase A hand over to the nibble table at 256 occurrences
        p[f"byte counters, {occ} occurrences"] = (ca.pack_piles([byte_counter_pile(random.Random(occ), occ)]), None)
    p["900 bases at depth 100"] = (synth_pile(1, 100, 777, window_len=900), None)  # more than the first plan's 64 tasks / 2048 members a window
    t200 = rand_seq(rng, 300)
    p["template only"] = (ca.pack_piles([[t200[:200]]]), None)
    p["template shorter than k"] = (ca.pack_piles([[t200[:5], t200[:40], t200[3:60]]]), None)
    p["unrelated pile"] = (ca.pack_piles([[rand_seq(rng, 200) for _ in range(10)]]), None)
    groups["default"] = ((9, 4, 8, 2, 150), None, p)
    head, tail = rand_seq(rng, 60), rand_seq(rng, 60)  # tier G: a graph of more than 2048 nodes
    groups["tier G"] = ((9, 2, 8, 2, 150), None, {"graph of more than 2048 nodes": (ca.pack_piles([[head + rand_seq(rng, rng.randrange(520, 640)) + tail for _ in range(8)]]), None)})
    t1100 = rand_seq(rng, 1100)
    groups["unconfigured, long template"] = ((9, 4, 8, 2, 150), None, {"1100-base template": (ca.pack_piles([[t1100] + [mutate(rng, t1100, 0.02) for _ in range(20)]]), WHY_TEMPLATE)})
    t2000 = rand_seq(rng, 2000)
    groups["configured 2056"] = ((9, 4, 8, 2, 150), 2056, {"2000-base template": (ca.pack_piles([[t2000] + [mutate(rng, t2000, 0.01) for _ in range(12)]]), None),
                                                           "pacbio depth 30": (synth_pile(1, 30, 4444), None)})
    return groups


def fillers(n=2000, first=50000):
    """Shallow windows (depth 4-8): a batch whose mean depth is low."""
    per = n // 5
    return concat([synth_pile(per, d, first + 1000 * d) for d in (4, 5, 6, 7, 8)])


class Run:
    """Per-window outcome: status, consensus, solid set, why code (0 unless stopped)."""

    def __init__(self, res, info, w):
        self.status = int(res.status[w])
        self.cons = res.consensus(w)
        self.solid = np.asarray(res.solid_kmers(w)).copy()
        self.why = int(info[w, 15]) if self.status == ca.WIN_OVERFLOW else 0

    def __repr__(self):
        return f"status {self.status} why {self.why} consensus of {len(self.cons)} bases"


def run_at(eng, hb, positions):
    res = eng.run(hb)
    info = eng.win_info(hb.n_windows)
    return [Run(res, info, p) for p in positions]


def same_run(got, ref, what):
    assert (got.status, got.why) == (ref.status, ref.why), f"{what}: {got!r}, alone {ref!r}"
    assert got.cons == ref.cons, f"{what}: consensus differs from the window alone"
    assert np.array_equal(got.solid, ref.solid), f"{what}: solid set differs from the window alone"


def new_engine(prm, conf):
    e = ca.Engine(ca.Params(*prm))
    if conf:
        e.configure(conf)
    return e


def run_device(eng, hb):
    """The same batch through cw_run_device (device buffers, as tests/test_gpu_hostpath.py drives it)."""
    import torch

    dev = torch.device("cuda", 0)
    prm = eng.params

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    res = alloc_results(hb, True, prm.solid, prm.k)
    t_in = (up(hb.win_first_seq, np.int32), up(hb.seq_len, np.int32), up(hb.seq_word_off, np.int64), up(np.concatenate([hb.bases, np.zeros(4, np.uint32)]), np.int32))
    t_out = [torch.zeros(len(res.cons), dtype=torch.uint8, device=dev), up(res.cons_off, np.int64), torch.zeros(hb.n_windows, dtype=torch.int32, device=dev),
             torch.full((hb.n_windows,), 255, dtype=torch.uint8, device=dev), torch.zeros(len(res.solid), dtype=torch.int32, device=dev), up(res.solid_off, np.int64),
             torch.zeros(hb.n_windows, dtype=torch.int32, device=dev)]
    torch.cuda.synchronize(dev)
    b = Batch(hb.n_windows, len(hb.seq_len), len(hb.bases), *[t.data_ptr() for t in t_in])
    r = Result(*[t.data_ptr() for t in t_out])
    eng.run_device(b, r)
    torch.cuda.synchronize()
    res.cons[:] = t_out[0].cpu().numpy()
    res.cons_len[:] = t_out[2].cpu().numpy().view(np.uint32)
    res.status[:] = t_out[3].cpu().numpy()
    res.solid[:] = t_out[4].cpu().numpy().view(np.uint32)
    res.solid_len[:] = t_out[6].cpu().numpy().view(np.uint32)
    return res


@pytest.fixture(scope="module")
def cat():
    return catalogue()


@pytest.fixture(scope="module")
def alone(cat):
    """Every probe alone on a fresh engine -- the reference of every other context -- checked against the oracle."""
    out = {}
    for g, (prm, conf, probes) in cat.items():
        for name, (hb, doc_why) in probes.items():
            e = new_engine(prm, conf)
            try:
                (r,) = run_at(e, hb, [0])
            finally:
                e.close()
            out[(g, name)] = r
    return out


def test_every_probe_alone_is_the_oracle_or_a_documented_stop(cat, alone):
    for g, (prm, conf, probes) in cat.items():
        for name, (hb, doc_why) in probes.items():
            r = alone[(g, name)]
            if doc_why is not None:
                assert (r.status, r.why) == (ca.WIN_OVERFLOW, doc_why), f"{g} / {name}: {r!r}"
                continue
            assert r.status != ca.WIN_OVERFLOW, f"{g} / {name}: {r!r}"
            exp, _ = oracle_lib.oracle_run(ca.Params(*prm), hb, threads=THREADS)
            assert r.status == int(exp.status[0]) and r.cons == exp.consensus(0), f"{g} / {name}: differs from the oracle"
            assert np.array_equal(r.solid, exp.solid_kmers(0)), f"{g} / {name}: solid set differs from the oracle"


def test_the_1024_and_1025_sequence_probes_lie_on_the_two_sides_of_the_hit_list(cat, alone):
    """The route witness of the test-aid library (consent_amd/engine.py INDEX_ROUTE): the pile of 1024 sequences fills its matrix from the hit list, the one of
    1025 does not, and neither has a matrix per template k-mer -- so the two probes are the edge their names say."""
    prm, conf, probes = cat["default"]
    with aids_engine(*prm, configure=conf) as e:
        for n, has, lacks in ((1024, "hit_list", "tfit"), (1025, "", "hit_list tfit")):
            name = f"pile of {n} sequences"
            res, route = route_alone(e, probes[name][0])
            assert_route(route, has=has, lacks=lacks, what=name)
            assert res.consensus(0) == alone[("default", name)].cons


def test_probes_among_copies_of_themselves(cat, alone):
    for g, (prm, conf, probes) in cat.items():
        e = new_engine(prm, conf)
        try:
            for name, (hb, _) in probes.items():
                n = 4 if hb.seq_len.size > 500 else 12
                for p, r in enumerate(run_at(e, concat([hb] * n), range(n))):
                    same_run(r, alone[(g, name)], f"{g} / {name}, copy {p} of {n}")
        finally:
            e.close()


def test_probes_among_shallow_fillers(cat, alone):
    fill = fillers()
    for g, (prm, conf, probes) in cat.items():
        e = new_engine(prm, conf)
        try:
            for name, (hb, _) in probes.items():
                for pos in (0, fill.n_windows // 2, fill.n_windows):
                    (r,) = run_at(e, insert(fill, hb, pos), [pos])
                    same_run(r, alone[(g, name)], f"{g} / {name} at {pos} of {fill.n_windows} shallow windows")
        finally:
            e.close()


def test_probes_inside_the_bench_batch(cat, alone):
    """All probes of a group in a 16 384-window depth-150 batch (synth_host(SynthSpec.pacbio(16384, 150))), at its start, middle and end."""
    bench = synth_host(ca.SynthSpec.pacbio(16384, 150))
    for g, (prm, conf, probes) in cat.items():
        e = new_engine(prm, conf)
        try:
            names = list(probes)
            for at in (0, bench.n_windows // 2, bench.n_windows):
                hb = concat([bench.slice(0, at)] + [probes[n][0] for n in names] + [bench.slice(at, bench.n_windows)])
                for name, r in zip(names, run_at(e, hb, range(at, at + len(names)))):
                    same_run(r, alone[(g, name)], f"{g} / {name} at {at} of the bench batch")
        finally:
            e.close()


def test_probes_on_an_engine_that_ran_a_larger_batch_before(cat, alone):
    """A batch of heavy windows first (900 bases at depth 100: the plan grows past x1) and then the bench batch (scratch that is reused, not
    cleared); then every probe alone on that engine."""
    heavy = synth_pile(48, 100, 9100, window_len=900)
    for g, (prm, conf, probes) in cat.items():
        e = new_engine(prm, conf)
        try:
            e.run(heavy)
            e.run(synth_pile(2048, 60, 20000))
            for name, (hb, _) in probes.items():
                (r,) = run_at(e, hb, [0])
                same_run(r, alone[(g, name)], f"{g} / {name} after larger batches")
        finally:
            e.close()


def test_probes_through_the_paths_that_run_a_batch_once(cat, alone):
    """cw_run_device and cw_submit + cw_wait, with every probe of a group among 600 shallow fillers.  These paths run a batch once
    (include/consent_amd.h, CW_MAX_BATCH_WINDOWS): a stop on a capacity of the batch's plan stands.  Here that is exactly one probe -- the deep
    pile, whose matrix slot the batch's low mean depth sizes at 1024 rows: CW_WHY_MATRIX, where alone it is corrected -- and every other probe
    equals the window alone."""
    fill = fillers(600, 70000)
    stops_here = {("default", "deep pile, global matrix fallback"): WHY_MATRIX}
    for g, (prm, conf, probes) in cat.items():
        e = new_engine(prm, conf)
        try:
            names = list(probes)
            hb = concat([fill.slice(0, 300)] + [probes[n][0] for n in names] + [fill.slice(300, fill.n_windows)])
            res_sub = alloc_results(hb, True, prm[1], prm[0])
            t, keep = e.submit(hb, res_sub)
            e.wait(t)
            info_sub = e.win_info(hb.n_windows)
            res_dev = run_device(e, hb)
            info_dev = e.win_info(hb.n_windows)
            for path, res, info in (("cw_submit + cw_wait", res_sub, info_sub), ("cw_run_device", res_dev, info_dev)):
                for i, name in enumerate(names):
                    r = Run(res, info, 300 + i)
                    if (g, name) in stops_here:
                        assert alone[(g, name)].status == ca.WIN_CONSENSUS
                        assert (r.status, r.why) == (ca.WIN_OVERFLOW, stops_here[(g, name)]), f"{g} / {name}, {path}: {r!r}"
                        # the slot elements it needed (WinInfo word 12): more than this batch's 1024 rows, within the 4100 of a re-run
                        assert 1024 * 1024 < int(info[300 + i, 12]) <= 1024 * 4100, int(info[300 + i, 12])
                        continue
                    same_run(r, alone[(g, name)], f"{g} / {name}, {path}")
            del keep
        finally:
            e.close()


# ---- one regression test per dependence ------------------------------------------------------------------------------------------
def test_a_deep_pile_gets_the_full_matrix_fallback_among_shallow_windows():
    """Dependence (1): the global position-matrix slot was sized from the batch's MEAN depth (16 x mean, 1024..4100 rows).  A 500-base
    window with ~480 anchors and 3000 near-identical members needs ~3000 rows: alone (mean depth 3001) it got 4100 and was corrected;
    among 2000 windows of depth 4-8 it got 1024 rows and, before the fix, stopped with status 2, why CW_WHY_MATRIX (5) (measured on the
    MI355X), and was never run again.  Now a window stopped on the matrix slot is run again with the slot at its full 4100 rows (grow_if_that_helps)."""
    rng = random.Random(0xDEE9)
    truth = rand_seq(rng, 520)
    deep = ca.pack_piles([[truth[:500]] + [mutate(rng, truth[:500], 0.004) for _ in range(3000)]])
    prm = ca.Params(9, 4, 8, 2, 150)
    e = ca.Engine(prm)
    try:
        (a,) = run_at(e, deep, [0])
        assert a.status == ca.WIN_CONSENSUS, a
        exp, _ = oracle_lib.oracle_run(prm, deep, threads=THREADS)
        assert a.cons == exp.consensus(0) and np.array_equal(a.solid, exp.solid_kmers(0))
        fill = fillers()
        hb = insert(fill, deep, 1000)
        assert hb.seq_len.size // hb.n_windows < 64  # a batch whose mean depth asks for the smallest slot
        (b,) = run_at(e, hb, [1000])
        same_run(b, a, "deep pile among shallow windows")
    finally:
        e.close()


def test_a_template_longer_than_the_plan_stops_the_same_way_in_every_batch():
    """Dependence (2): a template of more k-mers than the engine's plan provides for (1024 unconfigured, 492 after cw_configure(500)) used to
    borrow segment and arena room from its neighbours.  Before the fix (measured on the MI355X), an 1100-base window alone on an unconfigured
    engine stopped with status 2, why CW_WHY_SETUP (1), and the same window at positions 0, 32 and 64 of 64 short windows was corrected
    (status 0); a 600-base window after cw_configure(500) did the same.  Now both stop with CW_WHY_TEMPLATE (4) in every batch."""
    rng = random.Random(0x1100)
    for conf, tl in ((None, 1100), (500, 600)):
        t = rand_seq(rng, tl)
        probe = ca.pack_piles([[t] + [mutate(rng, t, 0.02) for _ in range(20)]])
        e = new_engine((9, 4, 8, 2, 150), conf)
        try:
            (a,) = run_at(e, probe, [0])
            assert (a.status, a.why) == (ca.WIN_OVERFLOW, WHY_TEMPLATE), f"template of {tl} bases alone, cw_configure({conf}): {a!r}"
            short = synth_pile(64, 20, 3000, window_len=200)
            for pos in (0, 32, 64):
                (b,) = run_at(e, insert(short, probe, pos), [pos])
                same_run(b, a, f"template of {tl} bases at {pos} of 64 short windows, cw_configure({conf})")
        finally:
            e.close()


def test_an_engine_takes_every_batch_up_to_the_limit_it_reports():
    """Dependence (3): the arena of a batch is addressed with 32-bit offsets, n_windows x (16 x (tmax + 16) + 4096) bytes.  After
    cw_configure(2056) (tmax 2048) that passes 2^32 above 115 704 windows, below the documented CW_MAX_BATCH_WINDOWS: before the fix a
    batch of 131 072 windows was refused as a whole (cw_run: CW_E_INVALID), and the native driver's runs of CW_MAX_BATCH_WINDOWS windows at
    `-l 2000` with it (measured on the MI355X: cw_run returned CW_E_INVALID, -1, for 131 072 windows after cw_configure(2056)).
    cw_max_batch_windows(e) now states the engine's limit: a batch of exactly that many windows runs, one more is
    refused before anything is launched."""
    tiny = ca.pack_piles([["ACGTACGTTGCAAGT"]])
    for conf in (None, 2056):
        e = new_engine((9, 4, 8, 2, 150), conf)
        try:
            n = e.max_batch_windows()
            assert 100000 <= n <= CW_MAX_BATCH_WINDOWS
            if conf is None:
                assert n == CW_MAX_BATCH_WINDOWS
            hb = concat([tiny] * n)
            got = e.run(hb, want_solid=False)
            assert not (got.status == ca.WIN_OVERFLOW).any(), f"cw_configure({conf}): {np.unique(got.status, return_counts=True)}"
            if n < CW_MAX_BATCH_WINDOWS:
                with pytest.raises(ca.EngineError):
                    e.run(concat([tiny] * (n + 1)), want_solid=False)
        finally:
            e.close()


def test_a_window_stopped_on_its_arena_slice_is_corrected_or_stops_never_wrong(aids, monkeypatch):
    """The arena's growth scale is clamped to 32-bit offsets: at tmax 1024, x4 fits a batch of up to 51 781 windows, x2 one of 103 563.
    CW_ARENA_DIV (test aid) divides every window's arena slice so that an ordinary window stops on it (CW_WHY_ARENA) at x1.  Alone the
    plan grows until the window fits and it is corrected; in a batch of 60 000 windows the scale stops at x2 and the window stops
    (status 2, CW_WHY_ARENA) -- the one outcome that include/consent_amd.h says may depend on the batch size.  Never a wrong answer."""
    prm = ca.Params(9, 4, 8, 2, 150)
    probe = synth_pile(1, 30, 4242)
    exp, _ = oracle_lib.oracle_run(prm, probe, threads=THREADS)
    monkeypatch.setenv("CW_ARENA_DIV", "64")
    e = ca.Engine(prm)
    try:
        (a,) = run_at(e, probe, [0])
        assert a.status == int(exp.status[0]) and a.cons == exp.consensus(0), a
    finally:
        e.close()
    big = concat([synth_pile(12000, 4, 200000 + 12000 * i, window_len=100) for i in range(5)])
    hb = insert(big, probe, 30000)
    e = ca.Engine(prm)
    try:
        (b,) = run_at(e, hb, [30000])
        assert (b.status, b.why) == (ca.WIN_OVERFLOW, WHY_ARENA) or (b.status == a.status and b.cons == a.cons), b
        assert b.status == ca.WIN_OVERFLOW, "the window was corrected above the clamp: the header's wording can be narrowed"
    finally:
        e.close()


def test_mixed_batch_fuzz_pass():
    """tools/fuzz_parity.py --mixed, a short seeded pass: windows of many generators in one batch, each compared with its own kind's batch and
    with the oracle; a mixed-only stop counts as a difference."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_parity.py"), "--mixed", "--configs", "4", "--seed", "7"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
