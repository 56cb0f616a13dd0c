"""The finish kernel's polish against a plain reference, per route.  Every other GPU test sees cw_finish_kernel through whole-window parity, on piles that
barely polish where the table is large and polish only where it is small.  Here every probe of tests/finish_probes.py -- one window, alone in its batch,
aimed at one edge of the kernel's table, count, bitmap and buffer roads -- runs on the product library and on the test-aid library.  Each run is compared
with the oracle (status, consensus, solid set: that locates a failure) and with the reference built without the oracle's finish (probe.ref.polished); on
the test-aid library the route witness (Engine.finish_route) must be the probe's hand-written route, and its two counters -- frames fin_link entered,
fin_neighbours calls it made -- the oracle's link_calls and nbr_calls exactly.  Then the things one window alone cannot show: the second pass beside
first-pass windows, two waves on their own global bitmaps, the caller's slots to the byte, and a wave's LDS after other windows have used it."""
import ctypes as C

import numpy as np
import pytest

import consent_amd as ca
from consent_amd import engine
from consent_amd.engine import FINISH_ROUTE, Batch, Result, alloc_results, concat_batches, route_names
from finish_probes import BY_NAME, FIN, LONG, PROBES, long_flank_pile, pack

pytestmark = pytest.mark.gpu
ORDERED = sorted(PROBES, key=lambda p: (p.prm, p.name))  # (engines are kept per parameter tuple)
WHY_OUT_CONS, WHY_OUT_SOLID = 12, 13  # csrc/cw_device.h CW_WHY_OUT_CONS, CW_WHY_OUT_SOLID


@pytest.fixture(scope="module")
def engines():
    cache = {}  # at most four engines alive, as in test_gpu_chain.py

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


def assert_window(got, w, probe, what=""):
    """Window w of `got` is the probe's: the oracle's status, consensus and solid set, and the reference's polished string."""
    exp = probe.ref.oracle
    assert int(got.status[w]) == int(exp.status[0]), f"{probe}{what}: status {got.status[w]} != {exp.status[0]}"
    assert got.consensus(w) == exp.consensus(0), f"{probe}{what}: consensus differs from the oracle's"
    assert np.array_equal(got.solid_kmers(w), exp.solid_kmers(0)), f"{probe}{what}: solid set differs from the oracle's"
    assert got.consensus(w) == probe.ref.polished, f"{probe}{what}: consensus differs from the reference's polish"


def run_alone(e, probe):
    got = e.run(probe.hb)
    assert int(got.status[0]) != ca.WIN_OVERFLOW, f"{probe}: stopped, why {int(e.win_info(1)[0, 15])}"
    assert_window(got, 0, probe)
    assert int(e.win_info(1)[0, 15]) == 0, probe  # (a window the second pass took keeps no `why` of the first)
    return e.finish_route()


@pytest.mark.parametrize("probe", ORDERED, ids=repr)
def test_finish_on_the_product_library(probe, engines):
    assert run_alone(engines("product", probe.prm), probe) == (0, 0, 0)  # no witness in the product's kernel


@pytest.mark.parametrize("probe", ORDERED, ids=repr)
def test_finish_route_and_walk_on_the_test_aid_library(probe, engines, aids):
    route, links, nbrs = run_alone(engines("aids", probe.prm), probe)
    assert route == probe.route, f"{probe}: went {route_names(route, FINISH_ROUTE)}, designed for {probe.route_names}"
    assert (links, nbrs) == (probe.ref.link_calls, probe.ref.nbr_calls), f"{probe}: {links} frames and {nbrs} neighbour calls, the oracle {probe.ref.link_calls} and {probe.ref.nbr_calls}"


# ---- several windows --------------------------------------------------------------------------------------------------------------------------
def run_batch(e, probes):
    got = e.run(concat_batches([p.hb for p in probes]))
    for w, p in enumerate(probes):
        assert_window(got, w, p, f" (window {w} of {len(probes)})")
    return got


SECOND_PASS = [p for p in PROBES if "second_pass" in p.route_names]


@pytest.mark.parametrize("which", ["product", "aids"])
def test_second_pass_windows_beside_first_pass_windows(which, engines, request):
    """Every second-pass probe in one batch with three first-pass windows of the same parameters: the same bytes as alone, and both passes wrote."""
    if which == "aids":
        request.getfixturevalue("aids")
    assert len(SECOND_PASS) >= 3 and all(p.prm == LONG for p in SECOND_PASS)
    first = [BY_NAME["the polish fills the buffer: 3062 to 3072"]] * 2 + [FirstPassWindow]
    e = engines(which, LONG)
    for p in SECOND_PASS:
        run_batch(e, [first[0], p, first[1], first[2]])
        assert not e.win_info(4)[:, 15].any()
        if which == "aids":
            assert e.finish_route()[0] & FINISH_ROUTE["first_pass"] and e.finish_route()[0] & FINISH_ROUTE["second_pass"]


class _Short:
    """A short window under the second-pass probes' parameters (flanks of 200 bases), as a probe: its reference comes from finish_probes.build_ref."""
    name, prm = "flanks of 200 bases", LONG

    def __init__(self):
        self._ref = None
        self.pile = long_flank_pile(3, 8, 200, True)
        self.hb = pack(self.pile)

    @property
    def ref(self):
        from finish_probes import build_ref

        if self._ref is None:
            self._ref = build_ref(self.pile, self.prm, self.hb)
            assert len(self._ref.raw) < FIN["CB"] and self._ref.walk.longest < FIN["CB"]
        return self._ref

    def __repr__(self):
        return self.name


FirstPassWindow = _Short()


@pytest.mark.parametrize("which", ["product", "aids"])
@pytest.mark.parametrize("names", [("bitmap k=12 n_solid=32769", "bitmap k=12 n_solid=33000", "bitmap k=12 n_solid=32768", "bitmap k=12 n_solid=32769"),
                                   ("bitmap k=9 n_solid=32769", "bitmap k=9 n_solid=32768", "bitmap k=9 n_solid=32769")], ids=["k=12", "k=9"])
def test_two_waves_on_their_own_global_bitmaps(which, names, engines, request):
    if which == "aids":
        request.getfixturevalue("aids")
    probes = [BY_NAME[n] for n in names]
    e = engines(which, probes[0].prm)
    run_batch(e, probes)
    if which == "aids":
        route, links, nbrs = e.finish_route()
        assert route & FINISH_ROUTE["vis_global"] and route & FINISH_ROUTE["vis_lds"]
        assert (links, nbrs) == (sum(p.ref.link_calls for p in probes), sum(p.ref.nbr_calls for p in probes))


# ---- a wave's LDS after other windows have used it -----------------------------------------------------------------------------------------
REUSE = {"compact": ("compact n_solid=1025", "tie on the compact table", "compact n_solid=2000"),
         "staged": ("staged n_solid=1024", "tie, the allele's letter first", "staged n_solid=64", "all solid", "staged k=9, A x9 solid and on the path", "weak at its first and last characters"),
         "global": ("global n_solid=3841", "tie on the global table")}


@pytest.mark.parametrize("which", ["product", "aids"])
def test_a_waves_lds_is_reused_across_routes(which, engines, request):
    """The compact table runs through the bitmap and the key slots, staged counts sit 64 words into the bitmap, and the bitmap is cleared only for the words
    this window's solid k-mers need: more windows than the first pass has waves, interleaved compact -> staged -> global -> compact ..., in two orders;
    every window's bytes are those of the probe alone (which are the reference's)."""
    import torch

    if which == "aids":
        request.getfixturevalue("aids")
    prm = BY_NAME[REUSE["compact"][0]].prm
    assert all(BY_NAME[n].prm == prm and r in BY_NAME[n].route_names for r, names in REUSE.items() for n in names)
    waves = FIN["WAVES"] * FIN["WGS_PER_CU"] * torch.cuda.get_device_properties(0).multi_processor_count
    e = engines(which, prm)
    for order in (("compact", "staged", "global"), ("global", "staged", "compact", "staged")):
        probes, i = [], 0
        while len(probes) <= waves + 64:
            for road in order:
                probes.append(BY_NAME[REUSE[road][i % len(REUSE[road])]])
            i += 1
        got = e.run(concat_batches([p.hb for p in probes]))
        assert not (got.status == ca.WIN_OVERFLOW).any()
        bad = [(w, p) for w, p in enumerate(probes) if got.consensus(w) != p.ref.polished or not np.array_equal(got.solid_kmers(w), p.ref.oracle.solid_kmers(0))]
        assert not bad, f"order {order}: {len(bad)} of {len(probes)} windows differ from their probe alone, the first: {bad[:4]}"


# ---- the caller's slots ------------------------------------------------------------------------------------------------------------------------
GUARD = 0xEE


def run_with_slots(e, probes, cons_caps, solid_caps):
    """cw_run_device with the given slot sizes (None: what alloc_results gives), every byte of both result arrays and 64 more behind them set to a guard
    value first: (results, cons array, solid array) as they come back."""
    import torch

    hb = concat_batches([p.hb for p in probes])
    res = alloc_results(hb, True, e.params.solid, e.params.k)
    for off, caps in ((res.cons_off, cons_caps), (res.solid_off, solid_caps)):
        sizes = np.diff(off.astype(np.int64))
        for w, c in enumerate(caps):
            if c is not None:
                sizes[w] = c
        off[1:] = np.cumsum(sizes)
    dev = torch.device("cuda", 0)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)
    t_in = (up(hb.win_first_seq, np.int32), up(hb.seq_len, np.int32), up(hb.seq_word_off, np.int64), up(np.concatenate([hb.bases, np.zeros(4, np.uint32)]), np.int32))
    W = hb.n_windows
    t_out = [torch.full((int(res.cons_off[-1]) + 64,), GUARD, dtype=torch.uint8, device=dev), up(res.cons_off, np.int64), torch.zeros(W, dtype=torch.int32, device=dev),
             torch.full((W,), 255, dtype=torch.uint8, device=dev), torch.full((4 * (int(res.solid_off[-1]) + 16),), GUARD, dtype=torch.uint8, device=dev), up(res.solid_off, np.int64),
             torch.zeros(W, dtype=torch.int32, device=dev)]
    torch.cuda.synchronize(dev)
    e.run_device(Batch(W, len(hb.seq_len), len(hb.bases), *[t.data_ptr() for t in t_in]), Result(*[t.data_ptr() for t in t_out]))
    torch.cuda.synchronize()
    cons, solid = t_out[0].cpu().numpy(), t_out[4].cpu().numpy().view(np.uint32)
    res.cons, res.solid = cons, solid
    res.cons_len[:] = t_out[2].cpu().numpy().view(np.uint32)
    res.status[:] = t_out[3].cpu().numpy()
    res.solid_len[:] = t_out[6].cpu().numpy().view(np.uint32)
    return res


def assert_guards(res, what):
    """Outside the entries each window reports, both arrays still hold the guard value: behind every consensus and solid set up to the next slot, in all of a
    stopped window's solid slot, and behind the last slot.  (A stopped window's own consensus slot is not looked at: the kernel may have written a consensus
    there before it found the solid slot too small -- the bytes are the window's, and it reports none of them.)"""
    for arr, off, lens, guard in ((res.cons, res.cons_off, res.cons_len, GUARD), (res.solid, res.solid_off, res.solid_len, GUARD * 0x01010101)):
        for w in range(len(lens)):
            if arr is res.cons and int(res.status[w]) == ca.WIN_OVERFLOW:
                continue
            rest = arr[int(off[w]) + int(lens[w]) : int(off[w + 1])]
            assert (rest == guard).all(), f"{what}: window {w} wrote behind its {int(lens[w])} entries"
        assert (arr[int(off[-1]) :] == guard).all(), f"{what}: written behind the last slot"


SLOT_CASES = [("consensus slot exact", "cons", 0, 0), ("consensus slot one short", "cons", -1, WHY_OUT_CONS), ("solid slot exact", "solid", 0, 0), ("solid slot one short", "solid", -1, WHY_OUT_SOLID),
              ("template slot exact", "tpl", 0, 0), ("template slot one short", "tpl", -1, WHY_OUT_CONS)]


@pytest.mark.parametrize("which", ["product", "aids"])
@pytest.mark.parametrize("case", SLOT_CASES, ids=lambda c: c[0])
def test_the_callers_slots_to_the_byte(which, case, engines, request):
    """An exact slot is written in full; a slot one short stops the window with the right `why`, no consensus and no solid set, and nothing is written into
    it; the bytes between the windows' own and behind the last slot keep their guard value; the other windows of the batch are what they are alone.
    The shrunken window is once the batch's middle window and once its last."""
    if which == "aids":
        request.getfixturevalue("aids")
    what, kind, short, why = case
    target = BY_NAME["a template shorter than k" if kind == "tpl" else "staged n_solid=128"]
    others = [BY_NAME["staged n_solid=64"], BY_NAME["all solid"]]
    e = engines(which, target.prm)
    assert all(p.prm == target.prm for p in others)
    for at in (1, 2):
        probes = others[:at] + [target] + others[at:]
        cons_caps, solid_caps = [None] * 3, [None] * 3
        if kind == "solid":
            solid_caps[at] = target.ref.n_solid + short
        else:
            cons_caps[at] = len(target.ref.polished) + short
        res = run_with_slots(e, probes, cons_caps, solid_caps)
        info = e.win_info(3)
        for w, p in enumerate(probes):
            if w == at and short:
                assert (int(res.status[w]), int(res.cons_len[w]), int(res.solid_len[w]), int(info[w, 15])) == (ca.WIN_OVERFLOW, 0, 0, why), f"{what} at {at}: {res.status[w]}, {res.cons_len[w]}, {res.solid_len[w]}, why {info[w, 15]}"
            else:
                assert_window(res, w, p, f" ({what}, window {w})")
                assert int(info[w, 15]) == 0
        assert_guards(res, f"{what} at {at}")
