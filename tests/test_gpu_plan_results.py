"""cw_plan_results_device (csrc/cw_pack.h cw_plan_need_kernel, cw_plan_scan_kernel; Engine.plan_results) against a plain statement of the slot rule of
include/consent_amd.h -- the consensus slot by k and template length, the solid slot "k-mers of the pile / solidThresh + 16" -- at the rule's thresholds, the
need kernel's lane stride and the scan's rounds; then the contract that matters: piles cut on the device run into exactly the planned slots, with guard bytes
behind them, and every window is the oracle's.  Last, a run that names its windows by pointer into a larger batch, as csrc/cw_driver.cpp consensus() issues
them.  Integers and bytes: every comparison is exact."""
import numpy as np
import pytest

import consent_amd as ca
import extract_probes as pb
import oracle_lib
from consent_amd import engine as en
from consent_amd.engine import Batch, HostBatch, Result

gpu = pytest.mark.gpu
GUARD = 64
S32, S64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
LIBRARIES = ("product", "aids")


def engine_on(library, prm):
    """An engine of the product library or of the -DCW_TEST_AIDS build of the same sources."""
    if library == "product":
        return ca.Engine(prm)
    prev = en.use_library(en.AIDS_LIB)
    try:
        eng = ca.Engine(prm)
    finally:
        en._LIB = prev
    assert eng.lib is not en.load_library()
    return eng


def cons_slot(k, tpl_len):
    """The header's prose: k >= 9 four templates + 1024, at least 3072; k = 8 sixteen templates + 1024; k < 8 the full 32768; never more than 32768."""
    if k >= 9:
        return min(max(4 * tpl_len + 1024, 3072), 32768)
    if k == 8:
        return min(16 * tpl_len + 1024, 32768)
    return 32768


def plan_reference(k, solid, windows):
    """windows: the sequence lengths of every window's pile, template first -> (cons_off, solid_off), n + 1 entries each."""
    cons, sol = [0], [0]
    for lens in windows:
        cons.append(cons[-1] + cons_slot(k, lens[0] if lens else 0))
        sol.append(sol[-1] + sum(max(0, n - k + 1) for n in lens) // solid + 16)
    return np.array(cons, np.uint64), np.array(sol, np.uint64)


def batch_of(windows):
    """A batch of sequences of these lengths (the planning reads no base)."""
    lens = np.array([n for w in windows for n in w], np.uint32)
    wfs = np.concatenate([[0], np.cumsum([len(w) for w in windows])]).astype(np.uint32)
    words = (lens.astype(np.uint64) + 15) // 16
    return HostBatch(wfs, lens, np.concatenate([[0], np.cumsum(words)[:-1]]).astype(np.uint64) if len(lens) else np.zeros(0, np.uint64), np.zeros(1, np.uint32))


TEMPLATES = (0, 1, 511, 512, 513, 7935, 7936, 7937, 1983, 1984, 1985)


def test_cons_slot_bytes_is_the_headers_rule():
    """The product's own restatement (engine.cons_slot_bytes, what alloc_results and bench.py size by) against the reference above, and the thresholds where
    they are said to be."""
    for k in (2, 7, 8, 9, 10, 16):
        tpl = np.array(sorted(set(TEMPLATES) | set(range(0, 9000, 37))), np.int64)
        assert en.cons_slot_bytes(k, tpl).tolist() == [cons_slot(k, int(t)) for t in tpl], k
    assert [cons_slot(9, t) for t in (0, 511, 512, 513, 7935, 7936, 7937)] == [3072, 3072, 3072, 3076, 32764, 32768, 32768]
    assert [cons_slot(8, t) for t in (0, 1, 1983, 1984, 1985)] == [1024, 1040, 32752, 32768, 32768] and cons_slot(7, 0) == 32768


def window_shapes(k, solid):
    shapes = [[]] + [[t] for t in TEMPLATES if t] + [[k - 1], [k], [k + 1]]
    for n in (63, 64, 65, 129):  # the need kernel's lanes take every 64th sequence
        shapes.append([100] + [5 + (7 * i) % 40 for i in range(n - 1)])
    for m in (1, 10):  # a k-mer total of solid * m - 1 and of solid * m
        for total in (solid * m - 1, solid * m):
            shapes.append([total + k - 1] if m == 1 else [k + 4, total - 5 + k - 1])  # (n bases hold n - k + 1 k-mers; k - 1 bases none)
    return shapes


def batches(k, solid):
    shapes = window_shapes(k, solid)
    yield shapes
    for n in (1, 4, 5, 1023, 1024, 1025, 2049):  # four windows a work-group; the scan's rounds of 1024
        yield [[30 + w % 50] + [(w * 7 + i * 11) % 40 for i in range(w % 4)] if w % 9 else [] for w in range(n)]
    yield [[]] * 3 + shapes[::-1] + [[]]


@gpu
@pytest.mark.parametrize("library", LIBRARIES)
@pytest.mark.parametrize("solid", [1, 4, 5])
@pytest.mark.parametrize("k", [16, 9, 8, 7])
def test_plan_results(k, solid, library):
    """Both arrays hold a sentinel before every call: each entry compared is one the library wrote, entry 0 included."""
    eng = engine_on(library, ca.Params(k, solid, 8, 2, 20))
    for windows in batches(k, solid):
        cons, sol = plan_reference(k, solid, windows)
        g_cons, g_sol, cons_total, solid_total = eng.plan_results(batch_of(windows), fill=S64)
        assert np.array_equal(g_cons, cons) and np.array_equal(g_sol, sol), (len(windows), np.flatnonzero(g_cons != cons)[:4], np.flatnonzero(g_sol != sol)[:4])
        assert (cons_total, solid_total) == (int(cons[-1]), int(sol[-1]))
    assert [sum(max(0, n - k + 1) for n in w) for w in window_shapes(k, solid)[-4:]] == [solid - 1, solid, 10 * solid - 1, 10 * solid]
    g_cons, g_sol, cons_total, solid_total = eng.plan_results(batch_of([]), fill=S64)  # no window: CW_OK (plan_results raises otherwise), totals 0, no launch
    assert (cons_total, solid_total) == (0, 0) and g_cons.tolist() == [S64] == g_sol.tolist()
    eng.close()


class DeviceRun:
    """A batch on the device once, result arrays for all of it with the sentinel in every element and GUARD bytes behind the consensus and solid arrays; runs
    name their windows by pointer, as the driver's do."""

    def __init__(self, eng, hb, cons_off, solid_off):
        import torch

        self.eng, self.hb, self.cons_off, self.solid_off = eng, hb, cons_off, solid_off
        n = hb.n_windows

        def up(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to("cuda:0")

        self.t_in = (up(hb.win_first_seq, np.int32), up(hb.seq_len, np.int32), up(hb.seq_word_off, np.int64), up(np.concatenate([hb.bases, np.zeros(4, np.uint32)]), np.int32))
        self.cons = torch.full((int(cons_off[-1]) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        self.solid = up(np.full(int(solid_off[-1]) + GUARD // 4, S32, np.uint32), np.int32)
        self.coff, self.soff = up(cons_off, np.int64), up(solid_off, np.int64)
        self.clen, self.slen = up(np.full(n, S32, np.uint32), np.int32), up(np.full(n, S32, np.uint32), np.int32)
        self.stat = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda:0")  # (as the driver sets it)
        torch.cuda.synchronize()

    def run(self, w0, w1):
        import torch

        hb = self.hb
        s0, s1 = int(hb.win_first_seq[w0]), int(hb.win_first_seq[w1])
        n_words = int(((hb.seq_len[s0:s1].astype(np.uint64) + 15) // 16).sum())
        wfs, lens, offs, bases = (t.data_ptr() for t in self.t_in)
        b = Batch(w1 - w0, s1 - s0, n_words, wfs + 4 * w0, lens, offs, bases)  # sequence indices and word offsets are the whole batch's
        r = Result(self.cons.data_ptr(), self.coff.data_ptr() + 8 * w0, self.clen.data_ptr() + 4 * w0, self.stat.data_ptr() + w0, self.solid.data_ptr(),
                   self.soff.data_ptr() + 8 * w0, self.slen.data_ptr() + 4 * w0)
        self.eng.run_device(b, r)
        torch.cuda.synchronize()
        return (self.cons.cpu().numpy(), self.clen.cpu().numpy().view(np.uint32), self.stat.cpu().numpy(), self.solid.cpu().numpy().view(np.uint32),
                self.slen.cpu().numpy().view(np.uint32))

    def check(self, got, done, prm):
        """The windows of `done` (ranges run so far) are the oracle's on that slice of the batch; every other element still holds what was sent."""
        cons, clen, stat, solid, slen = got
        co, so = self.cons_off.astype(np.int64), self.solid_off.astype(np.int64)
        cons_free, solid_free, win_free = np.ones(len(cons), bool), np.ones(len(solid), bool), np.ones(len(clen), bool)
        for w0, w1 in done:
            exp, _ = oracle_lib.oracle_run(prm, self.hb.slice(w0, w1))
            for i, w in enumerate(range(w0, w1)):
                assert int(stat[w]) == int(exp.status[i]), (w, int(stat[w]), int(exp.status[i]))
                assert cons[co[w] : co[w] + int(clen[w])].tobytes().decode() == exp.consensus(i), w
                assert np.array_equal(solid[so[w] : so[w] + int(slen[w])], exp.solid_kmers(i)), w
                assert clen[w] <= co[w + 1] - co[w] and slen[w] <= so[w + 1] - so[w]
                cons_free[co[w] : co[w] + int(clen[w])] = False
                solid_free[so[w] : so[w] + int(slen[w])] = False
                win_free[w] = False
        # (a slot's bytes beyond the consensus are the window's to use; what lies outside the run's slots, and the guards, are not)
        for w0, w1 in done:
            cons_free[co[w0] : co[w1]] = False
            solid_free[so[w0] : so[w1]] = False
        assert (cons[cons_free] == 0xA5).all() and (solid[solid_free] == S32).all() and cons_free[-GUARD:].all() and solid_free[-GUARD // 4 :].all()
        assert (clen[win_free] == S32).all() and (slen[win_free] == S32).all() and (stat[win_free] == 0xFF).all()


@gpu
@pytest.mark.parametrize("library", LIBRARIES)
def test_extracted_piles_run_into_exactly_the_planned_slots(library):
    """The geometry probes of k = 9 cut on the device, planned by plan_results and run into those slots: every window's status, consensus and solid set are the
    oracle's, and the 64 bytes behind the consensus and solid arrays stay as they were."""
    probes = [p for p in pb.catalogue() if p.kind == "geometry" and p.k == 9]
    m = pb.merged("geometry", probes)
    prm = ca.Params(9, 4, 8, 2, 20)
    eng = engine_on(library, prm)
    eng.configure(1100)  # the windows of 1024, 1025 and 1040 bases
    hb = eng.extract_piles(ca.pack_piles([m.reads]), np.array(m.ovl, np.uint32), np.array(m.jobs, np.uint32), 9)
    assert hb.n_windows == len(m.jobs) and hb.win_first_seq[-1] > hb.win_first_seq[-2]
    cons_off, solid_off, cons_total, solid_total = eng.plan_results(hb, fill=S64)
    ref = plan_reference(9, 4, [[int(n) for n in hb.seq_len[int(hb.win_first_seq[w]) : int(hb.win_first_seq[w + 1])]] for w in range(hb.n_windows)])
    assert np.array_equal(cons_off, ref[0]) and np.array_equal(solid_off, ref[1])
    dr = DeviceRun(eng, hb, cons_off, solid_off)
    dr.check(dr.run(0, hb.n_windows), [(0, hb.n_windows)], prm)
    eng.close()


@gpu
@pytest.mark.parametrize("library", LIBRARIES)
def test_a_run_names_its_windows_by_pointer_into_the_batch(library):
    """Twelve windows uploaded once; the windows [5, 9) and then all twelve run with win_first_seq + w0 and the whole batch's sequence arrays, results at
    cons_off + w0 and its like: every window equals the oracle on HostBatch.slice, and no result entry outside the run's windows changes."""
    prm = ca.Params(9, 4, 8, 2, 20)
    hb = en.synth_host(ca.SynthSpec.pacbio(12, 8, window_len=120))
    eng = engine_on(library, prm)
    cons_off, solid_off, _, _ = eng.plan_results(hb, fill=S64)
    dr = DeviceRun(eng, hb, cons_off, solid_off)
    dr.check(dr.run(5, 9), [(5, 9)], prm)
    dr.check(dr.run(0, 12), [(0, 12)], prm)
    eng.close()
