"""The seed run on the device (include/consent_amd.h cw_seed_run / cw_seed_run_device; Engine.seeds, place, polish_reads): every row and strand byte equals the
plain reference (tests/seed_probes.py) exactly, at k = 8, 11 and 15, over the strand vote's whole catalogue -- the edges of k and of the packed words, both sides
of the boundary between the launch classes, the capacities, the dense 16 383-base table, the group of several units -- and the seed run's own probes: repeats,
ties, bin edges, overhangs; nothing else is written; the bytes do not depend on the batch; the other runs of the engine do not notice it; and a contig longer
than a tile is placed on and polished from an unsorted bag of reads as the reference says."""
import ctypes as C

import numpy as np
import pytest

import consent_amd as ca
import seed_probes as sd
import strand_probes as st
import sw_op_probes as sp
from consent_amd.engine import Batch, HostBatch, Seeds, _ptr, synth_host

pytestmark = pytest.mark.gpu
E_INVALID = -1
FILL = 0x0BADBEEF
GUARD = 8


@pytest.fixture(scope="module")
def eng():
    e = ca.Engine(ca.Params(*sp.PRM))
    yield e
    e.close()


def seed(eng, groups, k, want_strand=True):
    """cw_seed_run on host buffers prefilled with a pattern: (rows, strand bytes or None)."""
    hb = groups if isinstance(groups, HostBatch) else ca.pack_piles(groups)
    S = len(hb.seq_len)
    rows = np.full(sd.ROW * S + GUARD, FILL, np.int32)
    strand = np.full(S + GUARD, 0x5A, np.uint8)
    b = hb.c_struct()
    out = Seeds(_ptr(rows), _ptr(strand) if want_strand else None, k)
    assert eng.lib.cw_seed_run(eng.handle, C.byref(b), C.byref(out)) == 0
    assert (rows[sd.ROW * S :] == FILL).all() and (strand[S if want_strand else 0 :] == 0x5A).all(), "bytes behind the outputs were written"
    return rows[: sd.ROW * S].reshape(S, sd.ROW), strand[:S] if want_strand else None


def check_exact(eng, groups, k, what):
    rows, strand = seed(eng, groups, k)
    want = sd.expected(groups, k)
    got = [tuple(int(v) for v in r) for r in rows]
    wrong = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    tally = {v: sum(1 for w in want if w[0] == v) for v in (sd.FWD, sd.REV, sd.IS_REF, sd.NONE)}
    print(f"{what}, k = {k}: {len(want)} sequences, forward / reverse / reference / none {tally[sd.FWD]} / {tally[sd.REV]} / {tally[sd.IS_REF]} / {tally[sd.NONE]}")
    assert not wrong, f"{what}, k = {k}: (sequence, got, want) {wrong[:5]}"
    assert [int(v) for v in strand] == [w[0] for w in want], "a strand byte is not its row's status"
    return want


# ---- the rows against the plain reference ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", sd.KS)
@pytest.mark.parametrize("name", ["edges", "boundary", "sets", "spread", "seeds"])
def test_every_row_equals_the_plain_reference(eng, name, k):
    groups = sd.catalogue(k)[name]
    want = check_exact(eng, groups, k, name)
    first = np.cumsum([0] + [len(g) for g in groups])
    if name == "boundary":  # references of k - 1, k, 2 048, 2 049, 16 383, 16 384 bases: both classes, both capacities
        assert [len(g[0]) for g in groups] == [k - 1, k, st.LDS_RMAX, st.LDS_RMAX + 1, st.RMAX, st.RMAX + 1]
        assert [w[0] for w in want[first[5] + 1 : first[6]]] == [sd.NONE] * 3 and [w[0] for w in want[first[0] + 1 : first[1]]] == [sd.NONE] * 3
        assert len(groups[3][-2]) == st.QMAX and want[first[4] - 2][0] == sd.REV and want[first[4] - 1] == (sd.NONE, 0, 0, 0)
        for g in (2, 3, 4):  # the copy and the reverse complement, exact slices: every position a hit unless its k-mer repeats, all on one diagonal
            assert [w[0] for w in want[first[g] + 1 : first[g] + 3]] == [sd.FWD, sd.REV], g
            assert all(w[1] > 200 and w[1] >= 4 * w[3] for w in want[first[g] + 1 : first[g] + 3]), g
    if name == "sets":
        assert want[1] == (sd.FWD, 0, -77, 0) and want[2] == (sd.FWD, 0, -77, 0)  # poly-A against poly-A: the one k-mer is everywhere, no seed
        if k == 8:
            assert len(groups[2][0]) == st.RMAX and want[first[2] + 1][0] == sd.FWD and want[first[2] + 2][0] == sd.REV  # the dense table
    if name == "spread":
        assert {w[0] for w in want[1:]} == {sd.FWD, sd.REV} and len(want) == 301
    if name == "edges":
        assert want[-1] == (sd.IS_REF, 0, 0, 0) and (sd.NONE, 0, 0, 0) in want and groups[0][-1] == ""
    if name == "seeds":
        assert min(w[2] for w in want) < -100 and any(w[0] == sd.REV and w[2] < 0 for w in want)  # negative DIAG, both strands


def test_k_of_0_is_k_of_11_and_the_strand_bytes_may_be_null(eng):
    groups = sd.catalogue(11)["edges"] + sd.catalogue(11)["seeds"]
    r0, s0 = seed(eng, groups, 0)
    r11, s11 = seed(eng, groups, 11)
    assert np.array_equal(r0, r11) and np.array_equal(s0, s11) and [tuple(int(v) for v in r) for r in r0] == sd.expected(groups, 0)
    rows, none = seed(eng, groups, 11, want_strand=False)
    assert none is None and np.array_equal(rows, r11)
    view = eng.seeds(groups, 11)  # the binding's view of the same
    assert np.array_equal(view.rows, r11) and np.array_equal(view.strands, s11) and tuple(view.row(1, 0)) == (sd.IS_REF, 0, 0, 0)
    assert eng.timings().keys() == {"strand_order", "seed", "seed_wide", "total"}


def test_the_bytes_do_not_depend_on_the_batch(eng):
    k = 11
    groups = [g for part in sd.catalogue(k).values() for g in part]
    together, together_s = seed(eng, groups, k)
    alone = [seed(eng, [g], k) for g in groups]
    assert np.array_equal(np.concatenate([a[0] for a in alone]), together) and np.array_equal(np.concatenate([a[1] for a in alone]), together_s)
    rev, rev_s = seed(eng, groups[::-1], k)
    first = np.cumsum([0] + [len(g) for g in groups[::-1]])
    assert np.array_equal(np.concatenate([rev[first[i] : first[i + 1]] for i in range(len(groups))][::-1]), together)
    assert np.array_equal(np.concatenate([rev_s[first[i] : first[i + 1]] for i in range(len(groups))][::-1]), together_s)


# ---- the device entry point ------------------------------------------------------------------------------------------------------------------------------------------

def test_the_device_entry_point_writes_its_outputs_and_nothing_else(eng):
    import torch

    dev = torch.device("cuda", eng.device)

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    k = 11
    groups = sd.catalogue(k)["seeds"] + sd.catalogue(k)["spread"] + [sd.catalogue(k)["boundary"][3][:4]]  # both launch classes
    hb = ca.pack_piles(groups)
    S = len(hb.seq_len)
    keep = (up(hb.win_first_seq, np.int32), up(hb.seq_len, np.int32), up(hb.seq_word_off, np.int64), up(np.concatenate([hb.bases, np.zeros(1, np.uint32)]), np.int32))
    t_rows = torch.full((sd.ROW * S + GUARD,), FILL, dtype=torch.int32, device=dev)
    t_strand = torch.full((S + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    b = Batch(hb.n_windows, S, len(hb.bases), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr())
    torch.cuda.synchronize(dev)
    fn = eng.lib.cw_seed_run_device
    for bad_k in (7, 16):
        assert fn(eng.handle, C.byref(b), C.byref(Seeds(t_rows.data_ptr(), t_strand.data_ptr(), bad_k)), None) == E_INVALID
    big = Batch(eng.max_batch_windows() + 1, S, len(hb.bases), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr())
    assert fn(eng.handle, C.byref(big), C.byref(Seeds(t_rows.data_ptr(), t_strand.data_ptr(), k)), None) == E_INVALID
    assert fn(eng.handle, C.byref(b), C.byref(Seeds(None, t_strand.data_ptr(), k)), None) == E_INVALID and fn(eng.handle, C.byref(b), None, None) == E_INVALID
    assert fn(eng.handle, None, C.byref(Seeds(t_rows.data_ptr(), None, k)), None) == E_INVALID
    none = Batch(0, 0, 0, None, None, None, None)  # no sequence: CW_OK, nothing launched
    assert fn(eng.handle, C.byref(none), C.byref(Seeds(t_rows.data_ptr(), None, k)), None) == 0
    torch.cuda.synchronize(dev)
    assert (t_rows.cpu().numpy() == FILL).all() and (t_strand.cpu().numpy() == 0x5A).all(), "a refused call wrote something"
    eng.seed_device(b, Seeds(t_rows.data_ptr(), t_strand.data_ptr(), k))
    torch.cuda.synchronize(dev)
    assert eng.timings().keys() == {"strand_order", "seed", "seed_wide", "total"}
    got_r, got_s = t_rows.cpu().numpy(), t_strand.cpu().numpy()
    want = sd.expected(groups, k)
    assert (got_r[sd.ROW * S :] == FILL).all() and (got_s[S:] == 0x5A).all(), "bytes behind the outputs were written"
    assert got_r[: sd.ROW * S].reshape(S, sd.ROW).tolist() == [list(w) for w in want] and [int(v) for v in got_s[:S]] == [w[0] for w in want]


# ---- beside the other runs ---------------------------------------------------------------------------------------------------------------------------------------------

def test_a_seed_run_between_the_other_runs_leaves_their_results_as_they_were(eng):
    windows = synth_host(ca.SynthSpec.pacbio(6, 12))
    piles = [windows.pile(w)[:6] for w in range(3)]
    pairs = sd.catalogue(11)["seeds"][4:6]

    def others():
        run = eng.run(windows)
        poa = eng.poa(piles)
        sw = eng.sw(pairs, want_indels=True)
        return ([run.consensus(w) for w in range(windows.n_windows)], run.status.tolist(), [poa.consensus(g) for g in range(len(piles))], poa.status.tolist(), sw.rows.tolist())

    before = others()
    rows, _ = seed(eng, pairs, 11)
    run = eng.run(windows)  # a window run right behind a seed run, which used the same scratch
    assert [run.consensus(w) for w in range(windows.n_windows)] == before[0]
    again, _ = seed(eng, pairs, 11)
    assert others() == before and np.array_equal(rows, again) and [tuple(int(v) for v in r) for r in rows] == sd.expected(pairs, 11)


# ---- a contig and a bag of reads -----------------------------------------------------------------------------------------------------------------------------------------

def contig():
    draft, reads, where, other = sd.draft_and_reads(**sd.CONTIG)
    return draft, list(reads) + [other[0]], where  # the last read belongs nowhere


@pytest.mark.parametrize("tile", [1000, 2100])  # tiles of the narrow and of the wide launch class; 3 000 bases: three tiles, and two with a shorter last one
def test_place_equals_the_reference_placements(eng, tile):
    draft, bag, where = contig()
    want = sd.place(draft, bag, tile, 0)
    got = eng.place(draft, bag, tile=tile)
    assert [None if p is None else (p.strand, p.position, p.hits, p.other) for p in got] == want
    assert got[-1] is None and None not in got[:-1]  # the unrelated read comes back None, every planted one is placed
    assert [p.strand for p in got[:-1]] == [sd.REV if turned else sd.FWD for _, turned in where]
    everything = eng.place(draft, bag, tile=tile, min_hits=0)
    assert everything[-1] is not None and everything[-1].hits < ca.SEED_MIN_HITS and everything[:-1] == got[:-1]
    with pytest.raises(ca.EngineError):
        eng.place(draft, bag, tile=tile, k=8)  # the default threshold is measured for k >= 11
    assert eng.place(draft, [], tile=tile) == [] and eng.place("", bag[:2], tile=tile) == [None, None]


@pytest.mark.parametrize("tile", [1000, 2100])
def test_polish_reads_equals_polish_of_the_reference_groups(eng, tile):
    draft, bag, where = contig()
    groups = sd.polish_groups(draft, bag, tile, 0)
    want = eng.polish(groups, 100)
    got = eng.polish_reads(draft, bag, window=100, tile=tile)
    assert got.sequence == "".join(p.sequence for p in want)
    assert [(w.members, w.status, w.kept_reference) for w in got.windows] == [(w.members, w.status, w.kept_reference) for p in want for w in p.windows]
    assert got.placements == eng.place(draft, bag, tile=tile) and got.placements[-1] is None
    assert len(got.windows) == 30 and max(w.members for w in got.windows) >= 3  # (the reads reach their windows: the placement is of use)
    with pytest.raises(ca.EngineError):
        eng.polish_reads(draft, bag, window=300, tile=1000)
