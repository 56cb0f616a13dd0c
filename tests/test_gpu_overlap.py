"""The overlap run on the device (include/consent_amd.h cw_overlap_*; Engine.overlap_index, overlap_rows, overlaps): every row, count and status equals the plain
reference (tests/overlap_probes.py) exactly -- over the probe families at k = 8, 11, 15 with and without sampling; at the edges of max_occ, of the slots and of
the read lengths; on both routes of the kernel; from one build over many runs in any split and order; nothing else is written; the refusals; beside the other
runs of the engine; host form and device form; the pile tuples; and the planted set of the CPU test through Engine.overlaps."""
import ctypes as C

import numpy as np
import pytest

import consent_amd as ca
import overlap_probes as op
import seed_probes as sd
import sw_op_probes as sp
from consent_amd.engine import Batch, OverlapIndexRef, OverlapParams, Overlaps, _ptr, synth_host

pytestmark = pytest.mark.gpu
E_INVALID, E_CAPACITY = -1, -4
FILL = 0x0BADBEEF
GUARD = 16


@pytest.fixture(scope="module")
def eng():
    e = ca.Engine(ca.Params(*sp.PRM))
    yield e
    e.close()


def same(got, want, what, first=0):
    """An OverlapRows against the reference's list of (status, n_rows, rows)."""
    assert len(got.status) == len(want)
    wrong = []
    for j, (status, n, rows) in enumerate(want):
        mine = [tuple(r) for r in got.of(j).tolist()] if got.status[j] == op.OK else []
        if (int(got.status[j]), int(got.n_rows[j]), mine) != (status, n, rows):
            wrong.append((first + j, int(got.status[j]), int(got.n_rows[j]), mine[:2], status, n, rows[:2]))
    assert not wrong, f"{what}: (query, got status / rows / first rows, want the same) {wrong[:3]}"


# ---- 1. the families -------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [8, 11, 15])
@pytest.mark.parametrize("sample", [0, 3])
def test_every_row_of_the_families_equals_the_plain_reference(eng, k, sample):
    for name, reads in (("family", op.family(k)[0]), ("geometry", op.geometry(k))):
        want = op.expected(reads, k, sample, 0, 2)
        index = eng.overlap_index(reads, k, sample)
        assert index.n_entries == op.Index(reads, k, sample).n_entries
        same(eng.overlap_rows(index, min_hits=2), want, f"{name}, k = {k}, sample = {sample}")
        if sample == 0:
            assert sum(w[1] for w in want) > 20
    assert eng.timings().keys() == {"ovl", "ovl_dense", "total"}


def test_k_zero_is_fifteen_and_the_default_sample_is_three(eng):
    reads = op.family(15)[0]
    same(eng.overlap_rows(eng.overlap_index(reads), min_hits=1), op.expected(reads, 15, 3, 0, 1), "the defaults")


# ---- 2. the edges ----------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_kmer_at_max_occ_votes_and_one_beyond_does_not(eng):
    reads, xs, ys = op.occurrence_edges()
    index = eng.overlap_index(reads, 11, 0, 3)
    got = eng.overlap_rows(index, min_hits=1)
    same(got, op.expected(reads, 11, 0, 3, 1), "max_occ = 3")
    assert [int(n) for n in got.n_rows] == [2, 2, 2, 0, 0, 0, 0]
    same(eng.overlap_rows(eng.overlap_index(reads, 11, 0, 4), min_hits=1), op.expected(reads, 11, 0, 4, 1), "max_occ = 4")


def test_a_read_beyond_the_longest_query_is_no_query_and_no_target(eng):
    reads = op.too_long()
    want = op.expected(reads, 15, 0, 0, 2)
    got = eng.overlap_rows(eng.overlap_index(reads, 15, 0), min_hits=2)
    same(got, want, "CW_SW_QMAX + 1 bases")
    assert int(got.status[1]) == op.NONE and all(int(r[0]) != 1 for j in range(len(reads)) for r in got.of(j))


def test_a_slot_exactly_full_one_short_and_of_no_row(eng):
    reads = op.family(11)[0]
    free = op.expected(reads, 11, 0, 0, 2)
    need = [w[1] for w in free]
    busy = [j for j, n in enumerate(need) if n >= 2]
    slots = list(need)
    slots[busy[0]] -= 1  # one short
    slots[busy[1]] = 0   # no slot at all
    want = op.expected(reads, 11, 0, 0, 2, slots=slots)
    assert [w[0] for w in want].count(op.SLOT) == 2 and want[busy[2]][0] == op.OK  # (every other slot is exactly full)
    index = eng.overlap_index(reads, 11, 0)
    got = eng.overlap_rows(index, min_hits=2, slots=slots, grow=False)
    same(got, want, "slots")
    assert int(got.n_rows[busy[0]]) == need[busy[0]] and (got.rows[int(got.row_off[busy[0]]) : int(got.row_off[busy[0] + 1])] == 0).all()  # the count, and no word
    same(eng.overlap_rows(index, min_hits=2, slots=1), free, "grown slots")  # the second run with the slots the counts ask for


# ---- 3. the dense route ----------------------------------------------------------------------------------------------------------------------------------------------

def test_a_query_with_more_distinct_keys_than_the_lds_table_takes_goes_the_dense_route(eng):
    reads = op.dense_reads()
    k, min_hits = op.DENSE_SET["k"], op.DENSE_SET["min_hits"]
    ix = op.Index(reads, k, 0)
    keys = [op.distinct_keys(ix, q) for q in range(len(reads))]
    assert keys[0] > op.LDS_CAP >= max(keys[1:])
    want = op.expected(None, min_hits=min_hits, ix=ix)
    index = eng.overlap_index(reads, k, 0)
    got = eng.overlap_rows(index, min_hits=min_hits, slots=64)
    assert eng.overlap_routes() == (len(reads) - 1, 1)
    same(got, want, "the dense route")
    assert want[0][1] > 10
    part = eng.overlap_rows(index, 1, 50, min_hits=min_hits)  # a range without the long query: nobody goes the dense route
    assert eng.overlap_routes() == (50, 0)
    same(part, want[1:51], "queries 1 .. 50", 1)


# ---- 4. one build, many runs -------------------------------------------------------------------------------------------------------------------------------------------

def test_one_index_answers_any_split_in_any_order_and_its_memory_serves_the_next_set(eng):
    reads = op.family(15)[0]
    want = op.expected(reads, 15, 0, 0, 2)
    index = eng.overlap_index(reads, 15, 0)
    half = len(reads) // 2
    whole = eng.overlap_rows(index, min_hits=2)
    b = eng.overlap_rows(index, half, None, min_hits=2)  # the second half first
    a = eng.overlap_rows(index, 0, half, min_hits=2)
    same(whole, want, "one call")
    same(a, want[:half], "the first half", 0)
    same(b, want[half:], "the second half", half)
    same(eng.overlap_rows(index, 3, 0, min_hits=2), [], "no query")
    # a second, smaller read set built into the same memory: the build clears it first
    other = op.geometry(15)
    second = eng.overlap_index(other, 15, 0)
    assert second.n_entries < index.n_entries
    second.mem = index.mem
    b2, ref = second.batch(), second.c_struct(1)
    assert eng.lib.cw_overlap_build_device(eng.handle, C.byref(b2), C.byref(ref), None) == 0
    same(eng.overlap_rows(second, min_hits=2), op.expected(other, 15, 0, 0, 2), "the second set in the first one's memory")


# ---- 5. the device entry points write their outputs and nothing else -------------------------------------------------------------------------------------------------

def test_the_device_entry_points_write_their_outputs_and_nothing_else(eng):
    import torch

    reads = op.family(11)[0]
    want = op.expected(reads, 11, 3, 0, 1)
    index = eng.overlap_index(reads, 11, 3)
    dev, S = index.mem.device, len(reads)
    words = int(eng.lib.cw_overlap_index_words(index.n_entries))
    mem = torch.full((GUARD + words + GUARD,), FILL, dtype=torch.int32, device=dev)
    slots = np.array([w[1] for w in want], np.uint64) + 1  # a row to spare in every slot
    row_off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(slots)])
    t_off = torch.from_numpy(row_off.view(np.int64)).to(dev)
    total = int(row_off[-1]) * op.ROW
    t_rows = torch.full((GUARD + total + GUARD,), FILL, dtype=torch.int32, device=dev)
    t_n = torch.full((GUARD + S + GUARD,), FILL, dtype=torch.int32, device=dev)
    t_status = torch.full((GUARD + S + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    b = index.batch()
    ref = OverlapIndexRef(mem.data_ptr() + 4 * GUARD, index.n_entries, OverlapParams(11, 3, 0, 1))
    n = C.c_uint64()
    assert eng.lib.cw_overlap_count_device(eng.handle, C.byref(b), C.byref(ref.prm), C.byref(n), None) == 0 and n.value == index.n_entries
    assert eng.timings().keys() == {"ovl_count", "total"}
    assert eng.lib.cw_overlap_build_device(eng.handle, C.byref(b), C.byref(ref), None) == 0
    torch.cuda.synchronize(dev)
    assert eng.timings().keys() == {"ovl_build_count", "ovl_build_insert", "ovl_build_assign", "ovl_build_fill", "total"}
    built = mem.cpu().numpy().view(np.uint32)
    assert (built[:GUARD] == FILL).all() and (built[GUARD + words :] == FILL).all(), "words round the index were written"
    out = Overlaps(t_rows.data_ptr() + 4 * GUARD, t_off.data_ptr(), t_n.data_ptr() + 4 * GUARD, t_status.data_ptr() + GUARD)
    eng.overlap_device(ref, b, 0, S, out)
    torch.cuda.synchronize(dev)
    rows, n_rows, status = t_rows.cpu().numpy(), t_n.cpu().numpy().view(np.uint32), t_status.cpu().numpy()
    assert (rows[:GUARD] == FILL).all() and (rows[GUARD + total :] == FILL).all() and (n_rows[:GUARD] == FILL).all() and (n_rows[GUARD + S :] == FILL).all()
    assert (status[:GUARD] == 0x5A).all() and (status[GUARD + S :] == 0x5A).all()
    got = ca.OverlapRows(rows[GUARD : GUARD + total].reshape(-1, op.ROW), row_off, n_rows[GUARD : GUARD + S], status[GUARD : GUARD + S], 0)
    same(got, want, "guarded outputs")
    for j in range(S):  # the spare row of every slot, and the whole slot of a query without rows
        assert (got.rows[int(row_off[j]) + want[j][1] : int(row_off[j + 1])] == FILL).all(), j
    assert np.array_equal(mem.cpu().numpy().view(np.uint32), built), "a run wrote the index"
    # an index built for another count is no index: every query says so, and no row is written
    bad = OverlapIndexRef(mem.data_ptr() + 4 * GUARD, index.n_entries - 1, ref.prm)
    if int(eng.lib.cw_overlap_index_words(index.n_entries - 1)) <= words:
        assert eng.lib.cw_overlap_build_device(eng.handle, C.byref(b), C.byref(bad), None) == 0
        t_rows.fill_(FILL)
        torch.cuda.synchronize(dev)
        eng.overlap_device(bad, b, 0, S, out)
        torch.cuda.synchronize(dev)
        assert (t_status.cpu().numpy()[GUARD : GUARD + S] == op.BAD_INDEX).all() and (t_n.cpu().numpy()[GUARD : GUARD + S] == 0).all() and (t_rows.cpu().numpy() == FILL).all()


# ---- 6. the refusals ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_what_is_refused_is_refused_before_anything_is_written(eng):
    import torch

    reads = op.geometry(11)
    index = eng.overlap_index(reads, 11, 0)
    dev, S = index.mem.device, len(reads)
    b, ref = index.batch(), index.c_struct(2)
    before = index.mem.clone()
    t_off = torch.arange(0, 8 * (S + 1), 8, dtype=torch.int64, device=dev)
    t_rows = torch.full((8 * S * op.ROW,), FILL, dtype=torch.int32, device=dev)
    t_n, t_status = torch.full((S,), FILL, dtype=torch.int32, device=dev), torch.full((S,), 0x5A, dtype=torch.uint8, device=dev)
    out = Overlaps(t_rows.data_ptr(), t_off.data_ptr(), t_n.data_ptr(), t_status.data_ptr())
    torch.cuda.synchronize(dev)
    count, build, run = eng.lib.cw_overlap_count_device, eng.lib.cw_overlap_build_device, eng.lib.cw_overlap_run_device
    n = C.c_uint64(77)
    prm_of = lambda **kw: OverlapParams(*[kw.get(f, getattr(ref.prm, f)) for f in ("k", "sample", "max_occ", "min_hits")])
    for bad in (prm_of(k=7), prm_of(k=16), prm_of(sample=9), prm_of(max_occ=65536)):
        assert count(eng.handle, C.byref(b), C.byref(bad), C.byref(n), None) == E_INVALID
        bad_ix = OverlapIndexRef(ref.mem, ref.n_entries, bad)
        assert build(eng.handle, C.byref(b), C.byref(bad_ix), None) == E_INVALID and run(eng.handle, C.byref(bad_ix), C.byref(b), 0, S, C.byref(out), None) == E_INVALID
    zero_hits = OverlapIndexRef(ref.mem, ref.n_entries, prm_of(min_hits=0))
    assert run(eng.handle, C.byref(zero_hits), C.byref(b), 0, S, C.byref(out), None) == E_INVALID
    assert count(eng.handle, None, C.byref(ref.prm), C.byref(n), None) == E_INVALID and count(eng.handle, C.byref(b), None, C.byref(n), None) == E_INVALID
    assert count(eng.handle, C.byref(b), C.byref(ref.prm), None, None) == E_INVALID and n.value == 77
    for bad_ix in (OverlapIndexRef(None, ref.n_entries, ref.prm), OverlapIndexRef(ref.mem + 4, ref.n_entries, ref.prm), OverlapIndexRef(ref.mem, 1 << 32, ref.prm)):
        assert build(eng.handle, C.byref(b), C.byref(bad_ix), None) == E_INVALID and run(eng.handle, C.byref(bad_ix), C.byref(b), 0, S, C.byref(out), None) == E_INVALID
    assert build(eng.handle, None, C.byref(ref), None) == E_INVALID and build(eng.handle, C.byref(b), None, None) == E_INVALID
    many = Batch(0, 1 << 24, b.n_words, None, b.seq_len, b.seq_word_off, b.bases)
    assert count(eng.handle, C.byref(many), C.byref(ref.prm), C.byref(n), None) == E_INVALID
    assert run(eng.handle, C.byref(ref), C.byref(b), 1, S, C.byref(out), None) == E_INVALID and run(eng.handle, C.byref(ref), C.byref(b), S, 1, C.byref(out), None) == E_INVALID
    assert run(eng.handle, C.byref(ref), C.byref(b), 0, S, None, None) == E_INVALID and run(eng.handle, None, C.byref(b), 0, S, C.byref(out), None) == E_INVALID
    for hole in ("rows", "row_off", "n_rows", "status"):
        bad_out = Overlaps(*[None if f == hole else getattr(out, f) for f in ("rows", "row_off", "n_rows", "status")])
        assert run(eng.handle, C.byref(ref), C.byref(b), 0, S, C.byref(bad_out), None) == E_INVALID
    assert run(eng.handle, C.byref(ref), C.byref(b), S, 0, C.byref(out), None) == 0  # no query: CW_OK, nothing launched
    torch.cuda.synchronize(dev)
    assert (t_rows.cpu().numpy() == FILL).all() and (t_status.cpu().numpy() == 0x5A).all() and torch.equal(index.mem, before), "a refused call wrote something"
    with pytest.raises(ca.EngineError):
        eng.overlaps(reads, k=11)  # the default threshold is measured for k = 15
    assert eng.overlaps([]) == [] and eng.overlaps(["ACGT", ""]) == [[], []]


# ---- 7. beside the other runs ------------------------------------------------------------------------------------------------------------------------------------------

def test_an_overlap_run_between_the_other_runs_leaves_their_results_as_they_were(eng):
    windows = synth_host(ca.SynthSpec.pacbio(6, 12))
    piles = [windows.pile(w)[:6] for w in range(3)]
    pairs = sd.catalogue(11)["seeds"][4:6]
    reads = op.geometry(11)
    want = op.expected(reads, 11, 0, 0, 2)

    def others():
        run = eng.run(windows)
        poa = eng.poa(piles)
        placed = eng.locate_rows(eng.locate_index(pairs[0][0], 11), pairs[0][1:])
        return ([run.consensus(w) for w in range(windows.n_windows)], run.status.tolist(), [poa.consensus(g) for g in range(len(piles))], poa.status.tolist(), placed.rows.tolist())

    before = others()
    index = eng.overlap_index(reads, 11, 0)
    same(eng.overlap_rows(index, min_hits=2), want, "before a window run")
    run = eng.run(windows)  # a window run right behind an overlap run, which used the same scratch
    assert [run.consensus(w) for w in range(windows.n_windows)] == before[0]
    same(eng.overlap_rows(index, min_hits=2), want, "behind a window run")
    assert others() == before
    same(eng.overlap_rows(index, min_hits=2), want, "behind a POA and a locate run")


# ---- 8. the host form, and the pile tuples -----------------------------------------------------------------------------------------------------------------------------

def test_the_host_form_equals_the_device_form(eng):
    reads = op.family(15)[0]
    want = op.expected(reads, 15, 3, 0, 1)
    rc, got = eng.overlap_run_host(reads, 15, 3, 0, 1, slots=[w[1] for w in want])
    assert rc == 0
    same(got, want, "cw_overlap_run")
    assert eng.timings().keys() == {"ovl", "ovl_dense", "total"}
    short = [max(w[1] - 1, 0) for w in want]
    rc, got = eng.overlap_run_host(reads, 15, 3, 0, 1, slots=short)
    assert rc == E_CAPACITY
    same(got, op.expected(reads, 15, 3, 0, 1, slots=short), "cw_overlap_run, slots one short")
    rc, got = eng.overlap_run_host([], 15, 3, 0, 1)
    assert rc == 0


def test_the_pile_tuples_are_the_first_rows(eng):
    import torch

    reads = op.family(11)[0]
    want = op.expected(reads, 11, 0, 0, 2)
    index = eng.overlap_index(reads, 11, 0)
    dev, S, max_support = index.mem.device, len(reads), 3
    slots = np.array([w[1] for w in want], np.uint64)
    slots[0] = 0  # a query whose slot is too small has no pile
    row_off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(slots)])
    t_off = torch.from_numpy(row_off.view(np.int64)).to(dev)
    t_rows = torch.zeros(int(row_off[-1]) * op.ROW, dtype=torch.int32, device=dev)
    t_n, t_status = torch.zeros(S, dtype=torch.int32, device=dev), torch.zeros(S, dtype=torch.uint8, device=dev)
    pile_off = np.arange(0, 4 * (S + 1), 4, dtype=np.uint64)  # four tuples a query: more than max_support
    pile_off[-1] -= 2  # the last query's slot holds two
    t_poff = torch.from_numpy(pile_off.view(np.int64)).to(dev)
    t_pile = torch.full((GUARD + int(pile_off[-1]) * 6 + GUARD,), FILL, dtype=torch.int32, device=dev)
    t_pn = torch.full((S + GUARD,), FILL, dtype=torch.int32, device=dev)
    out = Overlaps(t_rows.data_ptr(), t_off.data_ptr(), t_n.data_ptr(), t_status.data_ptr())
    torch.cuda.synchronize(dev)
    eng.overlap_device(index.c_struct(2), index.batch(), 0, S, out)
    assert eng.lib.cw_overlap_to_pile_device(eng.handle, C.byref(out), S, max_support, t_pile.data_ptr() + 4 * GUARD, t_poff.data_ptr(), t_pn.data_ptr(), None) == 0
    torch.cuda.synchronize(dev)
    assert eng.timings().keys() == {"ovl_pile", "total"}
    pile, pn = t_pile.cpu().numpy(), t_pn.cpu().numpy().view(np.uint32)
    assert (pile[:GUARD] == FILL).all() and (pile[GUARD + int(pile_off[-1]) * 6 :] == FILL).all() and (pn[S:] == FILL).all()
    tuples = pile[GUARD : GUARD + int(pile_off[-1]) * 6].reshape(-1, 6)
    assert want[0][1] > 0 and want[-4][1] > 0
    for j, (_, n, rows) in enumerate(want):
        keep = 0 if j == 0 else min(n, max_support, int(pile_off[j + 1] - pile_off[j]))
        assert int(pn[j]) == keep, j
        mine = tuples[int(pile_off[j]) : int(pile_off[j]) + keep].tolist()
        assert mine == [[r[4], r[5], r[0], r[6], r[7], r[1]] for r in rows[:keep]], j  # q_start, q_end, t_read, t_start, t_end, strand
        assert (tuples[int(pile_off[j]) + keep : int(pile_off[j + 1])] == FILL).all(), j


# ---- 9. a planted read set ---------------------------------------------------------------------------------------------------------------------------------------------

def test_overlaps_of_the_planted_set_equal_the_reference(eng):
    genome, reads, where = op.planted(*op.SET)
    want = [w[2] for w in op.expected(None, ix=op.planted_index(op.SET))]
    got = eng.overlaps(reads)
    assert [[o.astuple() for o in rows] for rows in got] == want
    assert sum(len(w) for w in want) > 2000 and got[0][0] == ca.Overlap(*want[0][0])
    index = eng.overlap_index(reads)
    assert eng.overlaps(index, min_hits=1) == [[ca.Overlap(*r) for r in w[2]] for w in op.expected(None, min_hits=1, ix=op.planted_index(op.SET))]
    lds, dense = eng.overlap_routes()
    print(f"120 planted reads: {lds} on the LDS route, {dense} on the dense route")
