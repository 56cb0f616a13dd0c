"""The locate run on the device (include/consent_amd.h cw_locate_build_device / cw_locate_run_device / cw_locate_run; Engine.locate_index, locate_rows, locate,
polish_reads(index=True)): every row and strand byte equals the plain reference (tests/locate_probes.py) exactly -- over the seed run's whole catalogue, where it
also equals the seed run's own rows; past every 16-bit and 10-bit field of the seed run, on a reference of 70 000 bases; on both routes of the kernel; from one
build over many runs; nothing else is written; the refusals; beside the other runs of the engine; host form and device form; and a contig placed and polished
through the index as the reference says."""
import ctypes as C

import numpy as np
import pytest

import consent_amd as ca
import locate_probes as lp
import seed_probes as sd
import strand_probes as st
import sw_op_probes as sp
from consent_amd.engine import Batch, LocateRef, Seeds, _ptr, synth_host

pytestmark = pytest.mark.gpu
E_INVALID = -1
FILL = 0x0BADBEEF
GUARD = 8


@pytest.fixture(scope="module")
def eng():
    e = ca.Engine(ca.Params(*sp.PRM))
    yield e
    e.close()


def host(eng, ref, reads, k, want_strand=True, out_k=0):
    """cw_locate_run on host buffers prefilled with a pattern: (rows, strand bytes or None)."""
    hr, hb = ca.pack_piles([[ref]]), ca.pack_piles([list(reads)])
    S = len(hb.seq_len)
    rows = np.full(sd.ROW * S + GUARD, FILL, np.int32)
    strand = np.full(S + GUARD, 0x5A, np.uint8)
    b = hb.c_struct()
    out = Seeds(_ptr(rows), _ptr(strand) if want_strand else None, out_k)
    assert eng.lib.cw_locate_run(eng.handle, _ptr(hr.bases), len(ref), k, C.byref(b), C.byref(out)) == 0
    assert (rows[sd.ROW * S :] == FILL).all() and (strand[S if want_strand else 0 :] == 0x5A).all(), "bytes behind the outputs were written"
    return rows[: sd.ROW * S].reshape(S, sd.ROW), strand[:S] if want_strand else None


def exact(rows, strands, want, what):
    got = [tuple(int(v) for v in r) for r in rows]
    wrong = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not wrong and len(got) == len(want), f"{what}: (read, got, want) {wrong[:5]}"
    assert [int(v) for v in strands] == [w[0] for w in want], f"{what}: a strand byte is not its row's status"


# ---- 1. the seed catalogue ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", sd.KS)
def test_every_row_of_the_seed_catalogue_equals_the_plain_reference_and_the_seed_run(eng, k):
    n_groups = beyond = 0
    for name, groups in sd.catalogue(k).items():
        seeds = eng.seeds(groups, k)
        for g, grp in enumerate(groups):
            if len(grp) < 2:
                continue
            index = eng.locate_index(grp[0], k)
            got = eng.locate_rows(index, grp[1:])
            exact(got.rows, got.strands, lp.expected(grp[0], grp[1:], k), f"{name}[{g}], k = {k}")
            if len(grp[0]) <= st.RMAX:  # the seed run takes this reference: bit for bit its rows
                assert got.rows.tolist() == [[int(v) for v in seeds.row(g, m)] for m in range(1, len(grp))], (name, g)
            else:
                beyond += 1
            n_groups += 1
    assert n_groups >= 15 and beyond == 1  # (the catalogue's reference of 16 384 bases: no vote in the seed run, rows here)


# ---- 2. past every 16-bit and 10-bit field ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [11, 15])
def test_a_reference_of_70000_bases_is_exact_at_every_edge(eng, k):
    draft, reads, names = lp.far_reads(k)
    want = lp.expected(draft, reads, k)
    got = eng.locate_rows(eng.locate_index(draft, k), reads)
    exact(got.rows, got.strands, want, f"70 000 bases, k = {k}")
    by = dict(zip(names[48:], want[48:]))
    twice = by["present twice"]  # no seed in the orientation that has it (the other one's k-mers are random: k = 11 finds a chance hit or two)
    assert (twice[1] if twice[0] == lp.FWD else twice[3]) == 0 and by["its own reverse complement"][0] == lp.FWD and by["over the start"][2] < 0
    assert max(w[2] for w in want) > 65535 and {w[0] for w in want[:24]} == {lp.FWD, lp.REV}
    assert eng.locate_routes() == (len(reads), 0) and eng.timings().keys() == {"locate", "locate_dense", "total"}


# ---- 3. the dense route ------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_read_with_more_distinct_bins_than_the_lds_table_takes_goes_the_dense_route(eng):
    ref, reads = lp.dense_reads()
    k = lp.DENSE["k"]
    pairs = [lp.distinct_pairs(q, ref, k) for q in reads]
    print(f"distinct (orientation, bin) pairs per read: {pairs}; the LDS route takes {lp.LDS_CAP}")
    assert pairs[0] > lp.LDS_CAP and min(pairs) <= lp.LDS_CAP  # by the reference alone: a read beyond the LDS route's capacity, and reads within it
    want = lp.expected(ref, reads, k)
    got = eng.locate_rows(eng.locate_index(ref, k), reads)
    lds, dense = eng.locate_routes()
    assert dense >= 1 and lds >= 1 and lds + dense == len(reads) and dense == sum(p > lp.LDS_CAP for p in pairs)
    exact(got.rows, got.strands, want, "1 000 000 bases, k = 11")
    assert want[1][0] == lp.REV and want[1][1] > 100 and want[5] == (lp.NONE, 0, 0, 0)


# ---- 4. one build, many runs -------------------------------------------------------------------------------------------------------------------------------------------

def test_one_index_answers_many_batches_in_any_order_and_its_memory_serves_the_next_reference(eng):
    k = 15
    draft, reads, _ = lp.far_reads(k)
    index = eng.locate_index(draft, k)
    a, b = list(reads[:30]), list(reads[30:])
    whole = eng.locate_rows(index, reads)
    ra, rb = eng.locate_rows(index, a), eng.locate_rows(index, b)  # two different batches against one index
    assert np.array_equal(np.concatenate([ra.rows, rb.rows]), whole.rows) and np.array_equal(np.concatenate([ra.strands, rb.strands]), whole.strands)
    back = eng.locate_rows(index, reads[::-1])  # the same reads in another order
    assert np.array_equal(back.rows[::-1], whole.rows) and np.array_equal(back.strands[::-1], whole.strands)
    exact(whole.rows, whole.strands, lp.expected(draft, reads, k), "one index")
    # a second, shorter reference built into the same table memory: the build clears it first
    other, _, _, _ = sd.draft_and_reads(**lp.CONTIG)
    second = ca.LocateIndex(len(other), k, eng.locate_index(other, k).bases, index.table)
    ref = second.c_struct()
    assert eng.lib.cw_locate_build_device(eng.handle, C.byref(ref), None) == 0
    probes = [other[100:400], lp.revcomp(other[19000:19700]), draft[100:400]]
    got = eng.locate_rows(second, probes)
    exact(got.rows, got.strands, lp.expected(other, probes, k), "the second reference in the first one's table")
    assert got.rows[2][sd.HITS] < lp.MIN_HITS <= got.rows[0][sd.HITS]  # the first reference's slice is nowhere any more


# ---- 5. the device entry points write their outputs and nothing else -------------------------------------------------------------------------------------------------

def device_setup(eng, ref, reads, k):
    import torch

    dev = torch.device("cuda", eng.device)

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    hr, hb = ca.pack_piles([[ref]]), ca.pack_piles([list(reads)])
    S, words = len(hb.seq_len), int(eng.lib.cw_locate_table_words(len(ref)))
    keep = dict(ref=up(np.concatenate([hr.bases, np.zeros(1, np.uint32)]), np.int32), len=up(hb.seq_len, np.int32), off=up(hb.seq_word_off, np.int64),
                bases=up(np.concatenate([hb.bases, np.zeros(1, np.uint32)]), np.int32),
                table=torch.full((GUARD + words + GUARD,), FILL, dtype=torch.int32, device=dev),
                rows=torch.full((sd.ROW * S + GUARD,), FILL, dtype=torch.int32, device=dev), strand=torch.full((S + GUARD,), 0x5A, dtype=torch.uint8, device=dev))
    r = LocateRef(keep["ref"].data_ptr(), len(ref), keep["table"].data_ptr() + 4 * GUARD, k)
    b = Batch(0, S, len(hb.bases), None, keep["len"].data_ptr(), keep["off"].data_ptr(), keep["bases"].data_ptr())
    torch.cuda.synchronize(dev)
    return dev, keep, r, b, S, words


def test_the_device_entry_points_write_their_outputs_and_nothing_else(eng):
    import torch

    k = 11
    draft, reads, _ = lp.far_reads(k)
    reads = reads[:8] + reads[48:]
    dev, keep, r, b, S, words = device_setup(eng, draft, reads, k)
    want = lp.expected(draft, reads, k)
    assert eng.lib.cw_locate_build_device(eng.handle, C.byref(r), None) == 0
    torch.cuda.synchronize(dev)
    assert eng.timings().keys() == {"locate_build", "total"}
    table = keep["table"].cpu().numpy().view(np.uint32)
    assert (table[:GUARD] == FILL).all() and (table[GUARD + words :] == FILL).all(), "words round the table were written"
    slots = table[GUARD : GUARD + words]
    used = slots[slots != 0xFFFFFFFF]
    assert ((used & 0x70000000) == 0).all() and ((used & 0x0FFFFFFF) <= len(draft) - k).all() and 0 < len(used) <= len(draft) - k + 1  # positions, and the flag
    assert len(used) == len({draft[j : j + k] for j in range(len(draft) - k + 1)})  # a slot a distinct k-mer
    for strand in (keep["strand"].data_ptr(), None):
        keep["rows"].fill_(FILL), keep["strand"].fill_(0x5A)
        torch.cuda.synchronize(dev)
        eng.locate_device(r, b, Seeds(keep["rows"].data_ptr(), strand, k))
        torch.cuda.synchronize(dev)
        got_r, got_s = keep["rows"].cpu().numpy(), keep["strand"].cpu().numpy()
        assert (got_r[sd.ROW * S :] == FILL).all() and (got_s[S if strand else 0 :] == 0x5A).all(), "bytes behind the outputs were written"
        assert got_r[: sd.ROW * S].reshape(S, sd.ROW).tolist() == [list(w) for w in want] and (strand is None or [int(v) for v in got_s[:S]] == [w[0] for w in want])
    assert np.array_equal(keep["table"].cpu().numpy().view(np.uint32), table), "a run wrote the table"


# ---- 6. edges and refusals ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [8, 15])
def test_the_edges_of_k_of_the_read_and_of_the_reference(eng, k):
    import random

    rng = random.Random(0xED6E + k)
    ref = sd.rand_seq(rng, 3000)
    reads = [ref[5 : 5 + k - 1], ref[5 : 5 + k], lp.revcomp(ref[70 : 70 + k]), sd.rand_seq(rng, st.QMAX - 3000) + ref, sd.rand_seq(rng, st.QMAX + 1), ""]
    want = lp.expected(ref, reads, k)
    assert [w[0] for w in want] == [lp.NONE, lp.FWD, lp.REV, lp.FWD, lp.NONE, lp.NONE] and want[1][1] == 1 == want[2][1] and len(reads[3]) == st.QMAX and want[3][1] > 2000
    rows, strands = host(eng, ref, reads, k)
    exact(rows, strands, want, f"edges, k = {k}")
    for short in ("", ref[: k - 1]):  # n = 0 and n = k - 1: no read has a vote
        rows, strands = host(eng, short, reads, k)
        assert (rows == [lp.NONE, 0, 0, 0]).all() and (strands == lp.NONE).all()
    rows, strands = host(eng, ref[:k], [ref[:k], ref[: k + 3]], k)  # n = k: one k-mer
    exact(rows, strands, lp.expected(ref[:k], [ref[:k], ref[: k + 3]], k), "n = k")


def test_what_is_refused_is_refused_before_anything_is_written(eng):
    import torch

    k = 11
    draft, reads, _ = lp.far_reads(k)
    dev, keep, r, b, S, words = device_setup(eng, draft[:5000], reads[48:52], k)
    build, run = eng.lib.cw_locate_build_device, eng.lib.cw_locate_run_device
    out = Seeds(keep["rows"].data_ptr(), keep["strand"].data_ptr(), 0)
    ref_of = lambda **kw: LocateRef(*[kw.get(f, getattr(r, f)) for f in ("bases", "len", "table", "k")])
    bad_refs = [ref_of(bases=None), ref_of(table=None), ref_of(len=1 << 28), ref_of(len=1 << 40), ref_of(k=7), ref_of(k=16)]  # (2^28: the pointers are small real buffers)
    for bad in bad_refs:
        assert build(eng.handle, C.byref(bad), None) == E_INVALID and run(eng.handle, C.byref(bad), C.byref(b), C.byref(out), None) == E_INVALID
    assert build(eng.handle, None, None) == E_INVALID and run(eng.handle, None, C.byref(b), C.byref(out), None) == E_INVALID
    assert run(eng.handle, C.byref(r), None, C.byref(out), None) == E_INVALID and run(eng.handle, C.byref(r), C.byref(b), None, None) == E_INVALID
    assert run(eng.handle, C.byref(r), C.byref(b), C.byref(Seeds(None, keep["strand"].data_ptr(), 0)), None) == E_INVALID
    for out_k in (8, 15, 16):  # neither 0 nor the reference's k
        assert run(eng.handle, C.byref(r), C.byref(b), C.byref(Seeds(keep["rows"].data_ptr(), None, out_k)), None) == E_INVALID
    assert run(eng.handle, C.byref(ref_of(k=0)), C.byref(b), C.byref(Seeds(keep["rows"].data_ptr(), None, 11)), None) == E_INVALID  # the reference's k is 15
    none = Batch(0, 0, 0, None, None, None, None)  # no read: CW_OK, nothing launched
    assert run(eng.handle, C.byref(r), C.byref(none), C.byref(out), None) == 0
    assert build(eng.handle, C.byref(ref_of(bases=None, len=0)), None) == 0  # no base: no pointer needed; the table is cleared
    torch.cuda.synchronize(dev)
    assert (keep["rows"].cpu().numpy() == FILL).all() and (keep["strand"].cpu().numpy() == 0x5A).all(), "a refused call wrote something"
    table = keep["table"].cpu().numpy().view(np.uint32)
    small = int(eng.lib.cw_locate_table_words(0))  # what the one build that ran cleared: the table of no base
    assert (table[:GUARD] == FILL).all() and (table[GUARD + small :] == FILL).all() and (table[GUARD : GUARD + small] == 0xFFFFFFFF).all() and small < words
    # the host form: the same refusals, and k = 0 with out->k = 15
    hr, hb = ca.pack_piles([[draft[:5000]]]), ca.pack_piles([list(reads[48:52])])
    rows, hbs = np.full(sd.ROW * S, FILL, np.int32), hb.c_struct()
    fn = eng.lib.cw_locate_run
    assert fn(eng.handle, None, 5000, k, C.byref(hbs), C.byref(Seeds(_ptr(rows), None, 0))) == E_INVALID
    assert fn(eng.handle, _ptr(hr.bases), 1 << 28, k, C.byref(hbs), C.byref(Seeds(_ptr(rows), None, 0))) == E_INVALID
    assert fn(eng.handle, _ptr(hr.bases), 5000, 16, C.byref(hbs), C.byref(Seeds(_ptr(rows), None, 0))) == E_INVALID
    assert fn(eng.handle, _ptr(hr.bases), 5000, k, C.byref(hbs), C.byref(Seeds(_ptr(rows), None, 15))) == E_INVALID
    assert fn(eng.handle, _ptr(hr.bases), 5000, k, None, C.byref(Seeds(_ptr(rows), None, 0))) == E_INVALID
    assert fn(eng.handle, _ptr(hr.bases), 5000, k, C.byref(hbs), C.byref(Seeds(None, None, 0))) == E_INVALID and (rows == FILL).all()
    assert fn(eng.handle, None, 0, k, C.byref(none), C.byref(Seeds(_ptr(rows), None, 0))) == 0 and (rows == FILL).all()
    r15, _ = host(eng, draft[:5000], reads[48:52], 0, out_k=15)
    assert [tuple(int(v) for v in x) for x in r15] == lp.expected(draft[:5000], reads[48:52], 15)


# ---- 7. beside the other runs ------------------------------------------------------------------------------------------------------------------------------------------

def test_a_locate_run_between_the_other_runs_leaves_their_results_as_they_were(eng):
    windows = synth_host(ca.SynthSpec.pacbio(6, 12))
    piles = [windows.pile(w)[:6] for w in range(3)]
    pairs = sd.catalogue(11)["seeds"][4:6]
    ref, reads = pairs[0][0], pairs[0][1:] + pairs[1][1:]

    def others():
        run = eng.run(windows)
        poa = eng.poa(piles)
        sw = eng.sw(pairs, want_indels=True)
        seeds = eng.seeds(pairs, 11)
        return ([run.consensus(w) for w in range(windows.n_windows)], run.status.tolist(), [poa.consensus(g) for g in range(len(piles))], poa.status.tolist(), sw.rows.tolist(),
                seeds.rows.tolist())

    before = others()
    rows, _ = host(eng, ref, reads, 11)
    run = eng.run(windows)  # a window run right behind a locate run, which used the same scratch
    assert [run.consensus(w) for w in range(windows.n_windows)] == before[0]
    again, _ = host(eng, ref, reads, 11)
    assert others() == before and np.array_equal(rows, again) and [tuple(int(v) for v in r) for r in rows] == lp.expected(ref, reads, 11)


# ---- 8. the host form equals the device form ---------------------------------------------------------------------------------------------------------------------------

def test_the_host_form_equals_the_device_form(eng):
    k = 15
    draft, reads, _ = lp.far_reads(k)
    dev_rows = eng.locate_rows(eng.locate_index(draft, k), reads)
    rows, strands = host(eng, draft, reads, k)
    assert np.array_equal(rows, dev_rows.rows) and np.array_equal(strands, dev_rows.strands)
    rows0, none = host(eng, draft, reads, 0, want_strand=False)  # k = 0 is 15; the strand bytes may be NULL
    assert none is None and np.array_equal(rows0, rows)
    assert eng.timings().keys() == {"locate", "locate_dense", "total"}


# ---- 9. a contig and a bag of reads ------------------------------------------------------------------------------------------------------------------------------------

def test_locate_equals_the_reference_placements(eng):
    draft, reads, where, other = sd.draft_and_reads(*lp.DRAFT)
    bag = list(reads) + list(other[:4])
    want = lp.locate(draft, bag, 0)
    index = eng.locate_index(draft)
    got = eng.locate(index, bag)
    assert [None if p is None else (p.strand, p.position, p.hits, p.other) for p in got] == want and got == eng.locate(draft, bag)
    assert got[24:] == [None] * 4 and None not in got[:24] and [p.strand for p in got[:24]] == [lp.REV if turned else lp.FWD for _, turned in where]
    everything = eng.locate(index, bag, min_hits=0)
    assert None not in everything and everything[-1].hits < ca.LOCATE_MIN_HITS and everything[:24] == got[:24]
    with pytest.raises(ca.EngineError):
        eng.locate(draft, bag, k=11)  # the default threshold is measured for k = 15
    assert eng.locate(draft, bag[:3], k=11, min_hits=14) == [None if p is None else ca.Placement(*p) for p in lp.locate(draft, bag[:3], 11, 14)]
    assert eng.locate(index, []) == [] and eng.locate("", bag[:2]) == [None, None]


def contig():
    draft, reads, where, other = sd.draft_and_reads(**lp.CONTIG)
    return draft, list(reads) + [other[0]], where  # the last read belongs nowhere


def same_polish(got, want):
    assert got.sequence == "".join(p.sequence for p in want)
    assert [(w.members, w.status, w.kept_reference) for w in got.windows] == [(w.members, w.status, w.kept_reference) for p in want for w in p.windows]


def test_polish_reads_through_the_index_equals_polish_of_the_reference_groups(eng):
    draft, bag, where = contig()
    want = eng.polish(lp.polish_groups(draft, bag, 5000, 0), 100)
    got = eng.polish_reads(draft, bag, window=100, tile=5000, index=True)
    same_polish(got, want)
    assert got.placements == eng.locate(draft, bag) and got.placements[-1] is None and None not in got.placements[:-1]
    assert len(got.windows) == 200 and max(w.members for w in got.windows) >= 3 and got.sequence != draft  # (the reads reach their windows)


def test_seeded_polish_reads_through_the_index_equals_polish_of_the_reference_group_and_spans(eng):
    draft, bag, where = contig()
    group, spans = lp.seeded_group(draft, bag, 0)
    want = eng.polish([group], 100, spans=spans)
    got = eng.polish_reads(draft, bag, window=100, index=True, seeded=True)
    same_polish(got, want)
    assert got.placements == eng.locate(draft, bag) and len(got.windows) == 200 and max(w.members for w in got.windows) >= 3
