"""Both strands on the device (include/consent_amd.h cw_strand_run / cw_strand_run_device / cw_revcomp / cw_revcomp_device; Engine.strands, revcomp, orient,
polish(orient=True)): every strand value and hit count equals the plain reference (tests/strand_probes.py) exactly, at k = 8, 11 and 15, over the edges of k and
of the packed words, the boundary between the two launch classes, the capacities, sets and ties, and a group that takes several units of work; the bytes do not
depend on the batch; the reverse complement equals pack_piles of the turned strings word for word and writes nothing else; and the existing runs, given the
oriented batch, compute what they compute for reads that were never turned."""
import ctypes as C

import numpy as np
import pytest

import consent_amd as ca
import strand_probes as st
import sw_cut_probes as cp
import sw_op_probes as sp
from consent_amd.engine import Batch, HostBatch, Strands, _ptr

pytestmark = pytest.mark.gpu
E_INVALID = -1
MAX_MSA = sp.PRM[4]
FILL = 0xABCDEF01
GUARD = 8


@pytest.fixture(scope="module")
def eng():
    e = ca.Engine(ca.Params(*sp.PRM))
    yield e
    e.close()


def vote(eng, groups, k, want_hits=True):
    """cw_strand_run on host buffers prefilled with a pattern: (strand bytes, hits or None)."""
    hb = groups if isinstance(groups, HostBatch) else ca.pack_piles(groups)
    S = len(hb.seq_len)
    strand = np.full(S + GUARD, 0x5A, np.uint8)
    hits = np.full(2 * S + GUARD, FILL, np.uint32)
    b = hb.c_struct()
    out = Strands(_ptr(strand), _ptr(hits) if want_hits else None, k)
    assert eng.lib.cw_strand_run(eng.handle, C.byref(b), C.byref(out)) == 0
    assert (strand[S:] == 0x5A).all() and (hits[2 * S if want_hits else 0 :] == FILL).all(), "bytes behind the outputs were written"
    return strand[:S], hits[: 2 * S].reshape(S, 2) if want_hits else None


def check_exact(eng, groups, k, what):
    strand, hits = vote(eng, groups, k)
    want = st.expected(groups, k)
    got = [(int(s), int(f), int(r)) for s, (f, r) in zip(strand, hits)]
    wrong = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    tally = {v: sum(1 for w in want if w[0] == v) for v in (st.FWD, st.REV, st.IS_REF, st.NONE)}
    print(f"{what}, k = {k}: {len(want)} sequences, forward / reverse / reference / none {tally[st.FWD]} / {tally[st.REV]} / {tally[st.IS_REF]} / {tally[st.NONE]}")
    assert not wrong, f"{what}, k = {k}: (sequence, got, want) {wrong[:5]}"
    return strand, hits


# ---- the vote against the plain reference ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", st.KS)
@pytest.mark.parametrize("name", ["edges", "boundary", "sets", "spread"])
def test_every_entry_equals_the_plain_reference(eng, name, k):
    groups = st.catalogue(k)[name]
    strand, hits = check_exact(eng, groups, k, name)
    want = st.expected(groups, k)
    if name == "boundary":  # the capacities: the 16 384-base reference's queries, and the one query beyond CW_SW_QMAX, are no vote; the one of CW_SW_QMAX bases is
        first = np.cumsum([0] + [len(g) for g in groups])
        assert [w[0] for w in want[first[5] + 1 : first[6]]] == [st.NONE] * 3 and [w[0] for w in want[first[0] + 1 : first[1]]] == [st.NONE] * 3
        assert want[first[4] - 1][0] == st.NONE and want[first[4] - 2][0] == st.REV and len(groups[3][-2]) == st.QMAX and len(groups[3][-1]) == st.QMAX + 1
        for g in (1, 2, 3, 4):  # the copy and the reverse complement (the random query's few chance hits go either way)
            assert [w[0] for w in want[first[g] + 1 : first[g] + 3]] == [st.FWD, st.REV], g
    if name == "sets":
        m = 77 - k + 1
        assert want[1] == (st.FWD, m, 0) and want[2] == (st.REV, 0, m) and want[3][0] == st.FWD  # poly-A / poly-T against poly-A
        assert want[5][0] == st.FWD and want[5][1] == want[5][2] == 100 - k + 1  # its own reverse complement: a tie
    if name == "spread":
        assert {w[0] for w in want[1:]} == {st.FWD, st.REV} and len(want) == 301
    if name == "edges":
        assert want[-1] == (st.IS_REF, 0, 0) and (st.NONE, 0, 0) in want and groups[0][-1] == ""


def test_k_of_0_is_k_of_11(eng):
    groups = st.catalogue(11)["edges"]
    s0, h0 = vote(eng, groups, 0)
    s11, h11 = vote(eng, groups, 11)
    assert np.array_equal(s0, s11) and np.array_equal(h0, h11) and [int(v) for v in s0] == [w[0] for w in st.expected(groups, 0)]


def test_the_bytes_do_not_depend_on_the_batch_and_hits_may_be_null(eng):
    k = 11
    groups = [g for part in st.catalogue(k).values() for g in part]
    together_s, together_h = vote(eng, groups, k)
    alone_s, alone_h = zip(*(vote(eng, [g], k) for g in groups))
    assert np.array_equal(np.concatenate(alone_s), together_s) and np.array_equal(np.concatenate(alone_h), together_h)
    rev_s, rev_h = vote(eng, groups[::-1], k)
    first = np.cumsum([0] + [len(g) for g in groups[::-1]])
    back_s = np.concatenate([rev_s[first[i] : first[i + 1]] for i in range(len(groups))][::-1])
    back_h = np.concatenate([rev_h[first[i] : first[i + 1]] for i in range(len(groups))][::-1])
    assert np.array_equal(back_s, together_s) and np.array_equal(back_h, together_h)
    no_hits, none = vote(eng, groups, k, want_hits=False)
    assert none is None and np.array_equal(no_hits, together_s)
    rows = eng.strands(groups, k)  # the binding's view of the same
    assert np.array_equal(rows.strands, together_s) and rows.strand(1, 0) == st.IS_REF and rows.hits(0, 1) == tuple(int(v) for v in together_h[1])


# ---- the reverse complement ------------------------------------------------------------------------------------------------------------------------------------------

def revcomp_batch():
    """Every length of REVCOMP_LENS twice in one batch: group 0 flagged -- its reference too -- group 1 not, under three other values."""
    strings = list(st.revcomp_strings())
    n = len(strings)
    strand = np.array([st.REV] * n + [(st.FWD, st.IS_REF, st.NONE)[i % 3] for i in range(n)], np.uint8)
    return strings, strand


def test_the_reverse_complement_equals_the_packed_turned_strings(eng):
    strings, strand = revcomp_batch()
    hb = ca.pack_piles([strings, strings])
    want = ca.pack_piles([[st.revcomp(s) for s in strings], strings])
    got = eng.revcomp(hb, strand)
    assert np.array_equal(got.bases, want.bases), f"first different word: {np.flatnonzero(got.bases != want.bases)[:3]}"
    assert got.pile(0)[0] == st.revcomp(strings[0]) and got.pile(0) == want.pile(0)  # (a flagged reference is reversed)
    assert np.array_equal(got.win_first_seq, hb.win_first_seq) and np.array_equal(got.seq_len, hb.seq_len) and np.array_equal(got.seq_word_off, hb.seq_word_off)
    assert np.array_equal(eng.revcomp(got, strand).bases, hb.bases)  # twice: the input, bit for bit
    everything = eng.revcomp(hb)  # strand == NULL
    assert np.array_equal(everything.bases, ca.pack_piles([[st.revcomp(s) for s in strings]] * 2).bases)
    assert eng.timings().keys() == {"revcomp", "total"}


def gapped():
    """The revcomp batch with four words between two sequences that belong to none, and the expected words with FILL in the gap and behind the end."""
    strings, strand = revcomp_batch()
    hb = ca.pack_piles([strings, strings])
    want = ca.pack_piles([[st.revcomp(s) for s in strings], strings])
    at = int(hb.seq_word_off[40])
    off = hb.seq_word_off.copy()
    off[40:] += np.uint64(4)
    gap = lambda w, fill: np.concatenate([w[:at], np.full(4, fill, np.uint32), w[at:]])
    return HostBatch(hb.win_first_seq, hb.seq_len, off, gap(hb.bases, 0x11111111)), strand, np.concatenate([gap(want.bases, FILL), np.full(GUARD, FILL, np.uint32)])


def test_words_of_no_sequence_are_never_written_on_the_host_path(eng):
    hb, strand, want = gapped()
    out = np.full(len(hb.bases) + GUARD, FILL, np.uint32)
    b = hb.c_struct()
    assert eng.lib.cw_revcomp(eng.handle, C.byref(b), _ptr(strand), _ptr(out)) == 0
    assert np.array_equal(out, want), f"first different word: {np.flatnonzero(out != want)[:3]}"


# ---- the device entry points -------------------------------------------------------------------------------------------------------------------------------------------

def test_the_device_entry_points_write_their_outputs_and_nothing_else(eng):
    import torch

    dev = torch.device("cuda", eng.device)

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    fill = FILL - (1 << 32)
    # the reverse complement, on the batch with a gap
    hb, strand, want = gapped()
    S, W = len(hb.seq_len), len(hb.bases)
    keep = (up(hb.win_first_seq, np.int32), up(hb.seq_len, np.int32), up(hb.seq_word_off, np.int64), up(hb.bases, np.int32), up(strand, np.uint8))
    t_out = torch.full((W + GUARD,), fill, dtype=torch.int32, device=dev)
    b = Batch(hb.n_windows, S, W, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr())
    torch.cuda.synchronize(dev)
    fn = eng.lib.cw_revcomp_device
    assert fn(eng.handle, C.byref(b), keep[4].data_ptr(), keep[3].data_ptr(), None) == E_INVALID  # bases_out == bases
    assert fn(eng.handle, C.byref(b), keep[4].data_ptr(), None, None) == E_INVALID and fn(eng.handle, None, keep[4].data_ptr(), t_out.data_ptr(), None) == E_INVALID
    eng.revcomp_device(b, keep[4].data_ptr(), t_out.data_ptr())
    torch.cuda.synchronize(dev)
    assert np.array_equal(u32(t_out), want), f"first different word: {np.flatnonzero(u32(t_out) != want)[:3]}"
    assert np.array_equal(u32(keep[3]), hb.bases)  # the input is not touched
    # the vote, on the edges and the spread group together
    k = 11
    groups = st.catalogue(k)["edges"] + st.catalogue(k)["spread"]
    hb = ca.pack_piles(groups)
    S = len(hb.seq_len)
    keep = (up(hb.win_first_seq, np.int32), up(hb.seq_len, np.int32), up(hb.seq_word_off, np.int64), up(np.concatenate([hb.bases, np.zeros(1, np.uint32)]), np.int32))
    t_strand = torch.full((S + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    t_hits = torch.full((2 * S + GUARD,), fill, dtype=torch.int32, device=dev)
    b = Batch(hb.n_windows, S, len(hb.bases), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr())
    torch.cuda.synchronize(dev)
    fn = eng.lib.cw_strand_run_device
    for bad_k in (7, 16):
        assert fn(eng.handle, C.byref(b), C.byref(Strands(t_strand.data_ptr(), t_hits.data_ptr(), bad_k)), None) == E_INVALID
    big = Batch(eng.max_batch_windows() + 1, S, len(hb.bases), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr())
    assert fn(eng.handle, C.byref(big), C.byref(Strands(t_strand.data_ptr(), t_hits.data_ptr(), k)), None) == E_INVALID
    assert eng.lib.cw_revcomp_device(eng.handle, C.byref(big), None, t_out.data_ptr(), None) == E_INVALID
    assert fn(eng.handle, C.byref(b), C.byref(Strands(None, t_hits.data_ptr(), k)), None) == E_INVALID and fn(eng.handle, C.byref(b), None, None) == E_INVALID
    none = Batch(0, 0, 0, None, None, None, None)  # no sequence: CW_OK, nothing launched
    assert fn(eng.handle, C.byref(none), C.byref(Strands(t_strand.data_ptr(), None, k)), None) == 0
    torch.cuda.synchronize(dev)
    assert (t_strand.cpu().numpy() == 0x5A).all() and (u32(t_hits) == FILL).all(), "a refused call wrote something"
    eng.strand_device(b, Strands(t_strand.data_ptr(), t_hits.data_ptr(), k))
    torch.cuda.synchronize(dev)
    assert eng.timings().keys() == {"strand_order", "strand", "strand_wide", "total"}
    got_s, got_h = t_strand.cpu().numpy(), u32(t_hits)
    want_rows = st.expected(groups, k)
    assert (got_s[S:] == 0x5A).all() and (got_h[2 * S :] == FILL).all(), "bytes behind the outputs were written"
    assert [int(v) for v in got_s[:S]] == [w[0] for w in want_rows] and got_h[: 2 * S].reshape(S, 2).tolist() == [[w[1], w[2]] for w in want_rows]


# ---- composition with the existing runs --------------------------------------------------------------------------------------------------------------------------------

def test_the_aligner_on_the_oriented_batch_has_the_rows_of_the_original(eng):
    original = list(cp.polish_input(**cp.SEED9)[1])
    mixed, planted = st.mixed_strands(original)
    oriented, rows = eng.orient([mixed])
    assert [rows.strand(0, m) for m in range(1, len(mixed))] == planted and rows.strand(0, 0) == st.IS_REF
    assert oriented.pile(0) == original
    want = eng.sw([original])
    assert np.array_equal(eng.sw(oriented).rows, want.rows)
    assert not np.array_equal(eng.sw([mixed]).rows, want.rows)  # (without the vote a turned read gets another, chance alignment)


def test_polish_with_orient_equals_the_polish_of_reads_that_were_never_turned(eng):
    original = list(cp.polish_input(**cp.SEED8)[1])
    mixed, planted = st.mixed_strands(original)
    want_seq, want_members = cp.polish([original], 100, MAX_MSA)[0]
    (got,) = eng.polish([mixed], 100, orient=True)
    print(f"seed 8, odd reads turned, orient: members a window {[w.members for w in got.windows]}")
    assert [w.members for w in got.windows] == want_members and got.sequence == want_seq
    assert got.strands == planted
    (blind,) = eng.polish([mixed], 100)
    print(f"seed 8, odd reads turned, as given: members a window {[w.members for w in blind.windows]}")
    assert blind.strands == [] and any(b.members < w for b, w in zip(blind.windows, want_members))  # what the feature is for
    (plain,) = eng.polish([original], 100)
    assert plain.strands == [] and plain.sequence == want_seq
    (same,) = eng.polish([original], 100, orient=True)  # nothing to turn: the same, and it says so
    assert same.sequence == want_seq and same.strands == [st.FWD] * (len(original) - 1)
