"""The POA batch behind a cut run and the polish on top of it (include/consent_amd.h cw_cut_groups_device; Engine.polish): the device builder's output equals
pack_piles of the plain reference's groups (tests/sw_cut_probes.py cut_groups) array for array and word for word, its capacity protocol is
cw_extract_piles_device's, and Engine.polish equals the reference composition -- cuts, spanning members, the oracle's POA, joined -- byte for byte."""
import ctypes as C
import random

import numpy as np
import pytest

import consent_amd as ca
import pileup_probes as pl
import poa_op_probes as pop
import sw_cut_probes as cp
import sw_op_probes as sp
import sw_path_probes as pp
from consent_amd.engine import Batch, HostBatch, SwCuts

pytestmark = pytest.mark.gpu
E_CAPACITY = -4
MAX_MSA = sp.PRM[4]


@pytest.fixture(scope="module")
def eng():
    e = ca.Engine(ca.Params(*sp.PRM))
    yield e
    e.close()


def seed8():
    return list(cp.polish_input(**cp.SEED8)[1])


def seed9():
    return list(cp.polish_input(**cp.SEED9)[1])


class Built:
    """A cut run and cw_cut_groups_device behind it, on device buffers: .sizes from a call with capacities of 0, then .rc / .batch / .grp_first from a call
    with capacities `short` below them (group, sequences, words)."""

    def __init__(self, eng, groups, W, short=(0, 0, 0)):
        import torch

        dev = torch.device("cuda", eng.device)

        def up(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

        hb = ca.pack_piles(groups)
        G, S = hb.n_windows, len(hb.seq_len)
        keep = (up(hb.win_first_seq, np.int32), up(hb.seq_len, np.int32), up(hb.seq_word_off, np.int64), up(np.concatenate([hb.bases, np.zeros(1, np.uint32)]), np.int32),
                up(eng._cut_slots(hb, W), np.int64))
        t_cuts = torch.zeros(max(int(eng._cut_slots(hb, W)[-1]), 1), dtype=torch.int32, device=dev)
        t_rows = torch.zeros(max(S, 1) * 8, dtype=torch.int32, device=dev)
        b = Batch(G, S, len(hb.bases), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr())
        cuts = SwCuts(t_cuts.data_ptr(), keep[4].data_ptr(), W)
        torch.cuda.synchronize(dev)
        eng.sw_cut_device(b, t_rows.data_ptr(), cuts)
        rc0, ng, ns, nw = eng.cut_groups_device(b, t_rows.data_ptr(), cuts)
        self.sizes, self.rc_size = (ng, ns, nw), rc0
        caps = (ng - short[0], ns - short[1], nw - short[2])
        fill = -0x12345678
        o_grp = torch.full((G + 1,), fill, dtype=torch.int32, device=dev)
        o_wfs = torch.full((ng + 1 + 2,), fill, dtype=torch.int32, device=dev)
        o_len = torch.full((ns + 2,), fill, dtype=torch.int32, device=dev)
        o_off = torch.full((ns + 2,), fill, dtype=torch.int64, device=dev)
        o_bases = torch.full((nw + 2,), fill, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.rc, ng2, ns2, nw2 = eng.cut_groups_device(b, t_rows.data_ptr(), cuts, o_grp.data_ptr(), o_wfs.data_ptr(), o_len.data_ptr(), o_off.data_ptr(), o_bases.data_ptr(), *caps)
        torch.cuda.synchronize(dev)
        assert (ng2, ns2, nw2) == self.sizes, "the totals do not depend on the capacities"
        u32 = lambda t: t.cpu().numpy().view(np.uint32)
        self.grp_first = u32(o_grp)
        wfs, lens, offs, bases = u32(o_wfs), u32(o_len), o_off.cpu().numpy().view(np.uint64), u32(o_bases)
        pad = np.uint32(fill & 0xFFFFFFFF)
        assert (wfs[ng + 1 :] == pad).all() and (lens[ns:] == pad).all() and (offs[ns:] == np.uint64(fill & 0xFFFFFFFFFFFFFFFF)).all() and (bases[nw:] == pad).all(), "words behind the output were written"
        self.batch = HostBatch(wfs[: ng + 1], lens[:ns], offs[:ns], bases[: max(nw, 1)] if nw else np.zeros(1, np.uint32))
        self.rows = t_rows.cpu().numpy().reshape(-1, 8)


def builder_groups():
    wide_q, wide_r = pp.planted_wide()
    return [cp.as_group(pl.classes()), seed9(), [wide_r, wide_q], [], ["", "ACGT"], [pl.round_edges()[0]]]


@pytest.mark.parametrize("W", [500, 64])
def test_the_device_builder_equals_the_packed_reference_groups(eng, W):
    groups = builder_groups()
    want_groups, want_first = cp.cut_groups(groups, W)
    want = ca.pack_piles(want_groups)
    got = Built(eng, groups, W)
    print(f"W = {W}: {got.sizes[0]} output groups, {got.sizes[1]} sequences, {got.sizes[2]} words; members a group {[len(g) - 1 for g in want_groups][:24]} ..")
    assert got.rc_size == E_CAPACITY and got.rc == 0  # capacities of 0 only size the output
    assert got.sizes == (len(want_groups), len(want.seq_len), int(sum((len(s) + 15) // 16 for g in want_groups for s in g)))
    assert got.grp_first.tolist() == want_first
    assert np.array_equal(got.batch.win_first_seq, want.win_first_seq)
    assert np.array_equal(got.batch.seq_len, want.seq_len)
    assert np.array_equal(got.batch.seq_word_off, want.seq_word_off)
    assert np.array_equal(got.batch.bases, want.bases), f"first different word: {np.flatnonzero(got.batch.bases != want.bases)[:3]}"
    assert int(got.rows[len(groups[0]) + len(groups[1]) + 1, 7]) == ca.SW_NO_PATH  # the group whose only query has no path: the backbone alone
    wide_first = want_first[2]
    assert all(len(g) == 1 for g in want_groups[wide_first : want_first[3]]) and want_first[3] == want_first[4] == want_first[5]  # a group of none, an empty reference


def test_the_seed_9_input_has_a_short_last_window_and_end_windows_with_the_backbone_alone(eng):
    groups = [seed9()]
    got = Built(eng, groups, 64)
    n = len(groups[0][0])
    T = cp.n_windows(n, 64)
    assert got.sizes[0] == T and n % 64 != 0 and int(got.batch.seq_len[int(got.batch.win_first_seq[T - 1])]) == n % 64
    members = np.diff(got.batch.win_first_seq.astype(np.int64)) - 1
    assert members[0] == 0 and members[-1] == 0 and members.max() >= 10
    assert "".join(got.batch.pile(w)[0] for w in range(T)) == groups[0][0]


@pytest.mark.parametrize("short", [(1, 0, 0), (0, 1, 0), (0, 0, 1)])
def test_one_too_few_of_each_capacity_is_refused(eng, short):
    got = Built(eng, [seed9(), cp.as_group(pl.run_start(64, False))], 64, short=short)
    assert got.rc == E_CAPACITY and got.rc_size == E_CAPACITY


def test_groups_of_none_only_give_no_output_group(eng):
    got = Built(eng, [[], []], 64)
    assert got.sizes == (0, 0, 0) and got.rc_size == 0 and got.rc == 0 and got.grp_first.tolist() == [0, 0, 0]


# ---- Engine.polish ---------------------------------------------------------------------------------------------------------------------------------------------------

def check_polish(got, want, what):
    assert len(got) == len(want)
    for g, (p, (seq, members)) in enumerate(zip(got, want)):
        print(f"{what}: group {g}: {len(p.sequence)} bases, members a window {[w.members for w in p.windows]}")
        assert [w.members for w in p.windows] == members, (what, g)
        assert all(w.status == ca.WIN_CONSENSUS and not w.kept_reference for w in p.windows)
        assert p.sequence == seq, f"{what}: group {g}: first difference at {next((i for i, (a, b) in enumerate(zip(p.sequence, seq)) if a != b), min(len(seq), len(p.sequence)))}"


def test_polish_equals_the_reference_composition_on_the_seed_8_input(eng):
    groups = [seed8()]
    check_polish(eng.polish(groups, 100), cp.polish(groups, 100, MAX_MSA), "seed 8")


def test_polish_equals_the_reference_composition_on_the_seed_9_input(eng):
    groups = [seed9()]
    check_polish(eng.polish(groups, 64), cp.polish(groups, 64, MAX_MSA), "seed 9")


def test_polish_of_both_in_one_call_and_beside_groups_without_windows(eng):
    groups = [seed8(), [], seed9(), [""], [pl.round_edges()[0]]]
    for W in (100, 64):
        got = eng.polish(groups, W)
        check_polish(got, cp.polish(groups, W, MAX_MSA), f"together, W = {W}")
        assert got[1].sequence == "" and got[1].windows == [] and got[3].sequence == "" and got[4].sequence == groups[4][0]
    assert eng.polish([[], []]) [0].sequence == "" and len(eng.polish([[], []])) == 2
    with pytest.raises(ca.EngineError):
        eng.polish(groups, 0)


def test_polish_brings_the_draft_nearer_to_its_truth(eng):
    truth, grp = cp.polish_input(**cp.SEED8)
    (p,) = eng.polish([list(grp)], 100)
    draft_d, polished_d = cp.edit_distance(grp[0], truth), cp.edit_distance(p.sequence, truth)
    print(f"seed 8: draft {draft_d} edits from the truth, polished on the device {polished_d}")
    assert polished_d < draft_d


def test_a_window_whose_group_stops_keeps_its_reference_piece_and_says_so(eng):
    """W = 5 000 on a 6 000-base reference with one spanning read: window 0's members are beyond the 4 095 bases any POA tier takes."""
    rng = random.Random(0x6000)
    ref = pop.rand_seq(rng, 6000)
    read = pop.ont_copy(rng, ref, 0.01)
    small = pop.rand_seq(rng, 300)  # its neighbour: three reads that span its one window
    groups = [[ref, read], [small] + [small[:20] + pop.ont_copy(rng, small[20:-20], 0.05) + small[-20:] for _ in range(3)]]
    want_groups, first = cp.cut_groups(groups, 5000)
    assert first == [0, 2, 3] and [len(g) for g in want_groups] == [2, 2, 4] and len(want_groups[0][1]) > 4095  # the read spans both windows
    got = eng.polish(groups, 5000)
    w0, w1 = got[0].windows
    assert (w0.members, w0.status, w0.kept_reference) == (1, ca.WIN_OVERFLOW, True)
    assert (w1.members, w1.status, w1.kept_reference) == (1, ca.WIN_CONSENSUS, False)
    assert got[0].sequence == ref[:5000] + pop.oracle_consensus(want_groups[1], MAX_MSA)
    assert got[1].sequence == pop.oracle_consensus(want_groups[2], MAX_MSA) and got[1].windows[0].members == 3 and not got[1].windows[0].kept_reference  # unaffected


def test_more_windows_than_a_poa_run_takes_are_refused(eng):
    ref = pl.round_edges()[0]
    limit = eng.max_batch_windows()
    n = limit // len(ref) + 1  # W = 1: a window a column
    with pytest.raises(ca.EngineError, match="split"):
        eng.polish([[ref]] * n, 1)
