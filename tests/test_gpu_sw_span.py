"""The span runs on the GPU (include/consent_amd.h cw_sw_span_run, cw_sw_path_span_run, cw_pileup_span_run, cw_sw_cut_span_run, cw_seed_spans_device;
csrc/cw_sw_op.h sw_unpack_from): every row, op, count and cut word of a spanned pair equals the existing run on the sliced reference with lo added back, and the
plain reference of tests/sw_span_probes.py -- for one query per launch class on references on both sides of the LDS limit and beyond CW_SW_RMAX, spans that
begin and end anywhere in a packed word, on a reference's last partial word, at the LDS / global switch and at the capacity; a whole-reference span is the
existing entry point bit for bit; the bases next to a span never take part; empty, inverted, clamped and oversized spans follow the header beside normal pairs;
the words depend on no batch composition; cw_seed_spans_device is its rule; and Engine.polish(seeded=True) / polish_reads(seeded=True) polish the contig of
tests/seed_probes.py exactly as the unspanned polish of the oriented reads does."""
import ctypes as C

import numpy as np
import pytest

import consent_amd as ca
import pileup_probes as pl
import seed_probes as sdp
import sw_op_probes as sp
import sw_path_probes as pp
import sw_span_probes as ss
from consent_amd import engine as en
from consent_amd.engine import Batch, HostBatch, SwSpans, _ptr
from test_sw_span_cpu import LISTED

pytestmark = pytest.mark.gpu
E_INVALID, E_CAPACITY = -1, -4
W = 100
JUNK = (0xFFFFFFFF, 0)  # what a reference's own entry holds: it is not read


@pytest.fixture(scope="module")
def eng():
    e = ca.Engine(ca.Params(*sp.PRM))
    yield e
    e.close()


class Spanned:
    """cases [(name, query, ref, lo, hi)] as groups by reference, and the four span runs over them."""

    def __init__(self, eng, cases, order=None):
        self.cases = cases
        refs = []
        for c in cases:
            if c[2] not in refs:
                refs.append(c[2])
        self.groups = [[r] + [c[1] for c in cases if c[2] == r] for r in refs]
        self.where = {}  # case index -> (group, member)
        lo, hi = [], []
        for g, r in enumerate(refs):
            lo.append(JUNK[0]); hi.append(JUNK[1])
            k = 0
            for i, c in enumerate(cases):
                if c[2] == r:
                    k += 1
                    self.where[i] = (g, k)
                    lo.append(c[3]); hi.append(c[4])
        self.spans = (np.array(lo, np.int64), np.array(hi, np.int64))
        self.plain = eng.sw(self.groups, want_indels=True, spans=self.spans)
        self.path = eng.sw_path(self.groups, spans=self.spans)
        self.eqx = eng.sw_path(self.groups, eqx=True, spans=self.spans)
        self.pile = eng.pileup(self.groups, spans=self.spans)
        self.cut = eng.sw_cut(self.groups, W, spans=self.spans)

    def check_against_the_plain_reference(self):
        want_counts = [np.zeros((len(g[0]), pl.COL), np.uint32) for g in self.groups]
        for i, (name, q, ref, lo, hi) in enumerate(self.cases):
            g, k = self.where[i]
            e = ss.span_expected(q, ref, lo, hi)
            assert tuple(int(x) for x in self.plain.row(g, k)) == e.plain_row, f"{name}: cw_sw_span_run"
            for run, what in ((self.path, "path"), (self.eqx, "path (EQX)"), (self.pile, "pileup"), (self.cut, "cut")):
                assert tuple(int(x) for x in run.row(g, k)) == e.row, f"{name}: the {what} run's row"
            assert tuple(self.path.ops(g, k)) == e.ops and tuple(self.eqx.ops(g, k)) == e.ops_eqx, f"{name}: ops"
            assert [int(x) for x in self.cut.cuts(g, k)] == e.cuts(W), f"{name}: cut words"
            want_counts[g] += e.counts
        for g in range(len(self.groups)):
            assert np.array_equal(self.pile.counts(g), want_counts[g]), f"group {g}: counts"
            assert int(self.path.row(g, 0)[en.SW_STATUS]) == ca.SW_IS_REF


def shifted(rows, lo):
    """Rows of a run on reference[lo:hi) in the whole reference's coordinates."""
    out = np.array(rows, np.int32).reshape(-1, en.SW_ROW).copy()
    pos = out[:, en.SW_SCORE] > 0
    out[pos, en.SW_REF_BEGIN] += lo
    out[pos, en.SW_REF_END] += lo
    return out


@pytest.fixture(scope="module")
def identity(eng):
    return Spanned(eng, ss.identity_cases())


def test_spanned_pairs_equal_the_plain_reference(identity):
    """Rows, ops, counts and cut words of every identity case: lo % 16 and hi % 16 in {0, 1, 15}, hi = n on a last partial word, spans of 2 048, 2 049 and
    16 383 columns, on references of 600, 2 049 and 16 401 bases, a query per launch class."""
    assert {len(c[1]) for c in identity.cases} >= set(ss.QUERY_LENS) and {len(c[2]) for c in identity.cases} == set(ss.REF_LENS)
    assert {c[4] - c[3] for c in identity.cases} >= {2048, 2049, sp.RMAX}
    assert sum(ss.span_expected(*c[1:]).row[0] > 0 for c in identity.cases) >= len(identity.cases) - 2  # (the probes do align)
    identity.check_against_the_plain_reference()


def test_spanned_pairs_equal_the_existing_runs_on_the_sliced_reference(eng, identity):
    cases = identity.cases
    sliced = [[c[2][c[3] : c[4]], c[1]] for c in cases]
    plain, path, pile = eng.sw(sliced, want_indels=True), eng.sw_path(sliced), eng.pileup(sliced)
    eqx, cut = eng.sw_path(sliced, eqx=True), eng.sw_cut(sliced, W)
    n_cut = 0
    for i, (name, q, ref, lo, hi) in enumerate(cases):
        g, k = identity.where[i]
        assert np.array_equal(shifted(plain.row(i, 1), lo)[0], identity.plain.row(g, k)), f"{name}: cw_sw_run on the slice"
        assert np.array_equal(shifted(path.row(i, 1), lo)[0], identity.path.row(g, k)), f"{name}: cw_sw_path_run on the slice"
        assert list(path.ops(i, 1)) == list(identity.path.ops(g, k)) and list(eqx.ops(i, 1)) == list(identity.eqx.ops(g, k)), f"{name}: ops"
        for run, mine in ((eqx, identity.eqx), (pile, identity.pile), (cut, identity.cut)):
            assert np.array_equal(shifted(run.row(i, 1), lo)[0], mine.row(g, k)), f"{name}: rows on the slice"
        if lo % W == 0:  # the slice's windows are the whole reference's from window lo / W on; before them every word is query_begin, behind them query_end + 1
            whole, part = [int(x) for x in identity.cut.cuts(g, k)], [int(x) for x in cut.cuts(i, 1)]
            t0 = lo // W
            assert whole[t0 : t0 + len(part) - 1] == part[:-1] and set(whole[:t0]) <= {part[0]} and set(whole[t0 + len(part) - 1 :]) == {part[-1]}, f"{name}: cut words on the slice"
            n_cut += 1
    assert n_cut >= 3
    for g, grp in enumerate(identity.groups):  # the slices' counts, each at its lo, add up to the whole reference's
        want = np.zeros((len(grp[0]), pl.COL), np.uint32)
        for i, c in enumerate(cases):
            if identity.where[i][0] == g:
                want[c[3] : c[4]] += pile.counts(i)
        assert np.array_equal(identity.pile.counts(g), want)


def test_a_reference_whose_words_are_the_batch_s_last(eng):
    """hi = n with n % 16 != 0 where nothing lies behind the reference's last partial word: the reference's words are packed last."""
    n, m = 600, 100
    ref, q = ss.ref_of(n), ss.query_on(n, m, n - m - 10, 3)
    hb = ca.pack_piles([[q, ref]])
    turned = HostBatch(hb.win_first_seq, hb.seq_len[[1, 0]].copy(), hb.seq_word_off[[1, 0]].copy(), hb.bases)  # sequence 0 is the reference, its words the last
    for lo in (n - 203, n - 195, n - 189):
        e = ss.span_expected(q, ref, lo, n)
        spans = ([0, lo], [0, n])
        assert tuple(int(x) for x in eng.sw_path(turned, spans=spans).row(0, 1)) == e.row and e.row[0] > 0
        assert [int(x) for x in eng.sw_cut(turned, W, spans=spans).cuts(0, 1)] == e.cuts(W)
        assert np.array_equal(eng.pileup(turned, spans=spans).counts(0), e.counts)


def test_a_whole_reference_span_is_the_existing_entry_point_bit_for_bit(eng):
    pairs = list(sp.instance_pairs().values())[::3] + list(sp.long_pairs().values())[:1] + list(sp.nothing_pairs().values())
    groups = [[r, q] for q, r in pairs]
    S = 2 * len(groups)
    for hi in ([len(g[i]) if i == 0 else len(g[0]) for g in groups for i in (0, 1)], [0xFFFFFFFF] * S):
        spans = (np.zeros(S, np.int64), np.array(hi, np.int64))
        assert np.array_equal(eng.sw(groups, True, spans=spans).rows, eng.sw(groups, True).rows)
        a, b = eng.sw_path(groups, eqx=True, spans=spans), eng.sw_path(groups, eqx=True)
        assert np.array_equal(a.rows, b.rows) and np.array_equal(a.n_ops, b.n_ops) and np.array_equal(a.ops_buf, b.ops_buf)
        a, b = eng.pileup(groups, spans=spans), eng.pileup(groups)
        assert np.array_equal(a.rows, b.rows) and np.array_equal(a.counts_buf, b.counts_buf)
        a, b = eng.sw_cut(groups, W, spans=spans), eng.sw_cut(groups, W)
        assert np.array_equal(a.rows, b.rows) and np.array_equal(a.cuts_buf, b.cuts_buf)


@pytest.mark.parametrize("n", ss.REF_LENS)
def test_the_bases_next_to_a_span_never_take_part(eng, n):
    """A query equal to ref[lo - 3 : hi + 3]: the alignment is clipped to [lo, hi), and no column outside counts anything."""
    ref = ss.ref_of(n)
    cases = []
    for lo, hi in ((203, 397), (208, 400), (n - 300 - 3, n - 3)):
        cases.append((f"n{n} [{lo}, {hi})", ref[lo - 3 : hi + 3], ref, lo, hi))
    run = Spanned(eng, cases)
    run.check_against_the_plain_reference()
    counts = run.pile.counts(0)
    for i, (_, q, _, lo, hi) in enumerate(cases):
        row = run.path.row(0, i + 1)
        assert tuple(int(x) for x in row[:5]) == (2 * (hi - lo), lo, hi - 1, 3, 3 + hi - lo - 1)
    covered = np.zeros(n, bool)
    for c in cases:
        covered[c[3] : c[4]] = True
    assert not counts[~covered].any()


def test_degenerate_spans_beside_normal_pairs(eng):
    """One group: hi <= lo, lo > hi, hi > n, lo >= n, a span of 16 384 columns (CW_SW_STOP for that pair alone, CW_E_CAPACITY from the host form) and of
    16 383, beside normal pairs; the reference's own row is CW_SW_IS_REF."""
    n = 20000
    ref = ss.ref_of(n)
    q = ref[5000:5200]
    spans = [(4900, 5400), (5100, 5100), (5400, 4900), (19000, 10 ** 9), (n, n + 5), (n + 7, 3), (100, 100 + sp.RMAX + 1), (4000, 4000 + sp.RMAX), (0, 0), (4990, 5210)]
    late = ref[19500:19700]
    cases = [(f"span {s}", late if s[0] == 19000 else q, ref, s[0], s[1]) for s in spans]
    run = Spanned(eng, cases)
    assert run.plain.rc == run.path.rc == run.pile.rc == run.cut.rc == E_CAPACITY
    run.check_against_the_plain_reference()
    status = [int(run.path.row(0, k + 1)[en.SW_STATUS]) for k in range(len(spans))]
    score = [int(run.path.row(0, k + 1)[en.SW_SCORE]) for k in range(len(spans))]
    assert status == [0, 0, 0, 0, 0, 0, ca.SW_STOP, 0, 0, 0] and [x > 0 for x in score] == [True, False, False, True, False, False, False, True, False, True]
    without = Spanned(eng, [c for k, c in enumerate(cases) if k != 6])
    assert without.path.rc == 0


def test_null_spans_are_invalid_with_an_engine(eng):
    hb = ca.pack_piles([["ACGTACGTACGT", "ACGTACG"]])
    b = hb.c_struct()
    rows = np.full((2, 8), 77, np.int32)
    lo, hi = np.zeros(2, np.uint32), np.full(2, 12, np.uint32)
    l = eng.lib
    assert l.cw_sw_span_run(eng.handle, C.byref(b), _ptr(rows), None, 0) == E_INVALID
    for spans in (SwSpans(None, _ptr(hi)), SwSpans(_ptr(lo), None)):
        assert l.cw_sw_span_run(eng.handle, C.byref(b), _ptr(rows), C.byref(spans), 0) == E_INVALID
        cut_off, words = np.array([0, 0, 2], np.uint64), np.full(2, 77, np.uint32)
        cuts = en.SwCuts(_ptr(words), _ptr(cut_off), 100)
        assert l.cw_sw_cut_span_run(eng.handle, C.byref(b), _ptr(rows), C.byref(cuts), C.byref(spans)) == E_INVALID
        assert (words == 77).all()
    assert (rows == 77).all()
    empty = Batch(0, 0, 0, None, None, None, None)
    assert l.cw_sw_span_run(eng.handle, C.byref(empty), None, None, 0) == E_INVALID  # no spans at all, even without sequences
    assert l.cw_sw_span_run(eng.handle, C.byref(empty), None, C.byref(SwSpans(None, None)), 0) == 0
    seed_rows = np.zeros((2, 4), np.int32)
    assert l.cw_seed_spans(eng.handle, C.byref(b), _ptr(seed_rows), 14, 64, 32, _ptr(lo), _ptr(hi)) == E_INVALID  # pad_shift > 31
    assert l.cw_seed_spans(eng.handle, C.byref(b), _ptr(seed_rows), 14, 64, 4, None, _ptr(hi)) == E_INVALID


def test_the_words_depend_on_no_batch_composition(eng, identity):
    cases = identity.cases
    parts = [Spanned(eng, cases[i::3]) for i in range(3)]
    for p in range(3):
        for j, i in enumerate(range(p, len(cases), 3)):
            g, k = identity.where[i]
            g2, k2 = parts[p].where[j]
            name = cases[i][0]
            assert np.array_equal(identity.path.row(g, k), parts[p].path.row(g2, k2)) and np.array_equal(identity.plain.row(g, k), parts[p].plain.row(g2, k2)), name
            assert list(identity.eqx.ops(g, k)) == list(parts[p].eqx.ops(g2, k2)), name
            assert np.array_equal(identity.cut.cuts(g, k), parts[p].cut.cuts(g2, k2)), name


def test_seed_spans_device_is_its_rule(eng):
    """The crafted rows of sw_span_probes.SEED_CASES -- a negative DIAG, DIAG + ... > n, hits at min_hits - 1 and at min_hits, IS_REF and NONE rows,
    pad_shift = 31, a reference of 2^31 - 1 columns -- through the device form: the kernel reads lengths and rows only, so the lengths are the cases' own."""
    import torch

    dev = torch.device("cuda", eng.device)
    for m, n, row, mh, pad, sh in ss.SEED_CASES:
        ref_row = (sdp.IS_REF, 0, 0, 0)
        first, second = (row, ref_row) if row[0] == sdp.IS_REF else (ref_row, row)  # (an IS_REF row is a group's first)
        lens = [m, 5] if row[0] == sdp.IS_REF else [n, m]
        t_wfs = torch.tensor([0, 2], dtype=torch.int32, device=dev)
        t_len = torch.from_numpy(np.array(lens, np.uint32).view(np.int32)).to(dev)
        t_off = torch.zeros(2, dtype=torch.int64, device=dev)
        t_bases = torch.zeros(4, dtype=torch.int32, device=dev)
        t_rows = torch.tensor([first, second], dtype=torch.int32, device=dev).reshape(-1)
        t_lo = torch.full((2,), 77, dtype=torch.int32, device=dev)
        t_hi = torch.full((2,), 77, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        b = Batch(1, 2, 4, t_wfs.data_ptr(), t_len.data_ptr(), t_off.data_ptr(), t_bases.data_ptr())
        eng.seed_spans_device(b, t_rows.data_ptr(), t_lo.data_ptr(), t_hi.data_ptr(), mh, pad, sh)
        torch.cuda.synchronize(dev)
        lo, hi = t_lo.cpu().numpy().view(np.uint32), t_hi.cpu().numpy().view(np.uint32)
        want = [ss.seed_spans(lens[0], lens[0], first, mh, pad, sh), ss.seed_spans(lens[1], lens[0], second, mh, pad, sh)]
        assert [(int(lo[i]), int(hi[i])) for i in (0, 1)] == want, (m, n, row)
        assert want[0] == (0, 0)
    assert "seed_spans" in eng.timings()


@pytest.fixture(scope="module")
def contig():
    draft, reads, _, _ = sdp.draft_and_reads(**sdp.CONTIG)
    keep = [r for r in range(len(reads)) if not {(0, r), (1, r), (2, r)} & set(LISTED)]  # (every read: the CPU test lists none)
    assert len(keep) * 10 >= len(reads) * 9
    return draft, [reads[r] for r in keep]


def same_polish(a, b):
    assert a.sequence == b.sequence
    assert [(w.members, w.status, w.kept_reference) for w in a.windows] == [(w.members, w.status, w.kept_reference) for w in b.windows]


def test_seed_spans_of_a_seed_run_and_the_seeded_polish(eng, contig):
    """Engine.polish(seeded=True) equals polish() of the same group with the reads oriented by the seed run's strands and no spans: sequence and per-window
    members bit for bit.  It rests on tests/test_sw_span_cpu.py: every read's spanned row equals its full row."""
    draft, reads = contig
    groups = [[draft] + list(reads)]
    seeds = eng.seeds(groups)
    lo, hi = eng.seed_spans(groups, seeds)
    lens = [len(x) for x in groups[0]]
    for s in range(len(lens)):
        assert (int(lo[s]), int(hi[s])) == ss.seed_spans(lens[s], len(draft), seeds.rows[s], en.SEED_MIN_HITS, ss.PAD, en.SPAN_PAD_SHIFT), s
    assert (hi[1:] > lo[1:]).all() and float(np.mean(hi[1:].astype(np.int64) - lo[1:])) < 0.5 * len(draft)
    oriented = eng.revcomp(groups, seeds.strands)
    full, part = eng.sw_cut(oriented, 500), eng.sw_cut(oriented, 500, spans=(lo, hi))
    assert np.array_equal(full.rows, part.rows) and np.array_equal(full.cuts_buf, part.cuts_buf)
    want = eng.polish(oriented, 500)[0]
    got = eng.polish(groups, 500, seeded=True)[0]
    same_polish(got, want)
    assert got.strands == [int(x) for x in seeds.strands[1:]] and sdp.REV in got.strands
    with pytest.raises(ca.EngineError):
        eng.polish(groups, 500, seeded=True, orient=True)
    # an unplaced read costs nothing and changes nothing
    other = sdp.draft_and_reads(**sdp.CONTIG)[3][:3]
    same_polish(eng.polish([[draft] + list(reads) + list(other)], 500, seeded=True)[0], want)


def test_polish_reads_seeded_is_one_group_without_tiles(eng, contig):
    draft, reads = contig
    got = eng.polish_reads(draft, reads, window=500, tile=1000, seeded=True)
    same_polish(got, eng.polish([[draft] + list(reads)], 500, seeded=True)[0])
    assert got.placements == eng.polish_reads(draft, reads, window=500, tile=1000).placements and None not in got.placements
    assert eng.polish_reads(draft, reads, window=500, tile=1100, seeded=True).sequence == got.sequence  # tile % window is no longer required
