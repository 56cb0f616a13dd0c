"""What the host-buffer entry points share (include/consent_amd.h: cw_sw_run, cw_sw_path_run, cw_pileup_run, cw_sw_cut_run and their span forms, cw_strand_run,
cw_seed_run, cw_seed_spans, cw_revcomp, cw_poa_run), held to one table: a malformed batch -- groups that do not begin at sequence 0, do not end at n_seqs or step
back, a sequence whose words end beyond n_words, slot offsets that step back -- is CW_E_INVALID and no output byte is written; a batch without sequences is CW_OK
and no output byte is written; a good batch is CW_OK and nothing behind an output is written.  The batch is the smallest that crosses a packed-word boundary and
holds a reference alone: a 24-base reference with two 20-base queries, and a group of one 17-base sequence.  A malformed batch only ever goes to a host form,
which refuses it before anything is enqueued; the values every form computes are the other operator tests' business."""
import ctypes as C
import types

import numpy as np
import pytest

import consent_amd as ca
import sw_op_probes as sp
from consent_amd.engine import SEED_ROW, SW_ROW, Batch, Pileup, Result, Seeds, Strands, SwCuts, SwPaths, SwSpans, _ptr

pytestmark = pytest.mark.gpu
E_INVALID = -1
FILL = 0x5A
GUARD = 8
WINDOW = 10  # the cut run's reference window: three windows on the 24-base reference


@pytest.fixture(scope="module")
def eng():
    e = ca.Engine(ca.Params(*sp.PRM))
    yield e
    e.close()


@pytest.fixture(scope="module")
def good(eng):
    """The good batch, what a span form and cw_seed_spans read beside it, and the good slot offsets of every form that has slots."""
    rng = np.random.default_rng(20)
    ref, alone = ("".join(rng.choice(list("ACGT"), n)) for n in (24, 17))
    hb = ca.pack_piles([[ref, ref[:20], ref[4:]], [alone]])
    z = types.SimpleNamespace(hb=hb, G=hb.n_windows, S=len(hb.seq_len), words=len(hb.bases))
    assert (z.G, z.S, z.words) == (2, 4, 8) and hb.seq_len.tolist() == [24, 20, 20, 17]
    lens = hb.seq_len.astype(np.int64)
    ref_len = np.array([24, 24, 24, 17], np.int64)
    is_ref = np.array([True, False, False, True])
    z.lo, z.hi = np.zeros(z.S, np.uint32), ref_len.astype(np.uint32)  # every column of the reference
    z.seed_rows = np.zeros((z.S, SEED_ROW), np.int32)
    z.seed_rows[:, 0] = np.where(is_ref, ca.STRAND_IS_REF, ca.STRAND_NONE)
    z.slots = {
        "path": np.cumsum([0] + (lens + ref_len).tolist()),  # sw_ops_bound
        "pile": np.cumsum([0] + np.where(is_ref, lens, 0).tolist()),
        "cut": np.cumsum([0] + np.where(is_ref, 0, ca.sw_cuts(ref_len, WINDOW)).tolist()),
        "poa": np.cumsum([0] + ca.poa_slot_bytes(np.array([24, 17])).tolist()),
    }
    return z


class Outputs:
    """The output arrays of one call: each filled with a pattern, 16-byte aligned, and GUARD elements longer than what the form may write."""

    def __init__(self):
        self.arrays = []

    def new(self, n, dtype):
        raw = np.full((n + GUARD) * np.dtype(dtype).itemsize + 16, FILL, np.uint8)
        at = -raw.ctypes.data % 16
        a = raw[at : at + (n + GUARD) * np.dtype(dtype).itemsize].view(dtype)
        self.arrays.append((a, n))
        return a

    def untouched(self):
        return all((a.view(np.uint8) == FILL).all() for a, _ in self.arrays)

    def guards_intact(self):
        return all((a[n:].view(np.uint8) == FILL).all() for a, n in self.arrays)


def call(eng, z, name, head, tail=()):
    """cw_<name>(engine, *head, *tail), or with the spans between the two for a span form"""
    mid = (C.byref(SwSpans(_ptr(z.lo), _ptr(z.hi))),) if "_span_" in name else ()
    return getattr(eng.lib, name)(eng.handle, *head, *mid, *tail)


# one function per host body: (engine, good batch's sizes and side inputs, entry point, batch struct, slot offsets, outputs) -> return value

def sw(eng, z, name, b, slot, out):
    return call(eng, z, name, (C.byref(b), _ptr(out.new(z.S * SW_ROW, np.int32))), (0,))


def sw_path(eng, z, name, b, slot, out):
    paths = SwPaths(_ptr(out.new(int(z.slots["path"][-1]), np.uint32)), _ptr(slot), _ptr(out.new(z.S, np.uint32)))
    return call(eng, z, name, (C.byref(b), _ptr(out.new(z.S * SW_ROW, np.int32)), C.byref(paths)), (0,))


def pileup(eng, z, name, b, slot, out):
    pile = Pileup(_ptr(out.new(int(z.slots["pile"][-1]) * ca.PILE_COL, np.uint32)), _ptr(slot))
    return call(eng, z, name, (C.byref(b), _ptr(out.new(z.S * SW_ROW, np.int32)), C.byref(pile)), (0,))


def sw_cut(eng, z, name, b, slot, out):
    cuts = SwCuts(_ptr(out.new(int(z.slots["cut"][-1]), np.uint32)), _ptr(slot), WINDOW)
    return call(eng, z, name, (C.byref(b), _ptr(out.new(z.S * SW_ROW, np.int32)), C.byref(cuts)))


def strand(eng, z, name, b, slot, out):
    return call(eng, z, name, (C.byref(b), C.byref(Strands(_ptr(out.new(z.S, np.uint8)), _ptr(out.new(z.S * 2, np.uint32)), 0))))


def seed(eng, z, name, b, slot, out):
    return call(eng, z, name, (C.byref(b), C.byref(Seeds(_ptr(out.new(z.S * SEED_ROW, np.int32)), _ptr(out.new(z.S, np.uint8)), 0))))


def seed_spans(eng, z, name, b, slot, out):
    return call(eng, z, name, (C.byref(b), _ptr(z.seed_rows), ca.SEED_MIN_HITS, ca.SPAN_PAD, ca.SPAN_PAD_SHIFT, _ptr(out.new(z.S, np.uint32)), _ptr(out.new(z.S, np.uint32))))


def revcomp(eng, z, name, b, slot, out):
    return call(eng, z, name, (C.byref(b), None, _ptr(out.new(z.words, np.uint32))))


def poa(eng, z, name, b, slot, out):
    res = Result(_ptr(out.new(int(z.slots["poa"][-1]), np.uint8)), _ptr(slot), _ptr(out.new(z.G, np.uint32)), _ptr(out.new(z.G, np.uint8)), None, None, None)
    return call(eng, z, name, (C.byref(b), C.byref(res)))


# entry point -> (its body above, the key of its slot offsets in good.slots or None)
FORMS = {
    "cw_sw_run": (sw, None), "cw_sw_span_run": (sw, None),
    "cw_sw_path_run": (sw_path, "path"), "cw_sw_path_span_run": (sw_path, "path"),
    "cw_pileup_run": (pileup, "pile"), "cw_pileup_span_run": (pileup, "pile"),
    "cw_sw_cut_run": (sw_cut, "cut"), "cw_sw_cut_span_run": (sw_cut, "cut"),
    "cw_strand_run": (strand, None), "cw_seed_run": (seed, None), "cw_seed_spans": (seed_spans, None), "cw_revcomp": (revcomp, None),
    "cw_poa_run": (poa, "poa"),
}
BROKEN = ["first group not at sequence 0", "last group not at n_seqs", "groups step back", "words beyond n_words", "slots step back"]


def run_form(eng, z, name, broken=None, empty=False):
    """One call of the entry point on the good batch, on it with one thing broken, or on the batch without sequences: (return value, its Outputs)."""
    body, key = FORMS[name]
    wfs, word_off = z.hb.win_first_seq.copy(), z.hb.seq_word_off.copy()
    slot = None if key is None else z.slots[key].astype(np.uint64)
    if broken == BROKEN[0]:
        wfs[0] = 1
    elif broken == BROKEN[1]:
        wfs[z.G] = z.S - 1
    elif broken == BROKEN[2]:
        wfs[1] = z.S + 1  # (with two groups, the only step back that leaves both ends where they belong)
    elif broken == BROKEN[3]:
        word_off[z.S - 1] = z.words - 1  # the 17-base sequence has two words
    elif broken == BROKEN[4]:
        slot[1] = slot[2] + 1
    b = Batch(0, 0, 0, None, None, None, None) if empty else Batch(z.G, z.S, z.words, _ptr(wfs), _ptr(z.hb.seq_len), _ptr(word_off), _ptr(z.hb.bases))
    out = Outputs()
    return body(eng, z, name, b, slot, out), out


@pytest.mark.parametrize("name,broken", [(n, k) for n in FORMS for k in BROKEN if k != BROKEN[4] or FORMS[n][1]])
def test_a_malformed_batch_is_refused_and_nothing_is_written(eng, good, name, broken):
    rc, out = run_form(eng, good, name, broken=broken)
    assert rc == E_INVALID, f"{name}, {broken}: returned {rc}"
    assert out.untouched(), f"{name}, {broken}: a refused call wrote to an output"


@pytest.mark.parametrize("name", FORMS)
def test_a_batch_without_sequences_is_ok_and_nothing_is_written(eng, good, name):
    rc, out = run_form(eng, good, name, empty=True)
    assert rc == 0, f"{name}: returned {rc}"
    assert out.untouched(), f"{name}: a call without sequences wrote to an output"


@pytest.mark.parametrize("name", FORMS)
def test_the_good_batch_runs_and_nothing_behind_an_output_is_written(eng, good, name):
    rc, out = run_form(eng, good, name)
    assert rc == 0, f"{name}: returned {rc}"
    assert out.guards_intact(), f"{name}: words behind an output were written"
