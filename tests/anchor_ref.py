"""The plain Python / numpy reference for the second half of cw_index_kernel (consent_amd/csrc/cw_index.h: anchors, position matrix, classification, masks,
correction rows, presence bits, hand-over): what the kernel writes into a window's anchor block (CwAbCarve), from the pile's strings and prm alone -- no
call into the library or the oracle.  tests/test_anchor_ref_cpu.py tests the reference against itself (the score identity below) and
tests/test_gpu_anchor_block.py compares the block read back (Engine.anchor_block) with it, byte for byte.

The block's contract (block_reference(pile, prm); DESIGN.md says the same):
  header    A, N, n_dirty (0 without bitsets), flags (1 use_bits, 2 one-word masks, 4 correction rows), n_rows (0 unless flag 4)
  ckey      the anchors' k-mers in template order, as integers in str2num order (chain_probes.anchors: template k-mers repeated in no sequence, held by
            at least min(common_kmers, N // 2) sequences)
  P[a][s]   the anchor's one position in sequence s, 0xFFFF when absent; columns N .. Np - 1 (Np = N rounded up to twice an odd number) are 0xFFFF
  classes   a sequence is clean when the positions of the anchors it holds increase strictly with the anchor index, else dirty: backward when the
            backward scan has strictly fewer bad anchors than the forward one, else forward (a tie goes forward); its bad anchors are those that set no
            new record in its direction (chain_probes.classify).  Without bitsets nothing is classified
  dirty     the dirty sequences -- as a set: the kernel's order depends on thread timing
  pres[a]   bit s iff s < N, P[a][s] is present and s is clean, or s is dirty, masks count (W = 1 word, or rows exist) and a is not bad in s; the bits
            s >= N of the last word are 0.  Without masks that count a dirty sequence has no bit anywhere
  badm[a]   with flag 2 only: bit d iff a is bad in dirty[d]; the bits d >= n_dirty are 0
  rowid     with flag 4 only: the anchors that are bad somewhere numbered in anchor order, the others 0xFF
  delta     with flag 4 only: delta[row(x)][y] = the dirty sequences in which x is bad and the pair (x, y) is in template order -- y > x: P[y] present and
            P[x] < P[y]; y < x: y not bad there, P[y] present and P[y] < P[x]; 0 for y = x and in the columns A .. Ap - 1 (Ap = A rounded up to 16)
Bytes the kernel does not write, which nothing compares: badm without flag 2 (no masks, or masks of W > 1 words), rowid and delta without flag 4 (the
layout has neither: P starts where rowid would), the header's bytes 20 .. 63, the gaps that align every part to 16 bytes, and anything behind P.

The score identity (rebuilt_scores): for every pair a < b the score the chain kernel reads out of the block (cw_chain.h, the scoring routes) is the plain
score #{s: both held, P[a][s] < P[b][s]}:
  without flag 1     over P, all Np columns (a pad never counts: it is 0xFFFF)
  with flag 1        popcount(pres[a] & pres[b]) over all Nw words, plus
    flag 4           delta[rowid[a]][b] + delta[rowid[b]][a], a missing row counting 0
    else flag 2      over the dirty sequences named in badm[a] | badm[b]: P[a] < P[b] and P[b] present
    else             the same over every dirty sequence
canonical(block) is what two blocks of the same window must have in common whatever order their dirty lists came out in."""
import numpy as np

from chain_probes import anchors, classify, index_arithmetic
from consent_amd.engine import AB_NONE16, ab_np
from index_probes import str2num

__all__ = ["block_reference", "plain_scores", "rebuilt_scores", "canonical", "assert_same_block", "assert_score_identity"]


class BlockRef:
    pass


def pack_bits(bits, words):
    """A x n booleans -> A x words u64, bit s of a row in word s // 64 at s % 64."""
    full = np.zeros((bits.shape[0], words * 64), np.uint8)
    full[:, : bits.shape[1]] = bits
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little")).view(np.uint64).reshape(bits.shape[0], words)


def block_reference(pile, prm):
    """The window's anchor block, the parts as Engine.anchor_block names them (dirty ascending, badm over that order), and what the reference knows
    besides: P32 (int32, -1 absent), direction and bad ({dirty sequence: ...}, of every dirty sequence the pile has, bitsets or not), arith
    (chain_probes.index_arithmetic), nk0."""
    k, common = prm[0], prm[2]
    r = BlockRef()
    r.sup, r.P32 = anchors(pile, k, common)
    r.A, r.N = len(r.P32), len(pile)
    A, N = r.A, r.N
    r.nk0 = max(len(pile[0]) - k + 1, 0)
    r.Nw, r.Np, r.Ap = (N + 63) // 64, ab_np(N), (A + 15) & ~15
    all_dirty, bad_rows, r.direction, r.bad = classify(r.P32, detail=True)
    r.all_dirty = all_dirty
    r.arith = ar = index_arithmetic(A, N, len(all_dirty), r.nk0, bad_rows)
    r.use_bits, r.has_bm, r.has_delta = ar["use_bits"], ar["one_word"], ar["fix"]
    r.n_dirty, r.n_rows = ar["n_dirty"], ar["n_rows"]
    r.flags = int(r.use_bits) | 2 * int(r.has_bm) | 4 * int(r.has_delta)
    held = r.P32 >= 0
    r.ckey = np.array([str2num(pile[0][p : p + k]) for p in r.P32[:, 0]], np.uint32) if A else np.zeros(0, np.uint32)
    r.P = np.full((A, r.Np), AB_NONE16, np.uint16)
    r.P[:, :N] = np.where(held, r.P32, AB_NONE16).astype(np.uint16)
    r.dirty = np.array(all_dirty if r.use_bits else [], np.uint16)
    isbad = np.zeros((A, N), bool)  # anchor a is bad in (dirty) sequence s
    for s in r.dirty:
        isbad[r.bad[int(s)], int(s)] = True
    r.isbad = isbad
    dirty_col = np.zeros(N, bool)
    dirty_col[r.dirty.astype(np.int64)] = True
    counts = ar["masks_count"]  # the masks count in the presence bits: one word, or rows made of wider ones
    bits = held & (~dirty_col[None, :] | (isbad == False if counts else False))
    r.pres = pack_bits(bits, r.Nw) if r.use_bits else None
    r.badm = pack_bits(isbad[:, r.dirty.astype(np.int64)], 1)[:, 0] if r.has_bm else None
    r.rowid = r.delta = None
    if r.has_delta:
        row_of = np.nonzero(isbad.any(axis=1))[0]
        assert len(row_of) == r.n_rows
        r.rowid = np.full(A, 0xFF, np.uint8)
        r.rowid[row_of] = np.arange(r.n_rows, dtype=np.uint8)
        delta = np.zeros((r.n_rows, r.Ap), np.int64)
        idx = np.arange(A)
        for s in r.dirty.astype(np.int64):
            ps, hs, bs = r.P32[:, s].astype(np.int64), held[:, s], isbad[:, s]
            xs = np.nonzero(bs)[0]
            px = ps[xs][:, None]
            after = (idx[None, :] > xs[:, None]) & hs[None, :] & (px < ps[None, :])
            before = (idx[None, :] < xs[:, None]) & ~bs[None, :] & hs[None, :] & (ps[None, :] < px)
            delta[r.rowid[xs].astype(np.int64), :A] += after | before
        assert delta.max(initial=0) <= 255
        r.delta = delta.astype(np.uint8)
    return r


def plain_scores(P32):
    """score(a, b) of chain_probes for every pair: A x A, the upper triangle filled."""
    A = len(P32)
    held = P32 >= 0
    S = np.zeros((A, A), np.int64)
    for a in range(A - 1):
        S[a, a + 1 :] = (held[a] & held[a + 1 :] & (P32[a] < P32[a + 1 :])).sum(axis=1)
    return S


def rebuilt_scores(b):
    """What the chain kernel's scoring routes make of a block (the module docstring's rules): A x A, the upper triangle filled."""
    A = b.A
    P = np.asarray(b.P)
    S = np.zeros((A, A), np.int64)

    def ordered(cols, named=None):  # over the sequences `cols` (all columns: None): P[a] < P[b], P[b] present; `named`: A x len(cols), a | b must name the sequence
        Pc = P if cols is None else P[:, cols]
        for a in range(A - 1):
            m = (Pc[a] < Pc[a + 1 :]) & (Pc[a + 1 :] != AB_NONE16)
            if named is not None:
                m &= named[a] | named[a + 1 :]
            S[a, a + 1 :] += m.sum(axis=1)

    if not b.use_bits:
        ordered(None)
        return S
    bits = np.unpackbits(np.ascontiguousarray(b.pres).view(np.uint8).reshape(A, -1), axis=1, bitorder="little").astype(np.float32)
    S += np.triu(np.rint(bits @ bits.T).astype(np.int64), 1)  # (exact: at most 2048 ones a row)
    dirty = np.asarray(b.dirty).astype(np.int64)
    if b.has_delta:
        D = np.zeros((A, A), np.int64)
        has = np.asarray(b.rowid) != 0xFF
        D[has] = np.asarray(b.delta)[np.asarray(b.rowid)[has].astype(np.int64), :A]
        S += np.triu(D + D.T, 1)
    elif b.has_bm:
        named = ((np.asarray(b.badm)[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
        assert not named[:, len(dirty) :].any(), "a mask names a dirty sequence the list does not have"
        ordered(dirty, named[:, : len(dirty)])
    elif len(dirty):
        ordered(dirty)
    return S


def assert_score_identity(b, P32, what):
    want, got = plain_scores(P32), rebuilt_scores(b)
    wrong = np.argwhere(np.triu(want != got, 1))
    assert len(wrong) == 0, f"{what}: {len(wrong)} pair scores rebuilt from the block differ from the plain score, first ({wrong[0][0]}, {wrong[0][1]}): {got[tuple(wrong[0])]} against {want[tuple(wrong[0])]}"


def canonical(b):
    """The compared fields of a block (BlockRef or AnchorBlock) as a dict of arrays, the dirty list ascending and the masks' bits moved with it."""
    c = {"header": np.array([b.A, b.N, b.n_dirty, b.flags, b.n_rows], np.int64), "ckey": np.asarray(b.ckey), "P": np.asarray(b.P)}
    if b.use_bits:
        dirty = np.asarray(b.dirty)
        order = np.argsort(dirty, kind="stable")
        c["pres"], c["dirty"] = np.asarray(b.pres), dirty[order]
        if b.has_bm:
            nd = len(dirty)
            badm = np.asarray(b.badm)
            named = ((badm[:, None] >> np.arange(nd, dtype=np.uint64)[None, :]) & np.uint64(1))[:, order]
            low = (named << np.arange(nd, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64) if nd else np.zeros(b.A, np.uint64)
            beyond = badm >> np.uint64(nd) << np.uint64(nd) if nd < 64 else np.zeros(b.A, np.uint64)  # (bits no dirty sequence has: zero, kept so that one set shows)
            c["badm"] = low | beyond
        if b.has_delta:
            c["rowid"], c["delta"] = np.asarray(b.rowid), np.asarray(b.delta)
    return c


def assert_same_block(got, want, what):
    """Every compared field of `got` equals `want`'s, byte for byte; the first difference is named."""
    g, w = canonical(got), canonical(want)
    assert list(g["header"]) == list(w["header"]), f"{what}: header (A, N, n_dirty, flags, n_rows) {list(g['header'])} against {list(w['header'])}"
    assert sorted(g) == sorted(w), (what, sorted(g), sorted(w))
    for name in ("ckey", "P", "dirty", "pres", "badm", "rowid", "delta"):
        if name not in w:
            continue
        assert g[name].shape == w[name].shape and g[name].dtype == w[name].dtype, f"{what}: {name} is {g[name].dtype}{g[name].shape}, expected {w[name].dtype}{w[name].shape}"
        diff = np.argwhere(g[name] != w[name])
        assert len(diff) == 0, f"{what}: {name} differs in {len(diff)} places, first at {tuple(int(x) for x in diff[0])}: {g[name][tuple(diff[0])]} against {w[name][tuple(diff[0])]}"
