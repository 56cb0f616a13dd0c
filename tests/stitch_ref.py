"""The read re-assembly once more, in plain Python / numpy (consent_amd/csrc/cw_stitch.h cw_stitch_kernel from its read loop to the end: alignConsensus,
trimRead(., 1), dropRead), restated from the prose of include/cw_policy.h (CW_SSW_*: match, mismatch, gap open / extend; the first reference column
that reaches the best score, the smallest query position in it) and the line citations of cw_stitch.h -- with what the kernel decides on the way:
eight trace words per window it aligned, the numbers of the reconciliation of two overlapping windows, and a route (a set of names, one per decision)
per window and per read.  No GPU, no oracle in here: tests/test_stitch_ref_cpu.py holds this file to the oracle, tests/test_gpu_stitch_routes.py holds
the kernel to this file.  A switch per decision (MUTANTS) makes the subtly wrong kernels the probes have to catch.  Test infrastructure only."""
import os
import re

import numpy as np

from sw_op_probes import GAP_EXT, GAP_OPEN, MATCH, MISMATCH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIN_OVERFLOW, READ_DROPPED, READ_CAPACITY = 2, 1, 2  # include/consent_amd.h


def header_constants():
    """The kernel's thresholds out of cw_stitch.h: nothing of them is restated here."""
    hdr = open(os.path.join(ROOT, "consent_amd", "csrc", "cw_stitch.h")).read()

    def num(pattern):
        return int(re.search(pattern, hdr).group(1))

    c = {name: num(rf"#define CW_ST_{name} (\d+)") for name in ("QMAX", "RMAX", "ROWS_BYTES")}
    c["DIR_BYTES"] = 1 << num(r"#define CW_ST_DIR_BYTES \(1u << (\d+)\)")
    c["HUGE_QMAX"] = num(r"#define CW_STH_QMAX (\d+)")
    c["LANES"] = num(r"rows_in_lds && width_d <= (\d+)")  # a band's row on the lanes of a wave
    c["MOVE"] = num(r"base < n; base \+= (\d+)\) \{ /\* lowest first")  # characters a gap move or a shift takes at a time
    c["MEM_SWEEP"] = num(r"if \(m > (\d+)\) return st_sweep_mem")  # the last launch: its register sweeps end here
    c["ORDER_CLAMP"] = num(r"min\(a\.jobs\[i\]\.win_count, (\d+)u\)")  # the order kernel's last class
    assert c["LANES"] == c["MOVE"]
    return c


ST = header_constants()

WINDOW_BITS = (
    "overflow_skipped", "template_aligned", "template_absent", "al_pos_clamped", "slice_clipped", "no_slice", "no_alignment", "query_clipped",
    "overlap", "guard_short_consensus", "guard_old_shorter", "guard_cur_shorter", "equal_ignoring_case", "by_solid", "by_upper",
    "old_wins", "tie", "cur_wins", "sub_no_score", "indels", "spliced", "emptied", "replaced_longer", "replaced_shorter", "replaced_same",
    "gap_right", "gap_left", "gap_right_far", "gap_left_far", "last_window",
    "band_lanes", "band_serial", "rows_global", "dirs_lds", "dirs_global", "band_doubled", "sub_mem_sweep",
)
READ_BITS = ("slot_too_small", "no_window", "outgrown", "last_launch", "no_upper", "one_upper", "trim_shift", "dropped", "handed_over")
MUTANTS = ("s1_ge_s2", "cut_le_cl", "solid_above_k", "slice_gt", "old_len_gt", "solid_of_previous", "drop_in_float", "trim_end_ge_beg", "old_from_emptied")

_CODE = np.full(256, 4, np.int64)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


def codes(s):
    return _CODE[np.frombuffer(s.encode("latin-1"), np.uint8)]


def sweep(q, r, cols, terminate=-1):
    """One local-alignment sweep of the query codes q over the reference columns `cols`, a numpy row per column, the in-column gap as a running maximum
    (exact because open >= ext and no cell is negative): (score, first column reaching it, smallest query position holding it there).  A letter other
    than ACGT scores 0 against everything."""
    m = len(q)
    H, E, t = np.zeros(m, np.int64), np.zeros(m, np.int64), np.arange(m)
    q_ok = q < 4
    best = (0, -1, 0)
    for i in cols:
        rc = r[i]
        s = np.where(q == rc, MATCH, -MISMATCH) * q_ok if rc < 4 else np.zeros(m, np.int64)
        E = np.maximum(np.maximum(E - GAP_EXT, H - GAP_OPEN), 0)
        diag = np.concatenate([[0], H[:-1]])
        hq = np.maximum(np.maximum(diag + s, E), 0)
        inc = np.maximum.accumulate(hq - GAP_OPEN + t * GAP_EXT)
        F = np.concatenate([[0], inc[:-1] - t[:-1] * GAP_EXT])
        H = np.maximum(hq, F)
        cm = int(H.max())
        if cm > best[0]:
            best = (cm, int(i), int(np.argmax(H)))
            if cm == terminate:
                break
    return best


def align(query, ref):
    """(score, ref_begin, ref_end, query_begin, query_end) of the strings: forward sweep, then a reverse sweep over the reversed prefix."""
    q, r = codes(query), codes(ref)
    if len(q) == 0 or len(r) == 0:
        return (0, 0, -1, 0, -1)
    score, col, row = sweep(q, r, range(len(r)))
    if score <= 0:
        return (0, 0, -1, 0, -1)
    _, bcol, brow = sweep(q[: row + 1][::-1], r, range(col, -1, -1), score)
    return (score, bcol, col, row - brow, row)


def banded_indels(ref, read, score, dir_bytes=None, lds_dir_bytes=None):
    """ssw's banded pass over code arrays (its rows h_b / e_b / h_c with their index rules and zeroed edge cells, as sw_op_probes.banded_best walks them,
    plus the three direction bytes of a cell), the band doubled until it reaches `score`, then the walk back from the last cell: (ins, del, bits, bands) --
    or None where a band's directions (and its rows, once they outgrow CW_ST_ROWS_BYTES) do not fit the wave's scratch."""
    dir_bytes = ST["DIR_BYTES"] if dir_bytes is None else dir_bytes
    lds_dir_bytes = ST["QMAX"] if lds_dir_bytes is None else lds_dir_bytes
    ref_len, read_len = len(ref), len(read)
    bits, bands = set(), []
    if ref_len <= 0 or read_len <= 0:
        return 0, 0, bits, bands
    band = abs(ref_len - read_len) + 1
    while True:
        bands.append(band)
        width, width_d = 2 * band + 3, 2 * band + 1
        rows_need, dir_need = 12 * min(width, ref_len + 3), 3 * min(width_d, ref_len + 1) * read_len
        rows_in_lds = rows_need <= ST["ROWS_BYTES"]
        if dir_need + (0 if rows_in_lds else (rows_need + 15) // 16 * 16) > dir_bytes:
            return None
        last = {"band_lanes" if rows_in_lds and width_d <= ST["LANES"] else "band_serial", "dirs_lds" if rows_in_lds and dir_need <= lds_dir_bytes else "dirs_global"}
        if not rows_in_lds:
            last.add("rows_global")
        h_b, e_b = np.zeros(width, np.int64), np.zeros(width, np.int64)
        dirs, best = [], 0
        for i in range(read_len):
            beg, end = max(0, i - band), min(ref_len - 1, i + band)
            if end < beg:
                dirs.append((beg, None))
                continue
            edge = min(end + 1, width - 1)
            h_b[0] = e_b[0] = h_b[edge] = e_b[edge] = 0
            xp = max(i - 1 - band, 0)
            t = np.arange(end - beg + 1)
            e_i = beg + t - xp + 1
            if i == 0:
                t1, t2 = np.full(len(t), -GAP_OPEN, np.int64), np.full(len(t), -GAP_EXT, np.int64)
            else:
                t1, t2 = h_b[e_i] - GAP_OPEN, e_b[e_i] - GAP_EXT
            e_new, dir_e = np.maximum(t1, t2), np.where(t1 > t2, 3, 2)
            e1 = np.maximum(e_new, 0)
            a, b = ref[beg : end + 1], read[i]
            diag = h_b[e_i - 1] + (np.where(a == b, MATCH, -MISMATCH) * (a < 4) if b < 4 else 0)
            hq = np.maximum(e1, diag)
            inc = np.maximum.accumulate(hq - GAP_OPEN + (t + 1) * GAP_EXT)
            ex = np.concatenate([[-(1 << 40)], inc[:-1]])
            f = np.maximum(ex, -GAP_EXT) - t * GAP_EXT
            f1 = np.maximum(f, 0)
            t1h = np.maximum(e1, f1)
            hc = np.maximum(t1h, diag)
            hc_prev, f_prev = np.concatenate([[0], hc[:-1]]), np.concatenate([[0], f[:-1]])
            dir_f = np.where(hc_prev - GAP_OPEN > f_prev - GAP_EXT, 5, 4)
            dir_h = np.where(t1h <= diag, 1, np.where(e1 > f1, dir_e, dir_f))
            e_b[1 : len(t) + 1] = e_new
            h_b[1 : len(t) + 1] = hc
            dirs.append((beg, (dir_e, dir_f, dir_h)))
            best = max(best, int(hc.max()))
        if best >= score or band > ref_len + read_len:
            break
        band *= 2
    bits |= last
    if len(bands) > 1:
        bits.add("band_doubled")
    ins = dele = 0
    i, j, state = read_len - 1, ref_len - 1, 2
    while i > 0 and j >= 0:
        x0, line = dirs[i]
        x = j - x0
        if x < 0 or x >= width_d or line is None or x >= len(line[0]):
            break
        d = int(line[state][x])
        if d == 1:
            i, j, state = i - 1, j - 1, 2
        elif d in (2, 3):
            i, state, ins = i - 1, 0 if d == 2 else 2, ins + 1
        elif d in (4, 5):
            j, state, dele = j - 1, 1 if d == 4 else 2, dele + 1
        else:
            break
    return ins, dele, bits, bands


def nb_solid(s, solid, k):
    """k-mers of s in the sorted set `solid`, under "anything but A, C, G is T"."""
    have = set(int(x) for x in solid)
    n = 0
    for p in range(len(s) - k + 1):
        v = 0
        for c in s[p : p + k]:
            v = (v << 2) | {"A": 0, "C": 1, "G": 2}.get(c, 3)
        n += v in have
    return n


def nb_upper(s):
    return sum("A" <= c <= "Z" for c in s)


class Window:
    """What the kernel decides for one window: .trace (the eight words, None where no alignment was tried), .facts (the reconciliation), .route."""

    def __init__(self):
        self.trace, self.facts, self.route = None, {}, set()


class Read:
    pass


def _pass(p, k, ws, wo, cap, huge, mut):
    """One kernel's pass over the read: (string or None, status, windows, read bits, alignments, "redo" when the wide kernel hands the read on)."""
    qmax = ST["HUGE_QMAX"] if huge else ST["QMAX"]
    read, pos, cons, tpls, solid, wstat = p["read"], p["pos"], p["cons"], p["tpls"], p["solid"], p["status"]
    n = len(cons)
    wins, bits, aligns = [Window() for _ in range(n)], set(), []
    if cap < len(read):
        bits.add("slot_too_small")
        return None, READ_CAPACITY, wins, bits, aligns, False
    if n == 0:
        bits.add("no_window")
    out = read.lower()
    gap = 0  # the gap buffer's left part: the kernel's GapBuf.L
    cur_pos = int(pos[0][0]) if n else 0
    old, old_end, old_w, have_old = "", 0, 0, False
    too_big = (None, READ_CAPACITY, wins, bits, aligns, not huge)  # the wide kernel hands on what the last launch reports as a capacity
    for w in range(n):
        W = wins[w]
        R = W.route
        if wstat[w] == WIN_OVERFLOW:
            R.add("overflow_skipped")
            continue
        long_enough = len(cons[w]) >= k
        cur = cons[w]
        if not long_enough:
            cur = tpls[w] if tpls[w] is not None else ""
            R.add("template_aligned" if tpls[w] is not None else "template_absent")
        if len(cur) > qmax:
            return too_big
        if cur_pos - wo < 0:
            R.add("al_pos_clamped")
        al_pos = max(0, cur_pos - wo)
        tot = len(out)
        clipped = al_pos + ws + 2 * wo > tot if "slice_gt" in mut else al_pos + ws + 2 * wo >= tot
        size_al = tot - al_pos if clipped else ws + 2 * wo
        if clipped:
            R.add("slice_clipped")
        if size_al <= 0:
            R.add("no_slice")
        if size_al <= 0 or len(cur) == 0:
            continue
        assert size_al <= ST["RMAX"]  # (the entry point refuses such a geometry)
        ref = out[al_pos : al_pos + size_al]
        al = align(cur, ref)
        aligns.append((cur, ref, al))
        W.trace = (al_pos, size_al) + al + (len(cur),)
        if al[0] <= 0:
            R.add("no_alignment")
            continue
        score, rb, re_, qb, qe = al
        beg, end = rb + al_pos, re_ + al_pos
        if qb > 0:
            R.add("query_clipped")
        cur = cur[qb : qe + 1]
        F = W.facts
        F.update(beg=beg, end=end)
        emptied = False
        if w != 0 and have_old and old_end >= beg:
            overlap = old_end - beg + 1
            R.add("overlap")
            F["overlap"] = overlap
            old_ok = len(old) > overlap if "old_len_gt" in mut else len(old) >= overlap
            if not long_enough:
                R.add("guard_short_consensus")
            if not old_ok:
                R.add("guard_old_shorter")
            if len(cur) < overlap:
                R.add("guard_cur_shorter")
            if long_enough and old_ok and len(cur) >= overlap:
                seq1, seq2 = old[len(old) - overlap :], cur[:overlap]
                if seq1.upper() == seq2.upper():
                    R.add("equal_ignoring_case")
                else:
                    if overlap > k if "solid_above_k" in mut else overlap >= k:
                        R.add("by_solid")
                        s1 = nb_solid(seq1, solid[w - 1 if "solid_of_previous" in mut else old_w], k)
                        s2 = nb_solid(seq2, solid[w], k)
                    else:
                        R.add("by_upper")
                        s1, s2 = nb_upper(seq1), nb_upper(seq2)
                    F.update(s1=s1, s2=s2)
                    R.add("old_wins" if s1 > s2 else "tie" if s1 == s2 else "cur_wins")
                    if s1 >= s2 if "s1_ge_s2" in mut else s1 > s2:
                        if overlap > ST["RMAX"]:  # (the last launch only)
                            return None, READ_CAPACITY, wins, bits, aligns, False
                        sub = align(seq1, seq2)
                        if huge and overlap > ST["MEM_SWEEP"]:
                            R.add("sub_mem_sweep")
                        ins = dele = 0
                        if sub[0] > 0:
                            band = banded_indels(codes(seq2)[sub[1] : sub[2] + 1], codes(seq1)[sub[3] : sub[4] + 1], sub[0], lds_dir_bytes=qmax)
                            if band is None:
                                return None, READ_CAPACITY, wins, bits, aligns, False
                            ins, dele, bbits, F["bands"] = band
                            R |= bbits
                        else:
                            R.add("sub_no_score")
                        aligns.append((seq1, seq2, sub + (ins, dele)))
                        if ins or dele:
                            R.add("indels")
                        cut = overlap - ins + dele
                        F.update(sub_score=sub[0], ins=ins, **{"del": dele}, cut=cut)
                        if cut <= len(cur) if "cut_le_cl" in mut else cut < len(cur):
                            if overlap + len(cur) - cut > qmax:
                                bits.add("handed_over")
                                return too_big
                            cur = seq1 + cur[cut:]
                            R.add("spliced")
                        else:
                            emptied = True
                            R.add("emptied")
        F["cl"] = 0 if emptied else len(cur)
        if (not emptied and len(cur) > 0) or (emptied and "old_from_emptied" in mut):
            if long_enough and not emptied:
                rl = end - beg + 1
                if len(out) - rl + len(cur) > cap:
                    bits.add("outgrown")
                    return None, READ_CAPACITY, wins, bits, aligns, False
                move = beg + rl - gap
                if move > 0:
                    R.add("gap_right_far" if move > ST["MOVE"] else "gap_right")
                elif move < 0:
                    R.add("gap_left_far" if -move > ST["MOVE"] else "gap_left")
                F["gap_move"] = move
                out = out[:beg] + cur.upper() + out[end + 1 :]
                gap = beg + len(cur)
                R.add("replaced_longer" if len(cur) > rl else "replaced_shorter" if len(cur) < rl else "replaced_same")
            if w + 1 < n:
                cur_pos = (cur_pos + int(pos[w + 1][0]) - int(pos[w][0]) - (end - beg + 1) + len(cur)) & 0xFFFFFFFF
                if cur_pos >= 1 << 31:
                    cur_pos -= 1 << 32
                old, old_w, have_old, old_end = cur, w, True, beg + len(cur) - 1
                F["cur_pos"] = cur_pos
            else:
                R.add("last_window")
    return out, 0, wins, bits, aligns, False


def stitch(p, k=9, window_size=100, window_overlap=10, do_trim=True, cap=None, mut=()):
    """The re-assembly of one read.  p: a dict with read, pos [(beg, end)], cons [str], tpls [str or None: the window has no sequence], solid [sorted
    k-mer codes], status [window status]; cap: the out slot's capacity (None: as Engine.stitch sizes it).  Returns a Read: .string, .status, .windows
    [Window], .route (the read's bits), .aligns [(query, reference, numbers)] of every alignment made."""
    mut = frozenset(mut)
    assert mut <= set(MUTANTS)
    cap = 2 * len(p["read"]) + 1024 if cap is None else cap
    out, status, wins, bits, aligns, redo = _pass(p, k, window_size, window_overlap, cap, False, mut)
    if redo:  # a consensus beyond CW_ST_QMAX: the last launch does the read again, from its start
        out, status, wins, b2, aligns, _ = _pass(p, k, window_size, window_overlap, cap, True, mut)
        bits = bits | b2 | {"last_launch"}
    r = Read()
    r.windows, r.aligns = wins, aligns
    if status == 0 and do_trim:
        ups = [x for x, c in enumerate(out) if "A" <= c <= "Z"]
        if not ups:
            bits.add("no_upper")
            out = ""
        elif not (ups[-1] >= ups[0] if "trim_end_ge_beg" in mut else ups[-1] > ups[0]):
            bits.add("one_upper")
            out = ""
        else:
            if len(ups) == 1:
                bits.add("one_upper")
            if ups[0] > 0:
                bits.add("trim_shift")
            out = out[ups[0] : ups[-1] + 1]
            ratio = np.float32(len(ups)) / np.float32(len(out))  # dropRead: the share in float, compared with the double 0.1
            if (ratio < np.float32(0.1)) if "drop_in_float" in mut else (float(ratio) < 0.1):
                bits.add("dropped")
                out, status = "", READ_DROPPED
    r.string, r.status, r.route = (out if status == 0 else ""), status, bits
    return r
