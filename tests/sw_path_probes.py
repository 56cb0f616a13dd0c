"""The reference of the path run's tests (cw_sw_path_run, consent_amd/csrc/cw_sw_path.h): ssw's banded pass with its direction codes and the walk back
(oracle/cw_oracle.cpp ssw_banded_indels), restated in numpy a row at a time -- sw_op_probes.banded_best is its fill half -- plus the run-length encoding, the
scratch rule of include/consent_amd.h and the expected row, op count and ops of a pair.  The oracle has no path output; tests/test_sw_path_cpu.py pins this
restatement to it (indel totals, spans, re-scored ops) for every probe the GPU tests use.  Test infrastructure only."""
import functools
import random

import numpy as np

import sw_op_probes as sp
from poa_op_probes import ont_copy, rand_seq

ALIGNED, STOP, IS_REF, NO_PATH, PATH_OPEN, PATH_SLOT = 0, 2, 3, 4, 5, 6  # include/consent_amd.h CW_SW_*
EQX = 4  # CW_SW_PATH_EQX
OP_M, OP_I, OP_D, OP_EQ, OP_X = 0, 1, 2, 7, 8
PATH_BYTES = 2 << 20  # CW_SW_PATH_BYTES
ROWS_LDS = 4096  # csrc/cw_stitch.h CW_ST_ROWS_BYTES
GO, GE = sp.GAP_OPEN, sp.GAP_EXT
CODE = {c: k for k, c in enumerate("ACGT")}


def path_fits(ref_span, query_span, band):
    """The scratch rule as include/consent_amd.h states it: a direction byte a cell, and the three rows once they outgrow 4096 bytes."""
    dirs = min(2 * band + 1, ref_span + 1) * query_span
    rows = 12 * min(2 * band + 3, ref_span + 3)
    return dirs + (0 if rows <= ROWS_LDS else (rows + 15) // 16 * 16) <= PATH_BYTES


def banded_dirs(ref, read, band):
    """One band of ssw_banded_indels over code arrays: (best score, de, df, dh) -- the oracle's three direction codes of every cell, [row, x] with
    x = j - max(i - band, 0) as its set_d has it, 0 where the band has no cell."""
    ref_len, read_len = len(ref), len(read)
    width, width_d = 2 * band + 3, 2 * band + 1
    h_b, e_b = np.zeros(width, np.int64), np.zeros(width, np.int64)
    de, df, dh = (np.zeros((read_len, min(width_d, ref_len + 1)), np.uint8) for _ in range(3))
    best = 0
    for i in range(read_len):
        beg, end = max(0, i - band), min(ref_len - 1, i + band)
        if end < beg:
            continue
        edge = min(end + 1, width - 1)
        h_b[0] = e_b[0] = h_b[edge] = e_b[edge] = 0
        xp = max(i - 1 - band, 0)
        t = np.arange(end - beg + 1)
        e_i = beg + t - xp + 1
        if i == 0:
            t1, t2 = np.full(len(t), -GO, np.int64), np.full(len(t), -GE, np.int64)
        else:
            t1, t2 = h_b[e_i] - GO, e_b[e_i] - GE
        e_new = np.maximum(t1, t2)
        code_e = np.where(t1 > t2, 3, 2)
        e1 = np.maximum(e_new, 0)
        diag = h_b[e_i - 1] + np.where(ref[beg : end + 1] == read[i], sp.MATCH, -sp.MISMATCH)
        hq = np.maximum(e1, diag)
        inc = np.maximum.accumulate(hq - GO + (t + 1) * GE)
        ex = np.concatenate([[-(1 << 40)], inc[:-1]])
        f = np.maximum(ex, -GE) - t * GE
        f1 = np.maximum(f, 0)
        t1h = np.maximum(e1, f1)
        hc = np.maximum(t1h, diag)
        hc_prev, f_prev = np.concatenate([[0], hc[:-1]]), np.concatenate([[0], f[:-1]])
        code_f = np.where(hc_prev - GO > f_prev - GE, 5, 4)
        n = len(t)
        de[i, :n], df[i, :n] = code_e, code_f
        dh[i, :n] = np.where(t1h <= diag, 1, np.where(e1 > f1, code_e, code_f))
        e_b[1 : n + 1] = e_new
        h_b[1 : n + 1] = hc
        best = max(best, int(hc.max()))
    return best, de, df, dh


def banded_dirs_serial(ref, read, band):
    """banded_dirs as the oracle writes it (oracle/cw_oracle.cpp ssw_banded_indels, the loop over the cells of a row): plain Python, small inputs only.  It
    pins banded_dirs' prefix-maximum form of the in-row gap, and with it the direction a tie takes, cell by cell (tests/test_sw_path_cpu.py)."""
    ref_len, read_len = len(ref), len(read)
    width, width_d = 2 * band + 3, 2 * band + 1
    h_b, e_b, h_c = [0] * width, [0] * width, [0] * width
    de, df, dh = (np.zeros((read_len, min(width_d, ref_len + 1)), np.uint8) for _ in range(3))
    best = 0

    def set_u(i, j):
        return j - max(i - band, 0) + 1

    for i in range(read_len):
        beg, end = max(0, i - band), min(ref_len - 1, i + band)
        edge = min(end + 1, width - 1)
        f = u = 0
        h_b[0] = e_b[0] = h_b[edge] = e_b[edge] = h_c[0] = 0
        for j in range(beg, end + 1):
            u, e, b, d = set_u(i, j), set_u(i - 1, j), set_u(i, j - 1), set_u(i - 1, j - 1)
            x = j - max(i - band, 0)
            t1 = -GO if i == 0 else h_b[e] - GO
            t2 = -GE if i == 0 else e_b[e] - GE
            e_b[u] = max(t1, t2)
            de[i, x] = 3 if t1 > t2 else 2
            t1, t2 = h_c[b] - GO, f - GE
            f = max(t1, t2)
            df[i, x] = 5 if t1 > t2 else 4
            e1, f1 = max(e_b[u], 0), max(f, 0)
            t1 = max(e1, f1)
            t2 = h_b[d] + (sp.MATCH if ref[j] == read[i] else -sp.MISMATCH)
            h_c[u] = max(t1, t2)
            best = max(best, h_c[u])
            dh[i, x] = 1 if t1 <= t2 else (de[i, x] if e1 > f1 else df[i, x])
        for j in range(1, u + 1):
            h_b[j] = h_c[j]
    return best, de, df, dh


def walk(de, df, dh, ref_len, read_len, band):
    """The oracle's walk from the end cell in state H.  Returns (closed, ins, del, steps): steps from the end to the begin (0 M, 1 I, 2 D); closed: the walk
    reached query row 0 at reference column 0, whose cell is then one more M (as ssw closes a path)."""
    i, j, state = read_len - 1, ref_len - 1, 2
    ins = dele = 0
    steps = []
    tabs = (de, df, dh)
    width_d = 2 * band + 1
    while i > 0 and j >= 0:
        x = j - max(i - band, 0)
        if x < 0 or x >= width_d:
            return False, ins, dele, steps
        c = int(tabs[state][i, x])
        if c == 1:
            i, j, state = i - 1, j - 1, 2
            steps.append(0)
        elif c in (2, 3):
            i, state = i - 1, 0 if c == 2 else 2
            ins += 1
            steps.append(1)
        elif c in (4, 5):
            j, state = j - 1, 1 if c == 4 else 2
            dele += 1
            steps.append(2)
        else:
            return False, ins, dele, steps
    if i == 0 and j == 0:
        steps.append(0)
        return True, ins, dele, steps
    return False, ins, dele, steps


def encode(steps_fwd, ref, read, eqx):
    """Run-length encode steps given in alignment order; under eqx an M step is '=' or 'X' by its bases."""
    ops, i, j = [], 0, 0
    for s in steps_fwd:
        c = s
        if s == 0 and eqx:
            c = OP_EQ if read[i] == ref[j] else OP_X
        if ops and ops[-1][1] == c:
            ops[-1][0] += 1
        else:
            ops.append([1, c])
        i += s != 2
        j += s != 1
    return [(n, c) for n, c in ops]


@functools.lru_cache(maxsize=None)
def reference(query, ref):
    """(status, ins, del, ops, ops under EQX, bands tried) of a pair by the restated pass: status ALIGNED, NO_PATH or PATH_OPEN (slots are the caller's)."""
    score, rb, re, qb, qe, _, _ = sp.oracle(query, ref)
    if score <= 0:
        return ALIGNED, 0, 0, (), (), ()
    r = np.array([CODE[c] for c in ref[rb : re + 1]], np.int64)
    q = np.array([CODE[c] for c in query[qb : qe + 1]], np.int64)
    band = abs(len(r) - len(q)) + 1
    bands = []
    while True:
        bands.append(band)
        if not path_fits(len(r), len(q), band):
            return NO_PATH, 0, 0, (), (), tuple(bands)
        best, de, df, dh = banded_dirs(r, q, band)
        if best >= score or band > len(r) + len(q):
            break
        band *= 2
    closed, ins, dele, steps = walk(de, df, dh, len(r), len(q), band)
    if not closed:
        return PATH_OPEN, ins, dele, (), (), tuple(bands)
    fwd = steps[::-1]
    return ALIGNED, ins, dele, tuple(encode(fwd, r, q, False)), tuple(encode(fwd, r, q, True)), tuple(bands)


def expected(query, ref, eqx=False, slot=None):
    """(row of 8, n_ops, ops) the path run owes the pair whose slot holds `slot` ops (None: enough)."""
    status, ins, dele, ops, ops_x, _ = reference(query, ref)
    five = sp.oracle(query, ref)[:5]
    ops = ops_x if eqx else ops
    if status == ALIGNED and slot is not None and len(ops) > slot:
        return five + (ins, dele, PATH_SLOT), len(ops), ()
    return five + (ins, dele, status), len(ops), ops


def rescore(ops, ref, read):
    """The score of a path over the aligned spans (match 2, mismatch 2, gap 3 + 1 per further base) and the bases it consumes: (score, query, reference)."""
    i = j = total = 0
    for n, c in ops:
        if c in (OP_M, OP_EQ, OP_X):
            total += sum(sp.MATCH if read[i + k] == ref[j + k] else -sp.MISMATCH for k in range(n))
            i, j = i + n, j + n
        else:
            total -= GO + (n - 1) * GE
            if c == OP_I:
                i += n
            else:
                j += n
    return total, i, j


def merge_eqx(ops):
    """'=' and 'X' runs back to M runs."""
    out = []
    for n, c in ops:
        c = OP_M if c in (OP_EQ, OP_X) else c
        if out and out[-1][1] == c:
            out[-1] = (out[-1][0] + n, c)
        else:
            out.append((n, c))
    return out


# ---- the probes --------------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def one_deletion(d, seed=0xDE1):
    """A query of two 150-base flanks, the reference with d unrelated bases between them and 30 random ones on either side: the spans differ by d, the band
    starts at d + 1 -- 2 (d + 1) + 1 cells a row: 63, 65, 67 for d = 30, 31, 32, the edge of a chunk of 64."""
    rng = random.Random(seed + d)
    P, S, D = rand_seq(rng, 150), rand_seq(rng, 150), rand_seq(rng, d)
    return P + S, rand_seq(rng, 30) + P + D + S + rand_seq(rng, 30)


@functools.lru_cache(maxsize=None)
def planted_small(n=30, g=40, seed=0x5A11):
    """A 60-base reference of two n-base halves and a query with g unrelated bases planted between them: the band starts at g + 1, wider than the matrix, so a
    row's stride is clipped to the reference span + 1."""
    rng = random.Random(seed)
    P, S, G = rand_seq(rng, n), rand_seq(rng, n), rand_seq(rng, g)
    return P + G + S, P + S


@functools.lru_cache(maxsize=None)
def planted_wide(part=1500, g=600, seed=0x1DE1):
    """planted() with 1 500-base parts and g = 600: bands up to 128 fit and do not reach the score, band 256 needs 513 x 5 100 bytes: NO_PATH."""
    rng = random.Random(seed + g + part)
    P, M, S, G1, G2 = (rand_seq(rng, k) for k in (part, part, part, g, g))
    return P + M + G2 + S, P + G1 + M + S


def band_pairs():
    out = {f"deletion of {d}": one_deletion(d) for d in (30, 31, 32)}
    out.update({"planted(10)": sp.planted(10), "planted(40)": sp.planted(40), "planted(300)": sp.planted(300), "band wider than the matrix": planted_small(),
                "unbalanced": sp.unbalanced()})
    return out


def class_pairs():
    out = {f"q{m}xr600": sp.embedded(1, m, 600) for m in (1, 2, 128, 129, 640, 641, 2048)}
    out["q200xr2049"], out["q700xr2049"] = sp.embedded(2, 200, 2049), sp.embedded(3, 700, 2049)
    return out


def long_pairs():
    out = dict(sp.long_pairs())
    out["q2100xr3000"] = sp.embedded(8, 2100, 3000)
    return out


def noisy_pairs(n=12, seed=0x9015):
    """Noisy copies of 60 to 600 bases at 12 % errors against their source between flanks."""
    rng = random.Random(seed)
    out = {}
    for k in range(n):
        m = rng.randrange(60, 601)
        src = rand_seq(rng, m)
        out[f"noisy {k} ({m})"] = (ont_copy(rng, src, 0.12), rand_seq(rng, 20) + src + rand_seq(rng, 20))
    return out


def all_probes():
    """Every (query, reference) the GPU tests compare with the reference, but the crowds and the mixed pairs (tests/test_sw_path_cpu.py samples those)."""
    out = {}
    for d in (band_pairs(), class_pairs(), long_pairs(), sp.tie_pairs(), sp.nothing_pairs(), noisy_pairs(), {"planted wide": planted_wide()}):
        out.update(d)
    return out


PATH_MAX_WAVES = 512  # csrc/cw_sw_path.h CW_SW_PATH_MAX_WAVES


def waves_of(n_seqs, cls, cus):
    """Waves of the path launch of query class `cls`: csrc/cw_plan.h plan_sw_path."""
    if cls == 2:
        return min(n_seqs, 256)
    most = min(cus * 4 if cls == 0 else cus, PATH_MAX_WAVES // 4)
    return 4 * max(1, min((n_seqs + 3) // 4, most))


CROWDS = sp.CROWDS  # more pairs than the path launches have waves too (tests/test_sw_path_cpu.py counts)
# of a crowd's thousands of pairs every pair is compared by its row (the oracle's seven numbers) and its path's invariants (spans, run-length form, re-scored
# ops); the restated pass costs milliseconds a pair, so every n-th pair of class 0 / 1 / 2 is compared op by op -- which wave takes which pair second is up to
# the run, so a sample meets reused buffers as surely as the whole would
CROWD_SAMPLE = {0: 13, 1: 5, 2: 3}
