"""The overlap run without a GPU (include/consent_amd.h cw_overlap_*; Engine.overlap_index, overlap_rows, overlaps, overlaps_paf; pipeline.correct_from_reads):
the symbols, constants and the plan exist, the index's size is what the header says, a missing engine is refused before the device is touched, the PAF writer's
lines parse back to the rows -- and the reference the GPU tests compare with (tests/overlap_probes.py) is held to its definition by hand-computed cases, agrees
with the locate run's window where the two definitions meet, and the three measured defaults (min_hits, the shortest overlap found without exception, the
distance of an end from the truth) are measured here."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import consent_amd as ca
import locate_probes as lp
import overlap_probes as op
from consent_amd import engine as en
from consent_amd import pipeline
from consent_amd.engine import _ptr

E_INVALID = -1


def header():
    return open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "consent_amd.h")).read()


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_header_declares_the_functions_the_structs_and_the_constants():
    text = header()
    for decl in ("int cw_overlap_count_device(cw_engine* e, const cw_batch* reads, const cw_overlap_params* prm, uint64_t* n_entries, void* hip_stream);",
                 "uint64_t cw_overlap_index_words(uint64_t n_entries);",
                 "int cw_overlap_build_device(cw_engine* e, const cw_batch* reads, const cw_overlap_index* index, void* hip_stream);",
                 "int cw_overlap_run(cw_engine* e, const cw_batch* reads, const cw_overlap_params* prm, const cw_overlaps* out);",
                 "typedef struct cw_overlap_params { uint32_t k, sample, max_occ, min_hits; } cw_overlap_params;"):
        assert decl in text, decl
    assert re.search(r"int cw_overlap_run_device\(cw_engine\* e, const cw_overlap_index\* index, const cw_batch\* reads, uint32_t first_query, uint32_t n_queries,", text)
    assert re.search(r"int cw_overlap_to_pile_device\(cw_engine\* e, const cw_overlaps\* rows, uint32_t n_queries, uint32_t max_support, struct cw_overlap\* pile,", text)
    for name, value in (("K", 15), ("SAMPLE", 3), ("MAX_OCC", 512), ("MIN_HITS", op.MIN_HITS), ("END_SLACK", op.END_SLACK)):
        assert re.search(rf"#define CW_OVL_{name}\s+{value}u", text), name
    assert "enum { CW_OVL_TARGET, CW_OVL_STRAND, CW_OVL_HITS, CW_OVL_DIAG, CW_OVL_Q_START, CW_OVL_Q_END, CW_OVL_T_START, CW_OVL_T_END, CW_OVL_ROW = 8 };" in text
    assert "enum { CW_OVL_OK = 0, CW_OVL_NONE = 1, CW_OVL_SLOT = 2, CW_OVL_DENSE = 3, CW_OVL_BAD_INDEX = 4 };" in text
    assert "n_seqs < 2^24" in text and "n_entries < 2^32" in text  # the limits are stated


def test_the_library_exports_them_and_the_binding_names_them():
    l = ca.load_library()
    for name in ("cw_overlap_count_device", "cw_overlap_index_words", "cw_overlap_build_device", "cw_overlap_run_device", "cw_overlap_run",
                 "cw_overlap_to_pile_device", "cw_debug_overlap_plan", "cw_debug_overlap_routes"):
        assert hasattr(l, name), name
    assert (ca.OVL_K, ca.OVL_SAMPLE, ca.OVL_MAX_OCC) == (op.K_DEFAULT, op.SAMPLE_DEFAULT, op.MAX_OCC_DEFAULT) == (15, 3, 512)
    assert (ca.OVL_MIN_HITS, ca.OVL_MIN_K, ca.OVL_MIN_OVERLAP, ca.OVL_END_SLACK) == (op.MIN_HITS, op.MIN_K, op.MIN_OVERLAP, op.END_SLACK)
    assert [ca.OVL_TARGET, ca.OVL_STRAND, ca.OVL_HITS, ca.OVL_DIAG, ca.OVL_Q_START, ca.OVL_Q_END, ca.OVL_T_START, ca.OVL_T_END, ca.OVL_ROW] == list(range(9))
    assert [ca.OVL_OK, ca.OVL_NONE, ca.OVL_SLOT, ca.OVL_DENSE, ca.OVL_BAD_INDEX] == [op.OK, op.NONE, op.SLOT, op.DENSE, op.BAD_INDEX]
    assert C.sizeof(ca.OverlapParams) == 16 and C.sizeof(ca.OverlapIndexRef) == 32 and C.sizeof(ca.Overlaps) == 32
    for name in ("overlap_index", "overlap_rows", "overlap_device", "overlap_routes", "overlap_run_host", "overlaps", "overlaps_paf"):
        assert hasattr(ca.Engine, name), name
    assert inspect.signature(ca.Engine.overlaps).parameters["min_hits"].default is None
    assert inspect.signature(ca.Engine.overlap_index).parameters["sample"].default == 3
    assert "paf_path" in inspect.signature(pipeline.correct_from_reads).parameters


def test_a_missing_engine_is_refused_without_a_device():
    l = ca.load_library()
    hb = ca.pack_piles([["ACGTACGTACGTACGTACGT"]])
    b = hb.c_struct()
    mem, rows, n = np.full(4096, 77, np.uint32), np.full(8, 77, np.int32), C.c_uint64(77)
    off, cnt, status = np.array([0, 1], np.uint64), np.full(1, 77, np.uint32), np.full(1, 77, np.uint8)
    prm = en.OverlapParams(0, 3, 0, 2)
    ix = en.OverlapIndexRef(_ptr(mem), 0, prm)
    out = en.Overlaps(_ptr(rows), _ptr(off), _ptr(cnt), _ptr(status))
    assert l.cw_overlap_count_device(None, C.byref(b), C.byref(prm), C.byref(n), None) == E_INVALID
    assert l.cw_overlap_build_device(None, C.byref(b), C.byref(ix), None) == E_INVALID
    assert l.cw_overlap_run_device(None, C.byref(ix), C.byref(b), 0, 1, C.byref(out), None) == E_INVALID
    assert l.cw_overlap_run(None, C.byref(b), C.byref(prm), C.byref(out)) == E_INVALID
    assert l.cw_overlap_to_pile_device(None, C.byref(out), 1, 4, _ptr(mem), _ptr(off), _ptr(cnt), None) == E_INVALID
    assert l.cw_debug_overlap_routes(None, _ptr(mem)) == E_INVALID
    assert (mem == 77).all() and (rows == 77).all() and (cnt == 77).all() and (status == 77).all() and n.value == 77


def test_the_index_is_a_header_three_tables_of_a_power_of_two_and_the_postings():
    words = ca.load_library().cw_overlap_index_words
    slots = lambda n: (words(n) - 16 - 2 * n) // 3
    assert words(0) == 16 + 3 * 1024 and slots(512) == 1024 and slots(513) == 2048
    for n in (0, 1, 777, 48285, 1 << 20, (1 << 20) + 1, 17250000, (1 << 30), (1 << 32) - 1):
        s = slots(n)
        assert 16 + 3 * s + 2 * n == words(n) and s & (s - 1) == 0 and s >= 1024 and (s >= 2 * n or s == 1 << 31) and (s == 1024 or s < 4 * n), n
    assert words(1 << 32) == 0 and words(1 << 40) == 0
    assert words(5) % 2 == 0  # the postings are 64-bit words behind an even number of 32-bit ones


def test_the_overlap_plan_is_its_arithmetic():
    l = ca.load_library()
    out = np.zeros(6, np.uint64)
    assert l.cw_debug_overlap_plan(8, 256, None) == E_INVALID and l.cw_debug_overlap_plan(8, 0, _ptr(out)) == E_INVALID
    up = lambda v: (v + 255) // 256 * 256
    dense_words = 6 << 18  # a dense pair of tables: 2^18 slots of a 64-bit key, a count, a 32-bit key and a 64-bit value
    for queries, cus in ((0, 256), (1, 256), (15, 256), (16, 256), (17, 256), (767, 256), (768, 256), (769, 256), (5, 8), (1 << 22, 304)):
        assert l.cw_debug_overlap_plan(queries, cus, _ptr(out)) == 0
        wgs, dense = max(1, min(queries, 3 * cus)), max(1, min(queries, 16))  # 48 KB of LDS a work-group: three a CU; at most 16 dense tables
        parts = [up(8 * 4), up(4 * queries), up(4 * dense_words * dense) if queries else 0]
        assert out.tolist() == [sum(parts)] + parts + [wgs, dense], (queries, cus)


# ---- the reference, by hand --------------------------------------------------------------------------------------------------------------------------------------

def test_the_reference_is_its_definition_on_cases_computed_by_hand():
    assert op.code("ACGT") == 0b00011011 and op.code("AAAC") == 1
    # AAAAAAAC: K = 1, R = GTTTTTTT = 0b10 then seven 0b11 -> c = 1, strand 0; its reverse complement reads c = 1, strand 1
    assert op.occurrences("AAAAAAAC", 8, 0) == [(1, 0, 0)] and op.occurrences("GTTTTTTT", 8, 0) == [(1, 0, 1)]
    assert op.occurrences(op.PALINDROME8, 8, 0) == []  # K == R: skipped
    assert op.occurrences("AAAAAAAC", 8, 1) == []  # 0x9E3779B1 >> 31 == 1: not sampled
    # c = 2: 2 x 0x9E3779B1 mod 2^32 = 0x3C6EF362, whose top bits are 001: sampled at 1 and 2, not at 3
    assert op.occurrences("AAAAAAAG", 8, 1) == op.occurrences("AAAAAAAG", 8, 2) == [(2, 0, 0)] and op.occurrences("AAAAAAAG", 8, 3) == []
    # two reads that share one exact stretch of 20 bases, k = 15, every k-mer: six votes on one diagonal
    x = "ACGGTCATTGCAGCTTAGCA"
    a, b = "TTTTT" + x, x + "GGGGGGG"  # x at 5 in a (m = 25), at 0 in b (n = 27)
    ix = op.Index([a, b], 15, 0)
    assert ix.n_entries == (25 - 14) + (27 - 14)
    c = op.votes(ix, 0)
    assert c == {(1, 0, (0 - 5 + 25) >> 6): 6}  # p - i + m = 20 for each of the six: bin 0
    status, rows = op.rows_of(ix, 0, 0, 1)
    # DIAG = 0 - 25; c0 = clamp(-25 + 64, -(25 - 15), 27 - 15) = 12; a = 0, z = min(25, 15) = 15: T 12 .. 26, Q 0 .. 14
    assert status == op.OK and rows == [(1, op.FWD, 6, -25, 0, 14, 12, 26)]
    # the same target turned: the votes land at p + k + i, p the turned target's position
    ix = op.Index([a, op.revcomp(b)], 15, 0)
    c = op.votes(ix, 0)
    assert set(c) == {(1, 1, (7 + 15 + 10) >> 6)} and sum(c.values()) == 6  # x's last 15-mer: turned at 7 of revcomp(b), at 5 + 5 of a; every pair sums alike
    assert op.rows_of(ix, 0, 0, 1)[1][0][:4] == (1, op.REV, 6, -25)
    assert op.rows_of(ix, 0, 0, 7)[1] == [] and op.rows_of(op.Index(["ACGT", b], 15, 0), 0)[0] == op.NONE
    assert op.coordinates(-25, 1, 25, 27, 15) == (10, 24, 12, 26)  # REV: Q_START = m - z, Q_END = m - 1 - a
    assert op.coordinates(-100, 0, 40, 600, 15) == (25, 39, 0, 14)  # c0 clamped to -(m - k) = -25: a = 25, z = 40
    # a second copy of a read is a target, the read itself never; rows by hits, then target, then strand
    ix = op.Index([x, x, "CCC" + x, op.revcomp(x)], 15, 0)
    assert [(r[0], r[1], r[2]) for r in op.rows_of(ix, 0, 0, 1)[1]] == [(1, 0, 6), (2, 0, 6), (3, 1, 6)]
    assert op.expected([x, x, "CCC" + x], 15, 0, 0, 1, slots=[2, 1, 0]) == [(op.OK, 2, op.rows_of(op.Index([x, x, "CCC" + x], 15, 0), 0, 0, 1)[1]), (op.SLOT, 2, []), (op.SLOT, 2, [])]


def test_the_probes_are_the_edges_they_are_named_for():
    reads, xs, ys = op.occurrence_edges()
    got = op.expected(reads, 11, 0, 3, 1)
    for q in xs:  # planted three times: occ == max_occ votes
        assert sorted(r[0] for r in got[q][2]) == [t for t in xs if t != q] and all(r[2] == 1 for r in got[q][2])
    assert all(got[q][1] == 0 for q in ys)  # planted four times: max_occ + 1 does not
    assert [e[1] for e in op.expected(reads, 11, 0, 4, 1)][3:] == [3, 3, 3, 3]  # (with max_occ = 4 they do)
    for k in (8, 11, 15):
        fam, notes = op.family(k)
        ix = op.Index(fam, k, 0)
        ex = op.expected(None, min_hits=2, ix=ix)
        a, b = notes["twice"]
        full = 300 - k + 1  # each copy reports the other with every k-mer, and no read reports itself
        assert (b, op.FWD, full) in [r[:3] for r in ex[a][2]] and (a, op.FWD, full) in [r[:3] for r in ex[b][2]] and all(r[0] != q for q, e in enumerate(ex) for r in e[2])
        q, t = notes["both"]
        assert {(r[0], r[1]) for r in ex[q][2]} >= {(t, op.FWD), (t, op.REV)}
        q, ts = notes["ties"]
        tied = [r for r in ex[q][2] if r[0] in ts]
        assert len({r[2] for r in tied}) == 1 and [r[0] for r in tied] == sorted(ts) and {r[1] for r in tied} == {op.FWD, op.REV}
        assert [ex[s][:2] for s in notes["short"]] == [(op.NONE, 0)] * 3
        assert min(len(r) for r in fam[:18]) >= 24 and max(len(r) for r in fam) <= 600
        geo = op.geometry(k)
        eg = op.expected(geo, k, 0, 0, 2)
        for j, s in enumerate(op.PLANTED_SUMS, 1):  # an exact slice at d = s - 40: its votes in the one bin s >> 6
            row = eg[j][2][0]
            assert row[:3] == (0, op.FWD, 40 - k + 1) and row[3] <= s - 40 < row[3] + 128, (k, s, row)
        vs0 = lambda j: [r for r in eg[j][2] if r[0] == 0][0]  # (the probes meet each other too)
        assert vs0(6)[3] < 0 and vs0(6)[4] == 16 and vs0(6)[6] == 0  # over the start: negative DIAG, the query begins 16 bases before the target
        assert vs0(7)[1] == op.FWD and vs0(7)[5] == 79 and vs0(8)[1] == op.REV and vs0(9)[1] == op.REV and vs0(8)[2] == vs0(6)[2]
        assert vs0(10)[7] == 599 and vs0(11)[6] == 0 and vs0(12)[1] == op.REV  # 20 shared bases at the target's end and start
        tiny = eg[-3][2][0]  # 24 bases on 30: m + n - k < 64, so DIAG + 64 lies beyond n - k and c0 is clamped there
        assert tiny[:2] == (len(geo) - 4, op.FWD) and tiny[3] + 64 > 30 - k and tiny[6:] == (30 - k, 29) and tiny[4:6] == (0, k - 1)
        halves = eg[-1][2][0]
        w = op.votes(op.Index(geo, k, 0), len(geo) - 1)
        bins = sorted(b for (t, o, b), n in w.items() if t == len(geo) - 2 and o == 0 and n >= 60 - k)
        assert len(bins) == 2 and w[len(geo) - 2, 0, bins[0]] == w[len(geo) - 2, 0, bins[1]] and halves[3] == ((bins[0] - 1) << 6) - 120  # two bins tie: the lower one's lower window
    long_set = op.too_long()
    el = op.expected(long_set, 15, 0, 0, 2)
    assert el[1][:2] == (op.NONE, 0) and all(r[0] != 1 for e in el for r in e[2]) and el[0][1] >= 2  # too long: no query, no target; its slices still meet
    dense = op.dense_reads()
    ixd = op.Index(dense, 8, 0)
    assert op.LDS_CAP < op.distinct_keys(ixd, 0) <= op.DENSE_CAP and max(op.distinct_keys(ixd, q) for q in range(1, len(dense))) <= op.LDS_CAP


def test_the_best_row_is_the_locate_runs_window_where_the_two_definitions_meet():
    """One long read and short reads, every k-mer, a huge max_occ: a short read's votes against the long one are the locate run's hits wherever the long read's
    k-mers are unique and neither strand of a k-mer occurs elsewhere.  With a long read free of repeats, and short reads free of repeated k-mers, HITS and DIAG of
    the row against the long read are the locate row's."""
    import random

    import seed_probes as sd
    from poa_op_probes import rand_seq

    rng = random.Random(0x10CA7E0)
    k = 15
    ref = rand_seq(rng, 5000)
    shorts = [ref[a : a + m] for a, m in ((0, 200), (1234, 333), (4700, 300))] + [op.revcomp(ref[2000:2400]), op.ont_copy_map(rng, ref[3000:3600], 0.1)[0]]
    reads = [ref] + shorts
    ix = op.Index(reads, k, 0)
    assert all(len({t for t, _, _ in v}) == len(v) or len(v) == 1 for v in ix.post.values())  # no k-mer twice in one read, on either strand
    for q in range(1, len(reads)):
        row = [r for r in op.rows_of(ix, q, 1 << 16, 1)[1] if r[0] == 0][0]
        want = lp.locate_of(reads[q], ref, k)
        assert (row[1], row[2], row[3]) == (want[sd.STATUS], want[sd.HITS], want[sd.DIAG]), (q, row, want)


# ---- the measured defaults ---------------------------------------------------------------------------------------------------------------------------------------

def test_the_chance_level_the_shortest_overlap_found_and_the_distance_of_the_ends():
    """The measurements behind CW_OVL_MIN_HITS, OVL_MIN_OVERLAP and CW_OVL_END_SLACK, on the planted set op.SET: 120 reads of 1 500 to 5 000 bases, ONT-mix errors
    at 10 - 12 %, every second read turned, from a random genome of 30 000 bases; the plain reference at k = 15, sample = 3.
      unrelated pairs (true intervals 1 000 bases or more apart): the largest HITS is 1 -> min_hits = max(2, 2 x 1) = 2
      planted overlaps of at least L bases, all found with the right strand: L = 2 000 is the smallest multiple of 250 (at 1 750, 4 of 1 532 are missed; at 250,
      262 of 3 116); the smallest HITS among those of 2 000 or more is 2
      the largest distance of one of the four reported ends from the true overlap's end over those: 79 -> the bound 79 + 64 = 143"""
    genome, reads, where = op.planted(*op.SET)
    ix = op.planted_index(op.SET)
    rows = [op.rows_of(ix, q, 0, 1)[1] for q in range(len(reads))]
    chance = max(r[2] for q, rs in enumerate(rows) for r in rs if op.gap_and_overlap(where[q], where[r[0]])[0] >= 1000)
    min_hits = max(2, 2 * chance)
    print(f"the largest HITS of unrelated pairs: {chance}; min_hits {min_hits}")
    assert min_hits == op.MIN_HITS == ca.OVL_MIN_HITS and ca.OVL_MIN_K == op.K_DEFAULT == ca.OVL_K

    def survey(L):
        pairs = missed = worst = 0
        least = 1 << 30
        for q in range(len(reads)):
            got = {r[0]: r for r in rows[q] if r[2] >= min_hits and r[1] == (where[q][2] ^ where[r[0]][2])}
            for t in range(len(reads)):
                ov = op.gap_and_overlap(where[q], where[t])[1]
                if t == q or ov < L:
                    continue
                pairs += 1
                if t not in got:
                    missed += 1
                    continue
                r, g0 = got[t], max(where[q][0], where[t][0])
                tq, tt = op.true_ends(where[q], len(reads[q]), g0, g0 + ov), op.true_ends(where[t], len(reads[t]), g0, g0 + ov)
                least, worst = min(least, r[2]), max(worst, abs(r[4] - tq[0]), abs(r[5] - tq[1]), abs(r[6] - tt[0]), abs(r[7] - tt[1]))
        return pairs, missed, least, worst

    found = {L: survey(L) for L in range(250, op.MIN_OVERLAP + 1, 250)}
    for L, (pairs, missed, least, worst) in found.items():
        print(f"L = {L}: {pairs} planted overlaps, {missed} missed, smallest HITS {least}, an end at most {worst} from the truth")
    assert min(L for L, f in found.items() if f[1] == 0) == op.MIN_OVERLAP == ca.OVL_MIN_OVERLAP and found[op.MIN_OVERLAP][0] > 1000
    assert found[op.MIN_OVERLAP][2] >= op.MIN_HITS
    assert found[op.MIN_OVERLAP][3] + 64 == op.END_SLACK == ca.OVL_END_SLACK


# ---- the PAF writer ------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_paf_lines_parse_back_to_the_rows(tmp_path):
    genome, reads, where = op.planted(*op.SMALL)
    names = [f"read{i}" for i in range(len(reads))]
    per = [e[2] for e in op.expected(None, ix=op.planted_index(op.SMALL))]
    path = str(tmp_path / "ovl.paf")
    n = en.write_paf(path, names, [len(r) for r in reads], per)
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) - 1 == n == sum(len(p) for p in per) > 40 and lines[:-1] == op.paf_lines(reads, names, per)
    back = [[] for _ in reads]
    order = []
    for line in lines[:-1]:
        qn, ql, qs, qe, strand, tn, tl, ts, te, hits, block, mapq = line.split("\t")
        q, t = names.index(qn), names.index(tn)
        assert int(ql) == len(reads[q]) and int(tl) == len(reads[t]) and mapq == "255" and int(block) == max(int(qe) - int(qs), int(te) - int(ts))
        back[q].append((t, int(strand == "-"), int(hits), int(qs), int(qe) - 1, int(ts), int(te) - 1))
        order.append(q)
    assert order == sorted(order)  # a query's lines together
    assert back == [[r[:3] + r[4:] for r in p] for p in per]
