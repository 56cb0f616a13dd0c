"""Designed inputs for the read re-assembly (consent_amd/csrc/cw_stitch.h cw_stitch_kernel from its read loop to the end): one read per probe with its window
positions, consensus strings, solid sets, templates and window statuses written by hand -- no probe runs the consensus kernels -- and, by hand as well, the
route the probe was designed to take: the exact set of decisions (tests/stitch_ref.py WINDOW_BITS) of the windows it is about, the read's (READ_BITS), and
the numbers it was built to produce.  tests/test_stitch_ref_cpu.py holds these routes to the reference's and the reference to the oracle;
tests/test_gpu_stitch_routes.py holds the kernel to both.  Test infrastructure only.

The default geometry -- k = 9, windows of 100 with an overlap of 10, two to five windows, consensuses of 60-140 characters -- is the smallest at which every
branch still exists; a probe that needs another names it.  Unless a probe says otherwise its read is random lower case, its windows lie at (0, 99), (90, 189),
(180, 279), ... and a window's consensus is the upper-cased read under it: then window 0 takes {al_pos_clamped, replaced_same, gap_right_far}, every later one
{overlap, equal_ignoring_case, replaced_same, gap_right_far}, the last one last_window as well."""
import functools
import random

import numpy as np

K = 9


class Probe:
    def __init__(self, name, read, wins, expect, read_route=(), facts=None, k=K, ws=100, wo=10, do_trim=True, cap=None, trace=None):
        """wins: [(beg, end, consensus, solid codes, template or None, status)]; expect: {window: "bits"}; facts: {window: {name: number}};
        trace: {window: {index of the eight words: number}}"""
        self.name, self.k, self.ws, self.wo, self.do_trim, self.cap = name, k, ws, wo, do_trim, cap
        self.p = dict(read=read, pos=[(w[0], w[1]) for w in wins], cons=[w[2] for w in wins], solid=[sorted(w[3]) for w in wins], tpls=[w[4] for w in wins],
                      status=[w[5] for w in wins])
        self.expect = {w: set(bits.split()) for w, bits in expect.items()}
        self.read_route, self.facts, self.trace = set(read_route), facts or {}, trace or {}


def rand_lower(seed, n):
    rng = random.Random(seed)
    return "".join(rng.choice("acgt") for _ in range(n))


def sub(s, *at):
    """s with the letters at the given positions replaced by the next letter of ACGT (the case kept)."""
    s = list(s)
    for x in at:
        c = s[x]
        nxt = "ACGT"["ACGT".index(c.upper()) - 3]
        s[x] = nxt if c.isupper() else nxt.lower()
    return "".join(s)


def code(kmer):
    v = 0
    for c in kmer:
        v = (v << 2) | {"A": 0, "C": 1, "G": 2}.get(c, 3)
    return v


def kmers(s, k=K):
    return {code(s[p : p + k]) for p in range(len(s) - k + 1)}


def win(read, a, b, cons=None, solid=(), tpl="", status=0, pos=None):
    """A window over read[a:b]: its consensus (default: the read under it, upper case), solid set, template (default: the read under it) and status."""
    pos = pos or (a, b - 1)
    return (pos[0], pos[1], read[a:b].upper() if cons is None else cons, solid, read[a:b].upper() if tpl == "" else tpl, status)


W0 = "al_pos_clamped replaced_same gap_right_far"
WN = "overlap equal_ignoring_case replaced_same gap_right_far"
PLAIN = "replaced_same gap_right_far"


def _slice_probes():
    out = []
    R = rand_lower(1, 300)
    out.append(Probe("plain three windows", R, [win(R, 0, 100), win(R, 90, 190), win(R, 180, 280)], {0: W0, 1: WN, 2: WN + " last_window"}))
    out.append(Probe("cur_pos below the overlap", R, [win(R, 9, 109), win(R, 99, 199)], {0: W0, 1: WN + " last_window"}, {"trim_shift"}, trace={0: {0: 0}}))
    out.append(Probe("cur_pos at the overlap", R, [win(R, 10, 110), win(R, 100, 200)], {0: PLAIN, 1: WN + " last_window"}, {"trim_shift"}, trace={0: {0: 0}}))
    for n, bits in ((199, " slice_clipped"), (200, " slice_clipped"), (201, "")):  # window 1: al_pos 80, 80 + 120 against the read's length
        Rn = rand_lower(2, n)
        out.append(Probe(f"slice end against a read of {n}", Rn, [win(Rn, 0, 100), win(Rn, 90, min(190, n))], {0: W0, 1: WN + " last_window" + bits},
                         trace={1: {0: 80, 1: min(120, n - 80)}}))
    for first, name in ((310, "at"), (311, "beyond")):  # al_pos = first - 10 against a read of 300: no slice; the window after it sees what this one saw
        out.append(Probe(f"cur_pos {name} the read's end", R, [win(R, 0, 100), win(R, 90, 190, pos=(first, first + 99)), win(R, 180, 280, pos=(first + 90, first + 189))],
                         {0: W0, 1: "slice_clipped no_slice", 2: "slice_clipped no_slice"}))
    return out


def _string_probes():
    out = []
    R = rand_lower(3, 300)
    tpl = sub(R[90:190].upper(), 50)
    out.append(Probe("consensus of k - 1: the template is aligned, nothing is replaced, it becomes old", R,
                     [win(R, 0, 100), win(R, 90, 190, cons=R[90:98].upper(), tpl=tpl), win(R, 180, 280)],
                     {0: W0, 1: "template_aligned overlap guard_short_consensus", 2: WN + " last_window"}, facts={1: {"cl": 100}, 2: {"overlap": 10}}))
    out.append(Probe("consensus of k", R, [win(R, 0, 100), win(R, 90, 190, cons=R[91:100].upper()), win(R, 180, 280)],
                     {1: "overlap equal_ignoring_case replaced_same", 2: PLAIN + " last_window"}, facts={1: {"overlap": 9, "cl": 9, "gap_move": 0}}))
    out.append(Probe("no sequence and a short consensus", R, [win(R, 0, 100), win(R, 90, 190, cons="ACGT", tpl=None), win(R, 180, 280)],
                     {1: "template_absent", 2: PLAIN + " last_window"}))
    out.append(Probe("an overflow window with consensus bytes", R, [win(R, 0, 100), win(R, 90, 190, cons=sub(R[90:190].upper(), 30, 31, 32), status=2), win(R, 180, 280)],
                     {1: "overflow_skipped", 2: PLAIN + " last_window"}))
    out.append(Probe("a consensus of Ns", R, [win(R, 0, 100), win(R, 90, 190, cons="N" * 80), win(R, 180, 280)], {1: "no_alignment", 2: PLAIN + " last_window"},
                     trace={1: {2: 0, 7: 80}}))
    c = R[90:190].upper()
    c = c[:20] + c[20:30].lower() + c[30:40] + "N" + c[41:60] + "N" + c[61:]
    out.append(Probe("lower case and single Ns inside a consensus", R, [win(R, 0, 100), win(R, 90, 190, cons=c), win(R, 180, 280)], {1: WN, 2: WN + " last_window"}))
    out.append(Probe("an overlap equal but for case", R, [win(R, 0, 100), win(R, 90, 190, cons=R[90:100] + R[100:190].upper()), win(R, 180, 280)], {1: WN}))
    for n in (1, 63, 64, 65, 130):  # the junk cannot be extended into: its letter differs from the three read letters before the window
        junk = next(ch for ch in "ACGT" if ch.lower() not in R[87:90]) * n
        out.append(Probe(f"junk of {n} in front of the consensus", R, [win(R, 0, 100), win(R, 90, 190, cons=junk + R[90:190].upper()), win(R, 180, 280)],
                         {1: WN + " query_clipped"}, trace={1: {5: n, 6: n + 99, 7: n + 100}}))
    return out


def _reconcile_probes():
    out = []
    R = rand_lower(4, 300)
    out.append(Probe("old_end = beg - 1", R, [win(R, 0, 100), win(R, 100, 190)], {1: PLAIN + " last_window"}, facts={1: {"beg": 100}}))
    out.append(Probe("old_end = beg", R, [win(R, 0, 100), win(R, 99, 190)], {1: WN + " last_window"}, facts={1: {"beg": 99, "overlap": 1}}))
    # an overlap of k - 1: upper-case counts.  Window 0 ends with `lo0` lower-case letters, window 1 begins with `lo1`, and they differ at read position 95.
    for lo0, lo1, verdict in ((0, 1, "old_wins"), (1, 1, "tie"), (1, 0, "cur_wins")):
        c0 = R[0:100].upper()
        c0 = c0[:97] + c0[97 : 97 + lo0].lower() + c0[97 + lo0 :]
        c1 = sub(R[92:190].upper(), 3)
        c1 = c1[:5] + c1[5 : 5 + lo1].lower() + c1[5 + lo1 :]
        tail = " band_lanes dirs_lds spliced" if verdict == "old_wins" else ""
        out.append(Probe(f"overlap k - 1, upper-case counts: {verdict}", R, [win(R, 0, 100, cons=c0), win(R, 92, 190, cons=c1)],
                         {1: f"overlap by_upper {verdict} replaced_same gap_right_far last_window" + tail}, facts={1: {"overlap": 8, "s1": 8 - lo0, "s2": 8 - lo1}}))
    # an overlap of k: one k-mer each, looked up in the window's own solid set
    for in0, in1, verdict in ((1, 0, "old_wins"), (1, 1, "tie"), (0, 0, "tie"), (0, 1, "cur_wins")):
        c1 = sub(R[91:190].upper(), 4)
        s0, s1 = ({code(R[91:100].upper())} if in0 else set()), ({code(c1[:9])} if in1 else set())
        tail = " band_lanes dirs_lds spliced" if verdict == "old_wins" else ""
        out.append(Probe(f"overlap k, solid k-mers {in0} against {in1}: {verdict}", R, [win(R, 0, 100, solid=s0), win(R, 91, 190, cons=c1, solid=s1)],
                         {1: f"overlap by_solid {verdict} replaced_same gap_right_far last_window" + tail}, facts={1: {"overlap": 9, "s1": in0, "s2": in1}}))
    out.append(Probe("old_len = overlap - 1", R, [win(R, 80, 100, pos=(0, 99)), win(R, 79, 190, pos=(89, 188))],
                     {0: "al_pos_clamped replaced_same gap_right_far", 1: "overlap guard_old_shorter replaced_same gap_right_far last_window"}, {"trim_shift"}, facts={1: {"overlap": 21}}))
    out.append(Probe("old_len = overlap: reconciled, old wins", R, [win(R, 80, 100, pos=(0, 99), solid=kmers(R[80:100].upper())), win(R, 80, 190, cons=sub(R[80:190].upper(), 5), pos=(90, 189))],
                     {1: "overlap by_solid old_wins band_lanes dirs_lds spliced replaced_same gap_right_far last_window"}, {"trim_shift"}, facts={1: {"overlap": 20, "s1": 12, "s2": 0}}))
    out.append(Probe("cl = overlap - 1, the gap moved left by 1", R, [win(R, 0, 100), win(R, 85, 99, pos=(90, 189)), win(R, 180, 280)],
                     {1: "overlap guard_cur_shorter replaced_same gap_left", 2: "replaced_same gap_right_far last_window"}, facts={1: {"overlap": 15, "cl": 14, "gap_move": -1}}))
    out.append(Probe("the gap moved left by 75", R, [win(R, 0, 100), win(R, 10, 25, pos=(10, 109)), win(R, 180, 280, pos=(100, 199))],
                     {1: "overlap guard_cur_shorter replaced_same gap_left_far"}, facts={1: {"overlap": 90, "cl": 15, "gap_move": -75}}))
    return out


def _old_wins_probes():
    """The earlier window wins an overlap of 30 (all k-mers of its tail are solid, none of the later window's), and the sub-alignment decides the cut."""
    out = []
    R = rand_lower(5, 300)
    tail = R[70:100].upper()
    s0 = kmers(tail)
    base = "overlap by_solid old_wins band_lanes"
    rest = R[100:170].upper()  # (window 1 is sliced from 60 to 180)
    later = win(R, 180, 280)
    out.append(Probe("old wins, substitutions only", R, [win(R, 0, 100, solid=s0), win(R, 70, 170, cons=sub(tail, 10, 20) + rest, pos=(70, 169)), later],
                     {1: base + " dirs_lds spliced replaced_same gap_right_far"}, facts={1: {"overlap": 30, "ins": 0, "del": 0, "cut": 30, "cl": 100, "s2": 0}}))
    # the later window lacks a letter the earlier one has: an insertion of the query (seq1); the splice restores the length
    out.append(Probe("old wins, insertions only", R, [win(R, 0, 100, solid=s0), win(R, 70, 170, cons=tail[:15] + tail[16:] + rest, pos=(70, 169)), later],
                     {1: base + " dirs_lds indels spliced replaced_same gap_right_far"}, facts={1: {"ins": 1, "del": 0, "cut": 29, "cl": 100}}))
    extra = "ACGT"[("ACGT".index(tail[15]) + 2) % 4]
    out.append(Probe("old wins, deletions only", R, [win(R, 0, 100, solid=s0), win(R, 70, 170, cons=tail[:15] + extra + tail[15:] + rest, pos=(70, 169)), later],
                     {1: base + " dirs_lds indels spliced replaced_same gap_right_far"}, facts={1: {"ins": 0, "del": 1, "cut": 31, "cl": 100}}))
    out.append(Probe("old wins, insertions and deletions", R, [win(R, 0, 100, solid=s0), win(R, 70, 170, cons=tail[:8] + tail[9:22] + extra + tail[22:] + rest, pos=(70, 169)), later],
                     {1: base + " dirs_lds indels spliced replaced_same gap_right_far"}, facts={1: {"ins": 1, "del": 1, "cut": 30, "cl": 100}}))
    out.append(Probe("old wins, cut = cl - 1: one character spliced on, the gap moved right by 1", R, [win(R, 0, 100, solid=s0), win(R, 70, 101, cons=sub(tail, 10) + R[100].upper(), pos=(70, 169)), later],
                     {1: base + " dirs_lds spliced replaced_same gap_right", 2: PLAIN + " last_window"}, facts={1: {"cut": 30, "cl": 31, "gap_move": 1}}))
    # emptied: the window after it must see the old and the cur_pos of the window before (its overlap of k is looked up in window 0's solid set)
    after = win(R, 91, 170, cons=sub(R[91:170].upper(), 4), pos=(75, 174))
    s0k = s0 | {code(R[91:100].upper())}
    out.append(Probe("old wins, cut = cl: emptied", R, [win(R, 0, 100, solid=s0k), win(R, 70, 100, cons=sub(tail, 10), pos=(70, 169)), after],
                     {1: base + " dirs_lds emptied", 2: "overlap by_solid old_wins band_lanes dirs_lds spliced replaced_same gap_right_far last_window"},
                     facts={1: {"cut": 30, "cl": 0}, 2: {"overlap": 9, "s1": 1, "s2": 0, "beg": 91}}))
    out.append(Probe("old wins, cut > cl: emptied", R, [win(R, 0, 100, solid=s0k), win(R, 70, 99, cons=tail[:15] + extra + tail[15:29], pos=(70, 169)), after],
                     {1: base + " dirs_lds indels emptied", 2: "overlap by_solid old_wins band_lanes dirs_lds spliced replaced_same gap_right_far last_window"},
                     facts={1: {"overlap": 30, "ins": 0, "del": 1, "cut": 31, "cl": 0}, 2: {"overlap": 9, "s1": 1}}))
    # after a skipped window the solid set is that of the window that set old, not that of the window before
    out.append(Probe("a skipped window between old and cur: old's solid set", R, [win(R, 0, 100, solid={code(R[91:100].upper())}), win(R, 90, 190, status=2), win(R, 91, 190, cons=sub(R[91:190].upper(), 4), pos=(180, 279))],
                     {1: "overflow_skipped", 2: "overlap by_solid old_wins band_lanes dirs_lds spliced replaced_same gap_right_far last_window"}, facts={2: {"s1": 1, "s2": 0}}))
    # solid sets of five entries: the hit on the first and on the last
    c = code(R[91:100].upper())
    for name, s5 in (("first", {c, c + 1, c + 2, c + 3, c + 4}), ("last", {c - 4, c - 3, c - 2, c - 1, c})):
        out.append(Probe(f"a hit on the {name} entry of a solid set", R, [win(R, 0, 100, solid=s5), win(R, 91, 190, cons=sub(R[91:190].upper(), 4))],
                         {1: "overlap by_solid old_wins band_lanes dirs_lds spliced replaced_same gap_right_far last_window"}, facts={1: {"s1": 1, "s2": 0}}))
    # a k-mer with a lower-case letter: counted as T
    c0 = R[0:93].upper() + R[93] + R[94:100].upper()
    as_t = code(R[91:93].upper() + "T" + R[94:100].upper())
    for name, s1set, verdict, s1 in (("its T reading is solid", {as_t}, "old_wins", 1), ("its own letter is solid", {code(R[91:100].upper())} - {as_t}, "tie", 0)):
        tail_bits = " band_lanes dirs_lds spliced" if verdict == "old_wins" else ""
        out.append(Probe(f"a k-mer with a lower-case letter, {name}", R, [win(R, 0, 100, cons=c0, solid=s1set), win(R, 91, 190, cons=sub(R[91:190].upper(), 4))],
                         {1: f"overlap by_solid {verdict} replaced_same gap_right_far last_window" + tail_bits}, facts={1: {"s1": s1, "s2": 0}}))
    # overlaps of 65 and 129 that differ in their last character only
    out.append(Probe("an overlap of 65 that differs in its last character", R, [win(R, 0, 100, solid=kmers(R[35:100].upper())), win(R, 35, 135, cons=sub(R[35:135].upper(), 64), pos=(45, 144))],
                     {1: "overlap by_solid old_wins band_lanes dirs_lds spliced replaced_same gap_right last_window"}, facts={1: {"overlap": 65, "s1": 57, "s2": 0, "cut": 65, "gap_move": 35}}))
    R4 = rand_lower(8, 400)
    out.append(Probe("an overlap of 129 that differs in its last character", R4, [win(R4, 0, 200, solid=kmers(R4[71:200].upper())), win(R4, 71, 271, cons=sub(R4[71:271].upper(), 128), pos=(81, 280))],
                     {1: "overlap by_solid old_wins band_lanes dirs_lds spliced replaced_same gap_right_far last_window"}, facts={1: {"overlap": 129, "s1": 121, "cut": 129}}, ws=200))
    # a sub-alignment without score at an overlap below k: window 0 is on its template, which carries eight letters the read lacks, so old_end lies eight
    # beyond where the template's alignment ends; its tail ACACACAC shares no letter with the lower-case head gtgtgtgt of window 1
    Rz = rand_lower(9, 84) + "acacacac" + "gtgtgtgt" + rand_lower(10, 100)
    ins8 = next(ch for ch in "ACGT" if ch.lower() not in Rz[58:62]) * 8
    out.append(Probe("a sub-alignment without score", Rz, [win(Rz, 0, 92, cons="ACGT", tpl=Rz[0:60].upper() + ins8 + Rz[60:92].upper(), pos=(0, 99)), win(Rz, 92, 190, cons=Rz[92:100] + Rz[100:190].upper(), pos=(90, 189))],
                     {0: "template_aligned al_pos_clamped", 1: "slice_clipped overlap by_upper old_wins sub_no_score spliced replaced_same gap_right_far last_window"},
                     {"trim_shift"}, facts={0: {"end": 91, "cl": 100}, 1: {"beg": 92, "overlap": 8, "s1": 8, "s2": 0, "sub_score": 0, "cut": 8}}))
    return out


def _gap_probes():
    out = []
    R = rand_lower(11, 300)
    for n, bit in ((64, "gap_right"), (65, "gap_right_far")):
        out.append(Probe(f"the gap moved right by {n}", R, [win(R, 0, 100), win(R, 90, 100 + n, pos=(90, 189))], {1: f"overlap equal_ignoring_case replaced_same {bit} last_window"},
                         facts={1: {"gap_move": n}}))
    out.append(Probe("the gap moved right by 200", R, [win(R, 0, 100), win(R, 200, 300)], {1: "slice_clipped replaced_same gap_right_far last_window"}, facts={1: {"gap_move": 200}}))
    out.append(Probe("a replace that shortens the read", R, [win(R, 0, 100, cons=R[0:50].upper() + R[51:100].upper()), win(R, 90, 190, pos=(90, 189))],
                     {0: "al_pos_clamped replaced_shorter gap_right_far", 1: WN + " last_window"}, facts={1: {"beg": 89}}))
    R2 = rand_lower(12, 280)
    out.append(Probe("a replace at the read's last character", R2, [win(R2, 0, 100), win(R2, 90, 190), win(R2, 180, 280)], {2: WN + " slice_clipped last_window"}, facts={2: {"end": 279}}))
    return out


def _band_probes():
    """Planted offsets as in sw_op_probes.planted, sized for a slice of at most 2048: the earlier window's tail is P + M + G2 + S, the later one's head P + G1 + M + S
    (flanks of `flank`, unrelated G1, G2 of g): equal spans, so the band starts at 1 and doubles until it holds the offset g."""
    out = []
    for name, flank, g, ws, wo, bits, bands in (("a band that stays on the lanes and doubles three times", 20, 5, 200, 10, "band_lanes dirs_global", [1, 2, 4, 8]),
                                                ("a band of 64: the serial loop", 50, 40, 400, 10, "band_serial dirs_global", [1, 2, 4, 8, 16, 32, 64]),
                                                ("rows beyond 4096 bytes", 150, 130, 700, 50, "band_serial rows_global dirs_global", [1, 2, 4, 8, 16, 32, 64, 128, 256])):
        n = 3 * flank + g
        R = rand_lower(13 + g, ws + 150 + n)
        a = ws - n  # the tail of window 0
        P, M, G2, S = R[a : a + flank], R[a + flank : a + 2 * flank], R[a + 2 * flank : a + 2 * flank + g], R[a + 2 * flank + g : ws]
        G1 = rand_lower(99 + g, g)
        head = (P + G1 + M + S).upper()
        out.append(Probe(name, R, [win(R, 0, ws, solid=kmers(R[a:ws].upper())), win(R, a, ws + 100, cons=head + R[ws : ws + 100].upper(), pos=(a + wo, a + wo + ws - 1))],
                         {1: "overlap by_solid old_wins indels spliced band_doubled replaced_same gap_right_far last_window " + bits},
                         facts={1: {"overlap": n, "ins": g, "del": g, "cut": n, "bands": bands}}, ws=ws, wo=wo))
    return out


def _launch_probes():
    out = []
    for n in (1022, 1023, 1024, 1500):  # the order kernel's last class: 1023 windows and more
        R = rand_lower(20 + n, 18 * n + 2)
        out.append(Probe(f"a read of {n} windows of 20 bases", R, [win(R, 18 * i, 18 * i + 20) for i in range(n)],
                         {0: "al_pos_clamped replaced_same gap_right", 1: "overlap equal_ignoring_case replaced_same gap_right", n - 1: "overlap equal_ignoring_case slice_clipped replaced_same gap_right last_window"},
                         ws=20, wo=2))
    # the last launch: a 2049-character consensus sends its read there; an overlap of more than 640 (the sub-alignment sweeps with its state in memory), one of fewer
    R = rand_lower(30, 3000)
    junk = "N" * 1049  # (N scores 0 against everything: the alignment ends where the read's copy ends)
    big = "overlap by_solid old_wins band_lanes dirs_lds spliced replaced_same gap_right_far"
    out.append(Probe("the last launch: overlaps of 700 and of 400", R, [win(R, 0, 1000, cons=junk[:500] + R[0:1000].upper() + junk[500:], solid=kmers(R[300:1000].upper())),
                                                                       win(R, 300, 1300, cons=sub(R[300:1300].upper(), 100, 300, 600), solid=kmers(R[900:1300].upper()), pos=(310, 1309)),
                                                                       win(R, 900, 1900, cons=sub(R[900:1900].upper(), 50, 150), pos=(910, 1909))],
                     {0: "al_pos_clamped query_clipped replaced_same gap_right_far", 1: big + " sub_mem_sweep", 2: big + " last_window"}, {"last_launch"},
                     facts={1: {"overlap": 700}, 2: {"overlap": 400}}, trace={0: {7: 2049, 5: 500}}, ws=1000, wo=50))
    # the wide kernel's hand-over: a consensus of 2048 aligned whole, spliced with an insertion more than deletions -- 2049 characters
    R = rand_lower(32, 4200)
    extra = "ACGT"["ACGT".index(R[2448].upper()) - 2]
    cur = R[900:1400].upper() + R[1401:2048].upper() + R[2048:2448].upper() + extra + R[2448:2948].upper()
    out.append(Probe("the hand-over: a splice that outgrows 2048 characters", R, [win(R, 0, 2048, solid=kmers(R[900:2048].upper())), win(R, 900, 2948, cons=cur, pos=(1000, 2847))],
                     {0: "al_pos_clamped replaced_same gap_right_far", 1: "overlap by_solid old_wins indels spliced band_lanes dirs_lds sub_mem_sweep replaced_longer gap_right_far last_window"},
                     {"handed_over", "last_launch"}, facts={1: {"overlap": 1148, "ins": 1, "del": 0, "cut": 1147, "cl": 2049}}, trace={1: {7: 2048, 5: 0, 6: 2047}}, ws=1848, wo=100))
    return out


def _trim_probes():
    """Reads of one letter with planted words: a consensus of Ns around a word aligns exactly where the word is."""
    out = []

    def planted(n, plants):
        r = ["t"] * n
        for at, word in plants:
            r[at : at + len(word)] = word.lower()
        return "".join(r)

    def around(word, at):
        return ("NN" + word + "NNNNNNN"[: max(2, K - 2 - len(word))], (max(0, at - 5), max(0, at - 5) + 99))

    def probe(name, n, plants, read_route, string=None, **kw):
        R = planted(n, plants)
        wins = []
        for at, word in plants:
            cons, pos = around(word, at)
            wins.append((pos[0], pos[1], cons, (), None, 0))
        p = Probe(name, R, wins, {}, read_route, **kw)
        p.string = string
        return p

    for trim in (True, False):
        t = "" if trim else ", not trimmed"
        out.append(probe("one upper-case character" + t, 200, [(50, "G")], {"one_upper"} if trim else (), "" if trim else None, do_trim=trim))
        out.append(probe("two adjacent upper-case characters" + t, 200, [(50, "GC")], {"trim_shift"} if trim else (), "GC" if trim else None, do_trim=trim))
        out.append(probe("10 upper-case characters of 100" + t, 300, [(20, "GCAGC"), (115, "CGACG")], {"trim_shift"} if trim else (), do_trim=trim))
        out.append(probe("9 upper-case characters of 91" + t, 300, [(20, "GCAGC"), (107, "CGAC")], {"trim_shift", "dropped"} if trim else (), "" if trim else None, do_trim=trim))
        for at in (0, 1, 64, 65):
            out.append(probe(f"the first upper-case character at {at}" + t, 200, [(at, "GCAGCAGGA")], ({"trim_shift"} if at else ()) if trim else (), "GCAGCAGGA" if trim else None, do_trim=trim))
    R = rand_lower(6, 250)
    for trim in (True, False):
        out.append(Probe("a read without a window" + ("" if trim else ", not trimmed"), R, [], {}, {"no_window", "no_upper"} if trim else {"no_window"}, do_trim=trim))
        out.append(Probe("no upper-case character: its only window does not align" + ("" if trim else ", not trimmed"), R, [win(R, 0, 100, cons="N" * 60)], {0: "al_pos_clamped no_alignment"},
                         {"no_upper"} if trim else (), do_trim=trim))
    return out


def _slot_probes():
    R = rand_lower(7, 260)
    longer = R[0:50].upper() + "A" + R[50:100].upper()  # the replace lengthens the read by one
    wins = [win(R, 0, 100, cons=longer), win(R, 90, 190)]
    return [Probe("a slot one byte smaller than the read", R, wins, {}, {"slot_too_small"}, cap=259, do_trim=False),
            Probe("a slot the growth of a replace outgrows by one", R, wins, {0: "al_pos_clamped"}, {"outgrown"}, cap=260, do_trim=False),
            Probe("a slot that holds the grown read exactly", R, wins, {0: "al_pos_clamped replaced_longer gap_right_far", 1: WN + " last_window"}, (), cap=261, do_trim=False)]


# Arms of the kernel no probe takes, and why.  (The wide kernel's nl > CW_ST_QMAX hand-over is NOT among them: "the hand-over" above reaches it.)
UNREACHABLE = {
    "size_al beyond CW_ST_RMAX": "a slice is at most window_size + 2 * window_overlap long, and cw_stitch_device refuses a geometry where that exceeds CW_ST_RMAX (CW_E_INVALID)",
    "overlap beyond CW_ST_RMAX in the last launch": "old ends at most window_size + 2 * window_overlap behind the next slice's start while window starts do not descend: cur_pos advances by the same "
    "cl - (end - beg + 1) that carries old_end beyond the replaced stretch.  tests/test_stitch_ref_cpu.py searches 300 random reads with consensuses of up to ten windows' "
    "length at small geometries: the largest overlap met is window_size + 2 * window_overlap exactly, never more",
}

# The subtly wrong kernels of tests/stitch_ref.py MUTANTS and the probe that catches each: its final string or status changes.
MUTANT_CAUGHT_BY = {
    "s1_ge_s2": "overlap k, solid k-mers 1 against 1: tie",
    "cut_le_cl": "old wins, cut = cl: emptied",
    "solid_above_k": "overlap k, solid k-mers 1 against 0: old_wins",
    "old_len_gt": "old_len = overlap: reconciled, old wins",
    "solid_of_previous": "a skipped window between old and cur: old's solid set",
    "trim_end_ge_beg": "one upper-case character",
    "old_from_emptied": "old wins, cut > cl: emptied",
}
# Two switches change nothing, on any input: they are recorded, not caught.
EQUIVALENT_MUTANTS = {
    "slice_gt": "where al_pos + window_size + 2 * window_overlap equals the read's length, the clipped size (length - al_pos) IS window_size + 2 * window_overlap: "
    "'>' and '>=' give the same slice (the three 'slice end against a read of ...' probes stand on the edge and pin the slice's two trace words)",
    "drop_in_float": "the share is a float; no float lies in [0.1, 0.1f), so r < 0.1 and r < 0.1f agree for every float r, and a share computed in double differs from the "
    "float one only for reads of more than 2^24 bases (the '10 of 100' and '9 of 91' probes stand on the edge)",
}


@functools.lru_cache(maxsize=None)
def catalogue():
    out = _slice_probes() + _string_probes() + _reconcile_probes() + _old_wins_probes() + _gap_probes() + _band_probes() + _trim_probes() + _slot_probes() + _launch_probes()
    assert len({p.name for p in out}) == len(out)
    return out


def results_of(probes):
    """The probes as one launch: (reads HostBatch-like piles, jobs, positions, template piles, results object) for Engine.stitch."""
    import consent_amd as ca

    class Res:
        pass

    jobs, pos, piles, cons, solid, status = [], [], [], [], [], []
    for ri, pr in enumerate(probes):
        p = pr.p
        jobs.append((ri, len(pos), len(p["cons"])))
        pos += p["pos"]
        piles += [[t] if t is not None else [] for t in p["tpls"]]
        cons += p["cons"]
        solid += p["solid"]
        status += p["status"]
    r = Res()
    r.cons = np.frombuffer(("".join(cons) + "\0").encode("latin-1"), np.uint8).copy()
    r.cons_len = np.array([len(c) for c in cons] + [0], np.uint32)
    r.cons_off = np.concatenate([[0], np.cumsum(r.cons_len[:-1])]).astype(np.uint64)
    r.status = np.array(status + [0], np.uint8)
    r.solid = np.array([x for s in solid for x in s] + [0], np.uint32)
    r.solid_len = np.array([len(s) for s in solid] + [0], np.uint32)
    r.solid_off = np.concatenate([[0], np.cumsum(r.solid_len[:-1])]).astype(np.uint64)
    return ca.pack_piles([[pr.p["read"].upper() for pr in probes]]), np.array(jobs, np.uint32).reshape(-1, 3), np.array(pos, np.uint32).reshape(-1, 2), ca.pack_piles(piles), r
