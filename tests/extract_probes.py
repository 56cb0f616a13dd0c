"""The designed probes of the pile extraction (csrc/cw_extract.h) for the plain reference of tests/extract_ref.py: each a small read set, overlaps and
window jobs with the notes of every overlap written down by hand (tests/test_extract_ref_cpu.py holds them to the reference's).  Test infrastructure only.

Unless a probe says otherwise: a template of 200 bases, the window [50, 99], a target of 150 bases, k = 9, and the probe once on each strand.

  overlap rows  [q_start, q_end, t_read, t_start, t_end, strand]   (cw_overlap, ends inclusive)
  job rows      [tpl_read, q_beg, q_end, ovl_first, ovl_count]     (cw_window_job)
"""
import functools
import random

import extract_ref as xr

K = 9
TPL, TGT, WIN = 200, 150, (50, 99)


def rand_seq(seed, n):
    rng = random.Random(seed)
    return "".join(rng.choice("ACGT") for _ in range(n))


class Probe:
    def __init__(self, name, reads, ovl, jobs, notes=None, k=K, kind="geometry", reference_throws=False):
        self.name, self.reads, self.ovl, self.jobs, self.k, self.kind = name, list(reads), [list(o) for o in ovl], [list(j) for j in jobs], k, kind
        self.notes = notes or {}  # job -> [set of notes per overlap], by hand; a job left out is not written down
        self.reference_throws = reference_throws

    def job_inputs(self, j):
        """Job j as the oracle and the reference take it: (oracle rows, template, targets, q_beg, q_end)."""
        tpl_read, q_beg, q_end, first, count = self.jobs[j]
        tpl = self.reads[tpl_read]
        mine = self.ovl[first : first + count]
        rows = [[len(tpl), o[0], o[1], o[5], len(self.reads[o[2]]), o[3], o[4], i] for i, o in enumerate(mine)]
        return rows, tpl, [self.reads[o[2]] for o in mine], q_beg, q_end

    def reference(self):
        """[(pile, notes)] of every job by tests/extract_ref.py."""
        return [xr.window_pile(*self.job_inputs(j), self.k) for j in range(len(self.jobs))]


def merged(name, probes):
    """The probes (of one k) as the jobs of one call over one shared read set."""
    assert len({p.k for p in probes}) == 1
    reads, ovl, jobs = [], [], []
    for p in probes:
        r0, o0 = len(reads), len(ovl)
        reads += p.reads
        ovl += [[o[0], o[1], o[2] + r0, o[3], o[4], o[5]] for o in p.ovl]
        jobs += [[j[0] + r0, j[1], j[2], j[3] + o0, j[4]] for j in p.jobs]
    return Probe(name, reads, ovl, jobs, None, probes[0].k, "merged", any(p.reference_throws for p in probes))


def geo(name, ov, notes, t_len=TGT, tpl_len=TPL, win=WIN, k=K, strands=(0, 1), throws=False):
    """One overlap ov = (q_start, q_end, t_start, t_end) of one template over one window, once per strand."""
    out = []
    for s in strands:
        reads = [rand_seq(name + "/template", tpl_len), rand_seq(name + "/target", t_len)]
        out.append(Probe(f"{name} ({'+-'[s]})", reads, [[ov[0], ov[1], 1, ov[2], ov[3], s]], [[0, win[0], win[1], 0, 1]], {0: [set(notes)]}, k, "geometry", throws))
    return out


def geometry():
    c = []
    # ---- the span test's edges (:117) ----
    c += geo("overlap ends on the window's first base", (10, 50, 20, 60), {"no_span"})
    c += geo("overlap ends one base into the window", (10, 51, 20, 61), {"right"})                # T[60:110]
    c += geo("overlap begins on the window's last base", (99, 150, 60, 111), {"no_span"})
    c += geo("overlap begins one base before the window's end", (98, 150, 60, 112), {"left"})    # t_beg = 60 - 48: T[12:62]
    c += geo("gate met exactly", (10, 150, 20, 60), {"inside"}, k=1)                              # shift 40: the one base T[60]
    c += geo("gate missed by one", (10, 150, 21, 60), {"t_gate"}, k=1)
    c += geo("overlap strictly inside the window", (60, 90, 20, 50), {"no_span"})                 # the dead arm's condition: no member
    # ---- inside: the window within the overlap ----
    for s in (0, 1, 15, 16, 17):
        c += geo(f"inside: shift {s}", (50 - s, 150, 3, 103 + s), {"inside"})                     # T[3 + s : 53 + s]
    for o in (0, 1, 15):
        c += geo(f"inside: first source base at word offset {o}", (50, 150, 16 + o, 116 + o), {"inside"})
    for n in (K - 1, K, 15, 16, 17, 31, 32, 33):
        c += geo(f"inside: a piece of {n} bases", (45, 150, 7, 7 + 5 + n - 1), {"inside"} | ({"short"} if n < K else set()))  # the slice ends n bases after the shift
    for n in (1024, 1025, 1040):
        c += geo(f"inside: a window of {n} bases", (0, 1099, 0, 1099), {"inside"}, t_len=1100, tpl_len=1100, win=(30, 30 + n - 1))
    # ---- left: the overlap begins inside the window (q_start - q_beg = 20) ----
    c += geo("left: target begin clamped at 0", (70, 150, 19, 99), {"left", "clamp0"})           # 19 - 20 = -1
    c += geo("left: target begin exactly 0", (70, 150, 20, 100), {"left"})
    c += geo("left: length cut by the read's end", (70, 150, 125, 149), {"left", "clamp_end"})   # t_beg 105: 105 + 49 = 154 > 149, 45 bases
    c += geo("left: length reaches the read's end", (70, 150, 120, 149), {"left"})               # t_beg 100: 100 + 49 = 149
    # ---- right: the overlap ends inside the window (end - q_end = 19) ----
    c += geo("right: target end clamped at the read's last base", (10, 80, 61, 131), {"right", "clamp_end"})  # 131 + 19 = 150; T[101:150], 49 bases
    c += geo("right: target end exactly the read's last base", (10, 80, 60, 130), {"right"})                   # 130 + 19 = 149; T[100:150]
    c += geo("right: piece begins below 0", (45, 80, 0, 20), {"right", "clamp0"})               # t_end 39: 39 - 50 + 1 = -10; length 40, T[5:40]
    c += geo("right: piece begins exactly at 0", (45, 80, 0, 30), {"right"})                     # t_end 49: 49 - 50 + 1 = 0;   length 50, T[5:50]
    # ---- the '-' strand's ends ----
    c += geo("'-': last output base is source base 0", (40, 150, 0, 59), {"inside"}, strands=(1,))          # revcomp(T[0:60])[10:60]
    c += geo("'-': first output base is the read's last base", (50, 150, 49, 149), {"inside"}, strands=(1,))
    c += geo("'-': a piece with a shift", (33, 150, 10, 127), {"inside"}, strands=(1,))                       # revcomp(T[10:128])[17:67]
    # ---- overlaps beyond the read ----
    c += geo("t_end one beyond the read", (40, 150, 40, 150), {"inside", "substr_clamp"})
    c += geo("t_end 100 beyond the read", (40, 150, 40, 250), {"inside", "substr_clamp"})
    c += geo("the slice begins on the read's end", (50, 150, 150, 260), {"inside", "substr_clamp", "short"})   # substr at pos == size: empty, no throw
    c += geo("t_start beyond the read: the reference throws", (40, 150, 151, 260), {"inside", "throw_tbeg"}, strands=(0,), throws=True)
    c += geo("shift beyond the cut slice: the reference throws", (40, 150, 145, 250), {"inside", "substr_clamp", "throw_shift"}, strands=(1,), throws=True)
    # ---- the template ----
    c += geo("window ends on the template's last base", (100, 199, 0, 99), {"inside"}, win=(150, 199))
    for p in geo("window ends one beyond the template", (100, 199, 0, 99), (), win=(151, 200)):
        p.notes = {0: []}  # an empty pile: no overlap is looked at
        c.append(p)
    for s in (0, 1):
        reads = [rand_seq("between/template", TPL), rand_seq("between/target", 200)]
        c.append(Probe(f"an empty pile between two full ones ({'+-'[s]})", reads, [[10, 190, 1, 5, 185, s]], [[0, 50, 99, 0, 1], [0, 151, 200, 0, 1], [0, 100, 149, 0, 1]],
                       {0: [{"inside"}], 1: [], 2: [{"inside"}]}))
        reads = [rand_seq("k1/template", TPL), rand_seq("k1/target", TGT)]
        c.append(Probe(f"k = 1: pieces of 1 and 0 bases ({'+-'[s]})", reads, [[10, 150, 1, 20, 60, s], [40, 150, 1, 140, 160, s]], [[0, 50, 99, 0, 2]],
                       {0: [{"inside"}, {"inside", "substr_clamp", "short"}]}, k=1))  # the second: T[140:150] is ten bases, the shift is ten
        reads = [rand_seq("k16/template", TPL), rand_seq("k16/target", TGT)]
        c.append(Probe(f"k = 16: pieces of 15 and 16 bases ({'+-'[s]})", reads, [[45, 150, 1, 7, 26, s], [45, 150, 1, 7, 27, s]], [[0, 50, 99, 0, 2]],
                       {0: [{"inside", "short"}, {"inside"}]}, k=16))
    return c


def pile_probe(name, kept):
    """One window with len(kept) overlaps over four targets, strands alternating: overlap i is kept (a piece of 50 bases) or dropped (8 bases) as kept[i] says."""
    reads = [rand_seq("pile/template", TPL)] + [rand_seq(f"pile/target {t}", TGT) for t in range(4)]
    ovl, notes = [], []
    for i, keep in enumerate(kept):
        shift, t_start = i % 20, i % 7
        ovl.append([50 - shift, 150, 1 + i % 4, t_start, t_start + shift + (100 if keep else 7), i % 2])
        notes.append({"inside"} if keep else {"inside", "short"})
    return Probe(name, reads, ovl, [[0, 50, 99, 0, len(kept)]], {0: notes}, K, "pile")


def piles():
    c = [pile_probe(f"{n} overlaps", [True] * n) for n in (0, 1, 63, 64, 65, 128, 129)]
    c.append(pile_probe("kept and dropped alternating", [i % 2 == 0 for i in range(129)]))
    c.append(pile_probe("the first 64 dropped and the 65th kept", [False] * 64 + [True]))
    c.append(pile_probe("lane 63 dropped, lane 0 of the next round kept", [True] * 63 + [False, True] + [True] * 10))
    c.append(pile_probe("lane 63 kept, lane 0 of the next round dropped", [True] * 64 + [False] + [True] * 10))
    reads = [rand_seq("shared/template", 300)] + [rand_seq(f"shared/target {t}", TGT) for t in range(3)]
    ovl = [[0, 299, 1, 0, 149, 0], [60, 200, 2, 10, 140, 1], [0, 70, 3, 30, 100, 0]]
    c.append(Probe("three jobs of one template share one overlap range", reads, ovl, [[0, 0, 49, 0, 3], [0, 45, 94, 0, 3], [0, 90, 139, 0, 3]],
                   {0: [{"inside"}, {"no_span"}, {"inside"}], 1: [{"inside"}, {"left", "clamp0"}, {"right"}], 2: [{"inside"}, {"inside"}, {"no_span"}]}, K, "pile"))
    reads = [rand_seq("each other/a", TPL), rand_seq("each other/b", TPL)]
    c.append(Probe("two templates whose targets are each other", reads, [[10, 150, 1, 20, 160, 0], [10, 150, 0, 20, 160, 1]], [[0, 50, 99, 0, 1], [1, 50, 99, 1, 1]],
                   {0: [{"inside"}], 1: [{"inside"}]}, K, "pile"))
    return c


def launch_probe(name, n_jobs, empty=()):
    """n_jobs windows of 12 bases down one template, job w with w % 3 overlaps of its own (the second one dropped where w is odd); the jobs of `empty` reach
    beyond the template."""
    tpl_len = n_jobs + 40
    reads = [rand_seq("launch/template", tpl_len)] + [rand_seq(f"launch/target {t}", 120) for t in range(3)]
    ovl, jobs, notes = [], [], {}
    for w in range(n_jobs):
        first, mine = len(ovl), []
        for i in range(w % 3):
            shift, t_start, keep = min(w, w % 5), w % 50, not (i == 1 and w % 2)
            ovl.append([w - shift, w + 11 + w % 4, 1 + (w + i) % 3, t_start, t_start + shift + (11 + w % 4 if keep else 7), (w + i) % 2])
            mine.append({"inside"} if keep else {"inside", "short"})
        if w in empty:
            jobs.append([0, tpl_len - 5, tpl_len + 6, first, w % 3])
            notes[w] = []
        else:
            jobs.append([0, w, w + 11, first, w % 3])
            notes[w] = mine
    return Probe(name, reads, ovl, jobs, notes, K, "launch")


def launches():
    c = [launch_probe(f"{n} jobs", n) for n in (1, 3, 4, 5, 1023, 1024)]
    c.append(launch_probe("1025 jobs, the last pile empty", 1025, {1024}))
    c.append(launch_probe("2049 jobs, the piles of jobs 0, 1024 and 2048 empty", 2049, {0, 1024, 2048}))
    return c


def catalogue():
    return geometry() + piles() + launches()


CATALOGUE = catalogue()
BY_NAME = {p.name: p for p in CATALOGUE}


@functools.lru_cache(maxsize=None)
def ref_of(name):
    """[(pile, notes)] of a catalogue probe's jobs by the plain reference: computed once, shared, not changed."""
    return BY_NAME[name].reference()


# the kernel wrong in one decision (extract_ref.MUTANTS) -> the probe whose pile it changes
MUTANT_CAUGHT_BY = {
    "span_ge_begin": "overlap ends on the window's first base (+)",
    "span_le_end": "overlap begins on the window's last base (+)",
    "gate_lt": "gate met exactly (+)",
    "no_clamp0": "left: target begin clamped at 0 (+)",
    "keep_gt_k": f"inside: a piece of {K} bases (+)",
    "minus_unclamped_slice": "t_end one beyond the read (-)",
    "shift_before_revcomp": "'-': a piece with a shift (-)",
}
# ... and the one that changes no pile: both clamps at t_len - 1 bound a length that the slice, which substr cuts at the read's end, bounds already
#   left:  length' = min(L, t_len - t_beg); the slice has at most t_len - t_beg bases, and the piece is min(length, slice) of them
#   right: t_end' = min(t_len - 1, t_end + d) gives the same slice (substr cuts it there anyway) and length' = min(L, t_end' + 1) >= min(L, slice)
EQUIVALENT_MUTANTS = ("no_clamp_end",)
