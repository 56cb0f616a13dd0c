"""Randomised differential test on the GPU box: engine vs oracle over random parameters, error profiles, depths and window
lengths.  Prints one line per configuration and a summary; exit code 1 on any difference.
  python tools/fuzz_parity.py [seconds [seed]]
  python tools/fuzz_parity.py --mixed [--configs N] [--seed S]   one batch of windows of several generators per parameter set (depths 0-3000,
      lengths 60-2000, low-complexity families, template-only windows), each window compared with its result in a batch of its own kind and with
      the oracle: a mixed-vs-own-kind difference is a difference, and so is a stop that happens only in the mixed batch
  CW_FUZZ_CAP_BAR=0 python tools/fuzz_parity.py --family divergent [--configs N] [--seed S]   (opt-in) piles of unrelated middles between a shared head
      and tail -- graphs beyond tier G's cells and members of 1 300-3 800 bases, widths on both sides of the 2 048-column blocks of tier X's fill --
      every window compared with the oracle; fails when no task reached tier X, and on any capacity stop above the bar"""
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import consent_amd as ca  # noqa: E402
from consent_amd.engine import concat_batches as concat, synth_host  # noqa: E402
import oracle_lib  # noqa: E402


WHY = {1: "SETUP", 2: "COUNT", 3: "SOLIDCAP", 4: "TEMPLATE", 5: "MATRIX", 6: "SEGMENTS", 7: "TASKS", 8: "POA", 9: "FIN_LEN", 10: "FIN_SOLID", 11: "FIN_POLISH",
       12: "OUT_CONS", 13: "OUT_SOLID", 14: "ARENA", 15: "ANCHORS"}  # cw_device.h CW_WHY_*
MAX_OVERFLOW_SHARE = float(os.environ.get("CW_FUZZ_CAP_BAR", "0.001"))  # a capacity stop is never a wrong answer, but more than one window in a thousand is a regression
# (CW_FUZZ_CAP_BAR: tools/fuzz_policy.sh raises the bar for the heaviest-bundle build, whose consensuses are longer on chance-anchor piles)


def low_complexity(batch, rng, kind):
    """Rewrites the piles of a synthetic batch in place into a family the random generator never draws: "homopolymer" (runs of one base),
    "tandem" (a short unit repeated with 3 % noise: every k-mer of the template repeats, so few anchors survive), "identical" (every sequence
    a copy of the template: every template k-mer is an anchor and the position matrix is at its largest)."""
    nrng = np.random.default_rng(rng.getrandbits(32))
    wfs, slen, off, bases = batch.win_first_seq, batch.seq_len, batch.seq_word_off, batch.bases
    shifts = (30 - 2 * np.arange(16, dtype=np.uint32))
    for w in range(batch.n_windows):
        s0, s1 = int(wfs[w]), int(wfs[w + 1])
        unit = nrng.integers(0, 4, rng.choice([1, 2, 3, 5, 7, 11]))
        tpl = nrng.integers(0, 4, int(slen[s0:s1].max()) + 64)
        for s in range(s0, s1):
            n = int(slen[s])
            if kind == "homopolymer":
                runs = nrng.integers(3, 40, n // 3 + 2)
                codes = np.repeat((np.cumsum(nrng.integers(1, 4, len(runs))) & 3), runs)[:n]
            elif kind == "tandem":
                codes = unit[(np.arange(n) + (s - s0)) % len(unit)]
                noise = nrng.random(n) < 0.03
                codes = np.where(noise, nrng.integers(0, 4, n), codes)
            else:
                codes = tpl[:n]
            pad = np.zeros((n + 15) // 16 * 16, np.uint32)
            pad[:n] = codes
            o = int(off[s])
            bases[o : o + len(pad) // 16] = (pad.reshape(-1, 16) << shifts[None, :]).sum(axis=1, dtype=np.uint64).astype(np.uint32)


def outcome(res, info, w):
    st = int(res.status[w])
    return st, (int(info[w, 15]) if st == ca.WIN_OVERFLOW else 0), res.consensus(w), bytes(np.asarray(res.solid_kmers(w)).tobytes())


def mixed(n_configs, seed):
    rng = random.Random(seed)
    n_win = n_diff = n_mixed_only = n_oracle = n_stops = 0
    why_hist = {}
    for cfg in range(n_configs):
        k = rng.choice([7, 8, 9, 9, 9, 10, 11, 13])
        prm = ca.Params(k, rng.choice([2, 3, 4, 4, 6]), rng.choice([2, 4, 8, 8, 12]), rng.choice([1, 2, 2, 5]), rng.choice([5, 20, 50, 150]))
        kinds = []
        for _ in range(rng.randint(3, 6)):
            r = rng.random()
            if r < 0.12:  # deep: a few piles of 1000-3000 sequences at low error (what keeps the counter table inside its capacity)
                depth, wlen, err, nw = rng.choice([1000, 2000, 3000]), rng.choice([200, 300, 500]), rng.choice([3, 5, 10]), rng.randint(1, 2)
            elif r < 0.22:  # template-only windows
                depth, wlen, err, nw = 0, rng.choice([16, 60, 300, 900]), 0, rng.randint(1, 8)  # (synthetic windows have 16 bases at least)
            elif r < 0.4:  # long windows (cw_configure below)
                depth, wlen, err, nw = rng.choice([4, 12, 30]), rng.choice([1200, 1500, 2000]), rng.choice([30, 60, 120]), rng.randint(1, 6)
            else:
                depth, wlen, err = rng.choice([1, 2, 4, 8, 16, 30, 60, 100, 150]), rng.choice([60, 150, 300, 500, 500, 700, 900]), rng.choice([0, 10, 50, 120, 150, 200])
                nw = max(2, min(48, 6000 // ((depth + 1) * max(wlen, 100) // 100)))
            mix = rng.choice([(10, 60, 30), (30, 30, 40), (34, 33, 33)])
            spec = ca.SynthSpec(rng.getrandbits(40), rng.getrandbits(20), nw, depth, wlen, err, mix[0], mix[1], mix[2], (wlen + 60 + wlen // 3) // 16 + 2)
            b = synth_host(spec)
            family = rng.choice(["random"] * 8 + ["homopolymer", "tandem", "identical"]) if depth else "random"
            if family != "random":
                low_complexity(b, rng, family)
            kinds.append((b, f"d{depth}/l{wlen}/e{err}/{family}"))
        conf = max(int(b.seq_len[b.win_first_seq[:-1]].max()) for b, _ in kinds)
        conf = conf if conf > 1024 + k - 1 else None
        own = []
        eng = ca.Engine(prm)
        try:
            if conf:
                eng.configure(conf)
            for b, _ in kinds:
                res = eng.run(b)
                info = eng.win_info(b.n_windows)
                own.append([outcome(res, info, w) for w in range(b.n_windows)])
        finally:
            eng.close()
        order = [(i, w) for i, (b, _) in enumerate(kinds) for w in range(b.n_windows)]
        rng.shuffle(order)
        hb = concat([kinds[i][0].slice(w, w + 1) for i, w in order])
        eng = ca.Engine(prm)
        try:
            if conf:
                eng.configure(conf)
            res = eng.run(hb)
            info = eng.win_info(hb.n_windows)
        finally:
            eng.close()
        exp, _ = oracle_lib.oracle_run(prm, hb, threads=16)
        diff = mixed_only = bad_oracle = stops = 0
        for pos, (i, w) in enumerate(order):
            got, ref = outcome(res, info, pos), own[i][w]
            if got[0] == ca.WIN_OVERFLOW:
                stops += 1
                why_hist[WHY.get(got[1], str(got[1]))] = why_hist.get(WHY.get(got[1], str(got[1])), 0) + 1
                if ref[0] != ca.WIN_OVERFLOW:
                    mixed_only += 1
            if got != ref:
                diff += 1
                print(f"  window {pos} ({kinds[i][1]} #{w}): mixed status {got[0]} why {got[1]}, own kind status {ref[0]} why {ref[1]}", flush=True)
            elif got[0] != ca.WIN_OVERFLOW and (got[0] != int(exp.status[pos]) or got[2] != exp.consensus(pos) or got[3] != bytes(np.asarray(exp.solid_kmers(pos)).tobytes())):
                bad_oracle += 1
                print(f"  window {pos} ({kinds[i][1]} #{w}): differs from the oracle", flush=True)
        n_win += len(order); n_diff += diff; n_mixed_only += mixed_only; n_oracle += bad_oracle; n_stops += stops
        print(f"mixed {cfg}: k={prm.k} solid={prm.solid} c={prm.common_kmers} A={prm.min_anchors} M={prm.max_msa} configure={conf} windows={len(order)} "
              f"kinds={[d for _, d in kinds]} stops={stops} DIFF={diff} MIXED_ONLY_STOPS={mixed_only} ORACLE_DIFF={bad_oracle}", flush=True)
    print(f"mixed: seed {seed}, {n_configs} configurations, {n_win} windows, {n_diff} differences mixed vs own kind, {n_mixed_only} mixed-only stops, "
          f"{n_oracle} differences from the oracle, {n_stops} stops by reason {why_hist}")
    return 1 if n_diff or n_mixed_only or n_oracle else 0


def divergent(n_configs, seed):
    rng = random.Random(seed)
    n_win = n_diff = n_stops = routed = done = 0
    widths = [(1300, 1500), (1940, 2000), (2030, 2070), (2080, 2160), (2400, 2800), (3000, 3800)]  # member middles (a piece is its middle and a few flank bases)
    for cfg in range(n_configs):
        k = rng.choice([9, 9, 10, 11, 12])
        prm = ca.Params(k, rng.choice([2, 3]), 8, rng.choice([1, 2]), rng.choice([20, 50, 150]))
        piles = []
        for _ in range(rng.randint(1, 3)):
            lo, hi = rng.choice(widths)
            members = rng.randint(8, 24 if hi <= 1500 else 12 if hi <= 2200 else 8)  # (keeps every alignment inside tier X's cells)
            head, tail = "".join(rng.choice("ACGT") for _ in range(60)), "".join(rng.choice("ACGT") for _ in range(60))
            tpl = head + "".join(rng.choice("ACGT") for _ in range(rng.randrange(400, 1900))) + tail
            piles.append([tpl] + [head + "".join(rng.choice("ACGT") for _ in range(rng.randrange(lo, hi + 1))) + tail for _ in range(members - 1)])
        hb = ca.pack_piles(piles)
        eng = ca.Engine(prm)
        try:
            eng.configure(2048 + k - 1)
            got = eng.run(hb)
            info = eng.win_info(hb.n_windows)
            x = eng.tier_x_counters()
        finally:
            eng.close()
        exp, _ = oracle_lib.oracle_run(prm, hb, threads=16)
        diff = stops = 0
        for w in range(hb.n_windows):
            if got.status[w] == ca.WIN_OVERFLOW:
                stops += 1
                print(f"  window {w}: stopped, why {WHY.get(int(info[w, 15]), int(info[w, 15]))}", flush=True)
            elif got.status[w] != exp.status[w] or got.consensus(w) != exp.consensus(w) or not np.array_equal(got.solid_kmers(w), exp.solid_kmers(w)):
                diff += 1
                print(f"  window {w}: differs from the oracle", flush=True)
        n_win += hb.n_windows; n_diff += diff; n_stops += stops; routed += x["routed"]; done += x["done"]
        print(f"divergent {cfg}: k={prm.k} solid={prm.solid} A={prm.min_anchors} M={prm.max_msa} windows={hb.n_windows} members={[len(p) for p in piles]} "
              f"tier X {x} stops={stops} DIFF={diff}", flush=True)
    share = n_stops / max(1, n_win)
    print(f"divergent: seed {seed}, {n_configs} configurations, {n_win} windows, {n_diff} differences from the oracle, {n_stops} stops, tier X routed {routed} done {done}")
    if not routed:
        print("FAILED: no task reached tier X")
        return 1
    if share > MAX_OVERFLOW_SHARE:
        print(f"FAILED: capacity stops above {MAX_OVERFLOW_SHARE} of the windows ({share:.5f})")
        return 1
    return 1 if n_diff else 0


def main():
    if "--family" in sys.argv:
        a = sys.argv[1:]
        opt = lambda name, d: int(a[a.index(name) + 1]) if name in a else d  # noqa: E731
        if a[a.index("--family") + 1] != "divergent":
            print("--family: only 'divergent' (the default run draws random, homopolymer, tandem and identical piles)")
            return 2
        return divergent(opt("--configs", 20), opt("--seed", 1))
    if "--mixed" in sys.argv:
        a = sys.argv[1:]
        opt = lambda name, d: int(a[a.index(name) + 1]) if name in a else d  # noqa: E731
        return mixed(opt("--configs", 200), opt("--seed", 1))
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 120
    rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    t_end = time.time() + seconds
    n_cfg = n_win_total = bad = n_over_total = n_win_short_k = n_over_short_k = 0
    why_hist = {}
    while time.time() < t_end:
        k = rng.choice([5, 6, 7, 8, 9, 9, 9, 10, 11, 13])
        solid = rng.choice([1, 2, 3, 4, 4, 6])
        common = rng.choice([2, 4, 8, 8, 12])
        min_anchors = rng.choice([1, 2, 2, 5, 10])
        depth = rng.choice([1, 2, 4, 8, 16, 30, 30, 60, 100, 150])
        max_msa = rng.choice([2, 5, 20, 20, 50, 150])
        wlen = rng.choice([60, 150, 300, 500, 500, 500, 700, 900])
        err = rng.choice([0, 10, 50, 120, 120, 150, 200, 300])
        mix = rng.choice([(10, 60, 30), (30, 30, 40), (100, 0, 0), (0, 100, 0), (0, 0, 100), (34, 33, 33)])
        nw = max(2, min(48, 20000 // ((depth + 1) * max(wlen, 100) // 100)))
        s_seed, s_first = rng.getrandbits(40), rng.getrandbits(20)
        spec = ca.SynthSpec(s_seed, s_first, nw, depth, wlen, err, mix[0], mix[1], mix[2], (wlen + 60 + wlen // 3) // 16 + 2)
        prm = ca.Params(k, solid, common, min_anchors, max_msa)
        batch = synth_host(spec)
        family = rng.choice(["random"] * 8 + ["homopolymer", "tandem", "identical"])
        if family != "random":
            low_complexity(batch, rng, family)
        eng = ca.Engine(prm)
        try:
            got = eng.run(batch)
            info = eng.win_info(nw)
        finally:
            eng.close()
        exp, _ = oracle_lib.oracle_run(prm, batch, threads=16)
        diff = 0
        for w in range(nw):
            if got.status[w] == ca.WIN_OVERFLOW:
                continue  # a documented capacity, not a wrong answer
            if got.status[w] != exp.status[w] or got.consensus(w) != exp.consensus(w) or not np.array_equal(got.solid_kmers(w), exp.solid_kmers(w)):
                diff += 1
        n_over = int((got.status == ca.WIN_OVERFLOW).sum())
        why_cfg = {}
        for w in range(nw):
            if got.status[w] == ca.WIN_OVERFLOW:
                why_cfg[WHY.get(int(info[w, 15]), "?")] = why_cfg.get(WHY.get(int(info[w, 15]), "?"), 0) + 1
                why_hist[WHY.get(int(info[w, 15]), str(int(info[w, 15])))] = why_hist.get(WHY.get(int(info[w, 15]), str(int(info[w, 15]))), 0) + 1
        n_cfg += 1
        if k < 8:  # with k-mers this short most anchors are chance hits and the segmented consensus comes out several times its template (until round 5
            n_win_short_k += nw  # 5 % of these windows stopped on the finish kernel's 3072-character strings; its second pass holds 32768): counted apart,
            n_over_short_k += n_over  # held to the same bar
        else:
            n_win_total += nw
            n_over_total += n_over
        bad += diff
        print(f"k={k} solid={solid} c={common} A={min_anchors} depth={depth} M={max_msa} len={wlen} err={err} mix={mix} family={family} windows={nw} overflow={n_over} "
              f"template={int((got.status == ca.WIN_TEMPLATE).sum())} DIFF={diff}" + (f" why={why_cfg} spec=({s_seed},{s_first})" if why_cfg else ""), flush=True)
    share = n_over_total / max(1, n_win_total)
    print(f"{n_cfg} configurations, {n_win_total + n_win_short_k} windows, {bad} differences; k >= 8: {n_over_total} of {n_win_total} windows stopped by a capacity ({share:.5f}); "
          f"k < 8: {n_over_short_k} of {n_win_short_k}; by reason: {why_hist}")
    share_short = n_over_short_k / max(1, n_win_short_k)
    if share > MAX_OVERFLOW_SHARE or share_short > float(os.environ.get("CW_FUZZ_CAP_BAR_SHORT_K", "0.002")):
        print(f"FAILED: capacity stops above {MAX_OVERFLOW_SHARE} of the windows (k >= 8: {share:.5f}; k < 8: {share_short:.5f})")
        return 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
