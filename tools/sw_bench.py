#!/usr/bin/env python3
"""Time the alignment operator alone (cw_sw_run_device, include/consent_amd.h): pairs/s and DP cells/s per shape, with and without the indel totals -- and with
--path through cw_sw_path_run_device, which returns the alignment's ops, with --pileup also through cw_pileup_run_device, which counts the paths into their
reference's columns, with --cut also through cw_sw_cut_run_device, which cuts every query at its reference's window boundaries -- with cw_last_timings' stages.

Input is synthetic: a group is one random reference and `--per-group` queries; a query is a stretch of its reference with 8 % substitutions and one deletion
of four bases (so the banded traceback starts at a band of 5) -- or, where the query is the longer one, the whole reference treated that way between random
flanks.  The shape 1540x1540 is another construction, tests/sw_op_probes.py planted(40): reference P + G1 + M + S, query P + M + G2 + S with random 500-base
P, M, S and unrelated 40-base G1, G2 -- the traceback's band starts at 1 and doubles to 64 (129 cells a row).

The shape 500x600x30, which --pileup adds, is 500 x 600 with 30 queries on every reference instead of --per-group: deeper columns, more adds to the same words.

The batch lives in device memory; a step is one cw_sw_run_device (or cw_sw_path_run_device, cw_pileup_run_device, cw_sw_cut_run_device) and a wait for it.  DP cells of a pair are query length x
reference length: the forward sweep's; the reverse sweep and the traceback come on top and are not counted, for any implementation.

    python tools/sw_bench.py                              # the six shapes (query x reference), each with and without indel totals
    python tools/sw_bench.py --shape 500x600 --pairs 65536 --steps 10
    python tools/sw_bench.py --path                       # a third measurement per shape: the path run
    python tools/sw_bench.py --pileup                     # a fourth beside it: the pileup run of the same batch, and the shape 500x600x30
    python tools/sw_bench.py --cut                        # a fifth: the cut run of the same batch at --window columns a window, on the shapes of --pileup
    python tools/sw_bench.py --strand                     # instead: the strand vote and the reverse complement beside the plain run and a device copy of the same batch
    python tools/sw_bench.py --seed                       # instead: the seed run (cw_seed_run_device) beside the strand vote and the plain run of the same batch
    python tools/sw_bench.py --span                       # instead: the plain and the cut run with and without the spans of a seed run, reads of 1 000 and 3 000 bases on 8 192
    python tools/sw_bench.py --locate                     # instead: the tiled seed run as Engine.place batches it beside cw_locate_build_device + cw_locate_run_device, one reference and one bag of reads
    python tools/sw_bench.py --oracle 4096                # also: so many 500 x 600 pairs through the oracle's cwo_ssw on --threads CPU threads

Prints one JSON line per measurement and a markdown table (DESIGN.md section 4.8 holds the first one, from a --path run).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import consent_amd as ca  # noqa: E402
from consent_amd.engine import Batch, HostBatch, LocateRef, Pileup, Seeds, Strands, SwCuts, SwPaths, SwSpans, sw_cuts  # noqa: E402

SHAPES = {"24x150": 262144, "100x600": 131072, "500x600": 65536, "2000x2048": 4096, "8000x2048": 512, "1540x1540": 2048}  # query x reference -> pairs of the default run
PLANTED = {"1540x1540": (500, 40)}  # shapes built as planted pairs: (part, g)
DEEP = {"500x600x30": 61440}  # query x reference x queries per reference: what --pileup adds
WIDE_GROUP = {"500x2048": 16384, "500x2048x16384": 16384}  # what --strand adds: 16 queries a reference, and ONE reference with all 16 384 queries -- equal lengths
SPAN = {"1000x8192": 2048, "3000x8192": 512}  # what --span runs: reads planted at 10 - 12 % errors in references of 8 192 bases, 16 a reference
LOCATE = {"5000x65536": 2048, "5000x1048576": 2048, "5000x4194304": 2048, "500x1048576": 16384}  # what --locate runs: read x reference -> reads of the bag
LOCATE_TILE = 8192  # Engine.place's default tile
PATH, PILE, CUT = "path", "pileup", "cut"  # the third, fourth and fifth mode beside flags 0 and CW_SW_WANT_INDELS


def pack(codes):
    """(n, L) 2-bit codes -> (n, ceil(L / 16)) words, most significant pair first."""
    n, L = codes.shape
    words = (L + 15) // 16
    c = np.zeros((n, words * 16), np.uint32)
    c[:, :L] = codes
    return (c.reshape(n, words, 16) << (30 - 2 * np.arange(16, dtype=np.uint32))).sum(axis=2, dtype=np.uint64).astype(np.uint32)


def make_groups(n_pairs, qlen, rlen, per_group, seed):
    """(HostBatch, references (G, rlen) codes, queries (G, per_group, qlen) codes)."""
    rng = np.random.default_rng(seed)
    G = max(1, n_pairs // per_group)
    refs = rng.integers(0, 4, (G, rlen), dtype=np.uint8)
    span = min(qlen, rlen - 4) if rlen > 8 else rlen  # reference bases a query covers, before the deletion
    src_len = span + 4 if rlen >= span + 4 else span
    start = rng.integers(0, rlen - src_len + 1, (G, per_group))
    src = refs[np.arange(G)[:, None, None], start[:, :, None] + np.arange(src_len)[None, None, :]]
    cut = rng.integers(1, max(2, span - 4), (G, per_group))
    keep = np.arange(span)[None, None, :]
    core = np.take_along_axis(src, np.where(keep < cut[:, :, None], keep, keep + (src_len - span)), axis=2)  # four bases deleted at `cut`
    sub = rng.random(core.shape) < 0.08
    core = np.where(sub, (core + rng.integers(1, 4, core.shape, dtype=np.uint8)) & 3, core).astype(np.uint8)
    queries = rng.integers(0, 4, (G, per_group, qlen), dtype=np.uint8)
    left = (qlen - span) // 2
    queries[:, :, left : left + span] = core
    rw, qw = pack(refs), pack(queries.reshape(-1, qlen))
    per = 1 + per_group
    lens = np.tile(np.array([rlen] + [qlen] * per_group, np.uint32), G)
    wlen = np.tile(np.array([rw.shape[1]] + [qw.shape[1]] * per_group, np.uint64), G)
    offs = np.concatenate([[0], np.cumsum(wlen)[:-1]]).astype(np.uint64)
    bases = np.concatenate([np.concatenate([rw[g], qw[g * per_group : (g + 1) * per_group].reshape(-1)]) for g in range(G)])
    return HostBatch(np.arange(G + 1, dtype=np.uint32) * per, lens, offs, bases), refs, queries


def make_planted(n_pairs, part, g, seed):
    """HostBatch of n_pairs groups of one planted pair each (tests/sw_op_probes.py planted): reference P + G1 + M + S, query P + M + G2 + S."""
    rng = np.random.default_rng(seed)
    P, M, S = (rng.integers(0, 4, (n_pairs, part), dtype=np.uint8) for _ in range(3))
    G1, G2 = (rng.integers(0, 4, (n_pairs, g), dtype=np.uint8) for _ in range(2))
    rw, qw = pack(np.concatenate([P, G1, M, S], axis=1)), pack(np.concatenate([P, M, G2, S], axis=1))
    L, W = 3 * part + g, rw.shape[1]
    bases = np.stack([rw, qw], axis=1).reshape(-1)
    return HostBatch(np.arange(n_pairs + 1, dtype=np.uint32) * 2, np.full(2 * n_pairs, L, np.uint32), np.arange(2 * n_pairs, dtype=np.uint64) * W, bases)


def bench_shape(eng, shape, n_pairs, per_group, flags, steps, warmup, seed, window=100):
    import torch

    qlen, rlen, *deep = (int(v) for v in shape.split("x"))
    per_group = deep[0] if deep else per_group
    if shape in PLANTED:
        hb = make_planted(n_pairs, *PLANTED[shape], seed)
    else:
        hb, _, _ = make_groups(n_pairs, qlen, rlen, per_group, seed)
    n_pairs = len(hb.seq_len) - hb.n_windows
    dev = torch.device("cuda", eng.device)

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    t_in = (up(hb.win_first_seq, np.int32), up(hb.seq_len, np.int32), up(hb.seq_word_off, np.int64), up(np.concatenate([hb.bases, np.zeros(4, np.uint32)]), np.int32))
    t_rows = torch.zeros(len(hb.seq_len) * 8, dtype=torch.int32, device=dev)
    b = Batch(hb.n_windows, len(hb.seq_len), len(hb.bases), t_in[0].data_ptr(), t_in[1].data_ptr(), t_in[2].data_ptr(), t_in[3].data_ptr())
    if flags == PATH:  # the slots: CW_SW_OPS_BOUND of every sequence and its reference
        wfs, lens = hb.win_first_seq.astype(np.int64), hb.seq_len.astype(np.int64)
        off = np.concatenate([[0], np.cumsum(lens + lens[np.repeat(wfs[:-1], np.diff(wfs))])]).astype(np.uint64)
        t_off, t_nops = up(off, np.int64), torch.zeros(len(hb.seq_len), dtype=torch.int32, device=dev)
        t_ops = torch.zeros(int(off[-1]) + 1, dtype=torch.int32, device=dev)
        paths = SwPaths(t_ops.data_ptr(), t_off.data_ptr(), t_nops.data_ptr())
    if flags == PILE:  # the slots: a reference's columns, none for a query
        wfs, lens = hb.win_first_seq.astype(np.int64), hb.seq_len.astype(np.int64)
        width = np.zeros(len(lens), np.int64)
        width[wfs[:-1]] = lens[wfs[:-1]]
        off = np.concatenate([[0], np.cumsum(width)]).astype(np.uint64)
        t_off, t_counts = up(off, np.int64), torch.zeros((int(off[-1]) + 1, ca.PILE_COL), dtype=torch.int32, device=dev)
        pile = Pileup(t_counts.data_ptr(), t_off.data_ptr())
    if flags == CUT:  # the slots: CW_SW_CUTS of its reference for a query, none for a reference
        wfs, lens = hb.win_first_seq.astype(np.int64), hb.seq_len.astype(np.int64)
        width = sw_cuts(lens[np.repeat(wfs[:-1], np.diff(wfs))], window)
        width[wfs[:-1]] = 0
        off = np.concatenate([[0], np.cumsum(width)]).astype(np.uint64)
        t_off, t_cuts = up(off, np.int64), torch.zeros(int(off[-1]) + 1, dtype=torch.int32, device=dev)
        cuts = SwCuts(t_cuts.data_ptr(), t_off.data_ptr(), window)
    torch.cuda.synchronize(dev)
    times, stages = [], {}
    for step in range(warmup + steps):
        t0 = time.perf_counter()
        if flags == PATH:
            eng.sw_path_device(b, C.c_void_p(t_rows.data_ptr()), paths, 0)
        elif flags == PILE:
            eng.pileup_device(b, C.c_void_p(t_rows.data_ptr()), pile, 0)
        elif flags == CUT:
            eng.sw_cut_device(b, C.c_void_p(t_rows.data_ptr()), cuts)
        else:
            eng.sw_device(b, C.c_void_p(t_rows.data_ptr()), flags)
        torch.cuda.synchronize(dev)
        if step >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
            for k, v in eng.timings().items():
                stages.setdefault(k, []).append(v)
    rows = t_rows.cpu().numpy().reshape(-1, 8)
    q = rows[rows[:, 7] != ca.SW_IS_REF]
    ms = float(np.median(times))
    extra = {}
    if flags == PATH:
        nops = t_nops.cpu().numpy()
        extra = {"mean_ops": round(float(nops[rows[:, 7] != ca.SW_IS_REF].mean()), 1), "no_path_rows": int((q[:, 7] == ca.SW_NO_PATH).sum()),
                 "open_rows": int((q[:, 7] == ca.SW_PATH_OPEN).sum()), "mean_indels": round(float(q[:, 5:7].sum(axis=1).mean()), 1)}
    if flags == PILE:
        counts = t_counts.cpu().numpy()[:-1].astype(np.int64)
        counted = int(((q[:, 7] == ca.SW_ALIGNED) & (q[:, 0] > 0)).sum())
        assert int(counts[:, ca.PILE_BEGIN].sum()) == int(counts[:, ca.PILE_END].sum()) == counted and int(counts[:, ca.PILE_DEL].sum()) == int(q[:, 6].sum())
        extra = {"counted_rows": counted, "columns": len(counts), "mean_depth": round(float(counts[:, : ca.PILE_DEL + 1].sum() / max(len(counts), 1)), 2),
                 "no_path_rows": int((q[:, 7] == ca.SW_NO_PATH).sum()), "open_rows": int((q[:, 7] == ca.SW_PATH_OPEN).sum()), "mean_indels": round(float(q[:, 5:7].sum(axis=1).mean()), 1)}
    if flags == CUT:
        words, is_q = t_cuts.cpu().numpy()[:-1].astype(np.int64), rows[:, 7] != ca.SW_IS_REF
        first, last = words[off[:-1][is_q].astype(np.int64)], words[off[1:][is_q].astype(np.int64) - 1]
        counted = (q[:, 7] == ca.SW_ALIGNED) & (q[:, 0] > 0)
        assert np.array_equal(first[counted], q[counted, 3]) and np.array_equal(last[counted], q[counted, 4] + 1) and not first[~counted].any() and not last[~counted].any()
        extra = {"window": window, "counted_rows": int(counted.sum()), "cut_words": len(words), "no_path_rows": int((q[:, 7] == ca.SW_NO_PATH).sum()),
                 "open_rows": int((q[:, 7] == ca.SW_PATH_OPEN).sum()), "slot_rows": int((q[:, 7] == ca.SW_CUT_SLOT).sum()), "mean_indels": round(float(q[:, 5:7].sum(axis=1).mean()), 1)}
    return {"shape": shape, "pairs": n_pairs, "indels": flags if flags in (PATH, PILE, CUT) else bool(flags), "steps": steps, **extra, "ms_per_batch": round(ms, 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3),
            "pairs_per_s": round(n_pairs / ms * 1e3), "dp_cells_per_s": float(f"{n_pairs * qlen * rlen / ms * 1e3:.4g}"), "mean_score": round(float(q[:, 0].mean()), 1),
            "no_indels_rows": int((q[:, 7] == ca.SW_NO_INDELS).sum()), "stopped_rows": int((q[:, 7] == ca.SW_STOP).sum()),
            "stage_ms": {k: round(float(np.median(v)), 3) for k, v in stages.items()}}


def device_copy(dst, src, n_bytes):
    """hipMemcpyAsync device to device on the null stream, through the HIP runtime this process has loaded: the yardstick of the reverse complement."""
    global _HIP
    if _HIP is None:
        _HIP = C.CDLL("libamdhip64.so")
        _HIP.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    rc = _HIP.hipMemcpyAsync(dst, src, n_bytes, 3, None)  # 3: hipMemcpyDeviceToDevice
    if rc != 0:
        raise RuntimeError(f"hipMemcpyAsync: {rc}")


_HIP = None


def bench_strand(eng, shape, n_pairs, per_group, steps, warmup, seed):
    """One batch in device memory, four measurements in this process: the plain cw_sw_run_device, cw_strand_run_device, cw_revcomp_device of every sequence
    (strand NULL: the most it can be asked for) and a device-to-device copy of the batch's words.  Per measurement the median of `steps` with the lowest and the
    highest, wall clock around the call and the wait for it, and the device's own time: between the run's first and last event for the plain and the strand run,
    between the two events around the one launch for the reverse complement (its stage) and for the copy (HIP events on its stream)."""
    import torch

    qlen, rlen, *deep = (int(v) for v in shape.split("x"))
    per_group = deep[0] if deep else per_group
    hb = make_planted(n_pairs, *PLANTED[shape], seed) if shape in PLANTED else make_groups(n_pairs, qlen, rlen, per_group, seed)[0]
    S, G, W = len(hb.seq_len), hb.n_windows, len(hb.bases)
    n_pairs = S - G
    dev = torch.device("cuda", eng.device)

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    t_in = (up(hb.win_first_seq, np.int32), up(hb.seq_len, np.int32), up(hb.seq_word_off, np.int64), up(np.concatenate([hb.bases, np.zeros(4, np.uint32)]), np.int32))
    t_rows = torch.zeros(S * 8, dtype=torch.int32, device=dev)
    t_strand = torch.zeros(S, dtype=torch.uint8, device=dev)
    t_hits = torch.zeros(2 * S, dtype=torch.int32, device=dev)
    t_out = torch.zeros(W + 4, dtype=torch.int32, device=dev)
    b = Batch(G, S, W, t_in[0].data_ptr(), t_in[1].data_ptr(), t_in[2].data_ptr(), t_in[3].data_ptr())
    votes = Strands(t_strand.data_ptr(), t_hits.data_ptr(), 0)
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    torch.cuda.synchronize(dev)

    def copy_words():
        ev[0].record()
        device_copy(t_out.data_ptr(), t_in[3].data_ptr(), W * 4)
        ev[1].record()

    runs = {"sw": lambda: eng.sw_device(b, C.c_void_p(t_rows.data_ptr()), 0), "strand": lambda: eng.strand_device(b, votes),
            "revcomp": lambda: eng.revcomp_device(b, None, t_out.data_ptr()), "copy": copy_words}
    out, stages = {}, {}
    for name, run in runs.items():
        wall, device = [], []
        for step in range(warmup + steps):
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize(dev)
            if step >= warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
                # (the reverse complement is one launch between its stage's two events, as the copy is one call between two events: like with like)
                device.append(ev[0].elapsed_time(ev[1]) if name == "copy" else eng.timings()["revcomp" if name == "revcomp" else "total"])
                if name == "strand":
                    for k, v in eng.timings().items():
                        stages.setdefault(k, []).append(v)
        out[name] = {"wall_ms": [round(float(np.median(wall)), 4), round(min(wall), 4), round(max(wall), 4)],
                     "device_ms": [round(float(np.median(device)), 4), round(min(device), 4), round(max(device), 4)]}
    strand = t_strand.cpu().numpy()
    is_q = np.ones(S, bool)
    is_q[hb.win_first_seq[:-1]] = False
    assert (strand[~is_q] == ca.STRAND_IS_REF).all() and (strand[is_q] != ca.STRAND_IS_REF).all()
    return {"shape": shape, "mode": "strand", "pairs": n_pairs, "groups": G, "words": W, "steps": steps, **out,
            "strand_over_sw": round(out["strand"]["device_ms"][0] / out["sw"]["device_ms"][0], 4), "revcomp_over_copy": round(out["revcomp"]["device_ms"][0] / max(out["copy"]["device_ms"][0], 1e-6), 3),
            "strand_ns_per_pair": round(out["strand"]["device_ms"][0] * 1e6 / n_pairs, 2), "forward": int((strand == ca.STRAND_FWD).sum()), "reverse": int((strand == ca.STRAND_REV).sum()),
            "none": int((strand == ca.STRAND_NONE).sum()), "stage_ms": {k: round(float(np.median(v)), 4) for k, v in stages.items()}}


def bench_seed(eng, shape, n_pairs, per_group, steps, warmup, seed):
    """One batch in device memory -- bench_strand's -- and three measurements in this process: the plain cw_sw_run_device, cw_strand_run_device and
    cw_seed_run_device.  Per measurement the median of `steps` with the lowest and the highest of the device's own time, between the run's first and last
    event, and the seed run's stages."""
    import torch

    qlen, rlen, *deep = (int(v) for v in shape.split("x"))
    per_group = deep[0] if deep else per_group
    hb = make_planted(n_pairs, *PLANTED[shape], seed) if shape in PLANTED else make_groups(n_pairs, qlen, rlen, per_group, seed)[0]
    S, G, W = len(hb.seq_len), hb.n_windows, len(hb.bases)
    n_pairs = S - G
    dev = torch.device("cuda", eng.device)

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    t_in = (up(hb.win_first_seq, np.int32), up(hb.seq_len, np.int32), up(hb.seq_word_off, np.int64), up(np.concatenate([hb.bases, np.zeros(4, np.uint32)]), np.int32))
    t_rows = torch.zeros(S * 8, dtype=torch.int32, device=dev)
    t_strand = torch.zeros(S, dtype=torch.uint8, device=dev)
    t_hits = torch.zeros(2 * S, dtype=torch.int32, device=dev)
    t_seed = torch.zeros(S * ca.SEED_ROW, dtype=torch.int32, device=dev)
    t_sbyte = torch.zeros(S, dtype=torch.uint8, device=dev)
    b = Batch(G, S, W, t_in[0].data_ptr(), t_in[1].data_ptr(), t_in[2].data_ptr(), t_in[3].data_ptr())
    votes, seeds = Strands(t_strand.data_ptr(), t_hits.data_ptr(), 0), Seeds(t_seed.data_ptr(), t_sbyte.data_ptr(), 0)
    torch.cuda.synchronize(dev)
    runs = {"sw": lambda: eng.sw_device(b, C.c_void_p(t_rows.data_ptr()), 0), "strand": lambda: eng.strand_device(b, votes), "seed": lambda: eng.seed_device(b, seeds)}
    out, stages = {}, {}
    for name, run in runs.items():
        device = []
        for step in range(warmup + steps):
            run()
            torch.cuda.synchronize(dev)
            if step >= warmup:
                device.append(eng.timings()["total"])
                if name == "seed":
                    for k, v in eng.timings().items():
                        stages.setdefault(k, []).append(v)
        out[name] = {"device_ms": [round(float(np.median(device)), 4), round(min(device), 4), round(max(device), 4)]}
    rows = t_seed.cpu().numpy().reshape(S, ca.SEED_ROW)
    is_q = np.ones(S, bool)
    is_q[hb.win_first_seq[:-1]] = False
    assert (rows[~is_q, 0] == ca.STRAND_IS_REF).all() and (rows[is_q, 0] != ca.STRAND_IS_REF).all() and np.array_equal(t_sbyte.cpu().numpy(), rows[:, 0].astype(np.uint8))
    return {"shape": shape, "mode": "seed", "pairs": n_pairs, "groups": G, "words": W, "steps": steps, **out,
            "seed_over_sw": round(out["seed"]["device_ms"][0] / out["sw"]["device_ms"][0], 4), "seed_over_strand": round(out["seed"]["device_ms"][0] / out["strand"]["device_ms"][0], 3),
            "seed_ns_per_pair": round(out["seed"]["device_ms"][0] * 1e6 / n_pairs, 2), "median_hits": int(np.median(rows[is_q, 1])),
            "stage_ms": {k: round(float(np.median(v)), 4) for k, v in stages.items()}}


def bench_locate(eng, shape, n_reads, steps, warmup, seed, k=0):
    """One random reference and one bag of reads -- slices of it with 10 % substitutions, every second one reverse-complemented -- in device memory, and in this
    process: the tiled seed run exactly as Engine.place batches it (a group per tile of LOCATE_TILE bases, each the tile and ALL reads, the words packed once and
    shared), cw_locate_build_device, and cw_locate_run_device against that index.  Per measurement the median of `steps` with the lowest and the highest of the
    device's own time, the locate run's stages, the reads of its two routes, and how many reads either way puts on the slice they were cut from."""
    import torch

    qlen, rlen = (int(v) for v in shape.split("x"))
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, (1, rlen), dtype=np.uint8)
    start = rng.integers(0, rlen - qlen + 1, n_reads)
    reads = ref[0][start[:, None] + np.arange(qlen)[None, :]]
    sub = rng.random(reads.shape) < 0.10
    reads = np.where(sub, (reads + rng.integers(1, 4, reads.shape, dtype=np.uint8)) & 3, reads).astype(np.uint8)
    turned = np.arange(n_reads) % 2 == 1
    reads[turned] = 3 - reads[turned][:, ::-1]
    rw, qw = pack(ref)[0], pack(reads)
    R, QW, T = n_reads, qw.shape[1], (rlen + LOCATE_TILE - 1) // LOCATE_TILE
    bases = np.concatenate([rw, qw.reshape(-1)])
    tile_len = np.minimum(LOCATE_TILE, rlen - LOCATE_TILE * np.arange(T)).astype(np.uint32)
    tile_off = (np.arange(T, dtype=np.uint64) * (LOCATE_TILE // 16)).astype(np.uint64)
    read_off = (len(rw) + np.arange(R, dtype=np.uint64) * QW).astype(np.uint64)
    lens = np.concatenate([np.concatenate([[tile_len[t]], np.full(R, qlen, np.uint32)]) for t in range(T)]).astype(np.uint32)
    offs = np.concatenate([np.concatenate([[tile_off[t]], read_off]) for t in range(T)]).astype(np.uint64)
    tiled = HostBatch(np.arange(T + 1, dtype=np.uint32) * np.uint32(R + 1), lens, offs, bases)
    dev = torch.device("cuda", eng.device)

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    t_bases = up(np.concatenate([bases, np.zeros(4, np.uint32)]), np.int32)
    t_in = (up(tiled.win_first_seq, np.int32), up(tiled.seq_len, np.int32), up(tiled.seq_word_off, np.int64))
    S = len(tiled.seq_len)
    t_seed = torch.zeros(S * ca.SEED_ROW, dtype=torch.int32, device=dev)
    t_rlen, t_roff = up(np.full(R, qlen, np.uint32), np.int32), up(read_off, np.int64)
    t_rows = torch.zeros(R * ca.SEED_ROW, dtype=torch.int32, device=dev)
    t_table = torch.empty(int(eng.lib.cw_locate_table_words(rlen)), dtype=torch.int32, device=dev)
    kk = k or ca.LOCATE_K
    b = Batch(T, S, len(bases), t_in[0].data_ptr(), t_in[1].data_ptr(), t_in[2].data_ptr(), t_bases.data_ptr())
    rb = Batch(0, R, len(bases), None, t_rlen.data_ptr(), t_roff.data_ptr(), t_bases.data_ptr())
    lref = LocateRef(t_bases.data_ptr(), rlen, t_table.data_ptr(), kk)
    seeds, lrows = Seeds(t_seed.data_ptr(), None, kk), Seeds(t_rows.data_ptr(), None, kk)
    torch.cuda.synchronize(dev)

    def build():
        if eng.lib.cw_locate_build_device(eng.handle, C.byref(lref), None) != 0:
            raise RuntimeError("cw_locate_build_device failed")

    runs = {"tiled": lambda: eng.seed_device(b, seeds), "build": build, "locate": lambda: eng.locate_device(lref, rb, lrows)}
    out, stages = {}, {}
    for name, run in runs.items():
        device = []
        for step in range(warmup + steps):
            run()
            torch.cuda.synchronize(dev)
            if step >= warmup:
                device.append(eng.timings()["total"])
                if name == "locate":
                    for key, v in eng.timings().items():
                        stages.setdefault(key, []).append(v)
        out[name] = {"device_ms": [round(float(np.median(device)), 4), round(min(device), 4), round(max(device), 4)]}
    routes = eng.locate_routes()
    # where the read, turned when it was planted turned, begins: its start; a window of SEED_SPAN diagonals holds it (substitutions only: no drift)
    rows = t_rows.cpu().numpy().reshape(R, ca.SEED_ROW)
    on = lambda st, dg: float(np.mean((st == turned) & (dg <= start) & (start < dg + ca.SEED_SPAN)))
    trows = t_seed.cpu().numpy().reshape(T, R + 1, ca.SEED_ROW)[:, 1:, :]
    best = np.argmax(np.where(trows[:, :, ca.SEED_STATUS] <= ca.STRAND_REV, trows[:, :, ca.SEED_HITS], -1), axis=0)
    pick = trows[best, np.arange(R)]
    return {"shape": shape, "mode": "locate", "k": kk, "reads": R, "tiles": T, "table_mb": round(t_table.numel() * 4 / 2**20, 1), "steps": steps, **out,
            "tiled_ns_per_pair": round(out["tiled"]["device_ms"][0] * 1e6 / (T * R), 1), "locate_ns_per_read": round(out["locate"]["device_ms"][0] * 1e6 / R, 1),
            "build_ns_per_base": round(out["build"]["device_ms"][0] * 1e6 / rlen, 3), "tiled_over_locate": round(out["tiled"]["device_ms"][0] / out["locate"]["device_ms"][0], 2),
            "routes": list(routes), "median_hits": int(np.median(rows[:, ca.SEED_HITS])), "locate_on_slice": round(on(rows[:, ca.SEED_STATUS] == ca.STRAND_REV, rows[:, ca.SEED_DIAG]), 4),
            "tiled_on_slice": round(on(pick[:, ca.SEED_STATUS] == ca.STRAND_REV, best * LOCATE_TILE + pick[:, ca.SEED_DIAG]), 4),
            "stage_ms": {key: round(float(np.median(v)), 4) for key, v in stages.items()}}


def make_planted_reads(n_pairs, qlen, rlen, per_group, seed):
    """HostBatch of groups of one random reference and per_group reads: a read copies qlen reference bases from a random start with 10 - 12 % errors (a rate
    drawn per read; substitutions, insertions and deletions a third each), every second read reverse-complemented."""
    rng = np.random.default_rng(seed)
    G = max(1, n_pairs // per_group)
    refs = rng.integers(0, 4, (G, rlen), dtype=np.uint8)
    seqs = []
    for g in range(G):
        seqs.append(refs[g])
        for k in range(per_group):
            a = int(rng.integers(0, rlen - qlen + 1))
            src = refs[g, a : a + qlen]
            rate = rng.uniform(0.10, 0.12)
            x = rng.random(qlen)
            take = np.where(x < rate / 3, 0, np.where(x < 2 * rate / 3, 2, 1))  # a deletion, an insertion behind the base, the base
            out = np.repeat(src, take)
            first = np.cumsum(take) - take  # where a base's copies begin
            ins = first[take == 2] + 1
            out[ins] = rng.integers(0, 4, len(ins), dtype=np.uint8)
            sub = first[(x >= 2 * rate / 3) & (x < rate)]
            out[sub] = (out[sub] + rng.integers(1, 4, len(sub), dtype=np.uint8)) & 3
            seqs.append((3 - out[::-1]).astype(np.uint8) if k % 2 else out)
    lens = np.array([len(x) for x in seqs], np.uint32)
    words = [pack(x[None, :])[0] for x in seqs]
    offs = np.concatenate([[0], np.cumsum([len(w) for w in words])[:-1]]).astype(np.uint64)
    return HostBatch(np.arange(G + 1, dtype=np.uint32) * (1 + per_group), lens, offs, np.concatenate(words))


def bench_span(eng, shape, n_pairs, per_group, steps, warmup, seed, window):
    """One batch of planted reads in device memory.  The seed side once per step -- cw_seed_run_device, cw_seed_spans_device, cw_revcomp_device by the seed
    run's strand bytes -- then, on the oriented batch, the plain run and the cut run without spans (cw_sw_run_device, cw_sw_cut_run_device) and with them
    (cw_sw_span_run_device, cw_sw_cut_span_run_device).  Device time between a run's first and last event, the median of `steps` with the lowest and highest."""
    import torch

    qlen, rlen = (int(v) for v in shape.split("x"))
    hb = make_planted_reads(n_pairs, qlen, rlen, per_group, seed)
    S, G, Wd = len(hb.seq_len), hb.n_windows, len(hb.bases)
    n_pairs = S - G
    dev = torch.device("cuda", eng.device)

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    t_in = (up(hb.win_first_seq, np.int32), up(hb.seq_len, np.int32), up(hb.seq_word_off, np.int64), up(np.concatenate([hb.bases, np.zeros(4, np.uint32)]), np.int32))
    t_turned = torch.zeros(Wd + 4, dtype=torch.int32, device=dev)
    t_rows, t_rows_s = torch.zeros(S * 8, dtype=torch.int32, device=dev), torch.zeros(S * 8, dtype=torch.int32, device=dev)
    t_seed, t_sbyte = torch.zeros(S * ca.SEED_ROW, dtype=torch.int32, device=dev), torch.zeros(S, dtype=torch.uint8, device=dev)
    t_lo, t_hi = torch.zeros(S, dtype=torch.int32, device=dev), torch.zeros(S, dtype=torch.int32, device=dev)
    wfs, lens = hb.win_first_seq.astype(np.int64), hb.seq_len.astype(np.int64)
    width = sw_cuts(lens[np.repeat(wfs[:-1], np.diff(wfs))], window)
    width[wfs[:-1]] = 0
    off = np.concatenate([[0], np.cumsum(width)]).astype(np.uint64)
    t_off = up(off, np.int64)
    t_cuts, t_cuts_s = torch.zeros(int(off[-1]) + 1, dtype=torch.int32, device=dev), torch.zeros(int(off[-1]) + 1, dtype=torch.int32, device=dev)
    b = Batch(G, S, Wd, t_in[0].data_ptr(), t_in[1].data_ptr(), t_in[2].data_ptr(), t_in[3].data_ptr())
    bo = Batch(G, S, Wd, t_in[0].data_ptr(), t_in[1].data_ptr(), t_in[2].data_ptr(), t_turned.data_ptr())  # the oriented batch
    seeds, spans = Seeds(t_seed.data_ptr(), t_sbyte.data_ptr(), 0), SwSpans(t_lo.data_ptr(), t_hi.data_ptr())
    cuts, cuts_s = SwCuts(t_cuts.data_ptr(), t_off.data_ptr(), window), SwCuts(t_cuts_s.data_ptr(), t_off.data_ptr(), window)
    torch.cuda.synchronize(dev)
    runs = {"seed": lambda: eng.seed_device(b, seeds), "seed_spans": lambda: eng.seed_spans_device(b, t_seed.data_ptr(), t_lo.data_ptr(), t_hi.data_ptr()),
            "revcomp": lambda: eng.revcomp_device(b, t_sbyte.data_ptr(), t_turned.data_ptr()),
            "sw": lambda: eng.sw_device(bo, C.c_void_p(t_rows.data_ptr()), 0), "sw_span": lambda: eng.sw_span_device(bo, C.c_void_p(t_rows_s.data_ptr()), spans, 0),
            "cut": lambda: eng.sw_cut_device(bo, C.c_void_p(t_rows.data_ptr()), cuts), "cut_span": lambda: eng.sw_cut_span_device(bo, C.c_void_p(t_rows_s.data_ptr()), cuts_s, spans)}
    out, stages, same = {}, {}, {}
    for name, run in runs.items():
        device = []
        for step in range(warmup + steps):
            run()
            torch.cuda.synchronize(dev)
            if step >= warmup:
                t = eng.timings()
                device.append(t["total"])
                for k, v in t.items():
                    stages.setdefault(name, {}).setdefault(k, []).append(v)
        out[name] = {"device_ms": [round(float(np.median(device)), 4), round(min(device), 4), round(max(device), 4)]}
        if name in ("sw_span", "cut_span"):  # the rows of the run without spans just before it
            same[name] = float((t_rows.cpu().numpy().reshape(S, 8) == t_rows_s.cpu().numpy().reshape(S, 8)).all(axis=1).mean())
    lo, hi = t_lo.cpu().numpy().view(np.uint32).astype(np.int64), t_hi.cpu().numpy().view(np.uint32).astype(np.int64)
    is_q = np.ones(S, bool)
    is_q[hb.win_first_seq[:-1]] = False
    span_len = (hi - lo)[is_q]
    med = lambda name: out[name]["device_ms"][0]
    seed_side = med("seed") + med("seed_spans") + med("revcomp")
    return {"shape": shape, "mode": "span", "pairs": n_pairs, "groups": G, "steps": steps, "window": window, **out, "placed": int((span_len > 0).sum()),
            "mean_span": round(float(span_len.mean()), 1), "cell_ratio": round(rlen / max(float(span_len.mean()), 1.0), 3),
            "sw_ratio": round(med("sw") / med("sw_span"), 3), "cut_ratio": round(med("cut") / med("cut_span"), 3),
            "sw_ratio_with_seed_side": round(med("sw") / (med("sw_span") + seed_side), 3), "cut_ratio_with_seed_side": round(med("cut") / (med("cut_span") + seed_side), 3),
            "seed_side_ms": round(seed_side, 4), "rows_equal": {k: round(v, 5) for k, v in same.items()},
            "stage_ms": {n: {k: round(float(np.median(v)), 4) for k, v in st.items()} for n, st in stages.items()}}


def oracle_rate(n_pairs, threads, seed):
    """n_pairs 500 x 600 pairs of the same construction through the oracle's cwo_ssw (oracle/liboracle.so) on `threads` threads: pairs/s, cells/s."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib

    fn = oracle_lib.oracle().cwo_ssw
    _, refs, queries = make_groups(n_pairs, 500, 600, 16, seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    work = [(letters[queries[g, k]].tobytes(), letters[refs[g]].tobytes()) for g in range(len(refs)) for k in range(queries.shape[1])]

    def one(p):
        out = np.zeros(7, np.int32)
        fn(p[0], len(p[0]), p[1], len(p[1]), C.c_void_p(out.ctypes.data))  # (ctypes releases the interpreter lock for the call)
        return int(out[0])

    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        scores = list(ex.map(one, work, chunksize=16))
    s = time.perf_counter() - t0
    return {"oracle": "cwo_ssw", "shape": "500x600", "pairs": len(work), "threads": threads, "seconds": round(s, 3), "pairs_per_s": round(len(work) / s),
            "dp_cells_per_s": float(f"{len(work) * 500 * 600 / s:.4g}"), "mean_score": round(float(np.mean(scores)), 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", action="append", help="query x reference, e.g. 500x600 (repeatable; default: the five of the table)")
    ap.add_argument("--pairs", type=int, default=0, help="pairs per batch (default: by shape)")
    ap.add_argument("--per-group", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rng-seed", type=int, default=0x5A11, help="of the synthetic input")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--path", action="store_true", help="also time the path run (cw_sw_path_run_device) on every shape")
    ap.add_argument("--pileup", action="store_true", help="time the path run and the pileup run (cw_pileup_run_device) of the same batch on every shape, and on 500x600x30")
    ap.add_argument("--cut", action="store_true", help="time the path run, the pileup run and the cut run (cw_sw_cut_run_device) of the same batch on the shapes of --pileup")
    ap.add_argument("--strand", action="store_true", help="instead of the alignment modes: cw_strand_run_device and cw_revcomp_device beside the plain run and a device-to-device copy of the same "
                    "batch, on the shapes of --cut, on 500x2048 and on one group of a 2 048-base reference with 16 384 queries of 500 bases")
    ap.add_argument("--seed", action="store_true", help="instead of the alignment modes: cw_seed_run_device beside cw_strand_run_device and the plain run of the same batch, on the shapes of --strand")
    ap.add_argument("--span", action="store_true", help="instead of the alignment modes: the plain run and the cut run without spans and with the spans of a seed run "
                    "(cw_seed_run_device + cw_seed_spans_device, timed beside them), reads of 1 000 and 3 000 bases planted at 10 - 12 % errors in references of 8 192")
    ap.add_argument("--locate", action="store_true", help="instead of the alignment modes: one reference and one bag of reads; the tiled seed run as Engine.place batches it beside "
                    "cw_locate_build_device and cw_locate_run_device, on 2 048 reads of 5 000 bases on 65 536, 1 048 576 and 4 194 304 bases and 16 384 reads of 500 on 1 048 576")
    ap.add_argument("--k", type=int, default=0, help="of --locate: k of both runs (0 = CW_LOCATE_K)")
    ap.add_argument("--window", type=int, default=100, help="reference columns a window of the cut run")
    ap.add_argument("--oracle", type=int, default=0, help="also time so many 500x600 pairs through the oracle on --threads CPU threads")
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    a.pileup = a.pileup or a.cut
    eng = ca.Engine(ca.Params(9, 4, 8, 2, 150), device=a.device)
    rows = []
    if a.locate:
        try:
            for shape in a.shape or list(LOCATE):
                rows.append(bench_locate(eng, shape, a.pairs or LOCATE.get(shape, 2048), a.steps, a.warmup, a.rng_seed, a.k))
                print(json.dumps(rows[-1]), flush=True)
        finally:
            eng.close()
        cell = lambda m: f"{m['device_ms'][0]:.3f} ({m['device_ms'][1]:.3f} - {m['device_ms'][2]:.3f})"
        print("\n| read x reference | reads | tiles | tiled seed run ms | ns / pair | build ms | ns / base | locate run ms | ns / read | locate, locate_dense ms | tiled / locate | dense reads | on the slice: tiled, locate |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['shape']} | {r['reads']} | {r['tiles']} | {cell(r['tiled'])} | {r['tiled_ns_per_pair']:.1f} | {cell(r['build'])} | {r['build_ns_per_base']:.3f} | {cell(r['locate'])} | "
                  f"{r['locate_ns_per_read']:.1f} | {r['stage_ms'].get('locate', 0):.3f}, {r['stage_ms'].get('locate_dense', 0):.3f} | {r['tiled_over_locate']:.1f} | {r['routes'][1]} | "
                  f"{r['tiled_on_slice']:.3f}, {r['locate_on_slice']:.3f} |")
        return
    if a.span:
        try:
            for shape in a.shape or list(SPAN):
                rows.append(bench_span(eng, shape, a.pairs or SPAN.get(shape, 1024), a.per_group, a.steps, a.warmup, a.rng_seed, a.window if a.window != 100 else 500))
                print(json.dumps(rows[-1]), flush=True)
        finally:
            eng.close()
        cell = lambda m: f"{m['device_ms'][0]:.2f} ({m['device_ms'][1]:.2f} - {m['device_ms'][2]:.2f})"
        print("\n| read x reference | pairs | mean span | cells n / span | plain ms | plain span ms | ratio | cut ms | cut span ms | ratio | seed + spans + revcomp ms | cut ratio with those | rows equal |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['shape']} | {r['pairs']} | {r['mean_span']:.0f} | {r['cell_ratio']:.2f} | {cell(r['sw'])} | {cell(r['sw_span'])} | {r['sw_ratio']:.2f} | {cell(r['cut'])} | {cell(r['cut_span'])} | "
                  f"{r['cut_ratio']:.2f} | {r['seed_side_ms']:.3f} | {r['cut_ratio_with_seed_side']:.2f} | {min(r['rows_equal'].values()):.4f} |")
        return
    if a.seed:
        try:
            for shape in a.shape or list(SHAPES) + list(DEEP) + list(WIDE_GROUP):
                rows.append(bench_seed(eng, shape, a.pairs or SHAPES.get(shape) or DEEP.get(shape) or WIDE_GROUP.get(shape, 16384), a.per_group, a.steps, a.warmup, a.rng_seed))
                print(json.dumps(rows[-1]), flush=True)
        finally:
            eng.close()
        cell = lambda m: f"{m['device_ms'][0]:.3f} ({m['device_ms'][1]:.3f} - {m['device_ms'][2]:.3f})"
        print("\n| query x reference | pairs | plain run ms | strand run ms | seed run ms | seed / plain | seed / strand | ns / pair |")
        print("|---|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['shape']} | {r['pairs']} | {cell(r['sw'])} | {cell(r['strand'])} | {cell(r['seed'])} | {r['seed_over_sw']:.4f} | {r['seed_over_strand']:.2f} | {r['seed_ns_per_pair']:.1f} |")
        return
    if a.strand:
        try:
            for shape in a.shape or list(SHAPES) + list(DEEP) + list(WIDE_GROUP):
                rows.append(bench_strand(eng, shape, a.pairs or SHAPES.get(shape) or DEEP.get(shape) or WIDE_GROUP.get(shape, 16384), a.per_group, a.steps, a.warmup, a.rng_seed))
                print(json.dumps(rows[-1]), flush=True)
        finally:
            eng.close()
        cell = lambda m: f"{m['device_ms'][0]:.3f} ({m['device_ms'][1]:.3f} - {m['device_ms'][2]:.3f})"
        print("\n| query x reference | pairs | plain run ms | strand run ms | strand / plain | ns / pair | reverse complement ms | device copy ms | revcomp / copy |")
        print("|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['shape']} | {r['pairs']} | {cell(r['sw'])} | {cell(r['strand'])} | {r['strand_over_sw']:.4f} | {r['strand_ns_per_pair']:.1f} | {cell(r['revcomp'])} | {cell(r['copy'])} | {r['revcomp_over_copy']:.2f} |")
        return
    try:
        for shape in a.shape or list(SHAPES) + (list(DEEP) if a.pileup else []):
            for flags in (0, ca.SW_WANT_INDELS) + ((PATH,) if a.path or a.pileup else ()) + ((PILE,) if a.pileup else ()) + ((CUT,) if a.cut else ()):
                rows.append(bench_shape(eng, shape, a.pairs or SHAPES.get(shape) or DEEP.get(shape, 16384), a.per_group, flags, a.steps, a.warmup, a.rng_seed, a.window))
                print(json.dumps(rows[-1]), flush=True)
    finally:
        eng.close()
    if a.oracle:
        print(json.dumps(oracle_rate(a.oracle, a.threads, a.rng_seed)), flush=True)
    order = ["sw_order", "sw_align", "sw_align_wide", "sw_align_long", "total"] + (["pile_clear"] if a.pileup else [])
    # a path run's, a pileup run's and a cut run's stages, in the same columns
    stage_of = {PATH: {"sw_align": "sw_path", "sw_align_wide": "sw_path_wide", "sw_align_long": "sw_path_long"}, PILE: {"sw_align": "pile", "sw_align_wide": "pile_wide", "sw_align_long": "pile_long"},
                CUT: {"sw_align": "cut", "sw_align_wide": "cut_wide", "sw_align_long": "cut_long"}}
    print("\n| query x reference | indel totals | pairs | ms / batch | pairs/s | DP cells/s | " + " | ".join(order) + " |")
    print("|---|---|---|---|---|---|" + "---|" * len(order))
    for r in rows:
        names = stage_of.get(r["indels"], {})
        print(f"| {r['shape']} | {r['indels'] if names else 'yes' if r['indels'] else 'no'} | {r['pairs']} | {r['ms_per_batch']:.2f} ({r['ms_min']:.2f} - {r['ms_max']:.2f}) | {r['pairs_per_s']:.3g} | {r['dp_cells_per_s']:.3g} | "
              + " | ".join(f"{r['stage_ms'].get(names.get(k, k), 0):.2f}" for k in order) + " |")


if __name__ == "__main__":
    main()
