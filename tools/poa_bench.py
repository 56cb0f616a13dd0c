#!/usr/bin/env python3
"""Time the POA operator alone (cw_poa_run_device, include/consent_amd.h): groups/s and DP cells/s per tier shape, with cw_last_timings' stages.

Input is synthetic: every group is `members` noisy copies (12 % errors, ONT mix 30:30:40 sub:ins:del) of its own random string, cut to `longest`
bases -- tests/poa_op_probes.py's construction, vectorised.  The batch lives in device memory; a step is one cw_poa_run_device and a wait for it.
DP cells of a group are counted as the oracle's restatement would fill them at the least: (members - 1) alignments of a member against a graph of
at least `longest` nodes, i.e. (members - 1) x longest x mean member length -- a lower bound that is the same for every implementation.

    python tools/poa_bench.py                         # the five shapes of the test catalogue, 16 384 groups each
    python tools/poa_bench.py --shape 100x10 --groups 4096 --steps 10

Prints one JSON line per shape and a markdown table (DESIGN.md section 4.7 holds the first one).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import consent_amd as ca  # noqa: E402
from consent_amd.engine import Batch, HostBatch, Result, poa_slot_bytes  # noqa: E402

SHAPES = ["24x12", "100x10", "200x8", "400x8", "900x6"]


def noisy_groups(n_groups, longest, members, rate, seed):
    """HostBatch of n_groups x members sequences, 2-bit packed: per group a random string of longest + longest / 8 + 2 bases, every member a noisy copy cut
    to `longest`."""
    if n_groups > 512:  # in slices: the masks below are several arrays of groups x members x bases
        parts = [noisy_groups(min(512, n_groups - g0), longest, members, rate, seed + g0) for g0 in range(0, n_groups, 512)]
        n_seqs, words = n_groups * members, (longest + 15) // 16
        return HostBatch(np.arange(n_groups + 1, dtype=np.uint32) * members, np.concatenate([p.seq_len for p in parts]), np.arange(n_seqs, dtype=np.uint64) * words,
                         np.concatenate([p.bases for p in parts]))
    rng = np.random.default_rng(seed)
    t_len = longest + longest // 8 + 2
    truth = rng.integers(0, 4, (n_groups, 1, t_len), dtype=np.uint8)
    x = rng.random((n_groups, members, t_len))
    dele, ins, sub = x < rate * 0.4, (x >= rate * 0.4) & (x < rate * 0.7), (x >= rate * 0.7) & (x < rate)
    base = np.broadcast_to(truth, x.shape)
    base = np.where(sub, (base + rng.integers(1, 4, x.shape, dtype=np.uint8)) & 3, base).astype(np.uint8)
    emit = np.where(dele, 0, np.where(ins, 2, 1))  # bases written per template base
    pos = np.cumsum(emit, axis=2) - emit  # where each one starts in the copy
    width = 2 * t_len
    out = np.zeros((n_groups, members, width), np.uint8)
    gi, mi, _ = np.indices(x.shape)
    keep = emit > 0
    first = np.where(ins, rng.integers(0, 4, x.shape, dtype=np.uint8), base)
    out[gi[keep], mi[keep], pos[keep]] = first[keep]
    out[gi[ins], mi[ins], pos[ins] + 1] = base[ins]
    lens = np.minimum(emit.sum(axis=2), longest).astype(np.uint32)
    words = (longest + 15) // 16
    codes = np.zeros((n_groups, members, words * 16), np.uint32)
    codes[:, :, :longest] = out[:, :, :longest]
    codes[np.arange(words * 16)[None, None, :] >= lens[:, :, None]] = 0  # unused low bits of the last word are zero
    packed = (codes.reshape(n_groups, members, words, 16) << (30 - 2 * np.arange(16, dtype=np.uint32))).sum(axis=3, dtype=np.uint64).astype(np.uint32)
    n_seqs = n_groups * members
    return HostBatch(np.arange(n_groups + 1, dtype=np.uint32) * members, lens.reshape(-1), np.arange(n_seqs, dtype=np.uint64) * words, packed.reshape(-1))


def bench_shape(eng, shape, n_groups, rate, steps, warmup, seed):
    import torch

    longest, members = (int(v) for v in shape.split("x"))
    hb = noisy_groups(n_groups, longest, members, rate, seed)
    dev = torch.device("cuda", eng.device)

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    cons_off = np.zeros(n_groups + 1, np.uint64)
    cons_off[1:] = np.cumsum(np.full(n_groups, (int(poa_slot_bytes(longest)) + 15) // 16 * 16, np.int64))
    t_in = (up(hb.win_first_seq, np.int32), up(hb.seq_len, np.int32), up(hb.seq_word_off, np.int64), up(np.concatenate([hb.bases, np.zeros(4, np.uint32)]), np.int32))
    t_cons = torch.zeros(int(cons_off[-1]), dtype=torch.uint8, device=dev)
    t_off, t_len, t_st = up(cons_off, np.int64), torch.zeros(n_groups, dtype=torch.int32, device=dev), torch.zeros(n_groups, dtype=torch.uint8, device=dev)
    b = Batch(n_groups, len(hb.seq_len), len(hb.bases), t_in[0].data_ptr(), t_in[1].data_ptr(), t_in[2].data_ptr(), t_in[3].data_ptr())
    r = Result(t_cons.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), t_st.data_ptr(), None, None, None)
    torch.cuda.synchronize(dev)
    times, stages = [], {}
    for step in range(warmup + steps):
        t0 = time.perf_counter()
        eng.poa_device(b, r)
        torch.cuda.synchronize(dev)
        if step >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
            for k, v in eng.timings().items():
                stages.setdefault(k, []).append(v)
    status = t_st.cpu().numpy()
    ms = float(np.median(times))
    lens = hb.seq_len.reshape(n_groups, members).astype(np.float64)
    cells = float(((members - 1) * longest * lens.mean(axis=1)).sum())
    c, _ = eng.profile()
    return {"shape": shape, "groups": n_groups, "members": members, "longest": longest, "error_rate": rate, "steps": steps, "ms_per_batch": round(ms, 3),
            "ms_min": round(min(times), 3), "ms_max": round(max(times), 3), "groups_per_s": round(n_groups / ms * 1e3), "dp_cells_per_s": float(f"{cells / ms * 1e3:.4g}"),
            "stopped_groups": int((status == ca.WIN_OVERFLOW).sum()), "mean_consensus": round(float(t_len.cpu().numpy().mean()), 1),
            "tasks_by_list": {"Q": int(c[6]), "M1": int(c[7]), "M2": int(c[8]), "L": int(c[9]), "S": int(c[0]) - int(c[6:12].sum())},
            "handed_over": {"to_S": int(c[18]), "to_L": int(c[21]), "to_G": int(c[22])},
            "stage_ms": {k: round(float(np.median(v)), 3) for k, v in stages.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", action="append", help="longest member x members, e.g. 100x10 (repeatable; default: the test catalogue's five)")
    ap.add_argument("--groups", type=int, default=16384)
    ap.add_argument("--error-rate", type=float, default=0.12)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-msa", type=int, default=150)
    ap.add_argument("--seed", type=int, default=0x90A0)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    eng = ca.Engine(ca.Params(9, 4, 8, 2, a.max_msa), device=a.device)
    rows = []
    try:
        for shape in a.shape or SHAPES:
            rows.append(bench_shape(eng, shape, a.groups, a.error_rate, a.steps, a.warmup, a.seed))
            print(json.dumps(rows[-1]), flush=True)
    finally:
        eng.close()
    order = ["poa_tasks", "poa_q", "poa", "poa_m1", "poa_m2", "poa_large", "poa_overflow", "poa_gather", "total"]
    print("\n| shape | groups | ms / batch | groups/s | DP cells/s | " + " | ".join(order) + " |")
    print("|---|---|---|---|---|" + "---|" * len(order))
    for r in rows:
        print(f"| {r['shape']} | {r['groups']} | {r['ms_per_batch']:.2f} | {r['groups_per_s']:.3g} | {r['dp_cells_per_s']:.3g} | " + " | ".join(f"{r['stage_ms'].get(k, 0):.2f}" for k in order) + " |")


if __name__ == "__main__":
    main()
