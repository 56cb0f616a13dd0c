"""Times the overlap run (cw_overlap_count_device, cw_overlap_build_device, cw_overlap_run_device) on planted read sets, and beside it -- same device, same
process -- the locate run of the same reads against the genome they were cut from (cw_locate_build_device + cw_locate_run_device): the same per-position work
against an index of one hit per k-mer, where the overlap index holds depth hits.

    python tools/ovl_bench.py                              # the default sets
    python tools/ovl_bench.py --set 4600000x30x5000        # genome bases x depth x read length, repeatable
    python tools/ovl_bench.py --sample 0 --k 15 --min-hits 4

A set: a random genome; depth x genome / read-length reads, slices of it with 10 % substitutions, every second one reverse-complemented.  Per measurement the
median of --steps with the lowest and the highest of the device's own time (cw_last_timings' total).  Prints one JSON line per set and a markdown table
(DESIGN.md section 4.8 holds one).
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import consent_amd as ca  # noqa: E402
from consent_amd.engine import Batch, LocateRef, OverlapIndexRef, OverlapParams, Overlaps, Seeds  # noqa: E402
from sw_bench import pack  # noqa: E402

SETS = ("100000x30x5000", "1000000x30x5000", "1000000x30x1000")
SLOT = 256  # rows a query's slot holds


def bench(eng, spec, k, sample, max_occ, min_hits, steps, warmup, seed):
    import torch

    glen, depth, qlen = (int(v) for v in spec.split("x"))
    R = glen * depth // qlen
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, (1, glen), dtype=np.uint8)
    start = rng.integers(0, glen - qlen + 1, R)
    reads = genome[0][start[:, None] + np.arange(qlen)[None, :]]
    reads = np.where(rng.random(reads.shape) < 0.10, (reads + rng.integers(1, 4, reads.shape, dtype=np.uint8)) & 3, reads).astype(np.uint8)
    turned = np.arange(R) % 2 == 1
    reads[turned] = 3 - reads[turned][:, ::-1]
    gw, qw = pack(genome)[0], pack(reads)
    bases = np.concatenate([gw, qw.reshape(-1)])
    read_off = (len(gw) + np.arange(R, dtype=np.uint64) * qw.shape[1]).astype(np.uint64)
    dev = torch.device("cuda", eng.device)

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    t_bases = up(np.concatenate([bases, np.zeros(4, np.uint32)]), np.int32)
    t_len, t_off = up(np.full(R, qlen, np.uint32), np.int32), up(read_off, np.int64)
    rb = Batch(0, R, len(bases), None, t_len.data_ptr(), t_off.data_ptr(), t_bases.data_ptr())
    prm = OverlapParams(k, sample, max_occ, min_hits)
    n = C.c_uint64()

    def count():
        if eng.lib.cw_overlap_count_device(eng.handle, C.byref(rb), C.byref(prm), C.byref(n), None) != 0:
            raise RuntimeError("cw_overlap_count_device failed")

    count()
    words = int(eng.lib.cw_overlap_index_words(n.value))
    t_mem = torch.empty(words // 2 + 1, dtype=torch.int64, device=dev)
    index = OverlapIndexRef(t_mem.data_ptr(), n.value, prm)
    t_roff = up(np.arange(R + 1, dtype=np.uint64) * SLOT, np.int64)
    t_rows = torch.zeros(R * SLOT * ca.OVL_ROW, dtype=torch.int32, device=dev)
    t_n, t_status = torch.zeros(R, dtype=torch.int32, device=dev), torch.zeros(R, dtype=torch.uint8, device=dev)
    out = Overlaps(t_rows.data_ptr(), t_roff.data_ptr(), t_n.data_ptr(), t_status.data_ptr())
    kk = k or ca.OVL_K
    t_table = torch.empty(int(eng.lib.cw_locate_table_words(glen)), dtype=torch.int32, device=dev)
    lref = LocateRef(t_bases.data_ptr(), glen, t_table.data_ptr(), kk)
    t_lrows = torch.zeros(R * ca.SEED_ROW, dtype=torch.int32, device=dev)
    lrows = Seeds(t_lrows.data_ptr(), None, kk)
    torch.cuda.synchronize(dev)

    def build():
        if eng.lib.cw_overlap_build_device(eng.handle, C.byref(rb), C.byref(index), None) != 0:
            raise RuntimeError("cw_overlap_build_device failed")

    def locate_build():
        if eng.lib.cw_locate_build_device(eng.handle, C.byref(lref), None) != 0:
            raise RuntimeError("cw_locate_build_device failed")

    runs = {"count": count, "build": build, "run": lambda: eng.overlap_device(index, rb, 0, R, out), "locate_build": locate_build,
            "locate": lambda: eng.locate_device(lref, rb, lrows)}
    res, stages = {}, {}
    for name, run in runs.items():
        device = []
        for step in range(warmup + steps):
            run()
            torch.cuda.synchronize(dev)
            if step >= warmup:
                device.append(eng.timings()["total"])
                if name in ("build", "run"):
                    for key, v in eng.timings().items():
                        stages.setdefault(key, []).append(v)
        res[name] = {"device_ms": [round(float(np.median(device)), 4), round(min(device), 4), round(max(device), 4)]}
    eng.overlap_device(index, rb, 0, R, out)
    torch.cuda.synchronize(dev)
    routes = eng.overlap_routes()
    n_rows, status = t_n.cpu().numpy().view(np.uint32), t_status.cpu().numpy()
    # a true overlap: the two slices share 1 000 bases or more
    order = np.argsort(start)
    true_pairs = int(sum(np.searchsorted(start[order], start[order][i] + qlen - 1000, side="right") - i - 1 for i in range(R))) * 2 if qlen > 1000 else 0
    positions = R * (qlen - kk + 1)
    run_ms, loc_ms = res["run"]["device_ms"][0], res["locate"]["device_ms"][0]
    return {"set": spec, "k": kk, "sample": sample, "max_occ": max_occ or ca.OVL_MAX_OCC, "min_hits": min_hits, "reads": R, "entries": int(n.value),
            "index_mb": round(words * 4 / 2**20, 1), "steps": steps, **res, "stage_ms": {key: round(float(np.median(v)), 4) for key, v in stages.items()},
            "run_ns_per_read": round(run_ms * 1e6 / R, 1), "run_ns_per_sampled_position": round(run_ms * 1e6 / max(int(n.value), 1), 2),
            "run_ns_per_position": round(run_ms * 1e6 / positions, 3), "dense_share": round(routes[1] / R, 5), "routes": list(routes),
            "status": {name: int((status == v).sum()) for name, v in (("ok", ca.OVL_OK), ("slot", ca.OVL_SLOT), ("dense", ca.OVL_DENSE))},
            "rows": int(n_rows[status == ca.OVL_OK].sum()), "true_pairs_1000": true_pairs, "run_over_locate": round(run_ms / loc_ms, 2), "depth": depth}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--set", action="append", help="genome bases x depth x read length (repeatable; default: %s)" % ", ".join(SETS))
    ap.add_argument("--k", type=int, default=0)
    ap.add_argument("--sample", type=int, default=ca.OVL_SAMPLE)
    ap.add_argument("--max-occ", type=int, default=0)
    ap.add_argument("--min-hits", type=int, default=ca.OVL_MIN_HITS)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rng-seed", type=int, default=0x0E71A9)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    eng = ca.Engine(ca.Params(9, 4, 8, 10, 150), device=a.device)
    rows = []
    try:
        for spec in a.set or SETS:
            rows.append(bench(eng, spec, a.k, a.sample, a.max_occ, a.min_hits, a.steps, a.warmup, a.rng_seed))
            print(json.dumps(rows[-1]), flush=True)
    finally:
        eng.close()
    cell = lambda m: f"{m['device_ms'][0]:.3f} ({m['device_ms'][1]:.3f} - {m['device_ms'][2]:.3f})"
    print("\n| genome x depth x read | reads | entries | index MB | count ms | build ms | run ms | ns / read | ns / sampled position | ovl, ovl_dense ms | dense share | "
          "rows | locate build ms | locate run ms | run / locate |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['set']} | {r['reads']} | {r['entries']} | {r['index_mb']} | {cell(r['count'])} | {cell(r['build'])} | {cell(r['run'])} | {r['run_ns_per_read']:.1f} | "
              f"{r['run_ns_per_sampled_position']:.2f} | {r['stage_ms'].get('ovl', 0):.3f}, {r['stage_ms'].get('ovl_dense', 0):.3f} | {r['dense_share']:.4f} | {r['rows']} | "
              f"{cell(r['locate_build'])} | {cell(r['locate'])} | {r['run_over_locate']:.1f} |")


if __name__ == "__main__":
    main()
