"""CPU: the host side of the native driver without a device (CW_DRIVER_DRY=1: the workers take the jobs and drop them).  What is
checked: the producer -- PAF piles -> window positions on helper threads -> jobs in pile order -- counts the same piles, windows,
overlaps and jobs with one helper and with several, the window total is what the oracle's getAlignmentWindowsPositions restatement
says for the same piles, and nothing is written.  (`bench.py --mode driver` uses the same switch for its feeder-ceiling figure.)"""
import json
import os
import subprocess
import sys

import consent_amd as ca
import oracle_lib
from test_gpu_pipeline import make_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")


def dry_run(fa, paf, threads, per_batch_env=None, j=3):
    argv = [os.path.join(BIN, "CONSENT-correction"), "-a", paf, "-s", "3", "-S", "150", "-l", "500", "-k", "9", "-c", "8", "-A", "2", "-f", "4", "-m", "50", "-j", str(j), "-r", fa, "-M", "150", "-p", "x"]
    # the dry run is a test aid: it exists in the -DCW_TEST_AIDS build of the library only (consent_amd/aids/, csrc/cw_env.h)
    env = dict(os.environ, CW_DRIVER_DRY="1", CW_DRIVER_STATS="1", CW_PRODUCER_THREADS=str(threads), LD_LIBRARY_PATH=os.path.join(ROOT, "consent_amd", "aids"))
    out = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-1500:]
    assert out.stdout == ""  # a dry run corrects nothing
    st = json.loads([ln for ln in out.stderr.splitlines() if ln.startswith("{")][-1])
    assert st["dry"] is True and st["producer_threads"] == threads
    return st


def test_dry_run_counts_do_not_depend_on_the_helpers_and_match_the_oracle(tmp_path):
    fa, paf = make_dataset(tmp_path, 5, n_reads=90, glen=16000)
    a = dry_run(fa, paf, 1)
    b = dry_run(fa, paf, 5, j=7)
    for k in ("piles", "windows", "jobs"):
        assert a[k] == b[k], (k, a[k], b[k])
    assert a["workers"] == 3 * a["workers_per_device"] and b["workers"] == 7 * b["workers_per_device"] and 1 <= a["workers_per_device"] <= 4  # no device touched
    o = oracle_lib.oracle()
    ix = ca.ReadIndex(fa)
    n_win = n_piles = 0
    for tpl, tpl_len, ov, _ in ca.PafReader(paf, ix, 150):
        rows = [[tpl_len, int(r[0]), int(r[1]), int(r[5]), int(ix.seq_len[int(r[2])]), int(r[3]), int(r[4]), i] for i, r in enumerate(ov)]
        n_win += len(oracle_lib.window_positions(o.cwo_window_positions, tpl_len, rows, 3, 500, 50))
        n_piles += 1
    assert n_win > 100
    assert (a["piles"], a["windows"]) == (n_piles, n_win)


# ---- the job plan (csrc/cw_driver_plan.h), pinned against the driver as it was before the plan had a header of its own ----
GOLDEN = os.path.join(ROOT, "tests", "golden", "driver_plan.json")
PLAN_KEYS = ("workers", "workers_per_device", "windows_per_job", "jobs", "piles", "windows")
# every branch of the plan; a record's "covers" names the ones it is there for, and check_covers() holds the record to each of them
PLAN_BRANCHES = {"workers_per_device_2", "workers_per_device_3", "workers_per_device_env", "device_list_repeated_id", "j_above_device_count", "j_below_device_count",
                 "jobs_per_device_3", "jobs_per_device_8", "floor_4096", "cap_32768", "between_floor_and_cap", "windows_per_batch_below_max", "windows_per_batch_above_max",
                 "job_windows_env"}
_DRY_CHILD = """
import ctypes as C, json, os, sys
from consent_amd.pipeline import DriverArgs, DriverStats
p = json.loads(sys.argv[1])
lib = C.CDLL(os.path.join(p["root"], "consent_amd", "aids", "libconsent_amd.so"))  # the dry run is a test aid (csrc/cw_env.h)
lib.cw_run_correction.argtypes = [C.POINTER(DriverArgs), C.c_int, C.POINTER(DriverStats)]
devs = p["devices"]
arr = (C.c_int32 * len(devs))(*devs) if devs else None
a = DriverArgs(b"", os.fsencode(p["paf"]), os.fsencode(p["fa"]), b"", b"", 3, 150, p["window_size"], 9, 8, 2, 4, p["window_overlap"], p["nb_threads"], 150, 0,
               C.cast(arr, C.POINTER(C.c_int32)) if devs else None, len(devs) if devs else 0, p["windows_per_batch"])
fd = os.open(os.devnull, os.O_WRONLY)
sys.exit(lib.cw_run_correction(C.byref(a), fd, None))
"""


def plan_dry_run(fa, paf, args, env):
    """cw_run_correction over ctypes (only that reaches windows_per_batch and an explicit device list) in a process of its own: the statistics line is on stderr"""
    p = dict(args, root=ROOT, fa=fa, paf=paf)
    e = {k: v for k, v in os.environ.items() if not k.startswith("CW_")}
    e.update(env, CW_DRIVER_DRY="1", CW_DRIVER_STATS="1", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", _DRY_CHILD, json.dumps(p)], capture_output=True, text=True, env=e, timeout=300)
    assert out.returncode == 0, out.stderr[-1500:]
    st = json.loads([ln for ln in out.stderr.splitlines() if ln.startswith("{")][-1])
    assert st["dry"] is True
    return st


def tpl_bases(fa):
    return sum(len(ln.strip()) for ln in open(fa) if not ln.startswith(">"))


def check_covers(rec, max_batch):
    """a record that claims a branch shows it: by its own numbers, and by the estimate the plan goes by (template bases / window step + 1)"""
    a, x, env = rec["args"], rec["expect"], rec.get("env", {})
    step = a["window_size"] - a["window_overlap"]
    est = rec["tpl_bases"] // step + 1
    devs = a["devices"] or env.get("CW_DEVICES")
    distinct = x["workers"] // x["workers_per_device"]
    chosen = not a["windows_per_batch"] and "CW_JOB_WINDOWS" not in env  # the plan chose the job size
    want = est // ((3 if est // distinct < 100000 else 8) * distinct) + 1
    holds = {
        "workers_per_device_2": not devs and "CW_WORKERS_PER_DEVICE" not in env and x["workers_per_device"] == 2 and est // distinct < 1000000,
        "workers_per_device_3": not devs and "CW_WORKERS_PER_DEVICE" not in env and x["workers_per_device"] == 3 and est // distinct >= 1000000,
        "workers_per_device_env": not devs and env.get("CW_WORKERS_PER_DEVICE") not in (None, "2", "3") and x["workers_per_device"] == int(env.get("CW_WORKERS_PER_DEVICE", 0)),
        "device_list_repeated_id": bool(a["devices"]) and len(set(a["devices"])) < len(a["devices"]) and x["workers"] == len(a["devices"]),
        "j_above_device_count": rec.get("hand_derived") and not devs and a["nb_threads"] > rec["probe"]["hip_devices"] and distinct == rec["probe"]["hip_devices"],
        "j_below_device_count": rec.get("hand_derived") and not devs and a["nb_threads"] < rec["probe"]["hip_devices"] and distinct == a["nb_threads"],
        "jobs_per_device_3": chosen and est // distinct < 100000 and want < min(32768, max_batch) and x["windows_per_job"] == max(4096, want),
        "jobs_per_device_8": chosen and est // distinct >= 100000 and want < min(32768, max_batch) and x["windows_per_job"] == max(4096, want),
        "floor_4096": chosen and want < 4096 and x["windows_per_job"] == 4096,
        "cap_32768": chosen and want >= 32768 and x["windows_per_job"] == 32768,
        "between_floor_and_cap": chosen and 4096 < x["windows_per_job"] < 32768,
        "windows_per_batch_below_max": 0 < a["windows_per_batch"] < max_batch and x["windows_per_job"] == a["windows_per_batch"],
        "windows_per_batch_above_max": a["windows_per_batch"] > max_batch and x["windows_per_job"] == max_batch,
        "job_windows_env": "CW_JOB_WINDOWS" in env and x["windows_per_job"] == int(env.get("CW_JOB_WINDOWS", 0)) and x["windows_per_job"] not in (4096, 32768, max_batch),
    }
    for c in rec["covers"]:
        assert holds[c], (rec["name"], c)


_PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include "cw_driver_plan.h"
int main(int argc, char** argv) { /* window_size window_overlap nb_threads windows_per_batch tpl_bases hip_devices max_batch workers_env job_windows_env virtual_devices */
    if (argc != 11) return 2;
    cw_driver_args a{};
    a.window_size = atoi(argv[1]); a.window_overlap = atoi(argv[2]); a.nb_threads = atoi(argv[3]); a.windows_per_batch = atoi(argv[4]);
    DriverPlanInput in;
    in.a = &a; in.tpl_bases = atoll(argv[5]); in.hip_devices = atoi(argv[6]); in.max_batch = atoi(argv[7]); in.workers_per_device = atoi(argv[8]); in.job_windows = atol(argv[9]);
    in.virtual_devices = atoi(argv[10]);
    DriverPlan p;
    if (cw_driver_plan(in, &p) != CW_OK) return 3;
    printf("{\"workers\": %zu, \"workers_per_device\": %zu, \"windows_per_job\": %u, \"queue_cap\": %zu, \"devices\": [", p.workers.size(), p.workers_per_device, p.windows_per_job, p.queue_cap);
    for (size_t i = 0; i < p.workers.size(); ++i) printf("%s[%d, %d, %d]", i ? ", " : "", p.workers[i].device, p.workers[i].phys, p.workers[i].owner);
    printf("]}\n");
    return 0;
}
"""


def test_job_plan_is_what_the_driver_chose_before_the_plan_had_a_header(tmp_path):
    """Replays tests/golden/driver_plan.json: dry runs of the driver as it was when workers, job size and queue were decided inside cw_run_correction (recorded
    there with the -DCW_TEST_AIDS library over ctypes), every number compared.  -j above or below the device count cannot be had from a dry run (its device
    count IS -j): those records were derived by hand from that code and are replayed through csrc/cw_driver_plan.h compiled into a small CPU program."""
    gold = json.load(open(GOLDEN))
    lib = ca.load_library()  # (cw_plan_max_batch_windows is host arithmetic: no device is asked)
    covered = set()
    for rec in gold["records"]:
        covered |= set(rec["covers"])
    assert covered >= PLAN_BRANCHES, sorted(PLAN_BRANCHES - covered)  # the grid itself: no branch left out
    probe = tmp_path / "plan_probe"
    (tmp_path / "plan_probe.cpp").write_text(_PROBE)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "consent_amd", "csrc"), str(tmp_path / "plan_probe.cpp"), "-o", str(probe)])
    sets = {}
    for rec in gold["records"]:
        a = rec["args"]
        max_batch = int(lib.cw_plan_max_batch_windows(9, a["window_size"]))
        if rec.get("hand_derived"):
            q = rec["probe"]
            out = subprocess.run([str(probe)] + [str(v) for v in (a["window_size"], a["window_overlap"], a["nb_threads"], a["windows_per_batch"], rec["tpl_bases"], q["hip_devices"], max_batch,
                                                                  q["workers_per_device_env"], q["job_windows_env"], q["virtual_devices"])], capture_output=True, text=True)
            assert out.returncode == 0, out.stderr
            got = json.loads(out.stdout)
            for k in ("workers", "workers_per_device", "windows_per_job", "queue_cap", "devices"):
                assert got[k] == rec["expect"][k], (rec["name"], k, got[k], rec["expect"][k])
        else:
            name = rec["dataset"]
            if name not in sets:
                d = tmp_path / name
                d.mkdir()
                ds = gold["datasets"][name]
                sets[name] = make_dataset(d, ds["seed"], n_reads=ds["n_reads"], glen=ds["glen"], read_len=tuple(ds["read_len"]))
                assert tpl_bases(sets[name][0]) == ds["tpl_bases"]
            assert rec["tpl_bases"] == gold["datasets"][name]["tpl_bases"]
            got = plan_dry_run(*sets[name], a, rec.get("env", {}))
            for k in PLAN_KEYS:
                assert got[k] == rec["expect"][k], (rec["name"], k, got[k], rec["expect"][k])
        check_covers(rec, max_batch)
