"""The engine's scratch plan at its limits: host arithmetic (cw_debug_plan, cw_debug_plan_caps), no GPU needed.

Per-window offsets into the solid table, the segment slots and the arena are 32-bit; the batch limit an engine states
(cw_max_batch_windows) must keep all three inside them, for every template length cw_configure can set; the index kernel's matrix
fallback slot must have the size its re-run after CW_WHY_MATRIX promises; the bench batch's plan must not grow."""
import ctypes as C
import itertools
import json
import os

import pytest

import consent_amd as ca

U32 = 0xFFFFFFFF
MAX_BATCH = 131072  # include/consent_amd.h CW_MAX_BATCH_WINDOWS
PF_ROWS_MAX = 4100  # cw_plan.h kPfRowsMax
CUS = 256


@pytest.fixture(scope="module")
def lib():
    lib = ca.load_library()
    lib.cw_debug_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.cw_debug_plan_caps.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
    lib.cw_plan_max_batch_windows.argtypes = [C.c_uint32, C.c_uint32]
    lib.cw_plan_max_batch_windows.restype = C.c_uint32
    return lib


def caps(lib, windows, depth, tmax, wlen=500, scale=1, pf_full=False, solid=4, k=9):
    """(total, solid entries, segment slots, arena bytes, arena scale, matrix rows, batch limit, task slots) of a batch of `windows` piles of
    depth + 1 sequences of about wlen bases."""
    n_seqs = windows * (depth + 1)
    n_words = n_seqs * ((wlen + 15) // 16 + 1)
    out = (C.c_uint64 * 8)()
    assert lib.cw_debug_plan_caps(k, solid, windows, n_seqs, n_words, CUS, scale, tmax, int(pf_full), out) == 0
    return dict(zip(("total", "solid", "seg", "arena", "arena_scale", "pf_rows", "limit", "tasks"), (int(x) for x in out)))


def expected_limit(tmax):
    return min(MAX_BATCH, U32 // (tmax + 2), U32 // (16 * (tmax + 16) + 4096))


@pytest.mark.parametrize("tmax", [128, 492, 1024, 1500, 2048])
def test_at_the_batch_limit_every_32_bit_capacity_fits(lib, tmax):
    c = caps(lib, 1, 30, tmax)
    n = c["limit"]
    assert n == expected_limit(tmax)
    assert (n == MAX_BATCH) == (tmax <= 1775)
    # the window-count-driven capacities at the limit, for short and for the longest templates of the plan, shallow and deep piles
    for depth, wlen in ((4, 100), (30, min(tmax + 8, 2056)), (150, min(tmax + 8, 2056))):
        at = caps(lib, n, depth, tmax, wlen=wlen)
        assert at["limit"] == n
        assert at["seg"] <= U32 and at["arena"] <= U32, at
        assert at["solid"] <= U32 or 16 * n * (depth + 1) * ((wlen + 15) // 16 + 1) // 4 > U32, at  # the solid table goes by bases, not windows
    over = caps(lib, n + 1, 4, tmax, wlen=100)
    if n < MAX_BATCH:
        assert over["arena"] > U32  # one window more would pass 2^32: refused (cw_submit, cw_run_device)
    assert over["limit"] == n


@pytest.mark.parametrize("tmax", [128, 492, 1024, 1500, 2048])
def test_the_driver_sizes_its_jobs_with_the_limit_its_engines_will_state(lib, tmax):
    k = 9
    assert lib.cw_plan_max_batch_windows(k, tmax + k - 1) == expected_limit(tmax)


def test_the_driver_limit_for_window_sizes(lib):
    """The driver calls cw_configure(window size): `-l 2000` is tmax 1992 at k = 9, under CW_MAX_BATCH_WINDOWS; `-l 500` and `-l 100` (tmax 128
    at least) are not; a window size beyond 2048 + k - 1, which cw_configure refuses, is held to the largest plan's limit."""
    assert lib.cw_plan_max_batch_windows(9, 2000) == U32 // (16 * (1992 + 16) + 4096) == 118566
    assert lib.cw_plan_max_batch_windows(9, 500) == MAX_BATCH
    assert lib.cw_plan_max_batch_windows(9, 100) == MAX_BATCH
    assert lib.cw_plan_max_batch_windows(11, 2058) == lib.cw_plan_max_batch_windows(9, 3000) == expected_limit(2048) == 115704


@pytest.mark.parametrize("tmax", [128, 492, 1024, 1500, 2048])
def test_the_matrix_slot_of_a_re_run_has_its_full_rows_whatever_the_mean_depth(lib, tmax):
    for windows, depth in ((2000, 4), (16384, 30), (16384, 150), (8, 3000)):
        first = caps(lib, windows, depth, tmax)
        assert first["pf_rows"] == min(max(16 * (depth + 2), 1024), PF_ROWS_MAX)  # mean depth + 1 sequences a pile, sixteen times, in 1024..4100
        rerun = caps(lib, windows, depth, tmax, pf_full=True)
        assert rerun["pf_rows"] == PF_ROWS_MAX
        grown = min(windows, CUS) * tmax * (PF_ROWS_MAX - first["pf_rows"]) * 2  # one slot per index work-group; nothing else changes
        assert abs(rerun["total"] - first["total"] - grown) < 256, (rerun, first)


def test_the_arena_scale_is_clamped_to_32_bit_offsets(lib):
    """x4 of the arena fits up to 51 781 windows at the default plan, x2 up to 103 563: include/consent_amd.h states this one dependence."""
    per = 16 * (1024 + 16) + 4096
    assert caps(lib, U32 // (4 * per), 4, 1024, wlen=100, scale=4)["arena_scale"] == 4
    assert caps(lib, U32 // (4 * per) + 1, 4, 1024, wlen=100, scale=4)["arena_scale"] == 2
    assert caps(lib, U32 // (2 * per) + 1, 4, 1024, wlen=100, scale=64)["arena_scale"] == 1
    for n in (30000, 60000, MAX_BATCH):
        for s in (1, 4, 16, 64):
            assert caps(lib, n, 4, 1024, wlen=100, scale=s)["arena"] <= U32


def test_the_bench_batch_plan_is_unchanged(lib):
    """tools/plan_sizes.py 16384 150: the first plan of the bench batch (16 384 windows, depth 150) -- its matrix slot still goes by the mean depth."""
    out = (C.c_uint64 * 15)()
    n_seqs = 16384 * 151
    assert lib.cw_debug_plan(9, 4, 16384, n_seqs, n_seqs * (500 // 16 + 2), CUS, 1, 1024, out) == 0
    c = caps(lib, 16384, 150, 1024)
    assert int(out[0]) == c["total"]
    assert c["pf_rows"] == 16 * 152
    assert int(out[0]) == 17975889152  # (the plan of the parent tree, byte for byte)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_numbers.json")
GRID_AXES = {"cus": [256, 64], "windows": [1, 24, 2048, 16384, 115704, 131072], "depth": [4, 30, 150], "tmax": [128, 492, 1024, 2048],
             "scale": [1, 4, 64], "pf_full": [0, 1]}


def plan_grid(lib, k=9, solid=4, wlen=500):
    """cw_debug_plan (15 numbers; it has no pf_full argument: recorded once per point of the other axes) and cw_debug_plan_caps (8 numbers)
    over GRID_AXES, in the order of itertools.product over the axes as listed; piles of depth + 1 sequences of wlen bases, as in caps()."""
    plan, caps8, rejected = [], [], []
    for cus, windows, depth, tmax, scale, pf_full in itertools.product(*GRID_AXES.values()):
        n_seqs = windows * (depth + 1)
        n_words = n_seqs * ((wlen + 15) // 16 + 1)
        if not pf_full:
            out15 = (C.c_uint64 * 15)()
            rc = lib.cw_debug_plan(k, solid, windows, n_seqs, n_words, cus, scale, tmax, out15)
            plan.append([int(x) for x in out15] if rc == 0 else None)
            if rc:
                rejected.append(["cw_debug_plan", cus, windows, depth, tmax, scale, pf_full, rc])
        out8 = (C.c_uint64 * 8)()
        rc = lib.cw_debug_plan_caps(k, solid, windows, n_seqs, n_words, cus, scale, tmax, pf_full, out8)
        caps8.append([int(x) for x in out8] if rc == 0 else None)
        if rc:
            rejected.append(["cw_debug_plan_caps", cus, windows, depth, tmax, scale, pf_full, rc])
    return {"axes": GRID_AXES, "k": k, "solid": solid, "wlen": wlen, "plan": plan, "caps": caps8, "rejected": rejected}


def test_the_plan_numbers_are_those_recorded_before_the_plan_moved(lib):
    """tests/golden/plan_numbers.json holds what the tree BEFORE the plan moved to cw_plan.h computed (the commit is named in the file): every
    number of every point of the grid, exactly."""
    gold = json.load(open(GOLDEN))
    got = plan_grid(lib, gold["k"], gold["solid"], gold["wlen"])
    assert gold["axes"] == GRID_AXES
    assert len(gold["plan"]) == 432 and len(gold["caps"]) == 864
    assert got["rejected"] == gold["rejected"]
    for name in ("plan", "caps"):
        assert len(got[name]) == len(gold[name]), name
        diff = [i for i, (a, b) in enumerate(zip(got[name], gold[name])) if a != b]
        assert not diff, (name, diff[:5], got[name][diff[0]], gold[name][diff[0]])
