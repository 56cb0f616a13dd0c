"""The POA tiers as a batched consensus operator (include/consent_amd.h cw_poa_run / cw_poa_run_device; csrc/cw_poa_op.h): every group's consensus is
byte-equal to the oracle's POA (tests/oracle_lib.py oracle_poa) of its first max_msa non-empty members -- for a probe of every tier, in any batch
composition, on the edges of the group semantics, beside groups that stop, and through both entry points of one engine that also runs windows."""
import ctypes as C
import random

import numpy as np
import pytest

import consent_amd as ca
import oracle_lib
import poa_op_probes as pp
from consent_amd.engine import Batch, Result, _ptr, alloc_poa_results, poa_slot_bytes, synth_host

pytestmark = pytest.mark.gpu
E_INVALID = -1
WHY_POA, WHY_OUT_CONS = 8, 12  # csrc/cw_device.h
N_TIER, N_OVER = 6, 18  # Engine.profile() counters: n_tier[6] from word 6, n_over[6] from word 18 (list 0 = tier Q, 1 M1, 2 M2, 3 L, 4 G)
PS_POA = 8  # csrc/cw_device.h CW_PS_POA: cycle totals of slab tier t's five phases at 8 + 5 t (0 = tier S)
LIST_OF = {"Q": 0, "M1": 1, "M2": 2, "L": 3}


@pytest.fixture(scope="module")
def eng():
    e = ca.Engine(ca.Params(*pp.PRM))
    yield e
    e.close()


def assert_oracle(res, g, group, what, max_msa=pp.MAX_MSA):
    assert int(res.status[g]) == ca.WIN_CONSENSUS, f"{what}: status {int(res.status[g])}"
    exp = pp.oracle_consensus(group, max_msa)
    got = res.consensus(g)
    assert got == exp, f"{what}: consensus of {len(got)} bases differs from the oracle's of {len(exp)}"


# ---- 1. every tier by shape ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def alone(eng):
    """Every probe alone in its batch: its result, the batch counters and tier X's."""
    out = {}
    for name in pp.SHAPES:
        res = eng.poa([pp.probe(name)])
        c, p = eng.profile()
        out[name] = (res, c.copy(), p.copy(), eng.tier_x_counters())
    return out


@pytest.mark.parametrize("name", list(pp.SHAPES))
def test_probe_of_every_tier_equals_the_oracle_and_ran_in_the_tier_the_rule_names(alone, name):
    longest, members = pp.SHAPES[name]
    res, c, p, x = alone[name]
    first, last = pp.route(members, longest), pp.last_tier(members, longest)
    print(f"{name}: routed to {first}, needs {last}; n_tier {c[N_TIER:N_TIER + 6]}, n_over {c[N_OVER:N_OVER + 6]}, tier X {x}, consensus {int(res.cons_len[0])}")
    assert_oracle(res, 0, pp.probe(name), name)
    assert int(c[0]) == 1, f"{name}: {int(c[0])} tasks"  # one group, one task
    if first == "S":  # tier S has no list: it takes the tasks no list holds, and its phases have cycles
        assert not c[N_TIER:N_TIER + 6].any() and p[PS_POA + 1] > 0, (c[N_TIER:N_TIER + 6], p[PS_POA:PS_POA + 5])
    else:
        assert int(c[N_TIER + LIST_OF[first]]) == 1, f"{name}: n_tier {c[N_TIER:N_TIER + 6]}"
    if last in ("G", "X"):  # members beyond tier L's 1 023 bases: handed to tier G
        assert int(c[N_OVER + 4]) >= 1, f"{name}: n_over {c[N_OVER:N_OVER + 6]}"
    if last == "X":  # ... beyond tier G's 2 047: on to tier X, which aligns it
        assert x["routed"] >= 1 and x["done"] == x["routed"] and x["stopped"] == 0, x
    else:
        assert x["routed"] == 0, x


# ---- 2. composition -----------------------------------------------------------------------------------------------------------------------------

def mixed_batch(order_seed):
    groups = [(name, pp.probe(name)) for name in pp.SHAPES] + [(f"q{i}", pp.q_group(i)) for i in range(200)]
    random.Random(order_seed).shuffle(groups)
    return groups


@pytest.fixture(scope="module")
def mixed(eng):
    """The probes and 200 tier-Q groups in one batch, in two orders: name -> consensus bytes, per order."""
    out = []
    for seed in (1, 2):
        groups = mixed_batch(seed)
        res = eng.poa([g for _, g in groups])
        assert (res.status == ca.WIN_CONSENSUS).all(), np.flatnonzero(res.status != ca.WIN_CONSENSUS)
        out.append({name: res.consensus(i) for i, (name, _) in enumerate(groups)})
    return out


def test_a_groups_bytes_do_not_depend_on_the_batch(alone, mixed):
    assert [n for n, _ in mixed_batch(1)] != [n for n, _ in mixed_batch(2)]
    assert mixed[0] == mixed[1]
    for name in pp.SHAPES:
        assert mixed[0][name] == alone[name][0].consensus(0), name
    for i in range(200):
        assert mixed[0][f"q{i}"] == pp.oracle_consensus(pp.q_group(i)), f"q{i}"


# ---- 3. edges -----------------------------------------------------------------------------------------------------------------------------------

def edge_groups():
    rng = random.Random(0xED6E)
    same = pp.rand_seq(rng, 70)
    third = pp.noisy_group(0xE1, 80, 5)
    return {
        "empty group": [],
        "one member": [pp.rand_seq(rng, 333)],
        "only empty sequences": ["", "", ""],
        "backbone is the third": ["", ""] + third,
        "twelve identical members": [same] * 12,
        "two unrelated members": [pp.rand_seq(rng, 90), pp.rand_seq(rng, 75)],
        "homopolymers of unequal length": ["A" * n for n in (40, 37, 44, 40, 31, 52)],
        "300 members of 20 bases": pp.noisy_group(0xE2, 20, 300),
        "300 members of 8 bases": pp.noisy_group(0xE3, 8, 300),  # this one the rule does send to tier Q, which hands a task of more than 255 members on
    }


@pytest.mark.parametrize("name", list(edge_groups()))
def test_edges_of_the_group_semantics(eng, name):
    group = edge_groups()[name]
    res = eng.poa([group])
    assert_oracle(res, 0, group, name)
    if not any(group):
        assert int(res.cons_len[0]) == 0
    if name == "one member":
        assert res.consensus(0) == group[0]
    if name == "backbone is the third":
        assert res.consensus(0) == oracle_lib.oracle_poa(group[2:])
    if name == "300 members of 8 bases":
        c, _ = eng.profile()
        assert int(c[N_TIER + 0]) == 1 and int(c[N_OVER + 0]) == 1, (c[N_TIER:N_TIER + 6], c[N_OVER:N_OVER + 6])  # routed to tier Q, handed on by it


def test_max_msa_takes_the_first_non_empty_members():
    group = pp.noisy_group(0xE4, 60, 12)
    group = group[:2] + [""] + group[2:]  # the empty one does not count
    e = ca.Engine(ca.Params(9, 4, 8, 2, 5))
    try:
        res = e.poa([group])
    finally:
        e.close()
    assert len(pp.aligned_members(group, 5)) == 5 and pp.aligned_members(group, 5)[2] == group[3]
    assert_oracle(res, 0, group, "max_msa 5 of twelve", max_msa=5)
    assert res.consensus(0) != pp.oracle_consensus(group), "the probe cannot tell five members from twelve"


# ---- 4. stops are the group's own -----------------------------------------------------------------------------------------------------------------

class DeviceRun:
    """One batch through cw_poa_run_device: torch device tensors in, the whole consensus buffer (filled with 0xEE before the run) and lengths / statuses back."""

    def __init__(self, eng, hb, slot_bytes=None):
        import torch

        dev = torch.device("cuda", eng.device)

        def up(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

        res = alloc_poa_results(hb, slot_bytes)
        G, total = hb.n_windows, int(res.cons_off[-1])
        t_in = (up(hb.win_first_seq, np.int32), up(hb.seq_len, np.int32), up(hb.seq_word_off, np.int64), up(np.concatenate([hb.bases, np.zeros(4, np.uint32)]), np.int32))
        t_cons = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device=dev)
        t_off, t_len, t_st = up(res.cons_off, np.int64), torch.zeros(G, dtype=torch.int32, device=dev), torch.full((G,), 255, dtype=torch.uint8, device=dev)
        b = Batch(G, len(hb.seq_len), len(hb.bases), t_in[0].data_ptr(), t_in[1].data_ptr(), t_in[2].data_ptr(), t_in[3].data_ptr())
        r = Result(t_cons.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), t_st.data_ptr(), None, None, None)
        torch.cuda.synchronize(dev)  # the engine launches on its own stream: torch's fills above must have landed
        eng.poa_device(b, r)
        torch.cuda.synchronize(dev)
        self.cons_off, self.cons, self.cons_len, self.status = res.cons_off, t_cons.cpu().numpy(), t_len.cpu().numpy().view(np.uint32), t_st.cpu().numpy()

    def slot(self, g):
        return self.cons[int(self.cons_off[g]) : int(self.cons_off[g + 1])]

    def consensus(self, g):
        return self.slot(g)[: int(self.cons_len[g])].tobytes().decode()


def test_a_member_beyond_the_last_tier_stops_its_group_only(eng, alone):
    names = ["24x12", "100x10", "900x6"]
    long_group = [pp.rand_seq(random.Random(0x4200), pp.POAX_LC + 105), "ACGTACGT"]
    groups = [pp.probe(names[0]), long_group, pp.probe(names[1]), pp.probe(names[2])]
    res = eng.poa(groups)
    assert int(res.status[1]) == ca.WIN_OVERFLOW and int(res.cons_len[1]) == 0
    assert int(eng.win_info(4)[1, 15]) == WHY_POA
    for g, name in ((0, names[0]), (2, names[1]), (3, names[2])):
        assert int(res.status[g]) == ca.WIN_CONSENSUS and res.consensus(g) == alone[name][0].consensus(0), name


def test_a_slot_too_small_is_a_stop_and_nothing_is_written_beyond_it(eng, alone):
    clean = [pp.rand_seq(random.Random(0xC1EA), 120)] * 6  # six identical members: the consensus is the member
    groups = [pp.probe("24x12"), clean, pp.probe("100x10")]
    hb = ca.pack_piles(groups)
    slots = [int(poa_slot_bytes(24)), 119, int(poa_slot_bytes(100))]  # the clean group's: its longest member - 1
    d = DeviceRun(eng, hb, np.array(slots))
    assert int(d.status[1]) == ca.WIN_OVERFLOW and int(d.cons_len[1]) == 0
    assert int(eng.win_info(3)[1, 15]) == WHY_OUT_CONS
    assert (d.slot(1) == 0xEE).all(), "the stopped group's slot was written to"
    for g, name in ((0, "24x12"), (2, "100x10")):
        assert int(d.status[g]) == ca.WIN_CONSENSUS and d.consensus(g) == alone[name][0].consensus(0), name
        assert (d.slot(g)[int(d.cons_len[g]) :] == 0xEE).all(), f"{name}: bytes behind the consensus were written"
    assert (d.cons[int(d.cons_off[-1]) :] == 0xEE).all(), "bytes behind the last slot were written"
    d2 = DeviceRun(eng, hb, np.array([slots[0], 120, slots[2]]))  # a slot of exactly the consensus: it fits
    assert int(d2.status[1]) == ca.WIN_CONSENSUS and d2.consensus(1) == clean[0]


# ---- 5. both entry points, one engine ---------------------------------------------------------------------------------------------------------------

def test_both_entry_points_and_window_runs_alternate_on_one_engine():
    groups = [g for _, g in mixed_batch(3)[:40]] + [[], [pp.rand_seq(random.Random(5), 50)]]
    hb = ca.pack_piles(groups)
    prm = ca.Params(9, 4, 8, 2, 150)
    e = ca.Engine(prm)
    try:
        host = e.poa(hb)
        first = [(int(host.status[g]), host.consensus(g)) for g in range(len(groups))]
        d = DeviceRun(e, hb)
        assert [(int(d.status[g]), d.consensus(g)) for g in range(len(groups))] == first
        piles = synth_host(ca.SynthSpec.pacbio(24, 30))
        got = e.run(piles)
        exp, _ = oracle_lib.oracle_run(prm, piles)
        for w in range(piles.n_windows):
            assert got.status[w] == exp.status[w] and got.consensus(w) == exp.consensus(w) and np.array_equal(got.solid_kmers(w), exp.solid_kmers(w)), w
        again = e.poa(hb)
        assert [(int(again.status[g]), again.consensus(g)) for g in range(len(groups))] == first
        assert set(e.timings()) >= {"poa_tasks", "poa_q", "poa", "poa_m1", "poa_m2", "poa_large", "poa_overflow", "poa_gather", "total"}, e.timings()
    finally:
        e.close()
    for g, group in enumerate(groups):
        assert first[g] == (ca.WIN_CONSENSUS, pp.oracle_consensus(group, 150)), g


# ---- 6. refused before anything is launched ---------------------------------------------------------------------------------------------------------

def test_solid_fields_and_oversized_batches_are_invalid(eng):
    hb = ca.pack_piles([pp.probe("24x12")])
    ok = eng.poa(hb)
    stages = eng.timings()
    res = alloc_poa_results(hb)
    b = hb.c_struct()
    dummy = np.zeros(4, np.uint64)
    for solid in ((_ptr(dummy), None, None), (None, _ptr(dummy), None), (None, None, _ptr(dummy)), (_ptr(dummy), _ptr(dummy), _ptr(dummy))):
        r = Result(_ptr(res.cons), _ptr(res.cons_off), _ptr(res.cons_len), _ptr(res.status), *solid)
        assert eng.lib.cw_poa_run(eng.handle, C.byref(b), C.byref(r)) == E_INVALID
        assert eng.lib.cw_poa_run_device(eng.handle, C.byref(b), C.byref(r), None) == E_INVALID
    r = Result(_ptr(res.cons), _ptr(res.cons_off), _ptr(res.cons_len), _ptr(res.status), None, None, None)
    big = Batch(eng.max_batch_windows() + 1, b.n_seqs, b.n_words, b.win_first_seq, b.seq_len, b.seq_word_off, b.bases)  # refused by its count alone: nothing is read
    assert eng.lib.cw_poa_run(eng.handle, C.byref(big), C.byref(r)) == E_INVALID
    assert eng.lib.cw_poa_run_device(eng.handle, C.byref(big), C.byref(r), None) == E_INVALID
    assert (res.status == 255).all() and not res.cons.any(), "a refused call wrote results"
    assert eng.timings() == stages, "a refused call launched something"
    assert eng.poa(hb).consensus(0) == ok.consensus(0)
