"""Every fill, walk, replay branch, coded row kind and rc 2 of the slab POA tiers (csrc/cw_poa.h poa_run) against a plain reference.  Every probe of
tests/poa_probes.py -- one group for cw_poa_run, alone in its batch -- gives the consensus of tests/poa_ref.py (written from include/cw_policy.h;
tests/test_poa_ref_cpu.py holds it to the oracle) byte for byte, or the documented stop, on the product library and on the test-aid library; the batch
counters show the tier it was routed to and every hand-over it names; on the test-aid library the route witness (Engine.poa_route) has the bits the probe
states and lacks the ones it excludes.  Then the whole catalogue in one batch, in two orders, against the bytes of each probe alone; and the closing test:
the union of the witnessed bits is every CW_PR_* bit but the ones poa_probes.UNREACHABLE and NOT_PROBED list, each with its reason."""
import random

import pytest

import consent_amd as ca
import poa_op_probes as pp
import poa_probes as cat
from consent_amd import engine
from consent_amd.engine import poa_route_names

pytestmark = pytest.mark.gpu
WHY_POA = 8  # csrc/cw_device.h CW_WHY_POA
N_TIER, N_OVER = 6, 18  # Engine.profile() counters: n_tier[6] from word 6, n_over[6] from word 18 (list 0 = tier Q, 1 M1, 2 M2, 3 L, 4 G)
LIST_OF = {"M1": 1, "M2": 2, "L": 3}
NAMES = list(cat.PROBES)
WITNESSED = {}  # probe -> the 'tier.bit' names the test-aid library reported for it alone


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(which):
        if which not in cache:
            cache[which] = ca.Engine(ca.Params(*pp.PRM))
        want = engine.AIDS_LIB if which == "aids" else engine.lib_path()
        assert cache[which].lib._name == want, (cache[which].lib._name, want)
        return cache[which]

    yield get
    for e in cache.values():
        e.close()


def run_alone(e, name):
    """The probe alone in its batch: the reference's consensus or the stated stop, and the counters of the tiers it names.  Returns its bytes."""
    p = cat.PROBES[name]
    res = e.poa([p.group])
    c, _ = e.profile()
    x = e.tier_x_counters()
    n_tier, n_over = [int(v) for v in c[N_TIER : N_TIER + 6]], [int(v) for v in c[N_OVER : N_OVER + 6]]
    print(f"{name}: status {int(res.status[0])}, consensus {int(res.cons_len[0])}, n_tier {n_tier}, n_over {n_over}, tier X {x}")
    if p.stops:
        assert int(res.status[0]) == ca.WIN_OVERFLOW and int(res.cons_len[0]) == 0, f"{name}: status {int(res.status[0])}"
        assert int(e.win_info(1)[0, 15]) == WHY_POA, name
    else:
        assert int(res.status[0]) == ca.WIN_CONSENSUS, f"{name}: status {int(res.status[0])}, why {int(e.win_info(1)[0, 15])}"
        exp = cat.reference(name)[0]
        got = res.consensus(0)
        assert got == exp, f"{name}: consensus of {len(got)} bases differs from the reference's of {len(exp)}"
    want_tier = [0] * 6
    if p.tiers and p.tiers[0] != "S":  # (tier S has no list: it takes the tasks no list holds)
        want_tier[LIST_OF[p.tiers[0]]] = 1
    assert n_tier == want_tier, f"{name}: n_tier {n_tier}, routed to {p.tiers[:1]}"
    assert n_over[3] == int("L" in p.tiers[1:]) and n_over[4] == int("G" in p.tiers[1:]) and n_over[0] == 0, f"{name}: n_over {n_over}, visits {p.tiers}"
    in_x = int("X" in p.tiers)
    assert (x["routed"], x["done"], x["stopped"]) == (in_x, int(in_x and not p.stops), int(in_x and p.stops)), f"{name}: tier X {x}"
    return (int(res.status[0]), res.consensus(0))


@pytest.fixture(scope="module")
def alone(engines):
    """Every probe alone on the product library, whose kernels hold no witness."""
    e = engines("product")
    out = {}
    for name in NAMES:
        out[name] = run_alone(e, name)
        assert poa_route_names(e.poa_route()) == set(), name
    return out


@pytest.mark.parametrize("name", NAMES)
def test_probe_alone_on_the_product_library(alone, name):
    assert name in alone


@pytest.mark.parametrize("name", NAMES)
def test_probe_and_its_route_on_the_test_aid_library(engines, aids, name):
    p = cat.PROBES[name]
    e = engines("aids")
    run_alone(e, name)
    went = poa_route_names(e.poa_route())
    WITNESSED[name] = went
    print(f"{name}: {sorted(went)}")
    assert p.has <= went, f"{name}: missing {sorted(p.has - went)}; went {sorted(went)}"
    assert not p.lacks & went, f"{name}: has {sorted(p.lacks & went)}, which it must lack"
    elsewhere = {b for b in went if b.split(".")[0] not in p.tiers}
    assert not elsewhere, f"{name}: bits of tiers it does not visit: {sorted(elsewhere)}"
    wrong_rc2 = {b for b in went if ".rc2_" in b} - p.has
    assert not wrong_rc2, f"{name}: hand-overs it does not state: {sorted(wrong_rc2)}"


def test_a_probes_bytes_do_not_depend_on_the_batch(engines, alone):
    """The whole catalogue in one batch, in two orders: every group's status and bytes are those of the group alone -- the stopped groups' neighbours included."""
    e = engines("product")
    orders = []
    for seed in (1, 2):
        names = list(NAMES)
        random.Random(seed).shuffle(names)
        orders.append(names)
        res = e.poa([cat.PROBES[n].group for n in names])
        info = e.win_info(len(names))
        for i, n in enumerate(names):
            assert (int(res.status[i]), res.consensus(i)) == alone[n], f"{n} at {i} of order {seed}"
            assert int(info[i, 15]) == (WHY_POA if cat.PROBES[n].stops else 0), n
        x = e.tier_x_counters()
        assert x["routed"] == sum("X" in p.tiers for p in cat.PROBES.values()) and x["stopped"] == sum("X" in p.tiers and p.stops for p in cat.PROBES.values()), x
    assert orders[0] != orders[1]


def test_every_reachable_bit_is_witnessed_and_no_unreachable_one(engines, aids):
    e = engines("aids")
    for name in NAMES:  # (run alone, this test witnesses the catalogue itself)
        if name not in WITNESSED:
            e.poa([cat.PROBES[name].group])
            WITNESSED[name] = poa_route_names(e.poa_route())
    seen = set().union(*WITNESSED.values())
    by = {b: sorted(n for n, w in WITNESSED.items() if b in w)[:2] for b in seen}
    for b in sorted(seen & set(cat.UNREACHABLE)):
        print(f"{b}: listed as unreachable ({cat.UNREACHABLE[b]}), witnessed by {by[b]}")
    assert not seen & set(cat.UNREACHABLE), sorted(seen & set(cat.UNREACHABLE))
    assert not seen & set(cat.NOT_PROBED), sorted(seen & set(cat.NOT_PROBED))
    reachable = cat.ALL_BITS - set(cat.UNREACHABLE) - set(cat.NOT_PROBED)
    assert seen == reachable, f"never witnessed: {sorted(reachable - seen)}"
    for b in sorted(reachable):  # ... and by a probe that names it: its consensus is the reference's
        assert any(b in cat.PROBES[n].has for n in by[b]) or any(b in p.has and b in WITNESSED[p.name] for p in cat.PROBES.values()), b
