"""The finish kernel's probe catalogue (tests/finish_probes.py) on the CPU: every probe's expected string and walk statistics are computed without the
kernel -- raw consensus from the plain chain reference and the oracle's POA, counts from numpy, weighting and polish from oracle_weight_polish -- and held
against oracle_run and against the plain Python walk; its designed numbers and its hand-written route are asserted from the header's constants; and
every table, count and bitmap road is shown to have probes whose answer depends on the polish.  A probe that misses its edge fails here, before
tests/test_gpu_finish.py runs it."""
import os
import re

import pytest

import consent_amd as ca
import finish_probes
import oracle_lib
from consent_amd import engine
from finish_probes import BY_NAME, FIN, PROBES, check_designed, route_from_constants
from index_probes import str2num

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
read = lambda *path: open(os.path.join(ROOT, *path)).read()


def sensitive(p):
    """A link succeeded and changed the string."""
    r = p.ref
    return r.walk.linked and r.link_calls > 0 and r.polished.upper() != r.weighted.upper()


@pytest.mark.parametrize("probe", PROBES, ids=repr)
def test_oracle_and_walk_agree_with_the_reference(probe):
    r = probe.ref
    assert int(r.oracle.status[0]) == (ca.WIN_CONSENSUS if r.has_chain else ca.WIN_TEMPLATE), probe
    assert r.oracle.consensus(0) == r.polished, f"{probe}: oracle_run's consensus is not the polish of the reference's raw consensus"
    assert r.walk.string == r.polished, f"{probe}: the Python walk spells another string than oracle_weight_polish"
    assert (r.walk.link_calls, r.walk.nbr_calls) == (r.link_calls, r.nbr_calls), f"{probe}: the walk counts {r.walk.link_calls} frames and {r.walk.nbr_calls} calls, the oracle {r.link_calls} and {r.nbr_calls}"


@pytest.mark.parametrize("probe", PROBES, ids=repr)
def test_probe_has_its_designed_numbers_and_route(probe):
    check_designed(probe)
    r = probe.ref
    names = route_from_constants(probe.prm[0], r.n_solid, r.max_count, len(r.raw), r.walk)
    assert probe.route_names == names, f"{probe}: the catalogue says {probe.route_names}, the constants and the walk {names}"
    # the side of each bound the route names, said once more in numbers
    k = probe.prm[0]
    if len(r.raw) >= k and r.has_chain:
        assert ("staged" in names) == (r.n_solid <= FIN["SKEYS"])
        assert ("compact" in names) == (FIN["SKEYS"] < r.n_solid <= FIN["K16_MAX"] and k <= 9)
        assert ("vis_global" in names) == (r.n_solid > 32 * FIN["VIS_WORDS"])
        assert ("cnt16" in names) == (r.n_solid <= FIN["SKEYS"] and r.max_count <= 65535)
    assert ("second_pass" in names) == (len(r.raw) > FIN["CB"] or r.walk.longest > FIN["CB"])
    assert max(len(r.raw), r.walk.longest, len(r.polished)) <= FIN["CB_BIG"]


def test_probe_names_are_unique():
    assert len({p.name for p in PROBES}) == len(PROBES)


def test_every_route_bit_has_a_probe():
    """... but `count_scan`, which no valid window reaches: a zone is k + 3 upper-case characters, a character the weighting leaves upper-case starts a solid
    k-mer, and everything the polish writes before it reads another zone keeps that true (a head extension writes the first letter of a solid
    predecessor; a link's path is solid k-mers, begins with the source anchor and ends with the destination anchor, so the k-mers across its two ends
    are the ones that were there).  walk() looks all eight zone k-mers up at every weak region: no probe meets one below the threshold (900 noisy piles at
    k = 5 .. 7 were tried as well).  The GPU test asserts the bit stays clear in every probe."""
    seen = set()
    for p in PROBES:
        seen.update(p.route_names)
    assert seen == set(engine.FINISH_ROUTE) - {"count_scan"}
    assert not any(p.ref.walk.scan for p in PROBES)


ROADS = ("staged", "compact", "global", "cnt16", "cnt_global", "vis_lds", "vis_global")


@pytest.mark.parametrize("road", ROADS)
def test_every_road_has_probes_whose_answer_depends_on_the_polish(road):
    """At least two probes per table, count and bitmap road in which a link succeeded and changed the string, one of them with twenty getNeighbours calls or more."""
    on = [p for p in PROBES if road in p.route_names and sensitive(p)]
    assert len(on) >= 2, (road, on)
    assert max(p.ref.nbr_calls for p in on) >= 20, (road, [(p, p.ref.nbr_calls) for p in on])


TIES = [p for p in PROBES if p.designed.get("tie")]


def test_tie_probes_cover_the_three_tables():
    assert {n for p in TIES for n in p.route_names} >= {"staged", "compact", "global"}


@pytest.mark.parametrize("probe", TIES, ids=repr)
def test_tie_probe_depends_on_the_tie(probe):
    """The walk met successors with equal counts, and anchor pairs with equal sums; the expected string changes when the loser of a tie has its count raised by one."""
    r = probe.ref
    k, solid = probe.prm[:2]
    assert r.walk.ties and r.walk.pair_ties
    changed = 0
    for _, loser in r.walk.ties:
        bumped = dict(r.counts)
        bumped[str2num(loser)] += 1
        changed += oracle_lib.oracle_weight_polish(r.raw, bumped, k, solid) != r.polished
    assert changed >= 1, probe


def test_the_allele_wins_or_loses_by_generation_order():
    """The two staged tie probes differ in the allele's letter alone: where it comes before the truth's in A, C, G, T the polished string spells the allele."""
    first, second = BY_NAME["tie, the truth's letter first"], BY_NAME["tie, the allele's letter first"]
    for p, spells_allele in ((first, False), (second, True)):
        truth, allele = p.pile[1], p.pile[3]
        assert p.ref.polished.upper() == (allele if spells_allele else truth), p


def test_sixteen_bit_probe_depends_on_the_high_bits():
    """poly-A 65536: with every count truncated to 16 bits the expected string changes (A x9 is no longer the best successor); poly-A 65535 fits and does not."""
    for name, changes in (("poly-A 65536", True), ("poly-A 65535", False)):
        p = BY_NAME[name]
        r = p.ref
        assert bool(p.designed.get("truncation")) == changes
        cut = {key: c & 0xFFFF for key, c in r.counts.items()}
        assert (oracle_lib.oracle_weight_polish(r.raw, cut, *p.prm[:2]) != r.polished) == changes, p


def test_header_constants_are_the_kernels():
    """FIN is read out of cw_finish.h; the policy constants the Python walk uses are include/cw_policy.h's; the compact table's bound is what its comment says."""
    pol = read("include", "cw_policy.h")
    define = lambda n: int(re.search(rf"#define {n}\s+(\d+)", pol).group(1))
    assert (finish_probes.ZONE, finish_probes.MAX_BRANCHES, finish_probes.MAX_ANCHORS) == (define("CW_DBG_ZONE"), define("CW_DBG_MAX_BRANCHES"), define("CW_DBG_MAX_ANCHORS"))
    assert FIN["K16_MAX"] == (FIN["VIS_WORDS"] + FIN["SKEYS"]) * 32 // 17 // 64 * 64 and FIN["SKEYS"] < FIN["K16_MAX"] < 32 * FIN["VIS_WORDS"]
    assert FIN["CB"] < FIN["CB_BIG"]


def test_route_table_is_the_kernels():
    """consent_amd/engine.py FINISH_ROUTE names the bits of csrc/cw_finish.h's CwFinRoute, FINISH_ROUTE_SLOT is CW_PS_FIN_ROUTE and the two counters follow it."""
    hdr = read("consent_amd", "csrc", "cw_finish.h")
    bits = {m.group(1).lower(): 1 << int(m.group(2)) for m in re.finditer(r"CW_FR_(\w+) = 1u << (\d+)", hdr)}
    assert bits == engine.FINISH_ROUTE
    dev = read("consent_amd", "csrc", "cw_device.h")
    slot = lambda n: int(re.search(rf"{n} = (\d+)", dev).group(1))
    assert (slot("CW_PS_FIN_ROUTE"), slot("CW_PS_FIN_LINKS"), slot("CW_PS_FIN_NBRS")) == (engine.FINISH_ROUTE_SLOT, engine.FINISH_ROUTE_SLOT + 1, engine.FINISH_ROUTE_SLOT + 2)
