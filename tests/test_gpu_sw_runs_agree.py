"""The alignment operator's four runs on one batch (cw_sw_run, cw_sw_path_run, cw_pileup_run, cw_sw_cut_run): all four share one pair-claim loop per launch
shape (csrc/cw_sw_op.h), and the three traced runs' pair bodies (sw_path_pair, pile_pair, cut_pair) are copies of one another up to the closed walk, so their
rows are one set of rows -- whichever run wrote them and whatever ran on the engine before.  This is what keeps the copies in step."""
import numpy as np
import pytest

import consent_amd as ca
import sw_op_probes as sp
import sw_path_probes as pp
from consent_amd.engine import SW_QUERY_END, SW_ROW, SW_SCORE, SW_STATUS

pytestmark = pytest.mark.gpu
WINDOW = 500


def one_of_each():
    """A pair of every launch class, a pair where nothing aligns, an empty query, a reference alone: (groups, the sequences that reach an alignment kernel)."""
    pairs = [pp.class_pairs()["q640xr600"], pp.class_pairs()["q2048xr600"], pp.long_pairs()["q2100xr3000"]]
    assert [len(q) for q, _ in pairs] == [640, 2048, 2100]  # class 0's longest, class 1's longest, class 2
    nothing = sp.nothing_pairs()
    pairs += [nothing["poly-A against poly-C"], nothing["empty query"]]
    groups = [[ref, query] for query, ref in pairs] + [[pairs[0][1]]]
    return groups, [1, 3, 5]


def test_the_four_runs_write_the_same_rows_in_either_order():
    groups, aligned = one_of_each()
    e = ca.Engine(ca.Params(*sp.PRM))
    try:
        rows = {"path": e.sw_path(groups).rows.copy(), "pileup": e.pileup(groups).rows.copy(), "cut": e.sw_cut(groups, WINDOW).rows.copy()}
        plain = e.sw(groups, want_indels=True).rows.copy()
        again = {"cut": e.sw_cut(groups, WINDOW).rows.copy(), "path": e.sw_path(groups).rows.copy(), "pileup": e.pileup(groups).rows.copy()}
    finally:
        e.close()
    want = rows["path"]
    assert want.shape == (11, SW_ROW)
    # full-size slots: no slot code, so the status column is compared with the rest
    assert set(want[:, SW_STATUS]) <= {ca.SW_ALIGNED, ca.SW_IS_REF}, want[:, SW_STATUS]
    assert [s for s in range(len(want)) if want[s, SW_SCORE] > 0] == aligned  # three pairs reach the alignment kernels, one of each class
    assert (want[9] == [0, 0, -1, 0, -1, 0, 0, ca.SW_ALIGNED]).all() and (want[10] == [0, 0, -1, 0, -1, 0, 0, ca.SW_IS_REF]).all()  # the empty query; the reference alone
    for name in ("pileup", "cut"):
        assert np.array_equal(rows[name], want), f"{name} run: rows differ from the path run's at {np.flatnonzero((rows[name] != want).any(axis=1))}"
    for name, got in again.items():
        assert np.array_equal(got, want), f"{name} run, second order: rows differ at {np.flatnonzero((got != want).any(axis=1))}"
    ends = slice(SW_SCORE, SW_QUERY_END + 1)
    assert np.array_equal(plain[:, ends], want[:, ends]), f"score and ends differ from the plain run's at {np.flatnonzero((plain[:, ends] != want[:, ends]).any(axis=1))}"
