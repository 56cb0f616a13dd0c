"""CPU: the plain restatement of the tier sort's class (tests/handoff_ref.py sort_class, csrc/cw_poa.h cw_sort_class) at its boundaries, every expected
class worked out by hand from the rule: tier Q's and H's lists go by member-count class x 16 + length step, largest first (127 - ...), tier Q's short half
128 higher; tier M1 by the depth-aware node estimate in steps of four; tiers M2 and L by eighths of an octave of members^2 x mean length above 2^13."""
import pytest

from handoff_ref import is_short, member_class, sort_class


def test_member_count_classes_step_at_4_8_12_16_24_32_64():
    assert [member_class(n) for n in (2, 3, 4, 7, 8, 11, 12, 15, 16, 23, 24, 31, 32, 63, 64, 150)] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7]
    # tier Q's list, a longest member of 20 bases (long half: step 10): 127 - (16 mc + 10)
    got = [sort_class(n, 20, 20, 0) for n in (3, 4, 7, 8, 11, 12, 15, 16, 23, 24, 31, 32, 63, 64)]
    assert got == [117, 101, 101, 85, 85, 69, 69, 53, 53, 37, 37, 21, 21, 5]
    # tier H's list goes by the same member classes (length step 20 >> 2 = 5)
    assert [sort_class(n, 20, 20, 5) for n in (3, 4, 63, 64)] == [122, 106, 26, 10]


def test_lengths_15_16_split_tier_q_in_short_and_long():
    assert is_short(3, 15) and not is_short(3, 16)
    assert sort_class(3, 15, 15, 0) == 128 + 127 - 7  # the short half lies behind all 128 classes of the long one
    assert sort_class(3, 16, 16, 0) == 127 - 8
    assert sort_class(3, 14, 14, 0) == 128 + 127 - 7 and sort_class(3, 13, 13, 0) == 128 + 127 - 6  # steps of two bases
    # a short task is also expected to stay below 36 nodes: ceil(15 (15 + n / 5) / 10) is 35, 36, 38 for 40, 45, 50 members
    assert is_short(40, 15) and is_short(45, 15) and not is_short(50, 15)
    assert sort_class(45, 15, 15, 0) == 128 + 127 - (6 * 16 + 7) and sort_class(50, 15, 15, 0) == 127 - (6 * 16 + 7)


def test_lengths_31_32_and_63_64_clamp():
    assert [sort_class(3, mx, mx, 0) for mx in (29, 30, 31, 32, 40)] == [113, 112, 112, 112, 112]
    assert [sort_class(3, mx, mx, 5) for mx in (31, 32, 62, 63, 64, 100)] == [120, 119, 112, 112, 112, 112]


def test_tier_m1_goes_by_the_node_estimate():
    assert sort_class(10, 100, 90, 1) == 127 - (170 >> 2)  # ceil(100 x 17 / 10) = 170 nodes
    assert sort_class(64, 120, 100, 1) == 127 - (((120 * 27 + 9) // 10) >> 2)
    assert sort_class(150, 255, 255, 1) == 0  # beyond 4 x 127 nodes: the first class


@pytest.mark.parametrize("lst", (2, 3))
def test_cost_octaves_begin_at_2_to_the_13(lst):
    # cost = members^2 x mean length + 1
    assert sort_class(8, 200, 127, lst) == 127   # 8129 < 2^13: the last class
    assert sort_class(8, 200, 128, lst) == 127   # 8193: the octave's first eighth, still the last class
    assert sort_class(8, 200, 144, lst) == 126   # 9217 = 2^13 x 9 / 8
    assert sort_class(8, 300, 255, lst) == 120   # 16321: the last eighth of that octave
    assert sort_class(8, 300, 256, lst) == 119   # 16385: the next octave
    assert sort_class(16, 300, 256, lst) == 103  # 2^16: three octaves up
    assert sort_class(150, 520, 500, lst) == 45  # 11 250 001 = 2^23 x 1.34: 8 x 10 + 2 eighths
    assert sort_class(1000, 1000, 1000, lst) == 0  # clamped
    assert sort_class(8, 128, 0, lst) == sort_class(8, 128, 128, lst)  # no mean recorded: the longest member stands in
