"""The class the tier sort orders a routed list by, restated plainly (csrc/cw_poa.h cw_sort_class), and what the chain kernel's flush is expected to put on
the lists of a batch.  The flush (cw_poa_tasks_kernel in an operator run) computes the class and writes it into the top byte of the list entry; the sort reads
nothing else.  tests/test_handoff_class_cpu.py pins the restatement's boundaries by hand, tests/test_gpu_handoff_lists.py holds the kernels to it."""
from poa_op_probes import route

COST_CLASSES = 128          # CW_SORT_COST_CLASSES: classes of one key, 0 = the largest tasks
Q8_LC, Q8_ROUTE_NODES = 15, 36  # CW_POAQ8_LC, CW_POAQ8_ROUTE_NODES: tier Q's short half (eight tasks to a wave)
LISTS = {"Q": 0, "M1": 1, "M2": 2, "L": 3, "H": 5}


def is_short(n, mx):
    return mx <= Q8_LC and (mx * (15 + n // 5) + 9) // 10 <= Q8_ROUTE_NODES


def member_class(n):
    for c, bound in enumerate((4, 8, 12, 16, 24, 32, 64)):
        if n < bound:
            return c
    return 7


def sort_class(n, mx, mean, lst):
    """Class of a task of n members, the longest of mx bases, mean length `mean` (floor), on list `lst` (0 tier Q's, 1 M1, 2 M2, 3 L, 5 H)."""
    if lst == 0:
        return (COST_CLASSES if is_short(n, mx) else 0) + (COST_CLASSES - 1) - (member_class(n) * 16 + (min(mx, 31) >> 1))
    if lst == 5:
        return (COST_CLASSES - 1) - (member_class(n) * 16 + (min(mx, 63) >> 2))
    if lst == 1:
        c = ((mx * (15 + n // 5) + 9) // 10) >> 2
    else:
        cost = n * n * (mean if mean else mx) + 1
        lg = cost.bit_length() - 1
        frac = (cost >> (lg - 3)) & 7 if lg >= 3 else 0
        c = max(lg * 8 + frac - 8 * 13, 0)  # eighths of an octave above 2^13
    return (COST_CLASSES - 1) - min(c, COST_CLASSES - 1)


def task_numbers(members):
    """(n, longest, mean) of a task's members [(sequence, start, length)] as the flush records them: PoaTask::n_members, max_len = longest | mean << 16."""
    lens = [l for _, _, l in members]
    return len(lens), max(lens), sum(lens) // len(lens)


def expected_lists(ref_tasks):
    """{list name: {key: class}} for tasks {key: members}: where cw_poa_route sends each (tier S has no list) and the class it carries there."""
    out = {name: {} for name in LISTS}
    for key, members in ref_tasks.items():
        n, mx, mean = task_numbers(members)
        tier = route(n, mx)
        if tier != "S":
            out[tier][key] = sort_class(n, mx, mean, LISTS[tier])
    return out
