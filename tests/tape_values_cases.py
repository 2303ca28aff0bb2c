"""Hand-made tapes and boxes at the edges of pipamd_tape_sweep_values, shared by the model's test and the GPU test.  A case
is (cells, nvar, nparm, lo, hi, ctx, edit): an unedited tape has edit None.  Test helper only."""
import tape_cases as tc
import tape_edit_model as te
import tape_sweep_model as sm
import tape_values_model as vm
from tape_cases import MAX64, MIN64
from tape_model import IF

NEGATE = dict(sol_bg=-1, sol_flags=2)


def theta(nparm=1):
    """the list (theta_0)"""
    return tc.leaf([([1] + [0] * nparm, 1)])


def scaled(c, nparm=1):
    """the list (c * theta_0); further columns are ignored"""
    return tc.leaf([([c] + [0] * nparm, 1)])


def lanes(nvar):
    """unknown i = (i + 1) * theta_0 - i: every unknown has its own minimum, maximum and sum"""
    return tc.leaf([([i + 1, -i], 1) for i in range(nvar)])


def leaf_chain(k):
    """k conditions i - theta_1 >= 0 on the LAST of two columns, each with a list of its own,
    (i + 2) theta_0 + theta_1 - i, the last else the list theta_0 + theta_1: the points of a row of the box are each at
    another leaf"""
    cells = []
    for i in range(k):
        cells += [(IF, 0, 0)] + tc.form([0, -1, i]) + tc.leaf([([i + 2, 1, -i], 1)])
    return cells + tc.leaf([([1, 1, 0], 1)])


def halves():
    """one unknown theta_0 / 2, a second theta_0: the first is a fraction at odd points"""
    return tc.leaf([([1, 0], 2), ([1, 0], 1)])


def where_constant():
    """5 wherever theta_0 + theta_1 > 0, NIL at the origin; the context 200 theta_0 - theta_1 >= 0 leaves k 1 .. 200 of
    the box [0,1] x [0,200] outside: the first SOLUTION point is k 201, in the second chunk"""
    cells = tc.iff([-1, -1, 0], tc.nil(), tc.leaf([([0, 0, 5], 1)]))
    return cells, 1, 2, [0, 0], [1, 200], [[1, 200, -1, 0]], None


def two_minima():
    """|theta_0 - 100| below 250, |theta_0 - 400| from there on, over [0, 599]: the minimum 0 at k 100 and at k 400, in
    chunks (and, with a workgroup a chunk, workgroups) 0 and 3"""
    def dist(c):
        return tc.iff([1, -c], tc.leaf([([1, -c], 1)]), tc.leaf([([-1, c], 1)]))
    return tc.iff([1, -250], dist(400), dist(100)), 1, 1, [0], [599], (), None


def results(case, bits):
    """the model's per-point results of a case"""
    cells, nvar, nparm, lo, hi, ctx, edit = case
    if edit is None:
        return sm.sweep(cells, nvar, nparm, 0, lo, hi, ctx, bits)[0]
    cols = te.point_cols(nparm, edit)
    assert len(lo) == cols
    return sm.apply_context(sm.box_points(lo, hi), ctx, nvar, 0,
                            lambda p: te.evaluate_cells(cells, nvar, nparm, 0, [p], edit, bits)[0])


def summary(case, bits):
    return vm.summarise(results(case, bits), case[1])


# ---- the edges, by name: (case, the widths it is for)
def edges():
    c120, c126 = 1 << 120, 1 << 126
    out = {
        "int64 top": ((theta(), 1, 1, [MAX64 - 299], [MAX64], (), None), (64, 128)),
        "int64 bottom": ((theta(), 1, 1, [MIN64], [MIN64 + 299], (), None), (64, 128)),
        "negate at MIN64": ((theta(), 1, 1, [MIN64], [MIN64 + 2], (), NEGATE), (64,)),
        "halves": ((halves(), 2, 1, [-7], [135], (), None), (64, 128)),
        "range leaves 128 bits": ((scaled(c120), 1, 1, [126], [129], (), None), (128,)),
    }
    for sign, c in (("+", 1), ("-", -1)):
        out[f"{sign}2^120 theta"] = ((scaled(c * c120), 1, 1, [1], [127], (), None), (128,))
        out[f"{sign}2^126, a column ignored"] = ((scaled(c * c126, 2), 1, 2, [1, 0], [1, 256], (), None), (128,))
    return out
