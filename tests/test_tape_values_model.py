"""tests/tape_values_model.py held to the reference and to closed forms: its figures over the golden grid [0,9]^2 of
tests/golden/tape_eval equal a direct reduction, written here, of the reference's recorded answers; at the edges of
tests/tape_values_cases.py they are the sums, minima and maxima one can write down.  Host only, Python ints only."""
import pytest

import tape_cases as tc
import tape_model as tm
import tape_sweep_model as sm
import tape_values_cases as vc
import tape_values_model as vm
from tape_cases import MAX64, MIN64


@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("name", ["int", "rat"])
def test_golden_box_is_a_reduction_of_the_recorded_answers(name, bits):
    g = tc.golden()
    cells = tc.cells_from_text(g["tapes"][name])
    res, summary = vm.sweep(cells, g["nvar"], g["nparm"], 0, [0, 0], [9, 9], (), bits)
    answers = g["answers"][name]
    assert tc.answers_of(res) == answers and len(answers) == 100
    solved = [k for k, a in enumerate(answers) if a is not None]
    assert summary["counts"] == {"solution": len(solved), "nil": 100 - len(solved), "range": 0, "outside": 0}
    assert summary["first"]["solution"] == solved[0] and len(summary["unknowns"]) == g["nvar"]
    for i, rec in enumerate(summary["unknowns"]):
        ints = [(answers[k][i][0], k) for k in solved if answers[k][i][1] == 1]
        fracs = [k for k in solved if answers[k][i][1] > 1]
        assert rec["n_int"] == len(ints) and rec["n_frac"] == len(fracs) and rec["n_unbounded"] == 0
        assert rec["n_int"] + rec["n_frac"] == len(solved)
        vals = [v for v, _ in ints]
        assert rec["sum"] == sum(vals) and rec["min"] == min(vals) and rec["max"] == max(vals)
        assert rec["k_min"] == min(k for v, k in ints if v == min(vals))
        assert rec["k_max"] == min(k for v, k in ints if v == max(vals))
    assert (sum(r["n_frac"] for r in summary["unknowns"]) > 0) == (name == "rat")
    w = vm.words(summary)
    assert len(w) == 8 + 16 * g["nvar"] and w[:8] == sm.words(sm.summarise(res, tm.check(cells, g["nvar"], g["nparm"])["leaves"]))[:8]


def test_int64_edges_need_the_second_limb():
    top = vc.summary(vc.edges()["int64 top"][0], 64)["unknowns"][0]
    assert top == {"n_int": 300, "n_frac": 0, "n_unbounded": 0, "min": MAX64 - 299, "k_min": 0, "max": MAX64, "k_max": 299,
                   "sum": 300 * MAX64 - 299 * 300 // 2}
    bottom = vc.summary(vc.edges()["int64 bottom"][0], 64)["unknowns"][0]
    assert bottom["sum"] == 300 * MIN64 + 299 * 300 // 2 and (bottom["min"], bottom["max"]) == (MIN64, MIN64 + 299)
    assert top["sum"] > MAX64 and bottom["sum"] < MIN64
    zero = dict.fromkeys(("solution", "nil", "range", "outside"), 0)
    w = vm.words({"counts": zero, "first": zero, "unknowns": [top, bottom]})
    # 300 (2^63 - 1) - 44850 = 150 * 2^64 - 45150; 300 * -2^63 + 44850 = -150 * 2^64 + 44850
    assert w[8 + 4:8 + 6] == [MAX64 - 299, 0] and w[8 + 10:8 + 13] == [-45150, 149, 0]
    assert w[24 + 4:24 + 6] == [MIN64, -1] and w[24 + 10:24 + 13] == [44850, -150, -1]      # sign-extended
    # the limbs say the number
    from piplib_amd.engine import values_summary
    assert values_summary(w, 2)["unknowns"] == [top, bottom]


def test_negate_at_min64_is_range_and_in_no_record():
    case = vc.edges()["negate at MIN64"][0]
    res = vc.results(case, 64)
    assert [r[0] for r in res] == [tm.ST_RANGE, tm.ST_SOLUTION, tm.ST_SOLUTION]
    s = vc.summary(case, 64)
    assert s["counts"]["range"] == 1 and s["first"]["range"] == 0
    assert s["unknowns"][0] == {"n_int": 2, "n_frac": 0, "n_unbounded": 0, "min": MAX64 - 1, "k_min": 2, "max": MAX64, "k_max": 1,
                                "sum": 2 * MAX64 - 1}


def test_128_bit_edges_need_the_third_limb():
    e = vc.edges()
    for sign in (1, -1):
        name = "+" if sign > 0 else "-"
        r = vc.summary(e[f"{name}2^120 theta"][0], 128)["unknowns"][0]
        assert r["n_int"] == 127 and r["sum"] == sign * (1 << 120) * 127 * 64 and abs(r["sum"]) > 1 << 128
        assert (r["min"], r["max"]) == ((1 << 120, 127 << 120) if sign > 0 else (-(127 << 120), -(1 << 120)))
        assert (r["k_min"], r["k_max"]) == ((0, 126) if sign > 0 else (126, 0))
        r = vc.summary(e[f"{name}2^126, a column ignored"][0], 128)["unknowns"][0]
        assert r["n_int"] == 257 and r["sum"] == sign * 257 * (1 << 126) and r["k_min"] == r["k_max"] == 0
        assert len(vm._limbs(r["sum"], 3)) == 3 and vm._limbs(r["sum"], 3)[2] == (64 if sign > 0 else -65)
    res = vc.results(e["range leaves 128 bits"][0], 128)
    assert [x[0] for x in res] == [tm.ST_SOLUTION, tm.ST_SOLUTION, tm.ST_RANGE, tm.ST_RANGE]
    r = vc.summary(e["range leaves 128 bits"][0], 128)
    assert r["counts"]["range"] == 2 and r["unknowns"][0]["n_int"] == 2 and r["unknowns"][0]["max"] == 127 << 120


def test_fractions_and_ties():
    s = vc.summary(vc.edges()["halves"][0], 64)
    half, whole = s["unknowns"]
    evens = [t for t in range(-7, 136) if t % 2 == 0]
    assert half["n_int"] == len(evens) and half["n_frac"] == 143 - len(evens) and half["sum"] == sum(t // 2 for t in evens)
    assert (half["min"], half["k_min"], half["max"], half["k_max"]) == (-3, 1, 67, 141)
    assert whole["n_int"] == 143 and whole["n_frac"] == 0 and whole["sum"] == sum(range(-7, 136))
    # a constant: the smallest k among the SOLUTION points, whatever comes before it (k 0 NIL, k 1 .. 200 OUTSIDE)
    res = vc.results(vc.where_constant(), 64)
    assert res[0][0] == tm.ST_NIL and all(r[0] == sm.ST_OUTSIDE for r in res[1:201]) and res[201][0] == tm.ST_SOLUTION
    r = vm.summarise(res, 1)["unknowns"][0]
    assert (r["min"], r["k_min"], r["max"], r["k_max"], r["n_int"], r["sum"]) == (5, 201, 5, 201, 201, 1005)
    # a minimum attained twice: the smaller k
    r = vc.summary(vc.two_minima(), 64)["unknowns"][0]
    assert (r["min"], r["k_min"], r["max"], r["k_max"], r["n_int"]) == (0, 100, 199, 599, 600)
    # decreasing: the minimum is at the last point
    r = vm.summarise(sm.sweep(vc.scaled(-3), 1, 1, 0, [0], [299])[0], 1)["unknowns"][0]
    assert (r["min"], r["k_min"], r["max"], r["k_max"]) == (-897, 299, 0, 0)


def test_nothing_to_report_and_the_context():
    zero = vm.empty_record()
    for cells in (tc.nil(), []):
        s = vm.sweep(cells, 2, 1, 0, [0], [9])[1]
        assert s["unknowns"] == [zero, zero] and s["counts"]["nil"] == 10
    s = vm.sweep(vc.theta(), 1, 1, 0, [0], [9], [[1, 0, -1]])[1]      # every point outside
    assert s["unknowns"] == [zero] and s["counts"]["outside"] == 10 and s["first"]["outside"] == 0
    assert vm.sweep(tc.leaf([]), 0, 1, 0, [0], [9])[1] == {"counts": {"solution": 10, "nil": 0, "range": 0, "outside": 0},
                                                          "first": {"solution": 0, "nil": -1, "range": -1, "outside": -1}, "unknowns": []}
    s = vm.sweep(tc.leaf([([7], 1)]), 1, 0, 0, [], [])[1]              # no columns: one point
    assert s["unknowns"][0] == dict(zero, n_int=1, min=7, max=7, k_min=0, k_max=0, sum=7)
    # OUTSIDE points count in k and in nothing else
    s = vm.sweep(vc.theta(), 1, 1, 0, [0], [9], [[1, 1, -4]])[1]
    assert s["unknowns"][0] == dict(zero, n_int=6, min=4, k_min=4, max=9, k_max=9, sum=39)
    assert vm.words(s)[8:24] == [6, 0, 0, 0, 4, 0, 4, 9, 0, 9, 39, 0, 0, 0, 0, 0]


def test_plan_arithmetic():
    info = {"leaves": 7, "ifs": 6, "news": 0, "words": 40, "slots": 3, "depth": 4, "staged": 1}
    assert vm.plan(info, 64, 3, 2, [0, 0], [9, 9]) == {"n_points": 100, "summary_words": 56, "work_bytes": 96 * 3 * 2, "staged": 1}
    assert vm.plan(info, 64, 0, 0, [], []) == {"n_points": 1, "summary_words": 8, "work_bytes": 0, "staged": 1}
    assert vm.plan(info, 64, 64, 1, [0], [128 * 2048])["work_bytes"] == 96 * 64 * 2 * 2048 == 24 << 20
    assert vm.plan(info, 64, 1, 1, [0], [128 * 2047 - 1])["work_bytes"] == 96 * 2 * 2047
    for nvar, lo, hi, code in ((65, [0], [9], tm.E_TOOLARGE), (-1, [0], [9], tm.E_INVALID), (65, [1], [0], tm.E_INVALID),
                               (3, [MIN64], [MAX64], tm.E_TOOLARGE)):
        with pytest.raises(tm.TapeError) as e:
            vm.plan(info, 64, nvar, 1, lo, hi)
        assert e.value.code == code
    assert vm.staged(dict(info, staged=0), 64) == 0 and vm.staged(dict(info, words=0), 64) == 0
    assert vm.staged(dict(info, words=(65536 - 256 * 8) // 8), 64) == 1 and vm.staged(dict(info, words=(65536 - 256 * 8) // 8 + 1), 64) == 0
