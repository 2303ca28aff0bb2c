"""-m gpu: engine.Tape.sweep_values -- over a box, per unknown the counts, the minimum and the maximum with the smallest k
that attains them and the exact sum, reduced on the device in two stages (pipamd_tape_sweep_values,
pip_tape_values_kernel and pip_tape_values_fold_kernel of csrc/pip_tape.hip), both cell widths.

Authorities: the reference's recorded answers on the golden grid (tests/golden/tape_eval/p5_grid.json);
pipamd_tape_sweep's head words and per-point arrays; tests/tape_values_model.py (held to the reference and to closed forms
by tests/test_tape_values_model.py) on the cases of tests/tape_values_cases.py.  Every word of every summary is compared;
no point is left out of any comparison."""
import ctypes as C

import numpy as np
import pytest

import tape_cases as tc
import tape_model as tm
import tape_sweep_model as sm
import tape_values_cases as vc
import tape_values_model as vm
from tape_cases import MAX64, MIN64
from test_gpu_tape_edit import family, solved
from test_gpu_tape_eval import _engine, _ints, _solve_p5
from test_gpu_tape_sweep import P5_CONTEXT, set_blocks

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]


def words_of(tensor):
    import torch
    torch.cuda.synchronize()
    return [int(v) for v in tensor.cpu().tolist()]


def hold(case, bits, want=None):
    """sweep_values of a case on the device: every word is the model's, the head words are pipamd_tape_sweep's bit for
    bit, and values_summary decodes to the model's dict.  Returns the model's summary."""
    from piplib_amd import engine as eng
    cells, nvar, nparm, lo, hi, ctx, edit = case
    t = eng.Tape(_engine(), cells, nvar, nparm, 0, bits, edit=edit)
    plan = t.values_plan(lo, hi)
    assert plan == vm.plan(t.info, bits, nvar, t.point_cols, lo, hi)
    got = t.sweep_values(lo, hi, ctx=(ctx if len(ctx) else None))
    head, _ = t.sweep(lo, hi, ctx=(ctx if len(ctx) else None), outputs=())
    got_words, head_words = words_of(got), words_of(head)
    t.close()
    want = want if want is not None else vc.summary(case, bits)
    assert len(got_words) == plan["summary_words"] == 8 + 16 * nvar
    assert got_words[:8] == head_words[:8]
    assert got_words == vm.words(want)
    assert eng.values_summary(got, nvar) == want
    assert sum(want["counts"].values()) == plan["n_points"]
    return want


# ---------------------------------------------------------------- 1. the golden box
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("name,nq", [("int", 1), ("rat", 0)])
def test_golden_box(name, nq, bits):
    g = tc.golden()
    cells, _ = _solve_p5(nq, bits)
    case = (cells, g["nvar"], g["nparm"], [0, 0], [9, 9], (), None)
    assert tc.answers_of(vc.results(case, bits)) == g["answers"][name]
    want = hold(case, bits)
    assert (sum(r["n_frac"] for r in want["unknowns"]) > 0) == (name == "rat")


# ---------------------------------------------------------------- 2. a reduction of the sweep's arrays
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("nq", [1, 0])
def test_equals_a_reduction_of_the_sweeps_arrays(nq, bits):
    import torch
    from piplib_amd import engine as eng
    g = tc.golden()
    cells, _ = _solve_p5(nq, bits)
    t = eng.Tape(_engine(), cells, g["nvar"], g["nparm"], 0, bits)
    lo, hi = [-3, -2], [12, 9]
    summary, out = t.sweep(lo, hi, outputs=("status", "x_num", "x_den"))
    got = t.sweep_values(lo, hi)
    torch.cuda.synchronize()
    assert torch.equal(got[:8].cpu(), summary[:8].cpu())
    st, xn, xd = out["status"].cpu().tolist(), _ints(out["x_num"], bits), _ints(out["x_den"], bits)
    assert len(st) == 16 * 12
    want = []
    for i in range(g["nvar"]):
        ints = [(xn[k][i], k) for k in range(len(st)) if st[k] == tm.ST_SOLUTION and xd[k][i] == 1]
        vals = [v for v, _ in ints]
        want.append({"n_int": len(ints), "n_frac": sum(st[k] == tm.ST_SOLUTION and xd[k][i] > 1 for k in range(len(st))),
                     "n_unbounded": 0, "min": min(vals), "k_min": min(k for v, k in ints if v == min(vals)),
                     "max": max(vals), "k_max": min(k for v, k in ints if v == max(vals)), "sum": sum(vals)})
    assert eng.values_summary(got, g["nvar"])["unknowns"] == want
    assert all(w["n_int"] + w["n_frac"] == st.count(tm.ST_SOLUTION) > 100 for w in want)
    t.close()


# ---------------------------------------------------------------- 3. chunk and grid edges
@pytest.mark.parametrize("bits", [64, 128])
def test_chunk_edges(bits):
    for n in (1, 127, 128, 129, 257):
        hold((tc.if_chain(5), 1, 1, [-2], [-2 + n - 1], (), None), bits)


@pytest.mark.parametrize("bits", [64, 128])
def test_grid_sizes_give_the_same_bits(bits):
    """1000 points through 1, 2 and 3 workgroups and the default grid: bit-equal, and the model's.  With one to three
    workgroups a wave takes several chunks in turn -- its accumulators carried from chunk to chunk, the slot rows decoded
    (and, at 128 bits, widened in place) again, a last turn with no live lane -- which no other box of this file asks of it"""
    import torch
    from piplib_amd import engine as eng
    case = (tc.if_chain(5), 1, 1, [-3], [996], (), None)
    t = eng.Tape(_engine(), case[0], 1, 1, 0, bits)
    seen = []
    try:
        for blocks in (1, 2, 3, 0):
            set_blocks(blocks)
            seen.append(t.sweep_values([-3], [996]))
            torch.cuda.synchronize()
    finally:
        set_blocks(0)
    assert words_of(seen[0]) == vm.words(vc.summary(case, bits))
    assert all(torch.equal(s, seen[0]) for s in seen[1:])
    t.close()


@pytest.mark.parametrize("bits", [64, 128])
def test_waves_and_workgroups_that_meet_nothing(bits):
    """a workgroup whose second wave holds no live point (168 points: 40 in the second chunk), one whose
    second wave sees only OUTSIDE points, and a last workgroup that sees nothing else: their partial rows are the identity"""
    hold((vc.lanes(3), 3, 1, [5], [172], (), None), bits)
    hold((vc.lanes(3), 3, 1, [0], [255], [[1, -1, 191]], None), bits)       # theta <= 191: the fourth wave is outside
    want = hold((vc.lanes(3), 3, 1, [0], [383], [[1, -1, 255]], None), bits)  # theta <= 255: the third workgroup is
    assert want["counts"] == {"solution": 256, "nil": 0, "range": 0, "outside": 128} and want["unknowns"][2]["k_max"] == 255


# ---------------------------------------------------------------- 4. where
@pytest.mark.parametrize("bits", [64, 128])
def test_where(bits):
    want = hold(vc.where_constant(), bits)
    assert want["unknowns"][0]["k_min"] == want["unknowns"][0]["k_max"] == want["first"]["solution"] == 201
    want = hold(vc.two_minima(), bits)
    assert (want["unknowns"][0]["min"], want["unknowns"][0]["k_min"]) == (0, 100)
    want = hold((vc.scaled(-3), 1, 1, [0], [299], (), None), bits)
    assert want["unknowns"][0]["k_min"] == 299 and want["unknowns"][0]["k_max"] == 0


# ---------------------------------------------------------------- 5. nothing to report
@pytest.mark.parametrize("bits", [64, 128])
def test_nothing_to_report(bits):
    zero = vm.empty_record()
    for case in ((tc.nil(), 2, 1, [0], [299], (), None),                      # a NIL tape
                 ([], 2, 1, [0], [299], (), None),                            # the empty tape
                 (vc.lanes(2), 2, 1, [0], [299], [[1, 0, -1]], None)):        # every point outside
        assert hold(case, bits)["unknowns"] == [zero, zero]
    want = hold((tc.leaf([]), 0, 1, [0], [299], (), None), bits)              # no unknowns: eight words
    assert want["unknowns"] == [] and want["counts"]["solution"] == 300
    want = hold((tc.leaf([([7], 1), ([-1], 2)]), 2, 0, [], [], (), None), bits)   # no columns: one point
    assert want["unknowns"] == [dict(zero, n_int=1, min=7, max=7, k_min=0, k_max=0, sum=7), dict(zero, n_frac=1)]


# ---------------------------------------------------------------- 6. / 7. the edges of int64 and of 128 bits
@pytest.mark.parametrize("name,bits", [(n, b) for n, (_, widths) in vc.edges().items() for b in widths])
def test_width_edges(name, bits):
    want = hold(vc.edges()[name][0], bits)
    r = want["unknowns"][0]
    if name.startswith("int64"):
        assert abs(r["sum"]) > MAX64 + 1 and (r["min"] == MIN64 or r["max"] == MAX64)
    if name == "negate at MIN64":
        assert want["counts"]["range"] == 1 and r["n_int"] == 2
    if "2^12" in name and "range" not in name:
        assert abs(r["sum"]) >= 1 << 128
    if name == "range leaves 128 bits":
        assert want["counts"]["range"] == 2 and r["n_int"] == 2


# ---------------------------------------------------------------- 8. a lane per unknown
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("nvar", [1, 63, 64])
def test_lane_per_unknown(nvar, bits):
    want = hold((vc.lanes(nvar), nvar, 1, [-5], [200], (), None), bits)
    for i, r in enumerate(want["unknowns"]):
        assert (r["min"], r["max"], r["k_min"], r["k_max"]) == (-5 * (i + 1) - i, 200 * (i + 1) - i, 0, 205)


def test_65_unknowns_are_too_large():
    import torch
    from piplib_amd import engine as eng
    t = eng.Tape(_engine(), vc.lanes(65), 65, 1, 0, 64)
    with pytest.raises(eng.TapeError) as e:
        t.values_plan([0], [9])
    assert e.value.code == tm.E_TOOLARGE
    summary = torch.zeros(8 + 16 * 65, dtype=torch.int64, device=t.dev)
    with pytest.raises(eng.TapeError) as e:
        t.sweep_values_into([0], [9], summary, torch.zeros(1 << 16, dtype=torch.int64, device=t.dev))
    assert e.value.code == tm.E_TOOLARGE
    t.close()


def test_call_refusals_with_a_real_tape():
    """null buffers, a work buffer a byte short and one that is not 8-byte aligned are PIPAMD_E_INVALID; the plan's size is
    taken"""
    import torch
    from piplib_amd import engine as eng
    t = eng.Tape(_engine(), vc.lanes(3), 3, 1, 0, 64)
    fn = eng.lib().pipamd_tape_sweep_values
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                   C.c_size_t, C.c_void_p]
    lo, hi = (C.c_int64 * 1)(0), (C.c_int64 * 1)(299)
    need = t.values_plan([0], [299])["work_bytes"]
    assert need == 96 * 3 * 2 * 3
    summary = torch.zeros(8 + 16 * 3, dtype=torch.int64, device=t.dev)
    work = torch.zeros(need // 8, dtype=torch.int64, device=t.dev)
    sp, wp = C.c_void_p(summary.data_ptr()), C.c_void_p(work.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream(t.dev).cuda_stream)
    assert fn(t.e._h, t._h, lo, hi, 0, 0, None, None, wp, need, st) == tm.E_INVALID
    assert fn(t.e._h, t._h, lo, hi, 0, 0, None, sp, None, need, st) == tm.E_INVALID
    assert fn(t.e._h, t._h, lo, hi, 0, 0, None, sp, wp, need - 1, st) == tm.E_INVALID
    assert fn(t.e._h, t._h, lo, hi, 0, 0, None, sp, C.c_void_p(work.data_ptr() + 4), need, st) == tm.E_INVALID   # not 8-byte aligned
    assert fn(t.e._h, None, lo, hi, 0, 0, None, sp, wp, need, st) == tm.E_INVALID
    assert fn(t.e._h, t._h, lo, hi, 0, 0, None, sp, wp, need, st) == 0
    assert words_of(summary) == vm.words(vc.summary((vc.lanes(3), 3, 1, [0], [299], (), None), 64))
    t.close()


# ---------------------------------------------------------------- 9. many leaves in a wave
@pytest.mark.parametrize("bits", [64, 128])
def test_many_leaves_in_a_wave(bits):
    """64 conditions on the last column: the 70 points of a row of the box are at 65 leaves, each with a form of its own"""
    want = hold((vc.leaf_chain(64), 1, 2, [0, 0], [2, 69], (), None), bits)
    assert want["unknowns"][0]["n_int"] == 210


# ---------------------------------------------------------------- 10. unbounded and fractional
@pytest.mark.parametrize("bits", [64, 128])
def test_unbounded_unknowns_of_an_edited_tape(bits):
    """the Maximize family (SOL_SHIFT): an unbounded unknown is counted in n_unbounded and nowhere else"""
    g = family("maximize")
    cells, info = solved("maximize", bits)
    pts = np.array(g["points"])
    lo, hi = pts.min(axis=0).tolist(), pts.max(axis=0).tolist()
    assert info["sol_flags"] & 1 and int(np.prod([h - l + 1 for l, h in zip(lo, hi)])) <= 4096
    want = hold((cells, info["nvar"], info["nparm"], lo, hi, (), info), bits)
    assert sum(r["n_unbounded"] for r in want["unknowns"]) > 0
    assert all(r["n_int"] + r["n_frac"] + r["n_unbounded"] == want["counts"]["solution"] for r in want["unknowns"])
    assert any(r["n_unbounded"] == 0 and r["n_int"] > 0 for r in want["unknowns"]) or info["nvar"] == 1


@pytest.mark.parametrize("bits", [64, 128])
def test_fractions(bits):
    want = hold(vc.edges()["halves"][0], bits)
    assert want["unknowns"][0]["n_frac"] == 72 and want["unknowns"][0]["n_int"] == 71 and want["unknowns"][1]["n_frac"] == 0
    # a hand-made unbounded unknown beside a bounded one (SOL_SHIFT on the big parameter's column)
    want = hold((tc.leaf([([5, 1, 0], 4), ([4, 1, 0], 4)]), 2, 2, [0, -8], [2, 91], (), dict(sol_bg=0, sol_flags=1)), bits)
    assert want["unknowns"][0]["n_unbounded"] == 300 and want["unknowns"][0]["n_int"] == 0 and want["unknowns"][1]["n_int"] == 75


# ---------------------------------------------------------------- 11. context
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("case", range(len(sm.edge_rows())))
def test_context_rows_at_the_edges(case, bits):
    rows, point, inside = sm.edge_rows()[case]
    cols = len(point)
    want = hold((tc.leaf([([0] * cols + [5], 1)]), 1, cols, point, point, rows, None), bits)
    assert want["counts"]["outside"] == int(not inside) and want["unknowns"][0]["n_int"] == int(inside)


@pytest.mark.parametrize("bits", [64, 128])
def test_context_of_two_rows_on_p5(bits):
    g = tc.golden()
    cells, _ = _solve_p5(1, bits)
    ctx = [[1] + r for r in P5_CONTEXT]
    want = hold((cells, g["nvar"], g["nparm"], [0, 0], [11, 11], ctx, None), bits)
    assert 40 <= want["counts"]["outside"] <= 100 and all(r["n_int"] <= 144 - want["counts"]["outside"] for r in want["unknowns"])


# ---------------------------------------------------------------- 12. both program paths
@pytest.mark.parametrize("k,staged", [(2015, 1), (2016, 0)])
def test_both_program_paths(k, staged):
    from piplib_amd import engine as eng
    cells = tc.if_chain(k)
    assert eng.values_plan(eng.tape_check(cells, 1, 1), 64, 1, 1, [0], [9])["staged"] == staged
    want = hold((cells, 1, 1, [k - 150], [k + 149], (), None), 64)
    assert want["counts"] == {"solution": 150, "nil": 150, "range": 0, "outside": 0}
    assert want["unknowns"][0] == dict(vm.empty_record(), n_int=150, min=k, k_min=150, max=k + 149, k_max=299,
                                       sum=sum(range(k, k + 150)))


# ---------------------------------------------------------------- 13. two streams
@pytest.mark.parametrize("bits", [64, 128])
def test_two_streams_and_no_accumulation(bits):
    import torch
    from piplib_amd import engine as eng
    g = tc.golden()
    cells = tc.cells_from_text(g["tapes"]["int"])
    t = eng.Tape(_engine(), cells, g["nvar"], g["nparm"], 0, bits)
    lo, hi, ctx = [-5, -5], [58, 58], [[1, 1, 1, -3]]
    plan = t.values_plan(lo, hi)
    single = t.sweep_values(lo, hi, ctx=ctx)
    torch.cuda.synchronize()
    assert words_of(single) == vm.words(vc.summary((cells, g["nvar"], g["nparm"], lo, hi, ctx, None), bits))
    bufs = [(torch.full((plan["summary_words"],), 7, dtype=torch.int64, device=t.dev),
             torch.full((plan["work_bytes"] // 8,), -3, dtype=torch.int64, device=t.dev)) for _ in range(2)]
    ctx_dev = torch.as_tensor(ctx, dtype=torch.int64, device=t.dev)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s, (summary, work) in zip(streams, bufs):
        with torch.cuda.stream(s):
            t.sweep_values_into(lo, hi, summary, work, ctx=ctx_dev)
    torch.cuda.synchronize()
    assert all(torch.equal(summary, single) for summary, _ in bufs)
    # again into the same buffers: nothing accumulates
    t.sweep_values_into(lo, hi, bufs[0][0], bufs[0][1], ctx=ctx_dev)
    torch.cuda.synchronize()
    assert torch.equal(bufs[0][0], single)
    t.close()
