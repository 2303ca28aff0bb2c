"""-m gpu: engine.TapeSet -- many compiled tapes evaluated in one launch (pipamd_tape_set_create / pipamd_tape_set_eval,
pip_tape_set_eval_kernel of csrc/pip_tape.hip).  The authority is engine.Tape.eval of each tape on its own points (held
to the reference and to the models by tests/test_gpu_tape_eval.py and tests/test_gpu_tape_edit.py): every point of a set
must get exactly that, padded with (0, 0) to the set's widest tape."""
import functools

import numpy as np
import pytest

import tape_cases as tc
import tape_model as tm
from test_gpu_tape_eval import _engine, _solve_p5
from test_gpu_tape_edit import FAMILIES, family, solved

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ST_BADINPUT = 10
NAMES = ("status", "leaf", "x_num", "x_den", "dual_num", "dual_den")
UNBOUNDED = (tc.iff([0, 1, -2], tc.leaf([([5, 2, 1], 4), ([4, 0, 3], 4)]), tc.nil()), 2, 2, 0, dict(sol_bg=0, sol_flags=7))


def mixed_tapes(bits):
    """[(Tape, points)]: the fixture tapes of pip_solve_many (edited), the p5 tape with and without its dual list, a NIL
    tape, an empty tape, an edited tape with an unbounded unknown, and a chain of 2016 conditions, which as a single tape
    is not staged -- different nvar, point columns, ndual and slots"""
    from piplib_amd import engine as eng
    e = _engine()
    out = []
    for name in FAMILIES:
        cells, info = solved(name, bits)
        out.append((eng.Tape(e, cells, info["nvar"], info["nparm"], 0, bits, edit=info), family(name)["points"][:30]))
    g = tc.golden()
    cells, _ = _solve_p5(1, bits)
    out.append((eng.Tape(e, cells, g["nvar"], g["nparm"], 0, bits), g["points"][:40]))
    cells, ndual = _solve_p5(0, bits, dual=True)
    out.append((eng.Tape(e, cells, g["nvar"], g["nparm"], ndual, bits), g["points"][40:70]))
    out.append((eng.Tape(e, tc.nil(), 2, 1, 0, bits), [[3], [-4], [0]]))
    out.append((eng.Tape(e, [], 1, 3, 0, bits), [[1, 2, 3], [4, 5, 6]]))
    cells, nvar, nparm, ndual, edit = UNBOUNDED
    out.append((eng.Tape(e, cells, nvar, nparm, ndual, bits, edit=edit), [[k] for k in range(-3, 8)]))
    chain = eng.Tape(e, tc.if_chain(2016), 1, 1, 0, bits)
    assert chain.info["staged"] == 0
    out.append((chain, [[0], [1], [700], [2015], [2016], [5000], [-1]]))
    return out


def layout(tapes, order):
    """(tape index per point, padded points) for the (tape, point) pairs of `order`"""
    cols = max(t.point_cols for t, _ in tapes)
    idx = np.array([i for i, _ in order], dtype=np.int32)
    pts = np.zeros((len(order), cols), dtype=np.int64)
    for k, (i, p) in enumerate(order):
        pts[k, :len(p)] = p
        pts[k, len(p):] = 77 + k  # (what a tape does not read must not matter)
    return idx, pts


def alone(tapes, order):
    """what Tape.eval gives every point of `order`, padded to the set's maxima: {name: array}"""
    import torch
    bits = tapes[0][0].bits
    ew = (2,) if bits == 128 else ()
    nv, nd = max(t.nvar for t, _ in tapes), max(t.ndual for t, _ in tapes)
    n = len(order)
    want = {"status": np.zeros(n, np.int32), "leaf": np.zeros(n, np.int32), "x_num": np.zeros((n, nv) + ew, np.int64),
            "x_den": np.zeros((n, nv) + ew, np.int64), "dual_num": np.zeros((n, nd) + ew, np.int64),
            "dual_den": np.zeros((n, nd) + ew, np.int64)}
    for i, (t, _) in enumerate(tapes):
        where = [k for k, (j, _) in enumerate(order) if j == i]
        if not where:
            continue
        pts = np.array([order[k][1] for k in where], dtype=np.int64).reshape(len(where), t.point_cols)
        out = t.eval(pts if t.point_cols else len(where))
        torch.cuda.synchronize()
        got = dict(zip(NAMES, (o.cpu().numpy() for o in out)))
        want["status"][where], want["leaf"][where] = got["status"], got["leaf"]
        want["x_num"][where, :t.nvar], want["x_den"][where, :t.nvar] = got["x_num"], got["x_den"]
        if t.ndual:
            want["dual_num"][where, :t.ndual], want["dual_den"][where, :t.ndual] = got["dual_num"], got["dual_den"]
    return want


def same(out, want, where=None):
    import torch
    torch.cuda.synchronize()
    for name, o in zip(NAMES, out):
        got = o.cpu().numpy()
        w = want[name]
        if where is not None:
            got, w = got[where], w[where]
        assert got.shape == w.shape and np.array_equal(got, w), (name, np.argwhere(got != w)[:5].tolist())


@functools.lru_cache(maxsize=None)
def mixed(bits):
    from piplib_amd import engine as eng
    tapes = mixed_tapes(bits)
    s = eng.TapeSet(_engine(), [t for t, _ in tapes])
    return tapes, s


@pytest.mark.parametrize("bits", [64, 128])
def test_a_mixed_set_sorted_and_dealt_round_robin(bits):
    tapes, s = mixed(bits)
    assert s.info["n"] == len(tapes) and s.info["bits"] == bits
    assert s.info["words"] == sum(t.info["words"] for t, _ in tapes)
    assert (s.info["point_cols"], s.info["nvar"], s.info["ndual"]) == (3, 5, max(t.ndual for t, _ in tapes))
    assert s.info["slots"] == max(t.info["slots"] for t, _ in tapes) and s.info["ndual"] > 0
    by_tape = [(i, p) for i, (_, pts) in enumerate(tapes) for p in pts]
    idx, pts = layout(tapes, by_tape)
    want = alone(tapes, by_tape)
    assert {tm.ST_SOLUTION, tm.ST_NIL} <= set(want["status"].tolist()) and (want["x_den"] == 0).any()
    same(s.eval(idx, pts), want)
    # the same points dealt round-robin: every wave serves many tapes
    n = len(tapes)
    queues = [[(i, p) for p in pts_i] for i, (_, pts_i) in enumerate(tapes)]
    dealt, k = [], 0
    while any(queues):
        if queues[k % n]:
            dealt.append(queues[k % n].pop(0))
        k += 1
    assert sorted(map(str, dealt)) == sorted(map(str, by_tape)) and [i for i, _ in dealt[:n]] == list(range(n))
    idx, pts = layout(tapes, dealt)
    same(s.eval(idx, pts), alone(tapes, dealt))


def test_tape_indices_outside_the_set():
    import torch
    tapes, s = mixed(64)
    n = len(tapes)
    order = [(k % n, tapes[k % n][1][k % len(tapes[k % n][1])]) for k in range(257)]
    idx, pts = layout(tapes, order)
    want = alone(tapes, order)
    same(s.eval(idx, pts), want)
    bad = [0, 128, 256]
    keep = [k for k in range(257) if k not in bad]
    for v in (-1, n, -(1 << 31), (1 << 31) - 1):
        wrong = idx.copy()
        wrong[bad] = v
        out = s.eval(wrong, pts)
        same(out, want, keep)
        torch.cuda.synchronize()
        assert out[0].cpu()[bad].tolist() == [ST_BADINPUT] * 3 and out[1].cpu()[bad].tolist() == [-1] * 3, v
        assert all(not o.cpu()[bad].any() for o in out[2:]), v


def test_point_counts_around_the_wave_and_the_workgroup():
    tapes, s = mixed(64)
    n = len(tapes)
    for count in (1, 63, 64, 65, 129, 257, 0):
        order = [((3 * k) % n, tapes[(3 * k) % n][1][k % len(tapes[(3 * k) % n][1])]) for k in range(count)]
        idx, pts = layout(tapes, order)
        out = s.eval(idx, pts)
        assert out[0].shape[0] == count
        same(out, alone(tapes, order))


@pytest.mark.parametrize("bits", [64, 128])
def test_a_set_of_one_tape_and_tapes_freed_before_eval(bits):
    from piplib_amd import engine as eng
    g = tc.golden()
    cells, _ = _solve_p5(1, bits)
    t = eng.Tape(_engine(), cells, g["nvar"], g["nparm"], 0, bits)
    order = [(0, p) for p in g["points"]]
    want = alone([(t, None)], order)
    s = eng.TapeSet(_engine(), [t])
    assert s.info == {"words": t.info["words"], "n": 1, "bits": bits, "point_cols": 2, "nvar": g["nvar"], "ndual": 0,
                      "slots": t.info["slots"]}
    t.close()  # the set has its own copy of the program
    out = s.eval(np.zeros(len(order), np.int32), np.array(g["points"], dtype=np.int64))
    assert len(out) == 4
    same(out, want)
    s.close()


@pytest.mark.parametrize("bits", [64, 128])
def test_tapes_of_2_and_32_slots(bits):
    from piplib_amd import engine as eng
    small = eng.Tape(_engine(), tc.iff([1, -2], tc.leaf([([3, 1], 2)]), tc.nil()), 1, 1, 0, bits)
    large = eng.Tape(_engine(), tc.new_chain(1, 30), 2, 1, 0, bits)
    assert (small.info["slots"], large.info["slots"]) == (2, 32)
    tapes = [(small, None), (large, None)]
    order = [(k % 2, [k - 40]) for k in range(150)]
    s = eng.TapeSet(_engine(), [small, large])
    assert s.info["slots"] == 32
    idx, pts = layout(tapes, order)
    same(s.eval(idx, pts), alone(tapes, order))


def test_mixed_widths_are_refused():
    from piplib_amd import engine as eng
    a = eng.Tape(_engine(), tc.nil(), 1, 1, 0, 64)
    b = eng.Tape(_engine(), tc.nil(), 1, 1, 0, 128)
    for tapes in ([a, b], [b, a], []):
        with pytest.raises(eng.TapeError) as e:
            eng.TapeSet(_engine(), tapes)
        assert e.value.code == tm.E_INVALID
    closed = eng.Tape(_engine(), tc.nil(), 1, 1, 0, 64)
    closed.close()
    with pytest.raises(eng.TapeError):
        eng.TapeSet(_engine(), [a, closed])  # a null entry
    import torch
    if torch.cuda.device_count() > 1:
        other = eng.Engine(1)
        with pytest.raises(eng.TapeError) as e:
            eng.TapeSet(other, [a])
        assert e.value.code == tm.E_INVALID


def test_null_outputs_and_two_streams():
    import torch
    tapes, s = mixed(64)
    by_tape = [(i, p) for i, (_, pts) in enumerate(tapes) for p in pts]
    idx, pts = layout(tapes, by_tape)
    want = alone(tapes, by_tape)
    for names in (("status",), ("x_num", "dual_den"), ("leaf", "x_den", "dual_num"), ()):
        out = s.eval_into(idx, pts, s.outputs(len(by_tape), names))
        torch.cuda.synchronize()
        assert set(out) == set(names)
        for k in names:
            assert np.array_equal(out[k].cpu().numpy(), want[k]), k
    d_idx = torch.as_tensor(idx, device="cuda").repeat(50)
    d_pts = torch.as_tensor(pts, device="cuda").repeat(50, 1).contiguous()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        a = s.eval(d_idx, d_pts)
    with torch.cuda.stream(s2):
        b = s.eval(d_idx, d_pts)
    torch.cuda.synchronize()
    for x, y, k in zip(a, b, NAMES):
        assert torch.equal(x, y), k
        assert np.array_equal(x.cpu().numpy()[:len(by_tape)], want[k]), k
