"""CPU-side checks of the set sweep's C interface through ctypes: pipamd_tape_set_sweep_plan against
tests/tape_set_sweep_model.py -- offsets, every refusal with its code and the job named in pipamd_last_error --, the job
struct's layout, and the null-pointer refusals of create, run and free that need no GPU."""
import ctypes as C

import pytest

import tape_model as tm
import tape_set_sweep_model as ssm
from tape_cases import MAX64, MIN64


@pytest.fixture(scope="module")
def lib():
    from piplib_amd import build, engine
    build.build(force=False, verbose=False)
    L = engine.lib()
    L.pipamd_tape_set_sweep_plan.argtypes = [C.c_int] + [C.c_void_p] * 6
    L.pipamd_tape_set_sweep_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pipamd_tape_set_sweep_run.argtypes = [C.c_void_p] * 4
    L.pipamd_tape_set_sweep_free.argtypes = [C.c_void_p]
    L.pipamd_tape_set_tape_info.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    return L


def c_plan(lib, jobs, leaves, point_cols, chunks=True):
    """jobs as the model takes them, (lo, hi, n_ctx, has_ctx) -> (rc, error text, points, summary_off, chunk_off)"""
    from piplib_amd.engine import TapeSweepJob
    n = len(jobs)
    arr, keep = (TapeSweepJob * max(1, n))(), []
    row = (C.c_int64 * 64)()
    for j, (lo, hi, n_ctx, has_ctx) in enumerate(jobs):
        clo, chi = (C.c_int64 * max(1, len(lo)))(*lo), (C.c_int64 * max(1, len(hi)))(*hi)
        keep += [clo, chi]
        arr[j].tape, arr[j].n_ctx = 0, n_ctx
        arr[j].lo, arr[j].hi = (C.addressof(clo) if len(lo) else None), (C.addressof(chi) if len(hi) else None)
        arr[j].ctx = C.addressof(row) if has_ctx else None
    cl, cc = (C.c_int64 * max(1, n))(*leaves), (C.c_int32 * max(1, n))(*point_cols)
    pts, so, co = (C.c_int64 * max(1, n))(), (C.c_int64 * (n + 1))(), (C.c_int64 * (n + 1))()
    rc = lib.pipamd_tape_set_sweep_plan(n, arr, cl, cc, pts, so, co if chunks else None)
    return rc, lib.pipamd_last_error().decode(), list(pts)[:n], list(so), list(co)


def box(n, at=5):
    return ([at], [at + n - 1], 0, False)


BIG = ([0, 0], [(1 << 19) - 1, (1 << 19) - 2], 0, False)  # 2^38 - 2^19 points


def test_the_job_struct():
    from piplib_amd.engine import TapeSweepJob
    assert C.sizeof(TapeSweepJob) == 32
    assert [getattr(TapeSweepJob, f).offset for f, _ in TapeSweepJob._fields_] == [0, 4, 8, 16, 24]


def test_offsets_are_the_models(lib):
    sizes, leaves = [1, 127, 128, 129, 257], [0, 3, 7, 1, 40]
    jobs = [box(n) for n in sizes] + [([], [], 2, True), box(1000, MIN64), box(3, MAX64 - 2)]
    leaves, cols = leaves + [2, 5, 0], [1] * 5 + [0, 1, 1]
    rc, _, pts, so, co = c_plan(lib, jobs, leaves, cols)
    want = ssm.plan(jobs, leaves, cols)
    assert rc == 0 and {"points": pts, "summary_off": so, "chunk_off": co} == want
    assert pts == sizes + [1, 1000, 3] and co[:7] == [0, 1, 2, 3, 5, 8, 9] and so[:3] == [0, 8, 22]
    # chunk_off may be left out; no job at all is a plan of nothing
    rc, _, pts2, so2, _ = c_plan(lib, jobs, leaves, cols, chunks=False)
    assert rc == 0 and (pts2, so2) == (pts, so)
    assert c_plan(lib, [], [], [])[0::2] == (0, [], [0])
    # the chunk prefix leaves 32 bits where the points may
    rc, _, pts, so, co = c_plan(lib, [BIG, box((1 << 19) - 1)], [1, 1], [2, 1])
    assert rc == 0 and pts == [(1 << 38) - (1 << 19), (1 << 19) - 1] and co == [0, (1 << 31) - (1 << 12), 1 << 31]


REFUSALS = {
    "lo above hi": ([box(3), box(3), box(3), ([1], [0], 0, False), box(3)], [1] * 5, [1] * 5),
    "n_ctx below 0": ([box(3), box(3), ([0], [1], -1, False)], [1] * 3, [1] * 3),
    "rows without ctx": ([([0], [1], 2, False)], [1], [1]),
    "32 point columns": ([box(1), ([0], [1], 0, False)], [1, 1], [1, 32]),
    "point columns below 0": ([([0], [1], 0, False)], [1], [-1]),
    "no bounds": ([box(1), ([], [], 0, False)], [1, 1], [1, 1]),
    "leaves below 0": ([box(1), box(1)], [1, -1], [1, 1]),
    "2^38 in one job": ([box(1), ([0, 0], [(1 << 19) - 1, (1 << 19) - 1], 0, False)], [1, 1], [1, 2]),
    "2^38 only by the sum": ([BIG, box((1 << 19) - 1), box(1)], [1] * 3, [2, 1, 1]),
    "the whole of int64 in one column": ([box(2), ([MIN64], [MAX64], 0, False)], [1, 1], [1, 1]),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_name_the_job(lib, name):
    jobs, leaves, cols = REFUSALS[name]
    # (the model has None where the C side has a null pointer: bounds left out of a job whose tape has columns)
    model_jobs = [((lo or None) if c > 0 else lo, (hi or None) if c > 0 else hi, n, h) for (lo, hi, n, h), c in zip(jobs, cols)]
    with pytest.raises(tm.TapeError) as e:
        ssm.plan(model_jobs, leaves, cols)
    rc, why, _, _, _ = c_plan(lib, jobs, leaves, cols)
    assert rc == e.value.code and rc in (tm.E_INVALID, tm.E_TOOLARGE)
    assert rc == (tm.E_TOOLARGE if "2^38" in name or "int64" in name else tm.E_INVALID)
    assert why.startswith("tape_set_sweep_plan: ") and f"{e.value}:" in why, (why, str(e.value))


def test_the_sum_just_below_the_limit_is_taken(lib):
    rc, _, pts, _, _ = c_plan(lib, [BIG, box((1 << 19) - 1)], [1, 1], [2, 1])
    assert rc == 0 and sum(pts) == (1 << 38) - 1


def test_too_many_jobs_and_null_arrays(lib):
    n = (1 << 20) + 1
    from piplib_amd.engine import TapeSweepJob
    arr = (TapeSweepJob * n)()
    cl, cc, pts, so = (C.c_int64 * n)(), (C.c_int32 * n)(), (C.c_int64 * n)(), (C.c_int64 * (n + 1))()
    assert lib.pipamd_tape_set_sweep_plan(n, arr, cl, cc, pts, so, None) == tm.E_TOOLARGE
    assert b"tape_set_sweep_plan" in lib.pipamd_last_error() and b"2^20" in lib.pipamd_last_error()
    # 2^20 jobs of one point each (0 columns) are taken
    assert lib.pipamd_tape_set_sweep_plan(n - 1, arr, cl, cc, pts, so, None) == 0
    assert so[n - 1] == 8 * (n - 1) and pts[n - 2] == 1
    one = (TapeSweepJob * 1)()
    for args in ((-1, one, cl, cc, pts, so, None), (1, None, cl, cc, pts, so, None), (1, one, None, cc, pts, so, None),
                 (1, one, cl, None, pts, so, None), (1, one, cl, cc, None, so, None), (1, one, cl, cc, pts, None, None),
                 (0, None, None, None, None, None, None)):
        assert lib.pipamd_tape_set_sweep_plan(*args) == tm.E_INVALID, args
        assert b"tape_set_sweep_plan" in lib.pipamd_last_error()
    assert lib.pipamd_tape_set_sweep_plan(0, None, None, None, None, so, None) == 0


def test_null_pointers_need_no_gpu(lib):
    """refused before any HIP call: the answers are the same with and without a device"""
    from piplib_amd.engine import TapeSweepJob
    one, out, so = (TapeSweepJob * 1)(), C.c_void_p(), (C.c_int64 * 2)()
    fake = C.c_void_p(C.addressof((C.c_int64 * 64)()))  # (never read: every call below has a null in front of it)
    assert lib.pipamd_tape_set_sweep_create(None, None, 1, one, C.byref(out), so) == tm.E_INVALID
    assert b"tape_set_sweep_create" in lib.pipamd_last_error()
    assert lib.pipamd_tape_set_sweep_create(None, fake, 1, one, C.byref(out), so) == tm.E_INVALID
    assert lib.pipamd_tape_set_sweep_create(fake, None, 1, one, C.byref(out), so) == tm.E_INVALID
    assert lib.pipamd_tape_set_sweep_create(None, None, 1, one, None, so) == tm.E_INVALID
    assert not out.value
    assert lib.pipamd_tape_set_sweep_run(None, None, None, None) == tm.E_INVALID
    assert b"tape_set_sweep_run" in lib.pipamd_last_error()
    assert lib.pipamd_tape_set_sweep_run(fake, None, fake, None) == tm.E_INVALID
    assert lib.pipamd_tape_set_sweep_run(None, fake, fake, None) == tm.E_INVALID
    lib.pipamd_tape_set_sweep_free(None)
    assert lib.pipamd_tape_set_tape_info(None, 0, None, None, None, None) == tm.E_INVALID
    assert b"tape_set_tape_info" in lib.pipamd_last_error()
