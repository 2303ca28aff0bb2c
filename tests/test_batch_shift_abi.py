"""pipamd_batch_load_shifted / _load_shifted_part / pipamd_batch_results_shifted: the entries exist -- in the library and
in the header -- without a new interface version, and refuse what include/piplib_amd.h says they refuse before any HIP
call.  Host only, no GPU: host memory stands in for the engine and the device arrays, which a refused call must not
look at."""
import ctypes as C
import os
import re

import pytest

from piplib_amd import engine as eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pipamd_batch_load_shifted", "pipamd_batch_load_shifted_part", "pipamd_batch_results_shifted", "pipamd_engine_set_lean_big"]
E_INVALID = -1
SENTINEL = 0x5A5A5A5A5A5A5A5A
NVAR, NI, BATCH = 2, 3, 4


def _desc(nparm=1, bigparm=NVAR + 1):
    return eng.BatchDesc(BATCH, NVAR, nparm, NI, bigparm, eng.T_INT, 4, 0, 64)


def _bufs():
    return [(C.c_int64 * 64)(*([SENTINEL] * 64)) for _ in range(4)]  # engine, workspace, rows / x_num, x_den


def _load(engine, ws, desc, rows, shift, first=None, count=None):
    L = eng.lib()
    if first is None:
        L.pipamd_batch_load_shifted.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(eng.BatchDesc), C.c_void_p, C.c_int, C.c_void_p]
        return L.pipamd_batch_load_shifted(engine, ws, desc, rows, shift, None)
    L.pipamd_batch_load_shifted_part.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(eng.BatchDesc), C.c_void_p, C.c_int, C.c_int,
                                                 C.c_int, C.c_void_p]
    return L.pipamd_batch_load_shifted_part(engine, ws, desc, rows, shift, first, count, None)


def _results(engine, ws, desc, shift, num, den):
    L = eng.lib()
    L.pipamd_batch_results_shifted.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(eng.BatchDesc), C.c_int] + [C.c_void_p] * 6
    return L.pipamd_batch_results_shifted(engine, ws, desc, shift, None, None, None, num, den, None)


@pytest.mark.parametrize("name", NAMES)
def test_exported_and_declared(name):
    assert hasattr(eng.lib(), name)
    header = open(os.path.join(ROOT, "include", "piplib_amd.h")).read()
    assert re.search(r"\bint\s+%s\s*\(\s*pipamd_engine\s*\*" % name, header)
    assert re.search(r"#define\s+PIPAMD_SHIFT_MAX\s+1\b", header) and re.search(r"#define\s+PIPAMD_SHIFT_URS\s+\(-1\)", header)


def test_interface_version_unchanged():
    assert eng.lib().pipamd_version() == 500
    header = open(os.path.join(ROOT, "include", "piplib_amd.h")).read()
    assert re.search(r"#define\s+PIPAMD_VERSION\s+500\b", header)


def test_refusals_before_any_hip_call():
    bufs = _bufs()
    e, ws, rows, den = [C.cast(a, C.c_void_p) for a in bufs]
    d = _desc()
    calls = [
        # null engine, workspace, descriptor, rows
        lambda: _load(None, ws, C.byref(d), rows, 1),
        lambda: _load(e, None, C.byref(d), rows, 1),
        lambda: _load(e, ws, None, rows, 1),
        lambda: _load(e, ws, C.byref(d), None, 1),
        lambda: _load(None, ws, C.byref(d), rows, -1, 0, 1),
        lambda: _load(e, ws, C.byref(d), None, -1, 0, 1),
        lambda: _results(None, ws, C.byref(d), 1, rows, den),
        lambda: _results(e, None, C.byref(d), 1, rows, den),
        lambda: _results(e, ws, None, 1, rows, den),
        # shift other than +-1
        lambda: _load(e, ws, C.byref(d), rows, 0),
        lambda: _load(e, ws, C.byref(d), rows, 2),
        lambda: _load(e, ws, C.byref(d), rows, -2, 0, 1),
        lambda: _results(e, ws, C.byref(d), 0, rows, den),
        # a descriptor that is not the shifted tableau's
        lambda: _load(e, ws, C.byref(_desc(0, -1)), rows, 1),
        lambda: _load(e, ws, C.byref(_desc(1, -1)), rows, 1),
        lambda: _load(e, ws, C.byref(_desc(2, NVAR + 1)), rows, 1),
        lambda: _load(e, ws, C.byref(_desc(2, NVAR + 2)), rows, -1, 0, 1),
        lambda: _results(e, ws, C.byref(_desc(0, -1)), 1, rows, den),
        lambda: _results(e, ws, C.byref(_desc(1, -1)), -1, rows, den),
        # first / count outside the batch
        lambda: _load(e, ws, C.byref(d), rows, 1, -1, 1),
        lambda: _load(e, ws, C.byref(d), rows, 1, 0, -1),
        lambda: _load(e, ws, C.byref(d), rows, 1, BATCH, 1),
        lambda: _load(e, ws, C.byref(d), rows, 1, 1, BATCH),
        lambda: _load(e, ws, C.byref(d), rows, 1, 0, BATCH + 1),
    ]
    for i, call in enumerate(calls):
        assert call() == E_INVALID, i
        assert eng.lib().pipamd_last_error()
    for a in bufs:
        assert all(x == SENTINEL for x in a)  # nothing was touched


def test_python_binding_is_there():
    assert eng.lib().pipamd_engine_set_lean_big(None, 1) == E_INVALID
    assert callable(eng.Engine.set_lean_big) and callable(eng.Batch.fetch_shifted) and eng.SHIFT_MAX == 1 and eng.SHIFT_URS == -1
    assert "shift" in eng.Batch.__init__.__code__.co_varnames
