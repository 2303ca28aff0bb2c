"""pipamd_batch_dual / pipamd_batch_dual_part: the entries exist -- in the library and in the header -- without a new
interface version, and refuse null arguments before any HIP call.  Host only, no GPU."""
import ctypes as C
import os
import re

import pytest

from piplib_amd import engine as eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pipamd_batch_dual", "pipamd_batch_dual_part"]
E_INVALID = -1
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _call(name, engine, ws, desc, rows, num, den):
    fn = getattr(eng.lib(), name)
    part = [C.c_int, C.c_int] if name.endswith("_part") else []
    fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(eng.BatchDesc), C.c_void_p] + part + [C.c_void_p] * 3
    args = [engine, ws, desc, rows] + ([0, 1] if part else []) + [num, den, None]
    return fn(*args)


@pytest.mark.parametrize("name", NAMES)
def test_exported_and_declared(name):
    assert hasattr(eng.lib(), name)
    header = open(os.path.join(ROOT, "include", "piplib_amd.h")).read()
    assert re.search(r"\bint\s+%s\s*\(\s*pipamd_engine\s*\*" % name, header)


def test_interface_version_unchanged():
    assert eng.lib().pipamd_version() == 500
    header = open(os.path.join(ROOT, "include", "piplib_amd.h")).read()
    assert re.search(r"#define\s+PIPAMD_VERSION\s+500\b", header)


@pytest.mark.parametrize("name", NAMES)
def test_null_arguments_are_invalid(name):
    """host memory stands in for the device arrays: a refused call must not look at any of them"""
    desc = eng.BatchDesc(1, 2, 0, 3, -1, eng.T_DUAL, 0, 0, 64)
    ws = (C.c_int64 * 64)(*([SENTINEL] * 64))
    rows = (C.c_int64 * 9)(*([SENTINEL] * 9))
    num = (C.c_int64 * 3)(*([SENTINEL] * 3))
    den = (C.c_int64 * 3)(*([SENTINEL] * 3))
    p = [C.cast(a, C.c_void_p) for a in (ws, rows, num, den)]
    assert _call(name, None, p[0], C.byref(desc), p[1], p[2], p[3]) == E_INVALID  # null engine
    assert eng.lib().pipamd_last_error()
    assert _call(name, None, None, None, None, None, None) == E_INVALID
    for a in (ws, rows, num, den):
        assert all(x == SENTINEL for x in a)  # nothing was touched


def test_python_binding_is_there():
    assert callable(eng.Batch.dual) and callable(eng.Batch.dual_part)
