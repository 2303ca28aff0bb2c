"""pipamd_batch_load_system / pipamd_batch_dual_system and their _part forms: the entries exist -- in the library and in
the header -- without a new interface version, the Python binding has them, and they refuse what include/piplib_amd.h
says they refuse before any HIP call.  Host only, no GPU: host memory stands in for the engine and the device arrays,
which a refused call must not look at."""
import ctypes as C
import os
import re

import pytest

from piplib_amd import engine as eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pipamd_batch_load_system", "pipamd_batch_load_system_part", "pipamd_batch_dual_system", "pipamd_batch_dual_system_part"]
E_INVALID = -1
SENTINEL = 0x5A5A5A5A5A5A5A5A
NVAR, NROWS, BATCH = 2, 3, 4
EQ = (C.c_int32 * 2)(0, 2)


def _desc(ni=NROWS + 2, nparm=0, bigparm=-1, tflags=eng.T_INT):
    return eng.BatchDesc(BATCH, NVAR, nparm, ni, bigparm, tflags, 4, 0, 64)


def _sys(nrows=NROWS, neq=2, eq=EQ, shift=0, simplify=0):
    return eng.System(nrows, neq, C.cast(eq, C.POINTER(C.c_int32)) if eq is not None else None, shift, simplify)


def _bufs():
    return [(C.c_int64 * 64)(*([SENTINEL] * 64)) for _ in range(5)]  # engine, workspace, rows, dual_num, dual_den


def _load(engine, ws, desc, sys_, rows, first=None, count=None):
    L = eng.lib()
    d = C.byref(desc) if desc is not None else None
    s = C.byref(sys_) if sys_ is not None else None
    if first is None:
        L.pipamd_batch_load_system.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(eng.BatchDesc), C.POINTER(eng.System), C.c_void_p,
                                               C.c_void_p]
        return L.pipamd_batch_load_system(engine, ws, d, s, rows, None)
    return L.pipamd_batch_load_system_part(engine, ws, d, s, rows, first, count, None)


def _dual(engine, ws, desc, sys_, rows, num, den, first=None, count=None):
    L = eng.lib()
    d = C.byref(desc) if desc is not None else None
    s = C.byref(sys_) if sys_ is not None else None
    if first is None:
        L.pipamd_batch_dual_system.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(eng.BatchDesc), C.POINTER(eng.System)] + [C.c_void_p] * 4
        return L.pipamd_batch_dual_system(engine, ws, d, s, rows, num, den, None)
    return L.pipamd_batch_dual_system_part(engine, ws, d, s, rows, first, count, num, den, None)


@pytest.mark.parametrize("name", NAMES)
def test_exported_and_declared(name):
    assert hasattr(eng.lib(), name)
    header = open(os.path.join(ROOT, "include", "piplib_amd.h")).read()
    assert re.search(r"\bint\s+%s\s*\(\s*pipamd_engine\s*\*" % name, header)
    assert re.search(r"typedef\s+struct\s+pipamd_system\s*\{[^}]*\bnrows\b[^}]*\bneq\b[^}]*\beq_rows\b[^}]*\bshift\b[^}]*\bsimplify\b[^}]*\}\s*pipamd_system\s*;",
                     header)


def test_interface_version_unchanged():
    assert eng.lib().pipamd_version() == 500
    header = open(os.path.join(ROOT, "include", "piplib_amd.h")).read()
    assert re.search(r"#define\s+PIPAMD_VERSION\s+500\b", header)
    assert "pipamd_batch_load_system" in header[header.index("Added since"):header.index("#define PIPAMD_VERSION")]


def test_system_struct_layout():
    """int32 nrows, neq | pointer eq_rows | int32 shift, simplify: as the header's struct on an LP64 target"""
    assert C.sizeof(eng.System) == 24
    assert [getattr(eng.System, n).offset for n in ("nrows", "neq", "eq_rows", "shift", "simplify")] == [0, 4, 8, 16, 20]


def test_refusals_before_any_hip_call():
    bufs = _bufs()
    e, ws, rows, num, den = [C.cast(a, C.c_void_p) for a in bufs]
    d, s = _desc(), _sys()
    big = dict(nparm=1, bigparm=NVAR + 1)
    rat = dict(tflags=eng.T_DUAL)
    calls = [
        # null engine, workspace, descriptor, system, rows
        lambda: _load(None, ws, d, s, rows),
        lambda: _load(e, None, d, s, rows),
        lambda: _load(e, ws, None, s, rows),
        lambda: _load(e, ws, d, None, rows),
        lambda: _load(e, ws, d, s, None),
        lambda: _load(None, ws, d, s, rows, 0, 1),
        lambda: _load(e, ws, d, None, rows, 0, 1),
        lambda: _load(e, ws, d, s, None, 0, 1),
        lambda: _dual(None, ws, _desc(**rat), s, rows, num, den),
        lambda: _dual(e, None, _desc(**rat), s, rows, num, den),
        lambda: _dual(e, ws, None, s, rows, num, den),
        lambda: _dual(e, ws, _desc(**rat), None, rows, num, den),
        lambda: _dual(e, ws, _desc(**rat), s, None, num, den),
        lambda: _dual(e, ws, _desc(**rat), s, rows, None, den),
        lambda: _dual(e, ws, _desc(**rat), s, rows, num, None, 0, 1),
        # shift not in {0, 1, -1}
        lambda: _load(e, ws, d, _sys(shift=2), rows),
        lambda: _load(e, ws, _desc(**big), _sys(shift=-2), rows, 0, 1),
        lambda: _dual(e, ws, _desc(**rat), _sys(shift=3), rows, num, den),
        # a descriptor that does not match the shift
        lambda: _load(e, ws, _desc(**big), _sys(shift=0), rows),
        lambda: _load(e, ws, _desc(nparm=0, bigparm=-1), _sys(shift=1), rows),
        lambda: _load(e, ws, _desc(nparm=1, bigparm=-1), _sys(shift=-1), rows),
        lambda: _load(e, ws, _desc(nparm=2, bigparm=NVAR + 1), _sys(shift=1), rows, 0, 1),
        lambda: _load(e, ws, _desc(nparm=1, bigparm=NVAR + 1), _sys(shift=0), rows, 0, 1),
        lambda: _dual(e, ws, _desc(**big, **rat), _sys(shift=0), rows, num, den),
        lambda: _dual(e, ws, _desc(**rat), _sys(shift=-1), rows, num, den),
        # nrows < 0; neq < 0 or > nrows; ni != nrows + neq
        lambda: _load(e, ws, _desc(ni=0), _sys(nrows=-1, neq=0, eq=None), rows),
        lambda: _load(e, ws, _desc(ni=NROWS - 1), _sys(neq=-1), rows),
        lambda: _load(e, ws, _desc(ni=2 * NROWS + 1), _sys(neq=NROWS + 1), rows),
        lambda: _load(e, ws, _desc(ni=NROWS), s, rows),
        lambda: _load(e, ws, _desc(ni=NROWS + 3), s, rows, 0, 1),
        lambda: _dual(e, ws, _desc(ni=NROWS + 1, **rat), s, rows, num, den),
        # eq_rows null with neq > 0, not strictly increasing, out of range
        lambda: _load(e, ws, d, _sys(eq=None), rows),
        lambda: _load(e, ws, d, _sys(eq=(C.c_int32 * 2)(2, 0)), rows),
        lambda: _load(e, ws, d, _sys(eq=(C.c_int32 * 2)(1, 1)), rows),
        lambda: _load(e, ws, d, _sys(eq=(C.c_int32 * 2)(1, NROWS)), rows),
        lambda: _load(e, ws, d, _sys(eq=(C.c_int32 * 2)(-1, 1)), rows, 0, 1),
        lambda: _dual(e, ws, _desc(**rat), _sys(eq=(C.c_int32 * 2)(2, 2)), rows, num, den),
        # simplify not 0 or 1, or 1 without PIPAMD_T_INT
        lambda: _load(e, ws, d, _sys(simplify=2), rows),
        lambda: _load(e, ws, d, _sys(simplify=-1), rows, 0, 1),
        lambda: _load(e, ws, _desc(tflags=0), _sys(simplify=1), rows),
        lambda: _dual(e, ws, _desc(**rat), _sys(simplify=1), rows, num, den),
        # first / count outside the batch
        lambda: _load(e, ws, d, s, rows, -1, 1),
        lambda: _load(e, ws, d, s, rows, 0, -1),
        lambda: _load(e, ws, d, s, rows, BATCH, 1),
        lambda: _load(e, ws, d, s, rows, 1, BATCH),
        lambda: _load(e, ws, d, s, rows, 0, BATCH + 1),
        lambda: _dual(e, ws, _desc(**rat), s, rows, num, den, -1, 1),
        lambda: _dual(e, ws, _desc(**rat), s, rows, num, den, 1, BATCH),
        # the dual entries: no PIPAMD_T_DUAL, or PIPAMD_T_INT
        lambda: _dual(e, ws, _desc(tflags=0), s, rows, num, den),
        lambda: _dual(e, ws, _desc(tflags=eng.T_INT), s, rows, num, den),
        lambda: _dual(e, ws, _desc(tflags=eng.T_INT | eng.T_DUAL), s, rows, num, den),
        lambda: _dual(e, ws, _desc(tflags=eng.T_INT | eng.T_DUAL), s, rows, num, den, 0, 1),
    ]
    for i, call in enumerate(calls):
        assert call() == E_INVALID, i
        assert eng.lib().pipamd_last_error()
    for a in bufs:
        assert all(x == SENTINEL for x in a)  # nothing was touched


def test_python_binding_is_there():
    for name in ("load_system", "load_system_part", "dual_system", "dual_system_part"):
        assert callable(getattr(eng.Batch, name)), name
    names = eng.Batch.__init__.__code__.co_varnames
    assert "system" in names and "eq_rows" in names and "simplify" in names
