"""pipamd_batch_load_matrices / pipamd_batch_dual_matrices and their _part forms: the entries exist -- in the library and in
the header -- without a new interface version, the Python binding has them, and they refuse what include/piplib_amd.h
says they refuse before any HIP call.  Host only, no GPU: host memory full of a sentinel stands in for the engine and the
device arrays, which a refused call must leave untouched."""
import ctypes as C
import os
import re

import pytest

from piplib_amd import engine as eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pipamd_batch_load_matrices", "pipamd_batch_load_matrices_part", "pipamd_batch_dual_matrices",
         "pipamd_batch_dual_matrices_part"]
E_INVALID, E_TOOLARGE = -1, -3
SENTINEL = 0x5A5A5A5A5A5A5A5A
NVAR, MAXROWS, BATCH = 2, 3, 4


def _desc(ni=2 * MAXROWS, nparm=0, bigparm=-1, tflags=eng.T_INT):
    return eng.BatchDesc(BATCH, NVAR, nparm, ni, bigparm, tflags, 4, 0, 64)


def _bufs():
    return [(C.c_int64 * 64)(*([SENTINEL] * 64)) for _ in range(6)]  # engine, workspace, rows, nrows, dual_num, dual_den


def _mat(nrows, max_rows=MAXROWS, shift=0, simplify=0, reserved=0):
    return eng.Matrices(max_rows, shift, simplify, reserved, nrows)


def _load(engine, ws, desc, m, rows, first=None, count=None):
    L = eng.lib()
    d = C.byref(desc) if desc is not None else None
    mm = C.byref(m) if m is not None else None
    if first is None:
        L.pipamd_batch_load_matrices.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(eng.BatchDesc), C.POINTER(eng.Matrices),
                                                 C.c_void_p, C.c_void_p]
        return L.pipamd_batch_load_matrices(engine, ws, d, mm, rows, None)
    return L.pipamd_batch_load_matrices_part(engine, ws, d, mm, rows, first, count, None)


def _dual(engine, ws, desc, m, rows, num, den, first=None, count=None):
    L = eng.lib()
    d = C.byref(desc) if desc is not None else None
    mm = C.byref(m) if m is not None else None
    if first is None:
        L.pipamd_batch_dual_matrices.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(eng.BatchDesc), C.POINTER(eng.Matrices)] + \
            [C.c_void_p] * 4
        return L.pipamd_batch_dual_matrices(engine, ws, d, mm, rows, num, den, None)
    return L.pipamd_batch_dual_matrices_part(engine, ws, d, mm, rows, first, count, num, den, None)


@pytest.mark.parametrize("name", NAMES)
def test_exported_and_declared(name):
    assert hasattr(eng.lib(), name)
    header = open(os.path.join(ROOT, "include", "piplib_amd.h")).read()
    assert re.search(r"\bint\s+%s\s*\(\s*pipamd_engine\s*\*" % name, header)
    assert re.search(r"typedef\s+struct\s+pipamd_matrices\s*\{[^}]*\bmax_rows\b[^}]*\bshift\b[^}]*\bsimplify\b[^}]*\breserved\b[^}]*"
                     r"\bd_nrows\b[^}]*\}\s*pipamd_matrices\s*;", header)


def test_interface_version_unchanged():
    assert eng.lib().pipamd_version() == 500
    header = open(os.path.join(ROOT, "include", "piplib_amd.h")).read()
    assert re.search(r"#define\s+PIPAMD_VERSION\s+500\b", header)
    note = header[header.index("Added since"):header.index("#define PIPAMD_VERSION")]
    assert "pipamd_batch_load_matrices" in note and "pipamd_batch_dual_matrices" in note


def test_matrices_struct_layout():
    """int32 max_rows, shift, simplify, reserved | pointer d_nrows: as the header's struct on an LP64 target"""
    assert C.sizeof(eng.Matrices) == 24
    assert [getattr(eng.Matrices, n).offset for n in ("max_rows", "shift", "simplify", "reserved", "d_nrows")] == [0, 4, 8, 12, 16]
    header = open(os.path.join(ROOT, "include", "piplib_amd.h")).read()
    assert "24 bytes, offsets 0 4 8 12 16" in header


def test_badinput_status():
    header = open(os.path.join(ROOT, "include", "piplib_amd.h")).read()
    assert re.search(r"#define\s+PIPAMD_ST_BADINPUT\s+10\b", header)
    assert eng.ST_BADINPUT == 10


def test_refusals_before_any_hip_call():
    bufs = _bufs()
    e, ws, rows, nrows, num, den = [C.cast(a, C.c_void_p) for a in bufs]
    d, m = _desc(), _mat(nrows)
    big = dict(nparm=1, bigparm=NVAR + 1)
    rat = dict(tflags=eng.T_DUAL)
    invalid = [
        # null engine, workspace, descriptor, m, rows
        lambda: _load(None, ws, d, m, rows),
        lambda: _load(e, None, d, m, rows),
        lambda: _load(e, ws, None, m, rows),
        lambda: _load(e, ws, d, None, rows),
        lambda: _load(e, ws, d, m, None),
        lambda: _load(None, ws, d, m, rows, 0, 1),
        lambda: _load(e, ws, None, m, rows, 0, 1),
        lambda: _load(e, ws, d, None, rows, 0, 1),
        lambda: _load(e, ws, d, m, None, 0, 1),
        lambda: _dual(None, ws, _desc(**rat), m, rows, num, den),
        lambda: _dual(e, None, _desc(**rat), m, rows, num, den),
        lambda: _dual(e, ws, None, m, rows, num, den),
        lambda: _dual(e, ws, _desc(**rat), None, rows, num, den),
        lambda: _dual(e, ws, _desc(**rat), m, None, num, den),
        lambda: _dual(e, ws, _desc(**rat), m, None, num, den, 0, 1),
        # the dual entries: a null output array
        lambda: _dual(e, ws, _desc(**rat), m, rows, None, den),
        lambda: _dual(e, ws, _desc(**rat), m, rows, num, None),
        lambda: _dual(e, ws, _desc(**rat), m, rows, num, None, 0, 1),
        # shift not in {0, 1, -1}
        lambda: _load(e, ws, d, _mat(nrows, shift=2), rows),
        lambda: _load(e, ws, _desc(**big), _mat(nrows, shift=-2), rows, 0, 1),
        lambda: _dual(e, ws, _desc(**rat), _mat(nrows, shift=3), rows, num, den),
        # a descriptor that does not match the shift
        lambda: _load(e, ws, _desc(**big), _mat(nrows, shift=0), rows),
        lambda: _load(e, ws, _desc(nparm=0, bigparm=-1), _mat(nrows, shift=1), rows),
        lambda: _load(e, ws, _desc(nparm=1, bigparm=-1), _mat(nrows, shift=-1), rows),
        lambda: _load(e, ws, _desc(nparm=2, bigparm=NVAR + 1), _mat(nrows, shift=1), rows, 0, 1),
        lambda: _load(e, ws, _desc(nparm=1, bigparm=NVAR + 1), _mat(nrows, shift=0), rows, 0, 1),
        lambda: _dual(e, ws, _desc(**big, **rat), _mat(nrows, shift=0), rows, num, den),
        lambda: _dual(e, ws, _desc(**rat), _mat(nrows, shift=-1), rows, num, den),
        # max_rows < 1; d->ni < 1
        lambda: _load(e, ws, d, _mat(nrows, max_rows=0), rows),
        lambda: _load(e, ws, d, _mat(nrows, max_rows=-1), rows, 0, 1),
        lambda: _load(e, ws, _desc(ni=0), m, rows),
        lambda: _load(e, ws, _desc(ni=-1), m, rows, 0, 1),
        lambda: _dual(e, ws, _desc(**rat), _mat(nrows, max_rows=0), rows, num, den),
        lambda: _dual(e, ws, _desc(ni=0, **rat), m, rows, num, den),
        # reserved != 0
        lambda: _load(e, ws, d, _mat(nrows, reserved=1), rows),
        lambda: _load(e, ws, d, _mat(nrows, reserved=-1), rows, 0, 1),
        lambda: _dual(e, ws, _desc(**rat), _mat(nrows, reserved=7), rows, num, den),
        # simplify not 0 or 1, or 1 without PIPAMD_T_INT
        lambda: _load(e, ws, d, _mat(nrows, simplify=2), rows),
        lambda: _load(e, ws, d, _mat(nrows, simplify=-1), rows, 0, 1),
        lambda: _load(e, ws, _desc(tflags=0), _mat(nrows, simplify=1), rows),
        lambda: _dual(e, ws, _desc(**rat), _mat(nrows, simplify=1), rows, num, den),
        # first / count outside the batch
        lambda: _load(e, ws, d, m, rows, -1, 1),
        lambda: _load(e, ws, d, m, rows, 0, -1),
        lambda: _load(e, ws, d, m, rows, BATCH, 1),
        lambda: _load(e, ws, d, m, rows, 1, BATCH),
        lambda: _load(e, ws, d, m, rows, 0, BATCH + 1),
        lambda: _dual(e, ws, _desc(**rat), m, rows, num, den, -1, 1),
        lambda: _dual(e, ws, _desc(**rat), m, rows, num, den, 1, BATCH),
        # the dual entries: no PIPAMD_T_DUAL, or PIPAMD_T_INT
        lambda: _dual(e, ws, _desc(tflags=0), m, rows, num, den),
        lambda: _dual(e, ws, _desc(tflags=eng.T_INT), m, rows, num, den),
        lambda: _dual(e, ws, _desc(tflags=eng.T_INT | eng.T_DUAL), m, rows, num, den),
        lambda: _dual(e, ws, _desc(tflags=eng.T_INT | eng.T_DUAL), m, rows, num, den, 0, 1),
        # ... and the same with no row counts (d_nrows NULL is not a refusal; what is wrong here is the rest)
        lambda: _load(e, ws, d, _mat(None, reserved=1), rows),
        lambda: _dual(e, ws, _desc(tflags=0), _mat(None), rows, num, den),
    ]
    toolarge = [
        # max_rows above the engine's 16,000 rows; for the dual entries d->ni above 8,192
        lambda: _load(e, ws, d, _mat(nrows, max_rows=16001), rows),
        lambda: _load(e, ws, d, _mat(nrows, max_rows=16001), rows, 0, 1),
        lambda: _dual(e, ws, _desc(**rat), _mat(nrows, max_rows=16001), rows, num, den),
        lambda: _dual(e, ws, _desc(ni=8193, **rat), m, rows, num, den),
        lambda: _dual(e, ws, _desc(ni=8193, **rat), m, rows, num, den, 0, 1),
    ]
    for want, calls in ((E_INVALID, invalid), (E_TOOLARGE, toolarge)):
        for i, call in enumerate(calls):
            assert call() == want, (want, i)
            assert eng.lib().pipamd_last_error()
    for a in bufs:
        assert all(x == SENTINEL for x in a)  # nothing was touched


def test_python_binding_is_there():
    for name in ("load_matrices", "load_matrices_part", "dual_matrices", "dual_matrices_part"):
        assert callable(getattr(eng.Batch, name)), name
    names = eng.Batch.__init__.__code__.co_varnames
    assert "matrices" in names and "nrows" in names and "ni" in names
