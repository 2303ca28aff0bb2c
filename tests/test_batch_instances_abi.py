"""pipamd_batch_load_instances / pipamd_batch_dual_instances and their _part forms: the entries exist -- in the library and
in the header -- without a new interface version, pipamd_instances is laid out as the binding mirrors it, and the entries
refuse what include/piplib_amd.h says they refuse before any HIP call.  Host only, no GPU: host memory full of a sentinel
stands in for the engine and the device arrays, which a refused call must leave untouched."""
import ctypes as C
import os
import re
import subprocess

import pytest

from piplib_amd import engine as eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pipamd_batch_load_instances", "pipamd_batch_load_instances_part", "pipamd_batch_dual_instances",
         "pipamd_batch_dual_instances_part"]
E_INVALID, E_TOOLARGE = -1, -3
SENTINEL = 0x5A5A5A5A5A5A5A5A
NVAR, NROWS, BATCH, NPARM = 2, 3, 4, 2


def _desc(ni=NROWS, nparm=0, bigparm=-1, tflags=eng.T_INT, nvar=NVAR):
    return eng.BatchDesc(BATCH, nvar, nparm, ni, bigparm, tflags, 4, 0, 64)


def _bufs():
    return [(C.c_int64 * 64)(*([SENTINEL] * 64)) for _ in range(6)]  # engine, workspace, matrix, points, dual_num, dual_den


_EQ = (C.c_int32 * 4)(1, 2, 0, 0)
_EQ_BAD = {"down": (C.c_int32 * 2)(2, 1), "same": (C.c_int32 * 2)(1, 1), "high": (C.c_int32 * 2)(0, NROWS),
           "negative": (C.c_int32 * 2)(-1, 1)}


def _in(arrays, nrows=NROWS, neq=0, eq=None, shift=0, simplify=0, nparm=NPARM, reserved=0):
    matrix, points = arrays
    sys = eng.System(nrows, neq, C.cast(eq, C.POINTER(C.c_int32)) if eq is not None else None, shift, simplify)
    return eng.Instances(sys, nparm, reserved, matrix, points)


def _load(engine, ws, desc, s, first=None, count=None):
    L = eng.lib()
    d = C.byref(desc) if desc is not None else None
    ss = C.byref(s) if s is not None else None
    if first is None:
        L.pipamd_batch_load_instances.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(eng.BatchDesc), C.POINTER(eng.Instances),
                                                  C.c_void_p]
        return L.pipamd_batch_load_instances(engine, ws, d, ss, None)
    return L.pipamd_batch_load_instances_part(engine, ws, d, ss, first, count, None)


def _dual(engine, ws, desc, s, num, den, first=None, count=None):
    L = eng.lib()
    d = C.byref(desc) if desc is not None else None
    ss = C.byref(s) if s is not None else None
    if first is None:
        L.pipamd_batch_dual_instances.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(eng.BatchDesc), C.POINTER(eng.Instances)] + \
            [C.c_void_p] * 3
        return L.pipamd_batch_dual_instances(engine, ws, d, ss, num, den, None)
    return L.pipamd_batch_dual_instances_part(engine, ws, d, ss, first, count, num, den, None)


@pytest.mark.parametrize("name", NAMES)
def test_exported_and_declared(name):
    assert hasattr(eng.lib(), name)
    header = open(os.path.join(ROOT, "include", "piplib_amd.h")).read()
    assert re.search(r"\bint\s+%s\s*\(\s*pipamd_engine\s*\*" % name, header)
    assert re.search(r"typedef\s+struct\s+pipamd_instances\s*\{[^}]*\bpipamd_system\s+sys\b[^}]*\bnparm\b[^}]*\breserved\b[^}]*"
                     r"\bd_matrix\b[^}]*\bd_points\b[^}]*\}\s*pipamd_instances\s*;", header)


def test_interface_version_unchanged():
    assert eng.lib().pipamd_version() == 500
    header = open(os.path.join(ROOT, "include", "piplib_amd.h")).read()
    assert re.search(r"#define\s+PIPAMD_VERSION\s+500\b", header)
    note = header[header.index("Added since"):header.index("#define PIPAMD_VERSION")]
    assert "pipamd_batch_load_instances" in note and "pipamd_batch_dual_instances" in note


def test_struct_layout_matches_the_header(tmp_path):
    """sizeof / offsetof as a C compiler sees the header against the ctypes structures of the binding"""
    mirrors = {"pipamd_instances": eng.Instances, "pipamd_system": eng.System}
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "piplib_amd.h"', "int main(void) {"]
    for s, cls in mirrors.items():
        src.append('printf("%%zu", sizeof(%s));' % s)
        src += ['printf(" %%zu", offsetof(%s, %s));' % (s, n) for n, _ in cls._fields_]
        src.append('printf("\\n");')
    src += ["return 0; }"]
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text("\n".join(src))
    subprocess.run(["gcc", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, check=True).stdout.decode().splitlines()
    for line, cls in zip(lines, mirrors.values()):
        got = [int(x) for x in line.split()]
        assert got == [C.sizeof(cls)] + [getattr(cls, n).offset for n, _ in cls._fields_], cls.__name__
    assert C.sizeof(eng.Instances) == 48
    assert [getattr(eng.Instances, n).offset for n, _ in eng.Instances._fields_] == [0, 24, 28, 32, 40]
    assert "48 bytes, offsets 0 24 28 32 40" in open(os.path.join(ROOT, "include", "piplib_amd.h")).read()


def test_refusals_before_any_hip_call():
    bufs = _bufs()
    e, ws, matrix, points, num, den = [C.cast(a, C.c_void_p) for a in bufs]
    arr = (matrix, points)
    d, s = _desc(), _in(arr)
    big = dict(nparm=1, bigparm=NVAR + 1)
    rat = dict(tflags=eng.T_DUAL)
    invalid = [
        # null engine, workspace, descriptor, `in`, matrix
        lambda: _load(None, ws, d, s),
        lambda: _load(e, None, d, s),
        lambda: _load(e, ws, None, s),
        lambda: _load(e, ws, d, None),
        lambda: _load(e, ws, d, _in((None, points))),
        lambda: _load(None, ws, d, s, 0, 1),
        lambda: _load(e, None, d, s, 0, 1),
        lambda: _load(e, ws, None, s, 0, 1),
        lambda: _load(e, ws, d, None, 0, 1),
        lambda: _load(e, ws, d, _in((None, points)), 0, 1),
        lambda: _dual(None, ws, _desc(**rat), s, num, den),
        lambda: _dual(e, None, _desc(**rat), s, num, den),
        lambda: _dual(e, ws, None, s, num, den),
        lambda: _dual(e, ws, _desc(**rat), None, num, den),
        lambda: _dual(e, ws, _desc(**rat), _in((None, points)), num, den),
        lambda: _dual(e, ws, _desc(**rat), None, num, den, 0, 1),
        # nparm < 0; reserved != 0; null points with nparm > 0
        lambda: _load(e, ws, d, _in(arr, nparm=-1)),
        lambda: _load(e, ws, d, _in(arr, nparm=-1), 0, 1),
        lambda: _load(e, ws, d, _in(arr, reserved=1)),
        lambda: _load(e, ws, d, _in(arr, reserved=-1), 0, 1),
        lambda: _load(e, ws, d, _in((matrix, None))),
        lambda: _load(e, ws, d, _in((matrix, None), nparm=1), 0, 1),
        lambda: _dual(e, ws, _desc(**rat), _in(arr, nparm=-7), num, den),
        lambda: _dual(e, ws, _desc(**rat), _in(arr, reserved=2), num, den),
        lambda: _dual(e, ws, _desc(**rat), _in((matrix, None)), num, den),
        lambda: _dual(e, ws, _desc(**rat), _in((matrix, None)), num, den, 0, 1),
        # the dual entries: a null output array
        lambda: _dual(e, ws, _desc(**rat), s, None, den),
        lambda: _dual(e, ws, _desc(**rat), s, num, None),
        lambda: _dual(e, ws, _desc(**rat), s, num, None, 0, 1),
        # shift not in {0, 1, -1}
        lambda: _load(e, ws, d, _in(arr, shift=2)),
        lambda: _load(e, ws, _desc(**big), _in(arr, shift=-2), 0, 1),
        lambda: _dual(e, ws, _desc(**rat), _in(arr, shift=3), num, den),
        # a descriptor that does not match the shift; in->nparm is not d->nparm
        lambda: _load(e, ws, _desc(**big), _in(arr, shift=0)),
        lambda: _load(e, ws, _desc(nparm=0, bigparm=-1), _in(arr, shift=1)),
        lambda: _load(e, ws, _desc(nparm=1, bigparm=-1), _in(arr, shift=-1)),
        lambda: _load(e, ws, _desc(nparm=2, bigparm=NVAR + 1), _in(arr, shift=1), 0, 1),
        lambda: _load(e, ws, _desc(nparm=NPARM, bigparm=-1), _in(arr, shift=0)),
        lambda: _dual(e, ws, _desc(**big, **rat), _in(arr, shift=0), num, den),
        lambda: _dual(e, ws, _desc(**rat), _in(arr, shift=-1), num, den),
        # nrows < 0; neq < 0 or > nrows; d->ni != nrows + neq
        lambda: _load(e, ws, _desc(ni=-1), _in(arr, nrows=-1)),
        lambda: _load(e, ws, d, _in(arr, neq=-1, eq=_EQ)),
        lambda: _load(e, ws, _desc(ni=2 * NROWS + 1), _in(arr, neq=NROWS + 1, eq=_EQ)),
        lambda: _load(e, ws, _desc(ni=NROWS + 1), s),
        lambda: _load(e, ws, _desc(ni=NROWS), _in(arr, neq=2, eq=_EQ), 0, 1),
        lambda: _dual(e, ws, _desc(ni=NROWS - 1, **rat), s, num, den),
        # eq_rows null with neq > 0, not strictly increasing, out of range
        lambda: _load(e, ws, _desc(ni=NROWS + 2), _in(arr, neq=2, eq=None)),
        lambda: _load(e, ws, _desc(ni=NROWS + 2), _in(arr, neq=2, eq=_EQ_BAD["down"])),
        lambda: _load(e, ws, _desc(ni=NROWS + 2), _in(arr, neq=2, eq=_EQ_BAD["same"]), 0, 1),
        lambda: _load(e, ws, _desc(ni=NROWS + 2), _in(arr, neq=2, eq=_EQ_BAD["high"])),
        lambda: _load(e, ws, _desc(ni=NROWS + 2), _in(arr, neq=2, eq=_EQ_BAD["negative"])),
        lambda: _dual(e, ws, _desc(ni=NROWS + 2, **rat), _in(arr, neq=2, eq=_EQ_BAD["down"]), num, den),
        # simplify not 0 or 1, or 1 without PIPAMD_T_INT
        lambda: _load(e, ws, d, _in(arr, simplify=2)),
        lambda: _load(e, ws, d, _in(arr, simplify=-1), 0, 1),
        lambda: _load(e, ws, _desc(tflags=0), _in(arr, simplify=1)),
        lambda: _dual(e, ws, _desc(**rat), _in(arr, simplify=1), num, den),
        # first / count outside the batch
        lambda: _load(e, ws, d, s, -1, 1),
        lambda: _load(e, ws, d, s, 0, -1),
        lambda: _load(e, ws, d, s, BATCH, 1),
        lambda: _load(e, ws, d, s, 1, BATCH),
        lambda: _load(e, ws, d, s, 0, BATCH + 1),
        lambda: _dual(e, ws, _desc(**rat), s, num, den, -1, 1),
        lambda: _dual(e, ws, _desc(**rat), s, num, den, 1, BATCH),
        # the dual entries: no PIPAMD_T_DUAL, or PIPAMD_T_INT
        lambda: _dual(e, ws, _desc(tflags=0), s, num, den),
        lambda: _dual(e, ws, _desc(tflags=eng.T_INT), s, num, den),
        lambda: _dual(e, ws, _desc(tflags=eng.T_INT | eng.T_DUAL), s, num, den),
        lambda: _dual(e, ws, _desc(tflags=eng.T_INT | eng.T_DUAL), s, num, den, 0, 1),
    ]
    toolarge = [
        # as the system entries: more rows than the engine holds; for the dual entries d->ni above 8,192
        lambda: _load(e, ws, _desc(ni=16001), _in(arr, nrows=16001)),
        lambda: _load(e, ws, _desc(ni=16001), _in(arr, nrows=16001), 0, 1),
        lambda: _dual(e, ws, _desc(ni=8193, **rat), _in(arr, nrows=8193), num, den),
        lambda: _dual(e, ws, _desc(ni=8193, **rat), _in(arr, nrows=8193), num, den, 0, 1),
        # nvar + nparm + 1 above 512: one column too many, far too many, and where the sum leaves int32
        lambda: _load(e, ws, d, _in(arr, nparm=512 - NVAR)),
        lambda: _load(e, ws, d, _in(arr, nparm=512 - NVAR), 0, 1),
        lambda: _load(e, ws, _desc(nvar=129), _in(arr, nparm=383)),
        lambda: _load(e, ws, d, _in(arr, nparm=2 ** 31 - 1)),
        lambda: _dual(e, ws, _desc(**rat), _in(arr, nparm=512 - NVAR), num, den),
        lambda: _dual(e, ws, _desc(**rat), _in(arr, nparm=100000), num, den, 0, 1),
    ]
    for want, calls in ((E_INVALID, invalid), (E_TOOLARGE, toolarge)):
        for i, call in enumerate(calls):
            assert call() == want, (want, i)
            assert eng.lib().pipamd_last_error()
    for a in bufs:
        assert all(x == SENTINEL for x in a)  # nothing was touched


def test_python_binding_is_there():
    for name in ("load_instances", "load_instances_part", "dual_instances", "dual_instances_part"):
        assert callable(getattr(eng.Batch, name)), name
    assert "instances" in eng.Batch.__init__.__code__.co_varnames
    assert [n for n, _ in eng.Instances._fields_] == ["sys", "nparm", "reserved", "d_matrix", "d_points"]
