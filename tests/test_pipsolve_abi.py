"""pipamd_pip_tableaux / pipamd_pip_solve_many / pipamd_pip_solve_many128: the entries exist -- in the library, the header
and the Python binding -- without a new interface version, their structures are laid out as the header says, and a
malformed problem gets PIPAMD_E_INVALID in its own rcs[i] before any HIP call.  Host only, no GPU: zeroed host memory
stands in for the engine (no problem of these calls reaches the device)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from piplib_amd import engine as eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pipamd_pip_tableaux", "pipamd_pip_solve_many", "pipamd_pip_solve_many128"]
E_INVALID = -1
OK_ROW = np.array([[1, 1, -1, 4]], dtype=np.int64)  # Nn = 1, Np = 1
OK_CTX = np.zeros((0, 3), dtype=np.int64)


@pytest.mark.parametrize("name", NAMES)
def test_exported_and_declared(name):
    assert hasattr(eng.lib(), name)
    header = open(os.path.join(ROOT, "include", "piplib_amd.h")).read()
    assert re.search(r"\bint\s+%s\s*\(\s*pipamd_engine\s*\*" % name, header)


def test_interface_version_unchanged():
    assert eng.lib().pipamd_version() == 500
    header = open(os.path.join(ROOT, "include", "piplib_amd.h")).read()
    assert re.search(r"#define\s+PIPAMD_VERSION\s+500\b", header)


def test_option_bits_as_the_header_numbers_them():
    header = open(os.path.join(ROOT, "include", "piplib_amd.h")).read()
    for name, bit in (("NQ", eng.PIP_NQ), ("MAXIMIZE", eng.PIP_MAXIMIZE), ("URS_PARMS", eng.PIP_URS_PARMS),
                      ("URS_UNKNOWNS", eng.PIP_URS_UNKNOWNS), ("DUAL", eng.PIP_DUAL)):
        assert re.search(r"#define\s+PIPAMD_PIP_%s\s+%d\b" % (name, bit), header), name


def test_struct_layout_matches_the_header(tmp_path):
    """sizeof / offsetof as a C compiler sees the header against the ctypes structures of the binding"""
    fields = {"pipamd_pip_problem": [n for n, _ in eng.PipSolveProblem._fields_],
              "pipamd_pip_info": [n for n, _ in eng.PipInfo._fields_]}
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "piplib_amd.h"', "int main(void) {"]
    for s, names in fields.items():
        src.append('printf("%%zu", sizeof(%s));' % s)
        src += ['printf(" %%zu", offsetof(%s, %s));' % (s, n) for n in names]
        src.append('printf("\\n");')
    src += ["return 0; }"]
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text("\n".join(src))
    subprocess.run(["gcc", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, check=True).stdout.decode().splitlines()
    for line, cls in zip(lines, (eng.PipSolveProblem, eng.PipInfo)):
        got = [int(x) for x in line.split()]
        assert got == [C.sizeof(cls)] + [getattr(cls, n).offset for n, _ in cls._fields_], cls.__name__
    assert C.sizeof(eng.PipSolveProblem) == 40 and C.sizeof(eng.PipInfo) == 48


def test_python_binding_is_there():
    assert callable(eng.pip_tableaux) and callable(eng.pip_solve_many)


class FakeEngine:
    """zeroed host memory where the engine would be: the calls below return before they would use it"""

    def __init__(self):
        self.mem = (C.c_char * 65536)()
        self._h = C.cast(self.mem, C.c_void_p)


@pytest.mark.parametrize("bits", [64, 128])
def test_null_arguments_fail_the_call(bits):
    fn = getattr(eng.lib(), "pipamd_pip_solve_many128" if bits == 128 else "pipamd_pip_solve_many")
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6
    e = FakeEngine()
    prob, info = (eng.PipSolveProblem * 1)(), (eng.PipInfo * 1)()
    cells, ncell, rcs = (C.c_void_p * 1)(), (C.c_size_t * 1)(), (C.c_int * 1)(7)
    assert fn(None, 1, prob, 0, 1, info, cells, ncell, rcs, None, None) == E_INVALID
    assert fn(e._h, -1, prob, 0, 1, info, cells, ncell, rcs, None, None) == E_INVALID
    for hole in range(5):
        args = [prob, info, cells, ncell, rcs]
        args[hole] = None
        assert fn(e._h, 1, args[0], 0, 1, *args[1:], None, None) == E_INVALID, hole
    assert rcs[0] == 7  # nothing was touched
    assert fn(e._h, 0, None, 0, 1, None, None, None, None, None, None) == 0  # n == 0 is PIPAMD_OK


MALFORMED = {
    "ncols < 2": eng.PipInput(np.zeros((1, 1), dtype=np.int64)),
    "ctx_cols of 1": eng.PipInput(OK_ROW, np.zeros((0, 1), dtype=np.int64)),
    "Nn < 0": eng.PipInput(np.zeros((1, 3), dtype=np.int64), np.zeros((0, 4), dtype=np.int64)),
    "bg is an unknown": eng.PipInput(OK_ROW, OK_CTX, bg=1),
    "bg beyond the parameters": eng.PipInput(OK_ROW, OK_CTX, bg=3),
    "bg below -1": eng.PipInput(OK_ROW, OK_CTX, bg=-2),
    "bg without parameters": eng.PipInput(np.array([[1, 1, 4]], dtype=np.int64), None, bg=2),
    "unknown option bits": eng.PipInput(OK_ROW, OK_CTX, options=32),
    "negative nrows": eng.PipInput(OK_ROW, OK_CTX, shape=(-1, 4, 0, 3)),
    "negative ctx_rows": eng.PipInput(OK_ROW, OK_CTX, shape=(1, 4, -1, 3)),
    "negative ncols": eng.PipInput(OK_ROW, OK_CTX, shape=(1, -4, 0, 3)),
    "ineqpar missing": eng.PipInput(OK_ROW, None, shape=(1, 4, 2, 3)),
    "context rows without columns": eng.PipInput(OK_ROW, None, shape=(1, 4, 2, 0)),
    "more than 512 columns": eng.PipInput(np.ones((1, 514), dtype=np.int64)),
    "512 columns and a new big parameter": eng.PipInput(np.ones((1, 513), dtype=np.int64), options=eng.PIP_MAXIMIZE),
}


@pytest.mark.parametrize("bits", [64, 128])
def test_malformed_problems_are_refused_one_by_one(bits):
    """each malformed problem gets PIPAMD_E_INVALID in its own rcs[i]; the void one beside them is PIPAMD_OK"""
    probs = list(MALFORMED.values()) + [eng.PipInput(None, OK_CTX)]
    out = eng.pip_solve_many(FakeEngine(), probs, bits=bits)
    for name, (cells, rc, st, piv, info) in zip(MALFORMED, out):
        assert rc == E_INVALID and cells is None and info["nvar"] == -1, name
    cells, rc, st, piv, info = out[-1]
    assert rc == 0 and cells == [] and info["is_void"] == 1 and piv == 0


def test_tableaux_refuses_malformed_before_any_hip_call():
    infos, tabs = eng.pip_tableaux(FakeEngine(), list(MALFORMED.values()) + [eng.PipInput(None)])
    assert all(t is None for t in tabs)
    assert [f["nvar"] for f in infos] == [-1] * len(MALFORMED) + [0] and infos[-1]["is_void"] == 1
