"""pipamd_traiter_many / pipamd_traiter_many128: the entries exist -- in the library and in the header -- without a new
interface version, and refuse bad arguments before any HIP call.  Host only, no GPU."""
import ctypes as C
import os
import re

import pytest

from piplib_amd import engine as eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pipamd_traiter_many", "pipamd_traiter_many128"]
E_INVALID = -1


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
def test_null_engine_is_invalid(name):
    fn = getattr(eng.lib(), name)
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
    prob = (eng.PipProblem * 1)(eng.PipProblem(1, 0, 0, 0, -1, 0, None, None))
    cells, ncell, rcs = (C.c_void_p * 1)(), (C.c_size_t * 1)(), (C.c_int * 1)(7)
    assert fn(None, 1, prob, None, 0, 1, cells, ncell, rcs, None, None) == E_INVALID
    assert rcs[0] == 7 and not cells[0]  # nothing was touched
    assert fn(None, 0, None, None, 0, 1, None, None, None, None, None) == E_INVALID


def test_python_binding_is_there():
    assert callable(eng.traiter_many)
