"""The batch layer's front ends share one body per step (csrc/pip_source.h, load_from / dual_from in csrc/pip_host.cpp): what
that sharing must not blur.  Host only, no GPU.

1. A refused call reports under the name of the entry that was called.  The refused calls are those the six
   test_batch_*_abi.py files list: their refusal tests run here once more against a library whose front-end entries look
   at pipamd_last_error() after every call that did not return PIPAMD_OK.
2. An empty part (count == 0) inside the batch is checked like any other part and then returns PIPAMD_OK without a HIP
   call and without a look at the engine, the workspace or the arrays, which host memory full of a sentinel stands in
   for.  (The whole-batch entries forward the descriptor's batch, which is never 0, as the count.)"""
import collections
import ctypes as C
import re

import pytest

import test_batch_dual_abi
import test_batch_instances_abi
import test_batch_matrices_abi
import test_batch_shift_abi
import test_batch_sparse_abi
import test_batch_system_abi
from piplib_amd import engine as eng

FORMS = ("system", "matrices", "sparse", "instances")
ENTRIES = ["pipamd_batch_%s_%s%s" % (op, f, p) for op in ("load", "dual") for f in FORMS for p in ("", "_part")] + \
    ["pipamd_batch_load_shifted", "pipamd_batch_load_shifted_part", "pipamd_batch_dual", "pipamd_batch_dual_part"]
SENTINEL = 0x5A5A5A5A5A5A5A5A
NVAR, NROWS, BATCH = 2, 3, 4


def who(entry):
    """pipamd_batch_load_sparse_part -> batch_load_sparse: the name the entry and its whole-batch form report under"""
    return re.sub(r"^pipamd_|_part$", "", entry)


class _Entry:
    """a front-end entry of the library; argtypes and the like go to the real function"""

    def __init__(self, L, name, refused):
        self.__dict__.update(L=L, name=name, fn=getattr(L, name), refused=refused)

    def __setattr__(self, k, v):
        setattr(self.fn, k, v)

    def __getattr__(self, k):
        return getattr(self.fn, k)

    def __call__(self, *a):
        rc = self.fn(*a)
        if rc != 0:
            msg = self.L.pipamd_last_error().decode()
            assert re.match(r"%s(_part)?: " % who(self.name), msg), (self.name, a, rc, msg)
            self.refused[self.name] += 1
        return rc


class _Lib:
    def __init__(self, L, refused):
        self.__dict__.update(L=L, refused=refused)

    def __getattr__(self, name):
        return _Entry(self.L, name, self.refused) if name in ENTRIES else getattr(self.L, name)


def test_a_refusal_names_the_entry_that_was_called(monkeypatch):
    refused = collections.Counter()
    real = eng.lib()
    monkeypatch.setattr(eng, "lib", lambda: _Lib(real, refused))
    for mod in (test_batch_system_abi, test_batch_matrices_abi, test_batch_sparse_abi, test_batch_instances_abi,
                test_batch_shift_abi):
        mod.test_refusals_before_any_hip_call()
    for name in test_batch_dual_abi.NAMES:
        test_batch_dual_abi.test_null_arguments_are_invalid(name)
    assert set(refused) == set(ENTRIES), set(ENTRIES) ^ set(refused)  # every entry was refused something, under its name


def _desc(ni, tflags):
    return eng.BatchDesc(BATCH, NVAR, 0, ni, -1, tflags, 4, 0, 64)


@pytest.mark.parametrize("first", [0, 1, BATCH])
def test_an_empty_part_is_ok_and_touches_nothing(first):
    L = eng.lib()
    bufs = [(C.c_int64 * 64)(*([SENTINEL] * 64)) for _ in range(8)]
    e, ws, rows, aux, cols, vals, num, den = [C.cast(a, C.c_void_p) for a in bufs]
    eq = (C.c_int32 * 2)(0, NROWS - 1)
    sys = eng.System(NROWS, 2, C.cast(eq, C.POINTER(C.c_int32)), 0, 0)
    descs = {"load": _desc(NROWS + 2, eng.T_INT), "dual": _desc(NROWS + 2, eng.T_DUAL)}
    source = {"system": [C.byref(sys), rows],
              "matrices": [C.byref(eng.Matrices(NROWS, 0, 0, 0, aux)), rows],
              "sparse": [C.byref(eng.Sparse(sys, 5, rows, cols, vals))],
              "instances": [C.byref(eng.Instances(sys, 2, 0, rows, aux))]}
    out = {"load": [], "dual": [num, den]}
    for op in ("load", "dual"):
        for form in FORMS:
            fn = getattr(L, "pipamd_batch_%s_%s_part" % (op, form))
            assert fn(e, ws, C.byref(descs[op]), *source[form], first, 0, *out[op], None) == 0, (op, form, L.pipamd_last_error())
    shifted = eng.BatchDesc(BATCH, NVAR, 1, NROWS, NVAR + 1, eng.T_INT, 4, 0, 64)
    assert L.pipamd_batch_load_shifted_part(e, ws, C.byref(shifted), rows, eng.SHIFT_MAX, first, 0, None) == 0, L.pipamd_last_error()
    assert L.pipamd_batch_dual_part(e, ws, C.byref(_desc(NROWS, eng.T_DUAL)), rows, first, 0, num, den, None) == 0, L.pipamd_last_error()
    for a in bufs:
        assert all(x == SENTINEL for x in a)
