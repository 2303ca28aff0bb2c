"""piplib_amd/csrc/pip_source.h -- what the batch layer's front ends refuse and how they fill the PipBatchSource their launch
reads -- on the CPU against a model of include/piplib_amd.h's rules: tests/batch_source_main.cpp includes that header
alone, is built with the host compiler under the address and undefined-behaviour sanitizers and run as a child process.

The descriptions are those of the test_batch_*_abi.py files -- a good one per form, and each of its fields made wrong in
turn, for the load and for the dual -- and the row counts 0, 1 and PIPAMD_SMAX with equalities at row 0 and at the last
row, where the mask's first and last bit are written.  The device pointers are addresses of nothing and the equality list
is a heap block of exactly its length: a check that read behind either would stop the program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_INVALID, E_TOOLARGE = 0, -1, -3
T_INT, T_DUAL = 1, 2
SMAX, MAXCOL, DUAL_MAXNI = 16000, 512, 8192
SHIFTED, SYSTEM, SPARSE, INSTANCES, MATRICES, TABLEAU = range(6)
K_TABLEAU, K_DENSE, K_MATRICES, K_CSR, K_INSTANCES = range(5)
WHO = ["batch_load_shifted", "batch_load_system", "batch_load_sparse", "batch_load_instances", "batch_load_matrices", "batch_dual"]
FIELDS = ("form dual e ws d nvar nparm ni bigparm tflags desc rows nrows shift simplify a b c num den eq_list neq").split()


def case(form, dual=0, **kw):
    """a description every check accepts, then `kw`; eq: the equality list"""
    c = dict(form=form, dual=dual, e=1, ws=1, d=1, nvar=2, nparm=0, ni=3, bigparm=-1, tflags=T_DUAL if dual else T_INT, desc=1,
             rows=1, nrows=3, shift=0, simplify=0, a=0, b=0, c=0, num=1, den=1, eq_list=1, neq=None, eq=())
    if form == SHIFTED:
        c.update(nparm=1, bigparm=3, shift=1)
    elif form == SPARSE:
        c.update(a=5, b=1, c=1)      # nnz, cols, vals
    elif form == INSTANCES:
        c.update(a=2, b=0, c=1)      # nparm, reserved, points
    elif form == MATRICES:
        c.update(a=0, b=1, ni=6)     # reserved, d_nrows
    c.update(kw)
    if c["neq"] is None:
        c["neq"] = len(c["eq"])
        if form in (SYSTEM, SPARSE, INSTANCES) and "ni" not in kw:
            c["ni"] = c["nrows"] + c["neq"]
    return c


def model(c):
    """(return code, the source's fields as batch_source_main prints them, the mask's rows)"""
    g = lambda k: c[k]  # noqa: E731
    form, shift = g("form"), g("shift")
    big = g("nparm") == 1 and g("bigparm") == g("nvar") + 1

    def simplify():
        return g("simplify") not in (0, 1) or (g("simplify") and not g("tflags") & T_INT)

    def plain():
        if not (g("e") and g("ws") and g("d") and g("desc") and g("rows")) or shift not in (0, 1, -1):
            return True
        return not big if shift else (g("nparm") != 0 or g("bigparm") != -1)

    def system():
        if plain():
            return E_INVALID
        if g("nrows") < 0 or g("neq") < 0 or g("neq") > g("nrows") or g("ni") != g("nrows") + g("neq"):
            return E_INVALID
        if g("nrows") > SMAX:
            return E_TOOLARGE
        if (g("neq") > 0 and not g("eq_list")) or simplify():
            return E_INVALID
        eq = g("eq")[:g("neq")]
        if any(r < 0 or r >= g("nrows") or (i > 0 and r <= eq[i - 1]) for i, r in enumerate(eq)):
            return E_INVALID
        return OK

    kind, rows, tail, mask = K_DENSE, 1, [0] * 9, list(g("eq")[:g("neq")])
    if form == SHIFTED:
        if not (g("e") and g("ws") and g("d")) or shift not in (1, -1) or not big or not g("rows"):
            return E_INVALID, None, None
        head, mask = [shift, 0, g("ni")], []
    elif form == TABLEAU:
        kind, head, rows, mask = K_TABLEAU, [0, 0, 0], g("rows"), []
    elif form == MATRICES:
        if plain() or g("nrows") < 1 or g("ni") < 1 or g("a") != 0:
            return E_INVALID, None, None
        if g("nrows") > SMAX:
            return E_TOOLARGE, None, None
        if simplify():
            return E_INVALID, None, None
        kind, head, tail, mask = K_MATRICES, [shift, g("simplify"), g("nrows")], [0] * 7 + [g("b"), g("nrows")], []
    else:
        rc = system()
        if rc == OK and form == SPARSE and (g("a") < 0 or (g("a") > 0 and not (g("b") and g("c")))):
            rc = E_INVALID
        if rc == OK and form == INSTANCES:
            if g("a") < 0 or g("b") != 0 or (g("a") > 0 and not g("c")):
                rc = E_INVALID
            elif g("nvar") + g("a") + 1 > MAXCOL:
                rc = E_TOOLARGE
        if rc:
            return rc, None, None
        head = [shift, g("simplify"), g("nrows")]
        if form == SPARSE:
            kind, rows, tail = K_CSR, 0, [1, g("b"), g("c"), g("a")] + [0] * 5
        elif form == INSTANCES:
            kind, rows, tail = K_INSTANCES, 0, [0] * 4 + [1, g("c"), g("a")] + [0] * 2
    if g("dual"):
        if not g("d") or (form == TABLEAU and not g("rows")) or not g("num") or not g("den"):
            return E_INVALID, None, None
        if not g("tflags") & T_DUAL or g("tflags") & T_INT:
            return E_INVALID, None, None
        if g("ni") > DUAL_MAXNI:
            return E_TOOLARGE, None, None
        if form == TABLEAU and (g("nparm") != 0 or g("bigparm") >= 0):
            return E_INVALID, None, None
    return OK, [kind] + head + [rows] + tail, mask


def cases():
    out = []
    for dual in (0, 1):
        for form in (SHIFTED, SYSTEM, SPARSE, INSTANCES, MATRICES, TABLEAU):
            if (form == SHIFTED and dual) or (form == TABLEAU and not dual):
                continue
            base = case(form, dual)
            out.append(base)
            # every pointer missing in turn, the shift and the descriptor against it, simplify, the dual's flags and bound
            wrong = [dict(e=0), dict(ws=0), dict(d=0), dict(desc=0), dict(rows=0), dict(num=0), dict(den=0), dict(shift=2),
                     dict(shift=-2), dict(shift=0 if base["shift"] else 1), dict(nparm=1, bigparm=3), dict(nparm=1, bigparm=-1),
                     dict(nparm=2, bigparm=3), dict(shift=1, nparm=1, bigparm=3), dict(shift=-1, nparm=1, bigparm=3),
                     dict(simplify=1), dict(simplify=2), dict(simplify=-1), dict(simplify=1, tflags=0), dict(tflags=0),
                     dict(tflags=T_INT | T_DUAL), dict(ni=DUAL_MAXNI, nrows=DUAL_MAXNI), dict(ni=DUAL_MAXNI + 1, nrows=DUAL_MAXNI + 1),
                     # the rows: counts, equalities that do not add up, the engine's limit, the list
                     dict(nrows=-1, ni=-1), dict(neq=-1), dict(ni=4), dict(ni=2), dict(nrows=3, neq=4, ni=7, eq=(0, 1, 2, 3)),
                     dict(nrows=SMAX + 1, ni=SMAX + 1), dict(nrows=SMAX, ni=SMAX), dict(eq=(1, 2), eq_list=0), dict(eq=(2, 1)),
                     dict(eq=(1, 1)), dict(eq=(0, 3)), dict(eq=(-1, 1)), dict(eq=(0, 2)), dict(eq=(0, 1, 2)),
                     # the forms' own fields
                     dict(a=-1), dict(a=1), dict(b=0), dict(c=0), dict(b=1), dict(a=0, b=0, c=0), dict(a=0, c=0),
                     dict(nvar=MAXCOL - 3, a=2), dict(nvar=MAXCOL - 2, a=2), dict(nrows=0, ni=0), dict(nrows=1, ni=0),
                     dict(nrows=3, ni=0)]
            out += [case(form, dual, **kw) for kw in wrong]
    # 0, 1 and PIPAMD_SMAX rows, equalities at row 0 and at the last row: the mask's first and last bit
    for form in (SYSTEM, SPARSE, INSTANCES):
        for dual in (0, 1):
            out += [case(form, dual, nrows=0), case(form, dual, nrows=1), case(form, dual, nrows=1, eq=(0,)),
                    case(form, dual, nrows=65, eq=(0, 63, 64)), case(form, dual, nrows=SMAX, eq=(0, SMAX - 1)),
                    case(form, dual, nrows=SMAX, eq=(SMAX - 1,)), case(form, dual, nrows=SMAX, eq=(0, SMAX)),
                    case(form, dual, nrows=SMAX, eq=tuple(range(0, SMAX, 63)))]
    out += [case(MATRICES, d, nrows=1, ni=1) for d in (0, 1)] + [case(MATRICES, d, nrows=SMAX, ni=SMAX // 2) for d in (0, 1)]
    out += [case(SHIFTED, ni=0), case(SHIFTED, ni=SMAX, shift=-1), case(TABLEAU, 1, ni=0), case(TABLEAU, 1, ni=DUAL_MAXNI)]
    return out


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("batch_source") / "batch_source")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "batch_source_main.cpp"), "-o", exe],
                   check=True, timeout=300)
    cs = cases()
    text = "".join(" ".join(str(c[k]) for k in FIELDS) + " %d %s\n" % (len(c["eq"]), " ".join(map(str, c["eq"]))) for c in cs)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(cs)
    return list(zip(cs, lines))


def test_cases_hold_the_edges():
    cs = cases()
    got = [model(c) for c in cs]
    assert {rc for rc, _, _ in got} == {OK, E_INVALID, E_TOOLARGE}
    for form in (SYSTEM, SPARSE, INSTANCES):
        for dual in (0, 1):
            masks = [(c["nrows"], m) for c, (rc, _, m) in zip(cs, got) if rc == OK and c["form"] == form and c["dual"] == dual]
            assert (0, []) in masks and (1, []) in masks and (1, [0]) in masks and (65, [0, 63, 64]) in masks
            # (a dual of PIPAMD_SMAX rows is refused for its ni, behind the form's check that has written the mask)
            assert dual or (SMAX, [0, SMAX - 1]) in masks


def test_refusals_and_sources(answers):
    """the return code, the entry's name at the head of a refusal's message, and every member of the source's kind"""
    for c, line in answers:
        rc, src, mask = model(c)
        part = [p.strip() for p in line.split("|")]
        assert int(part[0]) == rc, (c, line[:200])
        if rc:
            assert len(part) == 2 and part[1].startswith(WHO[c["form"]] + ": "), (c, line)
        else:
            assert part[1] == "" and [int(x) for x in part[2].split() + part[3].split()] == src, (c, line[:200], src)
            assert [int(x) for x in part[4].split()] == mask, (c, mask[:8])
