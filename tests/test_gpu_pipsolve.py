"""-m gpu: pip_solve(inequnk, ineqpar, Bg, options) for many problems in one call, the tableaux built on the device
(piplib_amd/csrc/pip_m2t.hip, pipamd_pip_tableaux / pipamd_pip_solve_many / pipamd_pip_solve_many128).

Authorities: tests/pipsolve_model.py for the built rows (bit for bit) and the info fields; the reference's printed text
and pivot counts stored in tests/golden/pipsolve (make_pipsolve_fixtures.py) and tests/golden/example/*.ll for the
answers; pipamd_traiter_many on the model-built problems for the cells; the CPU oracle's `pip` mode for fresh seeds."""
import functools
import glob
import os

import numpy as np
import pytest

import pipbatch as pb
import pipsolve_model as pm
from datfile import read_pip

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

E_INVALID, E_SOLVER, ST_RANGE = -1, -5, 7
TOP = (1 << 63) - 1


@pytest.fixture(scope="module")
def engines():
    from piplib_amd import engine as eng
    on, off = eng.Engine(0), eng.Engine(0)
    off.set_device_tree(False)
    return on, off


def _inp(p):
    from piplib_amd import engine as eng
    a = None if p["inequnk"] is None else np.array(p["inequnk"], dtype=np.int64)
    c = None if p["ineqpar"] is None else np.array(p["ineqpar"], dtype=np.int64)
    return eng.PipInput(a, c, p["bg"], p["options"])


def _prob(rng, nn, npar, nrow, ncrow, bg, options, eq=(), ceq=()):
    dom = rng.integers(-3, 4, size=(nrow, nn + npar + 2)).astype(np.int64)
    dom[:, 0] = 1
    dom[list(eq), 0] = 0
    ctx = rng.integers(-2, 3, size=(ncrow, npar + 2)).astype(np.int64)
    ctx[:, 0] = 1
    ctx[list(ceq), 0] = 0
    return dict(inequnk=dom, ineqpar=ctx, bg=bg, options=options)


def _width(rng, w):
    """a problem whose built domain tableau has w columns: Np = 3 + the new big parameter + 3 Urs_parms copies"""
    return _prob(rng, w - 8, 3, 3, 2, -1, pm.NQ | pm.MAXIMIZE | pm.URS_PARMS, eq=(1,), ceq=(0,))


@functools.lru_cache(maxsize=None)
def shapes():
    """the shapes at which the build kernel can go wrong, by name"""
    rng = np.random.default_rng(77)
    s = {"one row, Nn = 1, no context": [dict(inequnk=np.array([[1, 2, -6]]), ineqpar=None, bg=-1, options=pm.NQ)],
         "no rows": [dict(inequnk=np.zeros((0, 5), dtype=np.int64), ineqpar=np.zeros((0, 4), dtype=np.int64), bg=-1, options=0)],
         "all rows equalities": [_prob(rng, 3, 2, 5, 2, -1, pm.URS_UNKNOWNS, eq=range(5), ceq=range(2))],
         "an equality as first and as last row": [_prob(rng, 3, 2, 5, 1, 4, pm.MAXIMIZE, eq=(0, 4))],
         "Nl of 104 and 105": [_prob(rng, 4, 2, 100, 1, -1, pm.NQ, eq=(0, 50, 98, 99)),
                               _prob(rng, 4, 2, 100, 1, -1, pm.NQ, eq=(0, 1, 50, 98, 99))],
         "Urs_parms with Bg first, last, new": [_prob(rng, 2, 3, 4, 2, 3, pm.URS_PARMS | pm.MAXIMIZE, eq=(2,)),
                                                _prob(rng, 2, 3, 4, 2, 5, pm.URS_PARMS | pm.URS_UNKNOWNS, ceq=(1,)),
                                                _prob(rng, 2, 3, 4, 2, -1, pm.URS_PARMS | pm.MAXIMIZE, eq=(0,)),
                                                _prob(rng, 2, 3, 4, 2, 4, pm.URS_PARMS)],
         "a sum that wraps 64 bits": [dict(inequnk=np.array([[1, TOP, 1, 5, 0], [0, 1, 1, 0, 3]]), ineqpar=np.zeros((0, 3), dtype=np.int64),
                                           bg=-1, options=pm.MAXIMIZE)]}
    for w in (63, 64, 65, 127, 128, 129, 200, 512):
        s[f"{w} columns"] = [_width(rng, w)]
    s["all shapes in one ragged call"] = [p for v in list(s.values()) for p in v]
    return s


def _check_tableaux(e, probs):
    from piplib_amd import engine as eng
    infos, tabs = eng.pip_tableaux(e, [_inp(p) for p in probs])
    for k, (p, f, t) in enumerate(zip(probs, infos, tabs)):
        want, dom, ctx = pm.build(p["inequnk"], p["ineqpar"], p["bg"], p["options"])
        assert {n: f[n] for n in pm.INFO_FIELDS} == pm.info_of(want), k
        assert t[0].shape == (want["ni"], want["nvar"] + want["nparm"] + 1) and t[0].tolist() == dom, k
        assert t[1].shape == (want["nc"], want["nparm"] + 1) and t[1].tolist() == ctx, k
    return infos


@pytest.mark.parametrize("name", sorted(shapes()))
def test_tableaux_bit_for_bit(engines, name):
    infos = _check_tableaux(engines[0], shapes()[name])
    if name.endswith("columns"):
        assert infos[0]["nvar"] + infos[0]["nparm"] + 1 == int(name.split()[0])
    if name.startswith("Nl of"):
        assert [f["ni"] for f in infos] == [104, 105]


def test_wrapped_sum_is_refused_by_the_128_bit_entry(engines):
    """the 64-bit entry solves on the wrapped column (the reference's long long build); the overflow-safe flavour says
    PIPAMD_ST_RANGE for that problem and serves its neighbours"""
    from piplib_amd import engine as eng
    wrapping, plain = shapes()["a sum that wraps 64 bits"][0], shapes()["an equality as first and as last row"][0]
    true_big = pm.build(wrapping["inequnk"], wrapping["ineqpar"], -1, pm.MAXIMIZE, wrap=False)[1][0][4]
    assert true_big == 1 << 63  # the model's true integer leaves 64 bits
    out = eng.pip_solve_many(engines[0], [_inp(plain), _inp(wrapping), _inp(plain)], bits=128)
    assert (out[1][1], out[1][2]) == (E_SOLVER, ST_RANGE) and out[1][0] is None
    assert out[0][1] == out[2][1] == 0 and out[0][0] == out[2][0] and out[0][0]
    out64 = eng.pip_solve_many(engines[0], [_inp(wrapping)])
    assert out64[0][1] in (0, E_SOLVER) and out64[0][2] != ST_RANGE


def _reference_cells(e, g, bits):
    """pipamd_traiter_many on the model-built problems behind a context test of its own: (cells | None, pivots, void)"""
    from piplib_amd import engine as eng
    built = [pm.build(p["inequnk"], p["ineqpar"], p["bg"], p["options"]) for p in g]
    ctxp, mainp, flags = [], [], []
    for f, dom, ctx in built:
        if f["flags"] & pm.T_INT:
            dom, ctx = pm.simplified(dom, f["nvar"]), pm.simplified(ctx, f["nparm"])
        ctxp.append(pm.context_problem(f, ctx))
        mainp.append(pm.as_problem(f, dom, ctx))
        flags.append(f["flags"])
    ct = eng.traiter_many(e, ctxp, [pm.T_INT] * len(g), bits=bits)
    mt = eng.traiter_many(e, mainp, flags, bits=bits)
    out = []
    for (f, _, _), c, m in zip(built, ct, mt):
        assert f["nc"] > 0 and c[1] == 0  # (every golden problem has context rows)
        void = c[0][0][0] == pm.S_NIL
        cpiv = c[3]
        out.append(([] if void else m[0], cpiv + (0 if void else m[3]), void))
    return out


MODES = {"device tree": (0, 64), "host trees": (1, 64), "128 bits": (0, 128)}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(pm.FAMILIES))
def test_golden_family_in_one_call(engines, name, mode):
    from piplib_amd import engine as eng
    which, bits = MODES[mode]
    e, g = engines[which], pm.golden(name)
    out = eng.pip_solve_many(e, [_inp(p) for p in g], bits=bits)
    served, back = e.last_device_tree()
    want = _reference_cells(e, g, bits)
    for k, (p, (cells, rc, st, piv, info), (wcells, wpiv, wvoid)) in enumerate(zip(g, out, want)):
        assert rc == 0, (k, rc, st)
        assert pb.squash(pm.quast_text(cells, info, p["inequnk"])) == pb.squash(p["text"]), k
        assert piv == p["pivots"], (k, piv, p["pivots"])
        assert bool(info["is_void"]) == wvoid == (p["text"].strip() == "void"), k
        assert cells == wcells and piv == wpiv, k
        assert {n: info[n] for n in pm.INFO_FIELDS if n != "is_void"} == \
               {n: v for n, v in pm.info_of(pm.plan(p["inequnk"], p["ineqpar"], p["bg"], p["options"])).items() if n != "is_void"}, k
    if which == 1:
        assert (served, back) == (0, 0)
    elif name == "p3":
        assert served >= 1  # a condition, not a measurement: the device tree takes problems from the built buffer


def test_device_tree_hands_back_what_the_lockstep_entry_does(engines):
    """the same problems, model-built, through pipamd_solve_tableaux_lockstep: the device tree in front of it serves and
    hands back as many (the lock-step entry has no Compute_dual: the rational + Dual problems stay out of both calls)"""
    from piplib_amd import engine as eng
    e = engines[0]
    g = [p for p in pm.golden("p3") + pm.golden("p8") if not (p["options"] & pm.DUAL) or (p["options"] & pm.NQ)]
    out = eng.pip_solve_many(e, [_inp(p) for p in g])
    mine = e.last_device_tree()
    built = [pm.as_problem(*pm.build(p["inequnk"], p["ineqpar"], p["bg"], p["options"])) for p in g]
    ref = eng.solve_tableaux(e, built, simplify=True, lockstep=True)
    theirs = e.last_device_tree()
    assert mine == theirs and mine[0] >= 1 and sum(mine) == len(g)
    for k, ((cells, rc, st, piv, info), (text, rc2, st2, piv2)) in enumerate(zip(out, ref)):
        assert (rc, piv) == (rc2, piv2), k
        assert eng.tape_text(cells) == text, k


def test_reference_examples_in_one_call(engines):
    """the 15 inputs of the reference's example suite (example/Makefile.am) against its .ll files"""
    from piplib_amd import engine as eng
    names = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(pb.ROOT, "tests", "golden", "example", "*.pip")))
    assert len(names) == 15
    probs = []
    for n in names:
        ctx, bignum, dom, opts = read_pip(os.path.join(pb.ROOT, "tests", "golden", "example", n + ".pip"))
        options = (pm.NQ if opts.get("Nq", 1) else 0) | (pm.MAXIMIZE if opts.get("Maximize") else 0) | \
                  (pm.URS_PARMS if opts.get("Urs_parms") else 0) | (pm.URS_UNKNOWNS if opts.get("Urs_unknowns") else 0) | \
                  (pm.DUAL if opts.get("Compute_dual") else 0)
        bg = bignum + dom.shape[1] - ctx.shape[1] if bignum > 0 else bignum  # example.c gives it in context columns
        probs.append(dict(inequnk=dom, ineqpar=ctx, bg=bg, options=options))
    out = eng.pip_solve_many(engines[0], [_inp(p) for p in probs])
    for n, p, (cells, rc, st, piv, info) in zip(names, probs, out):
        want = open(os.path.join(pb.ROOT, "tests", "golden", "example", n + ".ll"), encoding="latin-1").read()
        assert rc == 0, n
        assert pb.squash(pm.quast_text(cells, info, p["inequnk"])) == pb.squash(pm.quast_part(want)), n


def test_ragged_call_keeps_every_problem_to_itself(engines):
    from piplib_amd import engine as eng
    e = engines[0]
    g = pm.golden("p3")
    inbox = [p for p in g if p["text"].strip() != "void"][:6]
    empty = next(p for p in g if p["text"].strip() == "void")
    wide = shapes()["129 columns"][0]
    null = dict(inequnk=None, ineqpar=empty["ineqpar"], bg=-1, options=pm.NQ)
    bad = dict(inequnk=inbox[0]["inequnk"], ineqpar=inbox[0]["ineqpar"], bg=1, options=pm.NQ)
    probs = [inbox[0], null, inbox[1], empty, bad, inbox[2], wide, inbox[3], inbox[4], inbox[5]]
    out = eng.pip_solve_many(e, [_inp(p) for p in probs])
    alone = [eng.pip_solve_many(e, [_inp(p)])[0] for p in probs]
    assert [(o[0], o[1], o[2], o[3]) for o in out] == [(o[0], o[1], o[2], o[3]) for o in alone]
    assert out[1][1] == 0 and out[1][0] == [] and out[1][4]["is_void"] == 1
    assert out[3][1] == 0 and out[3][0] == [] and out[3][4]["is_void"] == 1
    assert out[4][1] == E_INVALID and out[4][0] is None
    assert out[6][1] == 0 and out[6][4]["nvar"] + out[6][4]["nparm"] + 1 == 129
    for k in (0, 2, 5, 7, 8, 9):
        p, (cells, rc, st, piv, info) = probs[k], out[k]
        assert rc == 0 and piv == p["pivots"], k
        assert pb.squash(pm.quast_text(cells, info, p["inequnk"])) == pb.squash(p["text"]), k


@pytest.mark.parametrize("seed", [9001, 9002, 9003])
def test_fresh_seeds_against_the_cpu_oracle(engines, seed):
    from piplib_amd import engine as eng
    fam = pm.gen_family("p3", seed, count=32, exe=pb.ORACLEPIP)
    out = eng.pip_solve_many(engines[0], [_inp(p) for p, _, _ in fam])
    for k, ((p, text, _), (cells, rc, st, piv, info)) in enumerate(zip(fam, out)):
        assert rc == 0, (k, rc, st)
        assert pb.squash(pm.quast_text(cells, info, p["inequnk"])) == pb.squash(text), k
