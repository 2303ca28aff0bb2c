"""Whole problems at the 64-bit overflow line of the device-resident traiter() (piplib_amd/csrc/pip_quast.hip), for
tests/test_gpu_device_tree_overflow.py.  numpy and Python ints only; TEST INFRASTRUCTURE.

The problems have no parameters, so nothing forks: the tree is sort, then classify, pivot and cut until done, and
`chain()` below is that loop over the step models of tests/quast_step_model.py.  Each family is a pair around one flip
point: the largest coefficient M is chosen so that the first intermediate of the chain to leave 64 bits is of the kind the
family is named after -- a cross product of the pivot-column tournament, a product of the elimination, the determinant's
limbs -- and with M - 1 nothing leaves 64 bits.  At 128 bits nothing does either way.  tests/test_device_tree_overflow_model.py
(no GPU) holds those statements, and the chain's answers to the 128-bit oracle.
"""
from dataclasses import dataclass

import numpy as np

import bigint_pip as bp
import device_tree_edges as dte
import quast_step_model as qm


@dataclass
class Chained:
    cls: str        # fits | must | may at the width asked for
    stage: str      # must: the step whose intermediate left the width
    status: int     # bp.ST_SOLUTION | bp.ST_NIL (fits / may)
    pivots: int
    cuts: int
    num: list
    den: list


def problem(rows, nq=1):
    T = np.array(rows, dtype=np.int64)
    return dte.Problem(T.shape[1] - 1, 0, T.shape[0], 0, -1, nq, T, np.zeros((0, 1), np.int64))


def chain(p, Wb):
    """traiter() (traiter.c:628-791) on a problem without parameters, over the step models"""
    nvar, ni, ncol = p.nvar, p.ni, p.nvar + 1
    rows = [[int(x) for x in r] for r in p.ineq]
    spare = 64
    c = qm.Case("chain", qm.QS_SOLVE_PLAIN, nvar, ncol, [qm.UNIT] * nvar + [qm.UNKNOWN] * ni + [qm.ZERO] * spare,
                list(range(nvar)) + list(range(ni)) + [0] * spare, [1] * (nvar + ni + spare), rows + [[0] * ncol for _ in range(spare)],
                nligne=nvar + ni, ni=ni)
    o = qm._image(c, 1)
    trk = qm.Trk(Wb)
    pivots = cuts = 0
    status = None
    try:
        assert qm.sort_rows(o, nvar, nvar + ni, False, True) == 0
        while status is None:
            nligne = nvar + ni
            pivi = next((i for i in range(nligne) if o.flag[i] & qm.MINUS), nligne)
            if pivi >= nligne:
                pivi = qm.classify_rows(o, nvar, ncol, -1, nligne)
            if pivi >= nligne:
                assert not any(o.flag[i] & (qm.UNKNOWN | qm.CRITIC) for i in range(nligne))   # no parameters: nothing forks
                if not p.nq:
                    status = bp.ST_SOLUTION
                    break
                for i in range(nvar):   # integrer.c:305-534, constant cuts
                    if (o.flag[i] & qm.UNIT) or o.den[i] == 1:
                        continue
                    cut, ok = qm.make_cut(o, i, nvar, ncol, -1, ncol)
                    if not ok & 2:
                        continue
                    if not ok & 1:
                        status = bp.ST_NIL
                        break
                    o.val[ni][:] = cut
                    o.flag[nligne], o.ref[nligne], o.den[nligne] = qm.MINUS, ni, o.den[i]
                    pivi, ni, cuts = nligne, ni + 1, cuts + 1
                    break
                else:
                    status = bp.ST_SOLUTION
                if status is not None:
                    break
            pivots += 1
            assert pivots < 1000
            if qm.pivot_step(o, pivi, nvar, ncol, nvar + ni, trk) < 0:
                status = bp.ST_NIL
    except qm.Must as m:
        return Chained("must", m.args[0], None, pivots, cuts, None, None)
    num = [0 if o.flag[i] & qm.UNIT else o.val[o.ref[i]][nvar] for i in range(nvar)]
    den = [1 if o.flag[i] & qm.UNIT else o.den[i] for i in range(nvar)]
    return Chained("may" if trk.may else "fits", "", status, pivots, cuts, num, den)


# family -> (rows as a function of M, integer solve?, the flip point M, the step that leaves 64 bits at M)
_C = 1 << 31
FAMILIES = {
    # x0 >= 1 + C x1 + M x2 brings (1 | C | M) to logical row 0 without a product; the second pivot row (0 | C | 3) ties columns
    # 1 and 2 there, and the tournament forms C * M = 2^63; its elimination has multipliers (1, 1)
    "tournament": (lambda M: [[1, -_C, -M, -1], [0, _C, 3, -5]], 1, 1 << 32, "tournament"),
    "tournament_rational": (lambda M: [[1, -_C, -M, -1], [0, _C, 3, -5]], 0, 1 << 32, "tournament"),
    # the first elimination multiplies M by M: just past the 32-bit path's operands, M * M >= 2^63 from 3037000500 on
    "elimination_square": (lambda M: [[M, 1, -3], [1, M, -5], [1, 1, -1]], 1, 3037000500, "elimination"),
    "elimination_three": (lambda M: [[M, 1, 1, -3], [1, M, 1, -5], [1, 1, M, -7]], 1, 3037000500, "elimination"),
    "elimination_late": (lambda M: [[M, -1, -1], [-1, M, -1]], 1, 2097153, "elimination"),
    # four pivots of M on a diagonal: 31-bit pivots share limbs two by two, 32-bit ones take a limb each and the fourth finds none
    "determinant": (lambda M: [[M, 0, 0, 0, -1], [0, M, 0, 0, -1], [0, 0, M, 0, -1], [0, 0, 0, M, -1]], 0, 1 << 31, "determinant"),
}


def members():
    """name -> (problem, the family, M, at the flip point?)"""
    out = {}
    for name, (rows, nq, M, _) in FAMILIES.items():
        out["%s_at" % name] = (problem(rows(M), nq), name, M, True)
        out["%s_below" % name] = (problem(rows(M - 1), nq), name, M - 1, False)
    return out
