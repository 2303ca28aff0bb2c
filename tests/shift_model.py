"""The two transformations around a solve under a new big parameter, in Python ints: what tab_Matrix2Tableau writes for
Maximize / Urs_unknowns (tab.c:342-377) and what sol_vector_edit undoes in the answer (sol.c:435-512).  The model the
shifted batch entries (pipamd_batch_load_shifted, pipamd_batch_results_shifted) are held to.  Test helper only."""
from math import gcd

SHIFT_MAX, SHIFT_URS = 1, -1


def shift_rows(rows, shift):
    """rows: sequence of plain inequalities a_0 .. a_(n-1) | c  ->  shift > 0: -a_j | c | +sum a_j;  shift < 0: a_j | c | -sum a_j"""
    out = []
    for r in rows:
        a, c = [int(v) for v in r[:-1]], int(r[-1])
        out.append([-v for v in a] + [c, sum(a)] if shift > 0 else a + [c, -sum(a)])
    return out


def decode(big, cst, den, shift):
    """one unknown: big and constant numerators, denominator -> (x_num, x_den) in lowest terms, x_den == 0: unbounded"""
    big, cst, den = int(big), int(cst), int(den)
    g = gcd(cst, den)
    num = cst // g
    return (-num if shift > 0 else num), (den // g if big == den else 0)
