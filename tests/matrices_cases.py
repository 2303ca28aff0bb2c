"""Shared by the tests of the matrices batch entries (pipamd_batch_load_matrices, pipamd_batch_dual_matrices): ragged
batches of PolyLib matrices.  A family starts from shift_cases.plain_rows' systems -- the ones the existing goldens use --
and has a short list of classes (kept row indices, equality positions among the kept rows); the classes are dealt to the
systems by a seeded permutation.  System b's room of max_rows x (nvar + 2) words holds marker | row for its kept rows and
JUNK in every word beyond, so that a kernel that reads past a system's rows shows up in the result.  The model of system
b is system_model.tableau(kept rows, equalities, shift, simplify): nothing new is modelled.  Test helper only."""
import functools
from collections import namedtuple

import numpy as np

import shift_cases as sc
import system_model as sy

JUNK = 0x0123456789ABCDEF  # (as a marker: an inequality; as a coefficient: far beyond what a solve survives)
KW = dict(nnz=3, cmax=4, x0max=6)      # tests/test_gpu_batch_system.py's WIDE
KW5 = dict(nnz=3, cmax=3, x0max=5)     # s5's (tests/golden/make_system_fixtures.py)
# t3: every row holds with equality at the hidden point, so that systems with equalities around row 64 have solutions
# (with the default slack of 0 .. 3 per row, three equalities out of 65 rows over 3 unknowns are next to never feasible)
KW3 = dict(nnz=3, cmax=4, x0max=6, slackmax=0)


def _r5_classes(box):
    """one-row systems, the full system with and without a last-row equality, an all-equality system that fills the room
    exactly (2 * rows == ni), and mid-sized systems with their equalities in different places; box: the five rows
    -x_j + 12 >= 0 behind the eight generated ones"""
    if not box:  # 8 rows; the room is ni = 10
        return [((3,), ()), ((5,), (0,)), (tuple(range(8)), ()), (tuple(range(8)), (7,)),
                ((0, 1, 2, 3, 4), (0, 1, 2, 3, 4)), ((0, 2, 3, 5, 6, 7), (1, 4)), ((1, 2, 4, 5, 6), (0, 3)),
                (tuple(range(8)), (0, 4))]
    bx = (8, 9, 10, 11, 12)  # 13 rows; the room is ni = 14
    return [((3,), ()), ((5,), (0,)), (tuple(range(13)), ()), (tuple(range(13)), (12,)),
            ((0, 1, 2, 3, 4, 8, 9), (0, 1, 2, 3, 4, 5, 6)), ((0, 2, 3, 5, 6, 7) + bx, (1, 4)), ((1, 2, 4, 5, 6) + bx, (0, 3)),
            (tuple(range(7)) + bx, (0, 4))]


def _t3_classes(box):
    """63, 64, 65 and 70 rows around the edge of a 64-row mask word, with the equality sets {}, {0, 63}, {62, 63, 64} and
    {64}: each set goes to the shortest class that has its rows ({62, 63, 64} ends the 65-row system: its last
    equality is the first bit of the second word and its negation ends the tableau)"""
    return [(tuple(range(63)), ()), (tuple(range(64)), (0, 63)), (tuple(range(65)), (62, 63, 64)), (tuple(range(70)), (64,))]


def _w70_classes(box):
    return [(tuple(range(82)), (0, 11)), (tuple(range(40)), (39,)), (tuple(range(5, 82)), (3, 70))]


def _w131_classes(box):
    return [(tuple(range(139)), (3,)), (tuple(range(100)), (0, 99)), (tuple(range(2, 139)), ())]


def _bulk12_classes(box):
    return [(tuple(range(22)), (2, 9)), (tuple(range(22)), ()), (tuple(range(1, 22)), (1,)), (tuple(range(10)), (9,)),
            ((0, 2, 4, 6, 8) + tuple(range(10, 22)), (0, 3)), (tuple(range(3, 20)), (4, 5))]


# name -> (seed, nvar, generated rows, batch, keywords, classes(box), seed of the class permutation, boxes it has)
FAMILIES = {"r5": (41, 5, 8, 40, KW5, _r5_classes, 14, (0, 1)),  # (14: the first seed tests/golden/make_matrices_fixtures.py accepts)
            "t3": (45, 3, 67, 12, KW3, _t3_classes, 1, (1,)),
            "w70": (43, 70, 12, 16, KW, _w70_classes, 1, (1,)),
            "w131": (44, 131, 8, 8, KW, _w131_classes, 1, (1,)),
            "bulk12": (42, 12, 10, 2048, KW, _bulk12_classes, 1, (1,))}

Family = namedtuple("Family", "name box nvar max_rows ni room nrows classes cls systems")
# room: (batch, max_rows, nvar + 2) int64, read-only; nrows: (batch,) int32; ni: rows of the tallest tableau;
# classes: [(kept, eq)]; cls: (batch,) the class of each system; systems: [(kept rows as lists, eq)] per system


@functools.lru_cache(maxsize=None)
def family(name, box, perm_seed=None):
    seed, nvar, n, batch, kw, classes_of, pseed, boxes = FAMILIES[name]
    assert box in boxes
    plain = sc.plain_rows(seed, nvar, n, batch, kw, box)
    max_rows = plain.shape[1]
    classes = classes_of(box)
    for kept, eq in classes:
        assert 1 <= len(kept) <= max_rows and all(0 <= r < max_rows for r in kept) and all(0 <= p < len(kept) for p in eq)
    perm = np.random.default_rng(pseed if perm_seed is None else perm_seed).permutation(batch)
    cls = np.empty(batch, np.int64)
    cls[perm] = np.arange(batch) % len(classes)
    room = np.full((batch, max_rows, nvar + 2), JUNK, np.int64)
    nrows = np.empty(batch, np.int32)
    systems = []
    for b in range(batch):
        kept, eq = classes[cls[b]]
        rows = plain[b, list(kept)]
        nrows[b] = len(kept)
        room[b, :len(kept), 0] = 1
        room[b, list(eq), 0] = 0
        room[b, :len(kept), 1:] = rows
        systems.append((rows.tolist(), eq))
    room.setflags(write=False)
    nrows.setflags(write=False)
    cls.setflags(write=False)
    ni = max(len(kept) + len(eq) for kept, eq in classes)
    return Family(name, box, nvar, max_rows, ni, room, nrows, classes, cls, systems)


def members(fam, c):
    """the systems of class c, in batch order"""
    return [int(b) for b in np.nonzero(fam.cls == c)[0]]


def class_rows(fam, c):
    """(the plain rows of class c's systems, (members, nrows_c, nvar + 1) int64; its equality rows): what the uniform
    entry pipamd_batch_load_system takes"""
    kept, eq = fam.classes[c]
    return np.array([fam.systems[b][0] for b in members(fam, c)], dtype=np.int64).reshape(-1, len(kept), fam.nvar + 1), eq


def tableaux(fam, c, shift, simp):
    """the model's tableaux of class c's systems: (members, nrows_c + neq_c, ncol) int64"""
    rows, eq = class_rows(fam, c)
    return sy.tableaux(rows, eq, shift, simp)
