"""Sparse rows (CSR) of plain systems for the sparse batch entries (pipamd_batch_load_sparse, pipamd_batch_dual_sparse):
the conversion from the dense systems the other entries take, and the small systems of the byte-identity test.  Test
helper only."""
import numpy as np


def to_csr(dense_rows, stored=None):
    """dense_rows: (batch, nrows, nvar + 1) int64, unknowns then constant.  -> (row_ptr int64 [batch * nrows + 1],
    cols int32 [nnz], vals int64 [nnz]): the entries that are not zero, and those `stored` (a boolean array of the same
    shape) marks even where they are zero; a row's columns increase strictly, the constant is column nvar"""
    a = np.ascontiguousarray(dense_rows, dtype=np.int64)
    flat = a.reshape(-1, a.shape[-1])
    keep = flat != 0
    if stored is not None:
        keep |= np.asarray(stored, dtype=bool).reshape(flat.shape)
    row_ptr = np.zeros(len(flat) + 1, np.int64)
    row_ptr[1:] = np.cumsum(keep.sum(axis=1))
    r, c = np.nonzero(keep)  # (row-major: by row, then by column)
    return row_ptr, c.astype(np.int32), flat[r, c].copy()


def to_dense(row_ptr, cols, vals, batch, nrows, nvar):
    """the dense expansion of well-formed CSR arrays: (batch, nrows, nvar + 1) int64"""
    out = np.zeros((batch * nrows, nvar + 1), np.int64)
    for r in range(batch * nrows):
        for e in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            out[r, cols[e]] = vals[e]
    return out.reshape(batch, nrows, nvar + 1)


def edge_systems(nvar, nrows, seed, batch=3):
    """(dense rows (batch, nrows, nvar + 1), stored mask): small systems whose rows are, in turn, empty, the constant
    alone, one unknown alone (the last one in one system, the first in the next), every column stored, and sparse rows of
    one to four unknowns and a constant; one stored zero in the sparse rows of every system; values of either sign"""
    rng = np.random.default_rng(seed)
    a = np.zeros((batch, nrows, nvar + 1), np.int64)
    stored = np.zeros(a.shape, bool)
    for b in range(batch):
        for r in range(nrows):
            kind = (r + b) % 5
            if kind == 1:
                a[b, r, nvar] = rng.integers(-9, 10) or 5
            elif kind == 2:
                a[b, r, (nvar - 1) if b % 2 == 0 else 0] = rng.integers(2, 9) * (-1) ** r
            elif kind == 3:
                a[b, r] = rng.integers(1, 7, nvar + 1) * rng.choice([-2, 2, 4], nvar + 1)  # (a common factor: tab_simplify)
            elif kind == 4:
                k = rng.choice(nvar, size=min(nvar - 1, int(rng.integers(1, 5))), replace=False)
                a[b, r, k] = rng.integers(1, 6, len(k)) * rng.choice([-3, 3], len(k))
                a[b, r, nvar] = rng.integers(-12, 13)
                stored[b, r, rng.choice(np.flatnonzero(a[b, r, :nvar] == 0))] = True
            # kind 0: no entry at all
    return a, stored
