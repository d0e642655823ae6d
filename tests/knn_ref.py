"""Serial reference of ME.knn_query: numpy, one query at a time, coordinates in the CALLER's row order.

For a query at position p of sample b: the distances from p to every row of sample b of the support set, the rows lexsorted by
(distance, caller row), the first k taken, the cap applied afterwards (slots farther than the cap become -1 / -1 or +inf; they
are the last ones, the order being ascending).  Integer coordinates: int64 arithmetic, exact.  Float coordinates: float32,
d = (dx*dx + dy*dy) + dz*dz with dx = q.x - p.x, each numpy operation rounding once (no FMA)."""
import numpy as np


def knn_ref(support, k, queries, cap=None):
    """support [V, 4], queries [NQ, 4] (batch index first; both integer arrays or both float arrays): every query searches the
    rows of `support` with its batch index VALUE -> (int64 [NQ, k] rows of support, int64 / float32 [NQ, k] distances)"""
    c, qs = np.asarray(support), np.asarray(queries)
    integer = c.dtype.kind in "iu"
    assert integer == (qs.dtype.kind in "iu")
    kind = np.int64 if integer else np.float32
    none = -1 if integer else np.inf
    rows_of = {int(bi): np.flatnonzero(c[:, 0] == bi) for bi in np.unique(c[:, 0])}
    idx = np.full((qs.shape[0], k), -1, np.int64)
    d2 = np.full((qs.shape[0], k), none, kind)
    for i in range(qs.shape[0]):
        rows = rows_of[int(qs[i, 0])]
        d = qs[i, 1:4].astype(kind)[None, :] - c[rows, 1:4].astype(kind)
        d = d * d
        d = (d[:, 0] + d[:, 1]) + d[:, 2]
        assert d.dtype == kind
        first = np.lexsort((rows, d))[:k]                 # the last key is the primary one: distance, then caller row
        idx[i, :first.size], d2[i, :first.size] = rows[first], d[first]
        if cap is not None:
            far = d2[i] > (cap if integer else np.float32(cap))
            idx[i, far], d2[i, far] = -1, none
    return idx, d2


def knn_forms(support, k, rows=None, other=None, cap=None):
    """the three forms of knn_query over caller-order arrays: every row of support ([V, k]); rows: an integer array [B, M] of
    rows of support ([B, M, k]); other: a coordinate array [NQ, 4] like support ([NQ, k])"""
    c = np.asarray(support)
    if rows is not None:
        rows = np.asarray(rows)
        idx, d2 = knn_ref(c, k, c[rows.reshape(-1)], cap)
        return idx.reshape(rows.shape + (k,)), d2.reshape(rows.shape + (k,))
    return knn_ref(c, k, c if other is None else np.asarray(other), cap)
