"""Serial reference of ME.farthest_point_sampling: numpy, one sample at a time, coordinates in the CALLER's row order.

Pick 0 of a sample is start[b] (its lowest row without `start`); pick j is the row farthest from the nearest of the picks
0 .. j-1; np.argmax returns the first of equal values and a sample's rows are walked in ascending caller row, so the lowest row
wins a tie; rows already picked have distance 0 and take part like any other.  Integer coordinates: int64 arithmetic, exact.
Float coordinates: float32, d = (dx*dx + dy*dy) + dz*dz, each numpy operation rounding once (no FMA)."""
import numpy as np


def fps_ref(coords, num_samples, start=None):
    """coords [V, 4] (batch index first), an integer or a float array -> int64 [B, M], B = the batch indices present, ascending"""
    c = np.asarray(coords)
    integer = c.dtype.kind in "iu"
    batch = c[:, 0].astype(np.int64)
    present = np.unique(batch)
    out = np.empty((present.size, num_samples), np.int64)
    for i, bi in enumerate(present):
        rows = np.flatnonzero(batch == bi)
        p = c[rows, 1:4].astype(np.int64 if integer else np.float32)
        nearest = np.full(rows.size, np.iinfo(np.int64).max if integer else np.inf, p.dtype)
        pick = 0 if start is None else int(np.flatnonzero(rows == int(start[i]))[0])
        for j in range(num_samples):
            if j:
                d = p - p[pick]
                d = d * d
                nearest = np.minimum(nearest, (d[:, 0] + d[:, 1]) + d[:, 2])
                assert nearest.dtype == p.dtype
                pick = int(np.argmax(nearest))
            out[i, j] = rows[pick]
    return out


def lattice(n=4, seed=0, batch=0):
    """the full n x n x n lattice as int32 [n^3, 4], rows shuffled"""
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3)
    g = g[np.random.default_rng(seed).permutation(g.shape[0])]
    return np.concatenate([np.full((g.shape[0], 1), batch), g], 1).astype(np.int32)


def random_voxels(lengths, seed=0, side=40, batch_indices=None, interleave=True):
    """distinct random voxels, lengths[b] of them for sample b, as int32 [V, 4]; rows of the samples interleaved"""
    rng = np.random.default_rng(seed)
    parts = []
    for b, n in enumerate(lengths):
        s = side
        while s ** 3 < 2 * n:
            s *= 2
        cells = rng.choice(s ** 3, size=n, replace=False)
        xyz = np.stack([cells // (s * s), (cells // s) % s, cells % s], 1) - s // 2
        bi = b if batch_indices is None else batch_indices[b]
        parts.append(np.concatenate([np.full((n, 1), bi), xyz], 1))
    c = np.concatenate(parts).astype(np.int32)
    return c[rng.permutation(c.shape[0])] if interleave else c
