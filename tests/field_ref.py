"""Numpy restatements of the point <-> voxel layer family (TensorField quantisation, slice, trilinear interpolation): the
expectation the GPU tests compare the engine against.  Sets, maps and weights are restated exactly (integers; float32
operations in the order the header states); voxel features as a sequential float32 loop over the points in ascending index;
interpolated values and their gradient in float64.  tests/test_field_cpu.py pins these restatements against dense float64 torch
(grid_sample, index_add_)."""
import numpy as np
import torch
import torch.nn.functional as F

AVG, SUM, MAX, FIRST = 0, 1, 2, 3
LO, HI = -16384, 16384              # the packable coordinate range
MAX_BATCH = 0x7FFFF


def voxel_of(points, ts):
    """int64 [N, 4]: batch index taken as an integer, floor(p / ts) * ts per axis (float32 division: exact, ts is a power of
    two)"""
    p = np.asarray(points)
    if p.dtype.kind == "f":
        xyz = np.floor(p[:, 1:].astype(np.float32) / np.float32(ts)).astype(np.int64) * ts
    else:
        xyz = (p[:, 1:].astype(np.int64) // ts) * ts
    return np.concatenate([p[:, :1].astype(np.int64), xyz], 1)


def quantize_np(points, ts):
    """-> (coords int32 [V, 4] in first-occurrence order of the points, inverse int64 [N], first int64 [V]: the first point of
    every voxel)"""
    q = voxel_of(points, ts)
    seen, first = {}, []
    inverse = np.empty(len(q), np.int64)
    for n, c in enumerate(map(tuple, q.tolist())):
        r = seen.get(c)
        if r is None:
            r = seen[c] = len(first)
            first.append(n)
        inverse[n] = r
    first = np.asarray(first, np.int64)
    return q[first].astype(np.int32).reshape(-1, 4), inverse, first


def reduce_np(mode, feats, inverse, n_vox):
    """voxel features as the kernel is specified: the points of a voxel in ascending index; sum = a chain of float32 additions
    from 0, average = that sum divided once by float32(count), max = the first point, then every strictly greater one
    -> (out float32 [V, C], arg int64 [V, C] (max: the winning point), count int64 [V])"""
    feats = np.asarray(feats, np.float32)
    out = np.zeros((n_vox, feats.shape[1]), np.float32)
    arg = np.full((n_vox, feats.shape[1]), -1, np.int64)
    count = np.bincount(inverse, minlength=n_vox).astype(np.int64)
    if mode == FIRST:
        started = np.zeros(n_vox, bool)
        for n, v in enumerate(inverse):
            if not started[v]:
                out[v], started[v] = feats[n], True
        return out, arg, count
    started = np.zeros(n_vox, bool)
    for n, v in enumerate(inverse):
        if mode == MAX:
            better = feats[n] > out[v] if started[v] else np.ones(feats.shape[1], bool)
            out[v] = np.where(better, feats[n], out[v])
            arg[v] = np.where(better, n, arg[v])
            started[v] = True
        else:
            out[v] = out[v] + feats[n]
    if mode == AVG:
        out = out / count.astype(np.float32)[:, None]
    return out, arg, count


def reduce_backward_np(mode, dvox, inverse, arg, count):
    """float32 [N, C]: one division or one selection per element"""
    dvox = np.asarray(dvox, np.float32)
    g = dvox[inverse]
    if mode == AVG:
        return g / count[inverse].astype(np.float32)[:, None]
    if mode == MAX:
        return np.where(arg[inverse] == np.arange(len(inverse))[:, None], g, np.float32(0))
    return g


def interp_map_np(coords, points, ts):
    """-> (rows int32 [8, N], weights float32 [8, N]) as ms3d_interp_map states them: q = p / ts, f = floor(q), r = q - f in
    float32; corner j = bx + 2 by + 4 bz at (f + b) * ts with weight (wx * wy) * wz, w = r for the high corner and 1 - r for the
    low one; rows -1 for an absent corner, a corner or batch index outside the packable range, and every corner of a point
    with a non-finite entry (whose weights are 0)"""
    table = {}
    for r, c in enumerate(map(tuple, np.asarray(coords).tolist())):
        table.setdefault(c, r)
    p = np.asarray(points, np.float32)
    n = len(p)
    rows = np.full((8, n), -1, np.int32)
    weights = np.zeros((8, n), np.float32)
    finite = np.isfinite(p).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
        q = p[:, 1:] / np.float32(ts)
        f = np.floor(q)
        r = q - f
        for j in range(8):
            b = np.array([j & 1, (j >> 1) & 1, j >> 2])
            w = np.where(b[None, :] == 1, r, np.float32(1) - r).astype(np.float32)
            weights[j] = np.where(finite, (w[:, 0] * w[:, 1]) * w[:, 2], np.float32(0))
            corner = (f + b[None, :].astype(np.float32)) * np.float32(ts)
            ok = finite & (corner >= LO).all(1) & (corner < HI).all(1) & (p[:, 0] >= 0) & (p[:, 0] < MAX_BATCH + 1)
            for i in np.nonzero(ok)[0]:
                rows[j, i] = table.get((int(p[i, 0]), int(corner[i, 0]), int(corner[i, 1]), int(corner[i, 2])), -1)
    return rows, weights


def interp_np(x, rows, weights):
    """float64 [N, C]: sum over the corners present of weight * row"""
    x = np.asarray(x, np.float64)
    out = np.zeros((rows.shape[1], x.shape[1]), np.float64)
    for j in range(8):
        has = rows[j] >= 0
        out[has] += weights[j, has].astype(np.float64)[:, None] * x[rows[j, has]]
    return out


def interp_backward_np(dout, rows, weights, n_vox):
    """float64 [V, C]: the gradient of interp_np with respect to x"""
    dout = np.asarray(dout, np.float64)
    din = np.zeros((n_vox, dout.shape[1]), np.float64)
    for j in range(8):
        has = rows[j] >= 0
        np.add.at(din, rows[j, has], weights[j, has].astype(np.float64)[:, None] * dout[has])
    return din


def grid_sample64(dense, origin, points, ts):
    """the yardstick of the yardstick: float64 F.grid_sample (mode="bilinear" on a 5-D input is trilinear, padding_mode=
    "zeros", align_corners=True) of the dense tensor `dense` [B, C, Gx, Gy, Gz] -- laid out as sparse_ref.densify lays it out,
    cell (i, j, k) holding the voxel at (origin + (i, j, k)) * ts -- at the float points [N, 4] -> [N, C].  The grid must keep
    one empty cell of margin around the set.  A point whose batch index the dense tensor lacks gets zeros.  Differentiable
    with respect to `dense`."""
    B, C, gx, gy, gz = dense.shape
    p = torch.as_tensor(np.asarray(points, np.float64))
    out = torch.zeros((len(p), C), dtype=torch.float64)
    pieces = []
    for b in range(B):
        sel = torch.nonzero(p[:, 0].long() == b).view(-1)
        if sel.numel() == 0:
            continue
        idx = p[sel, 1:] / ts - origin                                # fractional cell index per axis (x, y, z)
        size = torch.tensor([gx, gy, gz], dtype=torch.float64)
        norm = 2.0 * idx / (size - 1) - 1.0
        grid = norm[:, [2, 1, 0]].view(1, -1, 1, 1, 3)                # grid_sample wants (W, H, D) = (z, y, x)
        val = F.grid_sample(dense[b:b + 1], grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        pieces.append((sel, val.view(C, -1).t()))
    for sel, val in pieces:
        out = out.index_put((sel,), val)
    return out
