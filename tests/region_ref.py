"""Kernel regions (RegionType / KernelGenerator): host restatements for the tests -- the offset rules written out on their
own (loops, not the engine's functions), a dictionary kernel map with its numpy inverse, and the dense cube a region kernel
embeds into, so that float64 F.conv3d / F.conv_transpose3d of the embedded kernel is the yardstick for values."""
import numpy as np
import torch


def cube_offsets(ks, dil, ts):
    """x fastest; odd sizes centred, even sizes reach forward"""
    i = np.arange(ks) - ((ks - 1) // 2 if ks % 2 else 0)
    return np.array([(x, y, z) for z in i for y in i for x in i], np.int64).reshape(-1, 3) * dil * ts


def cross_offsets(ks, dil, ts):
    """the centre first; then axis x at -h .. -1, +1 .. +h; then y; then z; times dilation * tensor stride"""
    assert ks % 2 == 1
    h = (ks - 1) // 2
    rows = [[0, 0, 0]]
    for axis in (0, 1, 2):
        for s in list(range(-h, 0)) + list(range(1, h + 1)):
            row = [0, 0, 0]
            row[axis] = s
            rows.append(row)
    assert len(rows) == 6 * h + 1
    return np.array(rows, np.int64).reshape(-1, 3) * dil * ts


def custom_offsets(rows, ts):
    """as written, times the tensor stride only"""
    return np.array(rows, np.int64).reshape(-1, 3) * ts


def dict_map(in_coords, out_coords, offsets):
    """nbr [K, Vout]: nbr[k][o] = row of in_coords at out_coords[o] + offsets[k] (first occurrence of a coordinate wins)"""
    table = {}
    for r, c in enumerate(np.asarray(in_coords).tolist()):
        table.setdefault(tuple(c), r)
    oc = np.asarray(out_coords).tolist()
    out = np.full((len(offsets), len(oc)), -1, np.int32)
    for k, (dx, dy, dz) in enumerate(np.asarray(offsets).tolist()):
        for o, (b, x, y, z) in enumerate(oc):
            out[k, o] = table.get((b, x + dx, y + dy, z + dz), -1)
    return out


def invert_np(nbr, vin):
    """inv [K, Vin]: inv[k][nbr[k][o]] = o (distinct output rows)"""
    inv = np.full((nbr.shape[0], vin), -1, np.int32)
    kk, oo = np.nonzero(nbr >= 0)
    inv[kk, nbr[kk, oo]] = oo
    return inv


def expand_np(coords, offsets):
    """every (b, xyz + offsets[k]) over the rows, in first-occurrence order of (row major, offset minor)"""
    seen, out = set(), []
    offs = np.asarray(offsets).tolist()
    for b, x, y, z in np.asarray(coords).tolist():
        for dx, dy, dz in offs:
            c = (b, x + dx, y + dy, z + dz)
            if c not in seen:
                seen.add(c)
                out.append(c)
    return np.array(out, np.int32).reshape(-1, 4)


def reach(unit_offsets):
    """r: the cube (2r + 1)^3 the offsets (in units of the tensor stride) fit in"""
    return int(np.abs(np.asarray(unit_offsets)).max()) if len(unit_offsets) else 0


def embed(W, unit_offsets, r):
    """W [K, Cin, Cout] over offsets in units of the tensor stride -> dense kernel [Cout, Cin, 2r+1, 2r+1, 2r+1] (x, y, z),
    W[k] at cell offsets[k] + r, zeros elsewhere: F.conv3d(d, embed(W), padding=r) is out[o] = sum_k x[o + off_k] W[k].
    Differentiable in W."""
    off = torch.as_tensor(np.asarray(unit_offsets)).long() + r
    assert int(off.min()) >= 0 and int(off.max()) <= 2 * r
    n = 2 * r + 1
    dw = torch.zeros((W.shape[2], W.shape[1], n, n, n), dtype=W.dtype)
    dw[:, :, off[:, 0], off[:, 1], off[:, 2]] = W.permute(2, 1, 0)
    return dw
