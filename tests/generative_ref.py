"""Host restatements for the generative layers (coordinate generation, pruning): numpy only, nothing of the engine.

The expected output set of a generative transposed convolution is restated twice: `expand_np` (candidates c = i * K + k, first
occurrence wins -- the ORDER the engine promises) and `dense_support` (the support of F.conv_transpose3d of the occupancy
indicator with an all-ones kernel, float64 -- the SET, from an operator that knows nothing about sparse tensors)."""
import numpy as np
import torch
import torch.nn.functional as F

# (kernel size, stride, dilation) of the generative layers under test, and the input tensor strides each is run at
GEOMS = [(2, 2, 1), (3, 2, 1), (4, 2, 1), (2, 2, 2), (3, 1, 1), (3, 1, 2), (5, 1, 1)]


def strides_for(stride):
    return (2, 4) if stride == 2 else (1, 2)


def offsets_np(ks, dil, ts):
    """k = ix + ks iy + ks^2 iz; odd sizes centred, even sizes reaching forward; times dilation * tensor stride"""
    i = np.arange(ks) - ((ks - 1) // 2 if ks % 2 else 0)
    return np.array([(x, y, z) for z in i for y in i for x in i], np.int64) * dil * ts


def _key(c):
    c = c.astype(np.int64)
    return (c[:, 0] << 48) | ((c[:, 1] + 32768) << 32) | ((c[:, 2] + 32768) << 16) | (c[:, 3] + 32768)


def first_unique(rows):
    """distinct rows of an int [n, 4] array in first-occurrence order"""
    if len(rows) == 0:
        return rows.reshape(0, 4)
    _, first = np.unique(_key(rows), return_index=True)
    return rows[np.sort(first)]


def expand_offsets_np(coords, offsets):
    cand = np.repeat(coords.astype(np.int64), len(offsets), axis=0)          # input row major ...
    cand[:, 1:] += np.tile(offsets, (len(coords), 1))                        # ... offset minor
    return first_unique(cand).astype(np.int32)


def expand_np(coords, ks, stride, dil, ts):
    """output set of a generative transposed convolution from tensor stride ts: offsets in units of ts // stride"""
    assert ts % stride == 0
    return expand_offsets_np(coords, offsets_np(ks, dil, ts // stride))


def downsample_np(coords, ts2):
    q = coords.copy()
    q[:, 1:] = np.floor_divide(q[:, 1:], ts2) * ts2
    return first_unique(q)


def member_np(rows, of):
    """bool [len(rows)]: the row is one of `of`"""
    return np.isin(_key(rows), _key(of))


def rows_np(query, of):
    """int32 [len(query)]: first row of `of` equal to the query row, -1 if none (Python dict)"""
    table = {}
    for r, c in enumerate(of.tolist()):
        table.setdefault(tuple(c), r)
    return np.array([table.get(tuple(c), -1) for c in query.tolist()], np.int32).reshape(-1)


def transpose_front_pad(ks, dil):
    """cells a centred (odd) kernel reaches in front of the first input cell; an even kernel reaches forward only"""
    return dil * (ks - 1) // 2 if ks % 2 else 0


def dense_support(coords, ks, stride, dil, ts, B, G):
    """the set of coordinates with a non-zero response of conv_transpose3d(occupancy, ones): sorted int64 keys.  coords:
    non-negative multiples of ts below G"""
    out_ts = ts // stride
    d = torch.zeros((B, 1, G // ts, G // ts, G // ts), dtype=torch.float64)
    c = torch.as_tensor(coords).long()
    d[c[:, 0], 0, c[:, 1] // ts, c[:, 2] // ts, c[:, 3] // ts] = 1.0
    y = F.conv_transpose3d(d, torch.ones((1, 1, ks, ks, ks), dtype=torch.float64), stride=stride, dilation=dil)
    nz = torch.nonzero(y[:, 0] != 0).numpy().astype(np.int64)
    nz[:, 1:] = (nz[:, 1:] - transpose_front_pad(ks, dil)) * out_ts
    return np.sort(_key(nz))
