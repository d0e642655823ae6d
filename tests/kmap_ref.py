"""Kernel maps as index pairs: host restatements for the tests, written on their own (plain loops and a Python dictionary,
nothing of the engine's) -- the packed pair lists of a table, and a dictionary kernel map over the coordinates the CALLER sees."""
import numpy as np

from region_ref import dict_map


def pairs_np(nbr, out_order=None, in_rename=None, vin=None):
    """(pairs int64 [2, P], start int32 [K + 1]) of a table nbr [K, Vout] (-1 = none): per offset k, walk the visible output
    rows j in ascending order, read v = nbr[k][out_order[j]] (out_order None = identity) and, when 0 <= v < vin, emit the pair
    (in_rename[v], j) (in_rename None = identity).  vin None: every non-negative entry is valid."""
    nbr = np.asarray(nbr)
    K, vout = nbr.shape
    rows = nbr.tolist()                                     # (Python ints once: the loops below are plain loops)
    order = None if out_order is None else np.asarray(out_order).tolist()
    rename = None if in_rename is None else np.asarray(in_rename).tolist()
    ins, outs, start = [], [], [0]
    for k in range(K):
        row = rows[k]
        for j in range(vout):
            v = row[j if order is None else order[j]]
            if v < 0 or (vin is not None and v >= vin):
                continue
            ins.append(v if rename is None else rename[v])
            outs.append(j)
        start.append(len(ins))
    return np.array([ins, outs], np.int64).reshape(2, -1), np.array(start, np.int32)


def visible_pairs(in_coords, out_coords, offsets, transposed=False):
    """{k: int64 [2, N_k]} over the rows of two coordinate arrays as the caller sees them (x.C, y.C), only the offsets that have
    a pair: forward C_out[o] + off_k == C_in[i], transposed C_out[o] - off_k == C_in[i]; o ascending inside an entry"""
    offsets = np.asarray(offsets, np.int64)
    nbr = dict_map(in_coords, out_coords, -offsets if transposed else offsets)
    out = {}
    for k in range(nbr.shape[0]):
        o = np.nonzero(nbr[k] >= 0)[0]
        if len(o):
            out[k] = np.stack([nbr[k][o].astype(np.int64), o.astype(np.int64)])
    return out
