"""numpy restatements of the operations across coordinate sets (union of sets, combine of features, broadcast of one row per
batch index): the expectation the GPU tests compare the engine against bit for bit.  tests/test_setops_cpu.py pins these
restatements themselves against dense float64 torch."""
import numpy as np

SUM, SUB, MUL = 0, 1, 2
ADD, MULTIPLY, CAT, COPY = 0, 1, 2, 3


def key(c):
    """one int64 per (b, x, y, z) row; coordinates may be negative"""
    c = np.asarray(c, np.int64)
    return ((c[:, 0] * 70000 + (c[:, 1] + 30000)) * 70000 + (c[:, 2] + 30000)) * 70000 + (c[:, 3] + 30000)


def union_np(sets):
    """sets: int32 [V_i, 4] arrays without repeats inside a set -> (out int32 [n, 4]: distinct rows in first-occurrence order
    of the concatenation, out_rows: per set int32 [V_i] row -> union row, in_row int32 [N, n]: union row -> row of set i or -1)"""
    seen, out, out_rows = {}, [], []
    for c in sets:
        rows = np.empty(len(c), np.int32)
        own = set()
        for r, k in enumerate(key(c).tolist() if len(c) else []):
            assert k not in own, "a coordinate repeats inside one set"
            own.add(k)
            u = seen.get(k)
            if u is None:
                u = seen[k] = len(out)
                out.append(c[r])
            rows[r] = u
        out_rows.append(rows)
    n = len(out)
    in_row = np.full((len(sets), n), -1, np.int32)
    for i, rows in enumerate(out_rows):
        in_row[i, rows] = np.arange(len(rows), dtype=np.int32)
    out = np.stack(out).astype(np.int32) if n else np.zeros((0, 4), np.int32)
    return out, out_rows, in_row


def combine_np(op, feats, in_row):
    """float32, the inputs present added in ascending input order onto a zero-filled result; subtract / multiply (two
    operands): the result receives a at a's rows and is then set to fn(out, b) at b's rows"""
    n, c = in_row.shape[1], feats[0].shape[1]
    out = np.zeros((n, c), np.float32)
    for i, f in enumerate(feats):
        here = np.nonzero(in_row[i] >= 0)[0]
        v = np.asarray(f, np.float32)[in_row[i, here]]
        if op == SUM or i == 0:
            out[here] = out[here] + v
        elif op == SUB:
            out[here] = out[here] - v
        else:
            out[here] = out[here] * v
    return out


def combine_backward_np(op, which, dout, out_row, other=None, other_row=None):
    """gradient of operand `which` (float32): dout at its union rows; subtract negates the second operand's; multiply scales by
    the other operand's row where it is present, passes a's through where b is absent and gives b zero where a is absent (the
    forward is 0 * b there)"""
    g = np.asarray(dout, np.float32)[out_row].copy()
    if op == SUB and which == 1:
        g = -g
    elif op == MUL:
        q = other_row[out_row]
        has = q >= 0
        g[has] = g[has] * np.asarray(other, np.float32)[q[has]]
        if which == 1:
            g[~has] = 0
    return g


def grow_np(x_batch, g_batch):
    """per row of x the row of the global tensor with its batch index, or -1"""
    where = {int(b): j for j, b in enumerate(g_batch)}
    return np.array([where.get(int(b), -1) for b in x_batch], np.int32)


def broadcast_np(mode, x, g, grow):
    """float32: x[r] (mode) g[grow[r]], the zero vector where grow is -1"""
    g = np.asarray(g, np.float32)
    gr = np.where(grow[:, None] >= 0, g[np.maximum(grow, 0)], np.float32(0)).astype(np.float32)
    if mode == COPY:
        return gr
    x = np.asarray(x, np.float32)
    if mode == ADD:
        return x + gr
    if mode == MULTIPLY:
        return x * gr
    return np.concatenate([x, gr], 1)


def broadcast_dg_np(mode, dout, x, grow, n_glob, cx):
    """float64 gradient of the global operand: per global row the sum of dout (times x for multiply; the global columns of
    dout for concatenate) over the voxels that read it"""
    d = np.asarray(dout, np.float64)
    if mode == CAT:
        d = d[:, cx:]
    if mode == MULTIPLY:
        d = d * np.asarray(x, np.float64)
    dg = np.zeros((n_glob, d.shape[1]), np.float64)
    ok = grow >= 0
    np.add.at(dg, grow[ok], d[ok])
    return dg
