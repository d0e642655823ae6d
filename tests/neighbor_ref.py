"""Serial numpy restatement of the neighbour ops (ME.neighbor_pool / neighbor_sum / knn_interpolate; csrc/neighbor.hip) over
CALLER-order rows: x [V, C], idx int64 [N, k] with any negative value = no neighbour.

sum / avg / max repeat the kernels' float32 chains in the stated order (values and arg), so they compare with torch.equal;
the weighted sum, its two gradients and every feature gradient are float64."""
import numpy as np


def pool_ref(x, idx, mode):
    """-> (out float32 [N, C], arg uint8 [N, C]: the winning slot of max, 255 without a valid slot).  One step per slot, all
    queries at once: per query that is the serial chain over its valid slots in ascending slot."""
    x, idx = np.asarray(x, np.float32), np.asarray(idx)
    N, k = idx.shape
    C = x.shape[1]
    acc = np.zeros((N, C), np.float32)
    arg = np.full((N, C), 255, np.uint8)
    seen = np.zeros(N, np.int64)
    rows = x if x.shape[0] else np.zeros((1, C), np.float32)
    for j in range(k):
        ok = idx[:, j] >= 0
        f = rows[np.where(ok, idx[:, j], 0)]
        if mode == "max":
            with np.errstate(invalid="ignore"):
                take = ok[:, None] & ((seen == 0)[:, None] | (f > acc))      # a NaN wins only from the first slot
            acc = np.where(take, f, acc)
            arg = np.where(take, np.uint8(j), arg)
        else:
            acc = np.where(ok[:, None], (acc + f).astype(np.float32), acc)
        seen += ok
    if mode == "avg":
        cnt = np.maximum(seen, 1).astype(np.float32)[:, None]
        acc = np.where((seen > 0)[:, None], (acc / cnt).astype(np.float32), acc)
    return acc, arg


def _gathered(x, idx):
    x, idx = np.asarray(x, np.float64), np.asarray(idx)
    ok = idx >= 0
    rows = x if x.shape[0] else np.zeros((1, x.shape[1]))
    return np.where(ok[..., None], rows[np.where(ok, idx, 0)], 0.0), ok


def wsum_ref(x, idx, w):
    """float64 [N, C]: sum over the valid slots of w[n, j] * x[idx[n, j]]; the weight of an invalid slot is not read"""
    g, ok = _gathered(x, idx)
    return np.einsum("nk,nkc->nc", np.where(ok, np.asarray(w, np.float64), 0.0), g)


def idw_ref(idx, d2, eps=1e-8):
    """float64 [N, k]: inverse-distance weights over the valid slots (float32(d2) + eps, as the op takes the distances)"""
    idx = np.asarray(idx)
    ok = idx >= 0
    d = np.asarray(d2).astype(np.float32).astype(np.float64)
    r = np.where(ok, 1.0 / (np.where(ok, d, 1.0) + np.float64(np.float32(eps))), 0.0)
    s = r.sum(1, keepdims=True)
    return np.where(ok, r / np.where(s > 0, s, 1.0), 0.0)


def feature_grad_ref(dout, idx, V, mode, w=None, arg=None):
    """float64 [V, C]: the gradient of pool (mode 'max' | 'avg' | 'sum') or of the weighted sum ('weighted') for x"""
    dout, idx = np.asarray(dout, np.float64), np.asarray(idx)
    dx = np.zeros((V, dout.shape[1]))
    n, j = np.nonzero(idx >= 0)
    g = dout[n]
    if mode == "avg":
        g = g / (idx >= 0).sum(1)[n][:, None]
    elif mode == "weighted":
        g = np.asarray(w, np.float64)[n, j][:, None] * g
    elif mode == "max":
        g = np.where(np.asarray(arg)[n] == j[:, None], g, 0.0)
    else:
        assert mode == "sum"
    np.add.at(dx, idx[n, j], g)
    return dx


def weight_grad_ref(dout, x, idx):
    """float64 [N, k]: <dout[n], x[idx[n, j]]>, 0 for an invalid slot"""
    g, _ = _gathered(x, idx)
    return np.einsum("nc,nkc->nk", np.asarray(dout, np.float64), g)


def table_ref(idx, V):
    """(entry_sorted int64 [E], seg_start int64 [V + 1]): the entries e = n * k + j with idx >= 0 grouped by row, ascending e
    inside a row -- a stable argsort"""
    flat = np.asarray(idx).reshape(-1)
    entries = np.flatnonzero(flat >= 0)
    order = np.argsort(flat[entries], kind="stable")
    seg = np.zeros(V + 1, np.int64)
    seg[1:] = np.cumsum(np.bincount(flat[entries], minlength=V))
    return entries[order], seg
