"""ME.utils: sparse_quantize / sparse_collate as the reference calls them
(data/dataset/general_dataset.py:159-163, data/data_module.py:94-96, model/general_model.py:187-189), and what training
scripts written against MinkowskiEngine start with beside them: labels through quantisation (`labels=`, `ignore_label=`),
batched_coordinates, batch_sparse_collate, SparseCollation.

Conventions chosen here without a copy of MinkowskiEngine to compare against: a voxel keeps a label only when ALL of its
points carry it, else it gets `ignore_label` (default -100); `ignore_label` is a label like any other in that vote, so a
voxel whose points all carry it keeps it and one real label beside it does not win the voxel."""
import logging

import numpy as np
import torch

from ..backend import get_backend

_log = logging.getLogger(__name__)
_I32 = torch.iinfo(torch.int32)


def _labels_i32(labels, n, ignore_label):
    """validate `labels` ([n], any integer dtype, tensor or ndarray) -> (int32 tensor, the dtype to hand back)"""
    if isinstance(labels, np.ndarray):
        if labels.dtype.kind not in "iu":
            raise ValueError(f"labels must be integers, got an array of dtype {labels.dtype}")
        if labels.shape != (n,):
            raise ValueError(f"labels must have shape ({n},), one per coordinate row, got {tuple(labels.shape)}")
        if labels.size and (int(labels.min()) < _I32.min or int(labels.max()) > _I32.max):
            raise ValueError(f"labels of dtype {labels.dtype} hold a value that does not fit int32")
        lo, hi = np.iinfo(labels.dtype).min, np.iinfo(labels.dtype).max
        work = torch.from_numpy(labels.astype(np.int32))
    elif torch.is_tensor(labels):
        if labels.dtype.is_floating_point or labels.dtype.is_complex or labels.dtype == torch.bool:
            raise ValueError(f"labels must be integers, got a tensor of dtype {labels.dtype}")
        if tuple(labels.shape) != (n,):
            raise ValueError(f"labels must have shape ({n},), one per coordinate row, got {tuple(labels.shape)}")
        info = torch.iinfo(labels.dtype)
        lo, hi = info.min, info.max
        if (lo < _I32.min or hi > _I32.max) and labels.numel():
            wide = labels.to(torch.int64)
            if int(wide.min()) < _I32.min or int(wide.max()) > _I32.max:
                raise ValueError(f"labels of dtype {labels.dtype} hold a value that does not fit int32")
        work = labels.to(torch.int32)
    else:
        raise ValueError(f"labels must be an integer tensor or ndarray of shape ({n},), got {type(labels).__name__}")
    ignore_label = int(ignore_label)
    if not _I32.min <= ignore_label <= _I32.max:
        raise ValueError(f"ignore_label {ignore_label} does not fit int32")
    if not lo <= ignore_label <= hi:
        raise ValueError(f"ignore_label {ignore_label} does not fit the labels' dtype {labels.dtype}")
    return work, labels.dtype


def _quantize_labels(work, uniq, inv, ignore_label):
    """int32 label of every voxel of (uniq, inv): the one all of its points share, else ignore_label"""
    be = get_backend()
    work = work.to(uniq.device)
    if uniq.is_cuda and hasattr(be, "quantize_labels"):
        return be.quantize_labels(work.contiguous(), uniq.contiguous(), inv.contiguous(), ignore_label)
    # CPU tensors, numpy input, DataLoader workers: the same rule over the maps (MinkowskiEngine's own is CPU-only)
    uniq_l, inv_l = uniq.long(), inv.long()
    first = work[uniq_l]
    out = first.clone()
    out[inv_l[work != first[inv_l]]] = ignore_label
    return out


def sparse_quantize(coordinates, features=None, return_index=False, return_inverse=False, quantization_size=None,
                    device="cpu", *, labels=None, ignore_label=-100, return_maps_only=False):
    """floor(coordinates / quantization_size) -> unique integer rows, FIRST occurrence wins, rows in
    first-occurrence order (canonical choice on every device).
    coordinates: [N, D] (D = 3, or 4 with a leading batch/cluster column), tensor or ndarray.

    The positional order is the reference's call form and differs from MinkowskiEngine's (which has `labels` and
    `ignore_label` in third and fourth place); `labels`, `ignore_label` and `return_maps_only` are keyword-only here, as
    MinkowskiEngine callers pass them.

    labels: integer tensor or ndarray [N] of any integer dtype.  A voxel keeps the label ALL of its points carry and gets
    `ignore_label` otherwise (`ignore_label` votes like any other label: a voxel whose points all carry it keeps it); one
    entry per returned coordinate row, in the same first-occurrence order, in the labels' own dtype, as an ndarray when
    `coordinates` is an ndarray and as a tensor on the coordinates' device otherwise (the other outputs of an ndarray call
    stay CPU tensors).  On the GPU the vote is ms3d_quantize_labels (csrc/labels.hip), elsewhere the same rule as a torch
    expression over the maps.  ValueError: labels that are not integers (float, bool), not of shape [N], hold a value outside
    int32, or an `ignore_label` outside int32 or outside the labels' dtype.

    return_maps_only: return `index`, or `(index, inverse)` with return_inverse, and nothing else; with `labels` it raises
    ValueError (the maps alone cannot carry the vote).

    Returns, in MinkowskiEngine's order: coords[, features][, labels][, index][, inverse]."""
    if return_maps_only and labels is not None:
        raise ValueError("return_maps_only=True returns the maps alone and cannot carry the vote of labels=")
    was_numpy = isinstance(coordinates, np.ndarray)
    c = torch.from_numpy(coordinates) if was_numpy else coordinates
    if labels is not None:
        work, label_dtype = _labels_i32(labels, c.size(0), ignore_label)
    if quantization_size is not None:
        c = torch.floor(c / quantization_size)
    c = c.to(torch.int32)
    c4 = c if c.size(1) == 4 else torch.cat([torch.zeros((c.size(0), 1), dtype=torch.int32, device=c.device), c], 1)
    uniq, inv = get_backend().sparse_quantize(c4.contiguous())
    uniq_l = uniq.long()
    if return_maps_only:
        maps = [uniq_l, inv.long()] if return_inverse else [uniq_l]
        if was_numpy:
            maps = [o.cpu() for o in maps]
        return maps[0] if len(maps) == 1 else tuple(maps)
    out = [c[uniq_l]]
    if features is not None:
        f = torch.from_numpy(features) if isinstance(features, np.ndarray) else features
        if torch.is_tensor(f) and f.is_cuda and f.dim() == 2 and f.dtype == torch.float32 and f.requires_grad:
            # the first-occurrence rows: a gather over UNIQUE indices -- the engine's row gather, whose backward is one
            # scatter launch (no two sources per row: order-independent) where torch's indexing backward sorts the index
            from . import functional as Fn
            out.append(Fn.gather_rows(f, uniq_l, max_dup=1))
        else:
            out.append(f[uniq_l.to(f.device)])
    if labels is not None:
        q = _quantize_labels(work, uniq, inv, int(ignore_label))
        labels_at = len(out)
        if was_numpy and not isinstance(label_dtype, np.dtype):
            label_dtype = torch.empty(0, dtype=label_dtype).numpy().dtype
        elif not was_numpy and isinstance(label_dtype, np.dtype):
            label_dtype = torch.from_numpy(np.empty(0, label_dtype)).dtype
        out.append(q.to(c.device) if was_numpy else q.to(device=c.device, dtype=label_dtype))
    if return_index:
        out.append(uniq_l)
    if return_inverse:
        out.append(inv.long())
    if was_numpy:
        out = [o.cpu() for o in out]
        if labels is not None:
            out[labels_at] = out[labels_at].numpy().astype(label_dtype)
    return out[0] if len(out) == 1 else tuple(out)


def batched_coordinates(coords, dtype=torch.int32, device=None):
    """list of [N_i, D] tensors or ndarrays -> [sum N_i, 1 + D] with the sample's position in the list as column 0.
    Float input is floored; an empty sample contributes no rows; an empty list or a non-integer `dtype` raises ValueError."""
    if not isinstance(dtype, torch.dtype) or dtype.is_floating_point or dtype.is_complex or dtype == torch.bool:
        raise ValueError(f"batched_coordinates needs an integer dtype, got {dtype}")
    coords = list(coords)
    if not coords:
        raise ValueError("batched_coordinates needs at least one sample, got an empty list")
    rows, width = [], None
    for b, c in enumerate(coords):
        c = torch.as_tensor(c)
        if c.numel() == 0:
            continue
        if c.dim() != 2:
            raise ValueError(f"sample {b}: coordinates must have shape [N, D], got {tuple(c.shape)}")
        if width is None:
            width = c.size(1)
        elif c.size(1) != width:
            raise ValueError(f"sample {b}: {c.size(1)} coordinate columns where the samples before it have {width}")
        if c.dtype.is_floating_point:
            c = torch.floor(c)
        c = c.to(dtype)
        rows.append(torch.cat([torch.full((c.size(0), 1), b, dtype=dtype, device=c.device), c], 1))
    if not rows:
        first = torch.as_tensor(coords[0])
        width = first.size(1) if first.dim() == 2 else 3
        bc = torch.zeros((0, 1 + width), dtype=dtype, device=first.device)
    else:
        bc = torch.cat(rows, 0)
    return bc if device is None else bc.to(device)


def sparse_collate(coords, feats, labels=None, dtype=torch.int32, device=None):
    """prepend the batch index column (batched_coordinates) and concatenate: -> (bcoords [sum V, 4], feats f32), and with
    `labels` (a list as long as `coords`) -> (bcoords, feats, labels): tensor / ndarray labels concatenated along dim 0 in
    their own dtype, a list with any other entry (strings, dicts) handed back as it is.  Lists of different lengths raise
    ValueError."""
    coords, feats = list(coords), list(feats)
    if len(feats) != len(coords) or (labels is not None and len(labels) != len(coords)):
        raise ValueError(f"sparse_collate needs lists of one length, got {len(coords)} coords, {len(feats)} feats"
                         + ("" if labels is None else f", {len(labels)} labels"))
    bc = batched_coordinates(coords, dtype=dtype, device=device)
    bf = torch.cat([torch.as_tensor(f, dtype=torch.float32) for f in feats], 0)
    if device is not None:
        bf = bf.to(device)
    if labels is None:
        return bc, bf
    if all(torch.is_tensor(l) or isinstance(l, np.ndarray) for l in labels):
        bl = torch.cat([torch.as_tensor(l) for l in labels], 0)
        if device is not None:
            bl = bl.to(device)
        return bc, bf, bl
    return bc, bf, labels


def batch_sparse_collate(data, dtype=torch.int32, device=None):
    """list of (coords, feats) or (coords, feats, labels) tuples -> sparse_collate of the unzipped lists"""
    columns = [list(col) for col in zip(*data)]
    if len(columns) not in (2, 3):
        raise ValueError(f"batch_sparse_collate needs (coords, feats) or (coords, feats, labels) tuples, got {len(columns)} fields")
    return sparse_collate(*columns, dtype=dtype, device=device)


class SparseCollation:
    """collate function over a list of (coords, feats, labels) -> (bcoords, feats, labels).  With limit_numpoints > 0 the
    batch ends in front of the sample that would take the running point count over the limit; one warning names how many
    samples were left out."""

    def __init__(self, limit_numpoints=-1, dtype=torch.int32, device=None):
        self.limit_numpoints = limit_numpoints
        self.dtype = dtype
        self.device = device

    def __call__(self, list_data):
        list_data = list(list_data)
        kept, total = [], 0
        for i, sample in enumerate(list_data):
            n = int(sample[0].shape[0])
            if self.limit_numpoints > 0 and total + n > self.limit_numpoints:
                _log.warning("SparseCollation: %d of %d samples dropped, %d points with the next one exceed limit_numpoints = %d",
                             len(list_data) - i, len(list_data), total + n, self.limit_numpoints)
                break
            kept.append(sample)
            total += n
        if not kept:
            raise ValueError(f"SparseCollation: no sample fits limit_numpoints = {self.limit_numpoints}"
                             if list_data else "SparseCollation needs at least one sample, got an empty list")
        coords, feats, labels = zip(*kept)
        return sparse_collate(coords, feats, list(labels), dtype=self.dtype, device=self.device)
