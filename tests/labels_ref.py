"""Serial yardstick of label quantisation: MinkowskiEngine's sequential wording, taken literally, over a coordinate list --
the first point of a voxel sets its label, any later point with a different label turns it into `ignore_label` for good.
One Python loop over the rows in their order, a dict from coordinate to voxel; nothing is shared with the order-independent
kernel (csrc/labels.hip) or the torch expression of ME.utils.sparse_quantize."""
import numpy as np


def quantize_labels_ref(coords, labels, ignore_label):
    """coords [N, D] integers, labels [N] -> (unique rows [M, D] in first-occurrence order, labels [M] int64,
    first-occurrence row [M], voxel of every row [N])"""
    coords = np.asarray(coords)
    labels = np.asarray(labels)
    voxel_of = {}
    rows, out, first, dead, inverse = [], [], [], [], []
    for i in range(coords.shape[0]):
        key = tuple(int(v) for v in coords[i])
        lab = int(labels[i])
        u = voxel_of.get(key)
        if u is None:
            u = voxel_of[key] = len(rows)
            rows.append(key)
            out.append(lab)
            first.append(i)
            dead.append(False)
        elif not dead[u] and lab != out[u]:
            out[u] = int(ignore_label)
            dead[u] = True                      # "for good": a later point that carries ignore_label cannot revive it either
        inverse.append(u)
    d = coords.shape[1] if coords.ndim == 2 else 0
    return (np.array(rows, np.int64).reshape(len(rows), d), np.array(out, np.int64), np.array(first, np.int64),
            np.array(inverse, np.int64))
