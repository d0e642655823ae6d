"""What the dense-crossing tests compare against, and a stand-in backend for the tests that run without a GPU.

The yardstick is torch on the CPU: `d = torch.zeros(shape); d[b, :, x, y, z] = F` for SparseTensor.dense, `mask.nonzero()` plus
advanced indexing for to_sparse; gradients come from autograd through those graphs.  Nothing here calls the engine."""
import torch


def dense_reference(coords, feats, shape, origin=(0, 0, 0), divisor=1):
    """zeros(shape) with feats stored at the cells (c - origin) / divisor of coords int [V, 4]; differentiable in feats"""
    d = torch.zeros(tuple(shape), dtype=feats.dtype)
    c = coords.long().cpu()
    xyz = (c[:, 1:] - torch.tensor(list(origin))) // divisor
    if c.size(0):
        d[c[:, 0], :, xyz[:, 0], xyz[:, 1], xyz[:, 2]] = feats.cpu()
    return d


def to_sparse_reference(x):
    """(coordinates int32 [n, 4] in nonzero order, features [n, C]) of a dense x [B, C, X, Y, Z]; differentiable in x"""
    idx = (x.detach() != 0).any(1).nonzero()
    return idx.to(torch.int32), x[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]]


def rows_at(x, coords):
    """x[b, :, x, y, z] for coords int [n, 4]; differentiable in x"""
    c = coords.long()
    return x[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]]


class TorchDenseBackend:
    """the four dense entry points of the backend restated in plain torch (any device), with call counters; spatial_order
    returns a fixed pseudo-random permutation so that a manager built with spatial_sort=True holds its rows in another order"""

    def __init__(self):
        self.calls = {"dense_cell_map": 0, "dense_scatter": 0, "dense_gather": 0, "dense_occupancy": 0}

    def spatial_order(self, coords):
        g = torch.Generator().manual_seed(coords.size(0))
        return torch.randperm(coords.size(0), generator=g).to(coords.device)

    def dense_cell_map(self, coords, origin, divisor, grid):
        self.calls["dense_cell_map"] += 1
        B, X, Y, Z = grid
        c = coords.long()
        d = c[:, 1:] - torch.tensor(list(origin), device=c.device)
        off = (d % divisor != 0).any(1)
        q = torch.div(d, divisor, rounding_mode="floor")
        size = torch.tensor([X, Y, Z], device=c.device)
        out = ~off & ((c[:, 0] < 0) | (c[:, 0] >= B) | (q < 0).any(1) | (q >= size).any(1))
        ok = ~off & ~out
        cell = ((c[:, 0] * X + q[:, 0]) * Y + q[:, 1]) * Z + q[:, 2]
        row_cell = torch.where(ok, cell, torch.full_like(cell, -1)).to(torch.int32)
        cell_row = torch.full((B * X * Y * Z,), -1, dtype=torch.int32, device=c.device)
        rows = torch.nonzero(ok).view(-1)
        for r in reversed(rows.tolist()):           # the lowest row wins
            cell_row[cell[r]] = r
        lost = int(ok.sum()) - int((cell_row >= 0).sum())
        return cell_row, row_cell, (int(out.sum()), int(off.sum()), lost)

    def dense_scatter(self, feats, cell_row, shape, row_index=None):
        self.calls["dense_scatter"] += 1
        B, C, X, Y, Z = shape
        r = cell_row.long()
        if row_index is not None:
            r = torch.where(r >= 0, row_index.long()[r.clamp(min=0)], r)
        rows = torch.where((r >= 0).view(-1, 1), feats[r.clamp(min=0)] if feats.size(0) else feats.new_zeros((r.numel(), C)),
                           feats.new_zeros(()))
        return rows.view(B, X * Y * Z, C).permute(0, 2, 1).reshape(B, C, X, Y, Z).contiguous()

    def dense_gather(self, grid, cells):
        self.calls["dense_gather"] += 1
        B, C, X, Y, Z = grid.shape
        flat = grid.reshape(B, C, X * Y * Z).permute(0, 2, 1).reshape(B * X * Y * Z, C)
        return flat[cells.long()].contiguous()

    def dense_occupancy(self, grid, keep_all=False):
        self.calls["dense_occupancy"] += 1
        B, C, X, Y, Z = grid.shape
        mask = torch.ones((B, X, Y, Z), dtype=torch.bool) if keep_all else (grid != 0).any(1)
        coords = mask.nonzero().to(torch.int32)
        cells = torch.nonzero(mask.view(-1)).view(-1).to(torch.int32)
        return mask.view(-1).to(torch.uint8), coords, cells

    def scatter_add_rows(self, src, idx, n_rows, max_dup=None, sorted_=None):
        return torch.zeros((n_rows, src.size(1)), dtype=src.dtype).index_add_(0, idx, src)
