"""The yardstick of the voxel-attention tests: a float64 torch function on the CPU, written on its own; it uses nothing of the
engine's.

It takes the coordinates, the features and the mask in the CALLER's order, loops over the batch indices present in ascending
order, takes the rows of each from the batch column, fills the blocked scores with -inf, applies softmax over the queries and
gives zero for a (row, head) without an unblocked query (softmax of an all -inf row is NaN: nan_to_num).  Gradients come from
autograd through this graph."""
import torch


def vattn_ref(x, keys, values, coords, num_heads, attn_mask=None, scale=None):
    """x [V, C], keys / values [B, Q, C]: float64 CPU tensors (leaves of the caller's graph); coords int [V, 4] (b, x, y, z) in
    the order of x's rows; attn_mask bool [V, Q] or None, True = may not attend -> out [V, C] float64 in the order of x's rows"""
    assert x.dtype == keys.dtype == values.dtype == torch.float64 and not x.is_cuda
    B, Q, C = keys.shape
    V = x.size(0)
    H = num_heads
    D = C // H
    scale = D ** -0.5 if scale is None else scale
    batch = coords[:, 0].cpu().long()
    present = sorted(set(batch.tolist()))
    assert len(present) == B, (present, B)
    out = x.new_zeros((V, C))
    for b, index in enumerate(present):
        rows = torch.nonzero(batch == index).view(-1)
        xh = x[rows].view(-1, H, D)
        kh, vh = keys[b].view(Q, H, D), values[b].view(Q, H, D)
        s = scale * torch.einsum("ihd,qhd->iqh", xh, kh)                       # [N_b, Q, H]
        if attn_mask is not None:
            blocked = attn_mask.cpu()[rows].unsqueeze(-1)                       # [N_b, Q, 1]
            s = s.masked_fill(blocked, float("-inf"))
        p = torch.nan_to_num(torch.softmax(s, dim=1), nan=0.0)
        out = out.index_add(0, rows, torch.einsum("iqh,qhd->ihd", p, vh).reshape(-1, C))
    return out
