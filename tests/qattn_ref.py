"""The yardstick of the query-attention tests: a float64 torch function on the CPU, written on its own; it uses nothing of the
engine's.

It takes the coordinates and the features in the CALLER's order, loops over the batch indices present in ascending order, takes
the rows of each from the batch column, fills the blocked scores with -inf, applies softmax over the rows and gives zero for a
(query, head) without an unblocked row (softmax of an all -inf column is NaN: nan_to_num).  Gradients come from autograd through
this graph."""
import torch


def qattn_ref(queries, k, v, coords, num_heads, attn_mask=None, scale=None):
    """queries [B, Q, C], k / v [V, C]: float64 CPU tensors (leaves of the caller's graph); coords int [V, 4] (b, x, y, z) in
    the order of k's rows; attn_mask bool [V, Q] or None, True = may not attend -> out [B, Q, C] float64"""
    assert queries.dtype == k.dtype == v.dtype == torch.float64 and not queries.is_cuda
    B, Q, C = queries.shape
    H = num_heads
    D = C // H
    scale = D ** -0.5 if scale is None else scale
    batch = coords[:, 0].cpu().long()
    present = sorted(set(batch.tolist()))
    assert len(present) == B, (present, B)
    outs = []
    for b, index in enumerate(present):
        rows = torch.nonzero(batch == index).view(-1)
        qh = queries[b].view(Q, H, D)
        kh, vh = k[rows].view(-1, H, D), v[rows].view(-1, H, D)
        s = scale * torch.einsum("qhd,ihd->qih", qh, kh)                       # [Q, N_b, H]
        if attn_mask is not None:
            blocked = attn_mask.cpu()[rows].t().unsqueeze(-1)                   # [Q, N_b, 1]
            s = s.masked_fill(blocked, float("-inf"))
        p = torch.nan_to_num(torch.softmax(s, dim=1), nan=0.0)
        outs.append(torch.einsum("qih,ihd->qhd", p, vh).reshape(Q, C))
    return torch.stack(outs) if outs else queries.new_zeros((0, Q, C))
