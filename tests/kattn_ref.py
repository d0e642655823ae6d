"""The yardstick of the kernel-map attention tests: a float64 torch function on the CPU, never the engine's own arithmetic.

It takes the features in the CALLER's order and the index pairs of CoordinateManager.kernel_map(in_key, out_key, ...) --
{k: int64 [2, N_k]} (input row, output row), which tests/test_kernelmap_gpu.py verifies against plain loops -- fills a
[Vout, K, H] score tensor with -inf, writes the present pairs' scores into it, takes softmax over K (nan_to_num for the rows
without any input), weights v and sums.  Gradients come from autograd through this graph."""
import torch


def kattn_ref(q, k, v, pairs, K, num_heads, rel_bias=None, scale=None):
    """q [Vout, C], k / v [Vin, C], rel_bias [K, H] or None: float64 CPU tensors (leaves of the caller's graph);
    pairs: {kk: int64 [2, N]} on any device -> out [Vout, C] float64"""
    assert q.dtype == k.dtype == v.dtype == torch.float64 and not q.is_cuda
    vout, C = q.shape
    H = num_heads
    D = C // H
    scale = D ** -0.5 if scale is None else scale
    qh, kh, vh = q.view(vout, H, D), k.view(-1, H, D), v.view(-1, H, D)
    s = torch.full((vout, K, H), float("-inf"), dtype=torch.float64)
    for kk, io in pairs.items():
        i, o = io[0].cpu(), io[1].cpu()
        sc = scale * (qh[o] * kh[i]).sum(-1)
        s[o, kk] = sc if rel_bias is None else sc + rel_bias[kk]
    p = torch.nan_to_num(torch.softmax(s, dim=1), nan=0.0)
    out = torch.zeros((vout, H, D), dtype=torch.float64)
    for kk, io in pairs.items():
        i, o = io[0].cpu(), io[1].cpu()
        out = out.index_add(0, o, p[o, kk].unsqueeze(-1) * vh[i])
    return out.reshape(vout, C)
