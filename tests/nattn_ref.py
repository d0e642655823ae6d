"""float64 torch restatement of ME.neighbor_attention (csrc/nattn.hip) on the CPU, over CALLER-order rows: plain gathers, a
masked softmax and autograd for every gradient.  It calls nothing of the engine.

  out[n, h, :] = sum_j softmax_j(scale * <q[n, h], k[i, h]> + bias[n, j, h]) v[i, h, :],  i = idx[n, j] >= 0

A query without a valid slot is zeros; the bias of an invalid slot is not read (it may be NaN) and its gradient is 0."""
import torch

RTOL = 1e-4              # the project's bar: of the reference tensor's largest magnitude (tests/test_geometry_gpu.py)


def nattn_ref(q, k, v, idx, H, bias=None, scale=None):
    """q [N, C], k / v [V, C], bias [N, kk, H] or None: float64 tensors (leaves or not); idx int64 [N, kk] -> out [N, C]"""
    N, C = q.shape
    kk, D = idx.size(1), C // H
    scale = D ** -0.5 if scale is None else scale
    ok = idx >= 0
    if k.size(0) == 0 or N == 0:
        return (q.sum() + k.sum() + v.sum()) * 0 + torch.zeros((N, C), dtype=torch.float64)
    rows = idx.clamp(min=0)
    kg, vg = k[rows].view(N, kk, H, D), v[rows].view(N, kk, H, D)
    s = torch.einsum("nhd,njhd->njh", q.view(N, H, D), kg) * scale
    if bias is not None:
        s = s + torch.where(ok[:, :, None], bias, torch.zeros((), dtype=torch.float64))
    s = torch.where(ok[:, :, None], s, torch.full((), float("-inf"), dtype=torch.float64))
    m = s.detach().amax(1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros((), dtype=torch.float64))
    p = torch.exp(s - m)
    den = p.sum(1, keepdim=True)
    p = p / torch.where(den > 0, den, torch.ones((), dtype=torch.float64))
    vg = torch.where(ok[:, :, None, None], vg, torch.zeros((), dtype=torch.float64))
    return torch.einsum("njh,njhd->nhd", p, vg).reshape(N, C)


def run_ref(fq, fk, fv, idx, H, bias, g, scale=None):
    """float32 / float64 inputs (torch tensors, any device) -> dict of float64 out, dq, dk, dv, db (None without a bias) for the
    loss sum(out * g)"""
    q, k, v = (f.detach().double().cpu().clone().requires_grad_(True) for f in (fq, fk, fv))
    idx = idx.cpu().reshape(-1, idx.size(-1))
    b = None
    if bias is not None:
        b = bias.detach().double().cpu().reshape(idx.size(0), idx.size(1), H).clone().requires_grad_(True)
    out = nattn_ref(q.view(-1, q.size(-1)), k, v, idx, H, b, scale)
    (out * g.detach().double().cpu().reshape(out.shape)).sum().backward()
    db = None if b is None else torch.nan_to_num(b.grad, nan=0.0) * (idx >= 0)[:, :, None]
    return dict(out=out.detach(), dq=q.grad.view(out.shape), dk=k.grad, dv=v.grad, db=db)


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item() if b.numel() else 0.0


WORST = {}               # the largest error seen per tensor name, printed when the GPU suite's module ends


def check(name, got, want, tol=RTOL):
    assert tuple(got.shape) == tuple(want.shape), (name, tuple(got.shape), tuple(want.shape))
    assert bool(torch.isfinite(got).all()), name
    e = rel_err(got, want)
    key = name.split()[-1]
    WORST[key] = max(WORST.get(key, 0.0), e)
    print(f"{name}: rel err {e:.3e} (bound {tol:.0e})")
    assert e <= tol, (name, e)
