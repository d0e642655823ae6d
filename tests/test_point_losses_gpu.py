"""GPU parity of the fused per-point losses (csrc/losses.hip through minsu3d_amd.loss.point_losses) against the float64
restatement of tests/losses_ref.py, at the places the three kernels can go wrong: the padded LDS row stride and ragged
last tiles, the scalar route of the scale kernel (N * C not a multiple of 4), the whole accepted range of C (the tile is
dynamic LDS, above 64 KB from C = 64), the grid strides of all three kernels, the eps clamp of the normalisation, rows
without label or instance, large logits, N = 0, and the autograd contract of the node.

Tolerance.  For every case the float32 torch formulation (GeneralModel._point_losses_torch on the GPU) is measured against
the float64 reference on the same inputs; the kernel must be within TWICE that error (a different but equally valid
float32 operation order) plus 4 float32 ulps of the largest reference magnitude of the compared tensor (torch may happen
to be exact).  Every measured pair is printed (pytest -s)."""
import numpy as np
import pytest
import torch

import losses_ref as LR

gpu = pytest.mark.gpu
W = (0.7, 1.3, 0.4)
NAMES = ("semantic loss", "norm loss", "dir loss", "d scores", "d offsets")


@pytest.fixture(autouse=True)
def _hip_backend(request):
    if request.node.get_closest_marker("gpu"):
        from minsu3d_amd import backend
        from minsu3d_amd.backend import HipBackend
        backend.set_backend(HipBackend())        # tests/conftest.py puts the previous one back


def run_fused(inp, weights=W, use=(0, 1, 2), views=False):
    """the five outputs of run_ref from the fused node; use: the losses that enter the backward pass; views: scores and
    offsets handed over as non-contiguous views (every second column of a wider buffer)"""
    from minsu3d_amd.loss.point_losses import point_losses
    s = inp["scores"].cuda().requires_grad_(True)
    p = inp["pred_offsets"].cuda().requires_grad_(True)
    sv, pv = s, p
    if views:
        wide = lambda t: torch.stack([t, torch.full_like(t, 7.0)], dim=2).reshape(t.size(0), -1)[:, ::2]
        sv, pv = wide(s), wide(p)
        assert not sv.is_contiguous() and not pv.is_contiguous() and torch.equal(sv, s) and torch.equal(pv, p)
    losses = point_losses(sv, pv, inp["labels"].cuda(), inp["centre"].cuda(), inp["xyz"].cuda(), inp["instance_ids"].cuda())
    assert all(l.dim() == 0 and l.dtype == torch.float32 for l in losses)
    sum(weights[i] * losses[i] for i in use).backward()
    torch.cuda.synchronize()
    return [l.detach().cpu() for l in losses], s.grad.cpu(), p.grad.cpu()


def flat(res):
    losses, gs, go = res
    return list(losses) + [gs, go]


def within(case, got, tor, ref):
    """the rule of the module docstring on the three losses and the two gradients; -> [(kernel error, torch error)]"""
    out = []
    for what, g, t, r in zip(NAMES, flat(got), flat(tor), flat(ref)):
        assert g.dtype == torch.float32 and g.shape == r.shape, (case, what)
        if r.numel() == 0:
            continue
        assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(r).all()), (case, what)
        ek, et = float((g.double() - r).abs().max()), float((t.double() - r).abs().max())
        floor = 4 * float(np.spacing(np.float32(float(r.abs().max()))))
        print("PLOSS %-28s %-13s kernel %.3e torch %.3e floor %.3e max|ref| %.3e" % (case, what, ek, et, floor,
                                                                                 float(r.abs().max())))
        assert ek <= 2 * et + floor, (case, what, ek, et, floor)
        out.append((ek, et))
    return out


def check(case, inp):
    got = run_fused(inp)
    within(case, got, LR.run_torch(inp, W, "cuda"), LR.run_ref(inp, W))
    return got


# ------------------------------------------------------------------------------------------ lane and tile edges
# N * C mod 4 decides the route of the scale kernel (0: float4, else scalar); one pair per residue is named here
RESIDUE = {(256, 7): 0, (777, 20): 0, (1, 1): 1, (255, 7): 1, (257, 1): 1, (1, 2): 2, (257, 2): 2, (255, 1): 3, (777, 7): 3}
assert set(RESIDUE.values()) == {0, 1, 2, 3}


@gpu
@pytest.mark.parametrize("c", [1, 2, 7, 20])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 777])
def test_lane_and_tile_edges(n, c):
    """C = 2, 20: the padded row stride CP = C | 1 differs from C; N = 255, 257, 777: ragged last tile, 1: a single row;
    C = 7 at N = 255 / 777: the scalar route of the scale kernel walks its grid stride (N * C > 4 * the 3 N threads)"""
    if (n, c) in RESIDUE:
        assert n * c % 4 == RESIDUE[(n, c)]
    check("N=%d C=%d" % (n, c), LR.make_inputs(n, c, seed=1000 * n + c))


# ------------------------------------------------------------------------------------------ the accepted range of C
@gpu
@pytest.mark.parametrize("c", [63, 64, 65, 96])
def test_accepted_range_of_c(c):
    """256 * (C | 1) * 4 bytes of dynamic LDS: 64512 at C = 63, 66560 at 64 and 65 (past 64 KB), 99328 at 96"""
    check("N=300 C=%d" % c, LR.make_inputs(300, c, seed=c))


@gpu
def test_c_above_the_range_is_refused():
    from minsu3d_amd import _lib
    with pytest.raises(_lib.HipLibraryError, match="ms3d_point_losses_forward failed with code %d" % _lib.E_UNSUPPORTED):
        run_fused(LR.make_inputs(300, 97, seed=97))


# ------------------------------------------------------------------------------------------ grid strides
N_STRIDE = 524288 + 256 + 3
_stride_case = {}


def stride_case():
    """2050 tiles over 2048 blocks (the forward tile loop strides and the finalize kernel's threads walk two partials),
    3 N > 4096 * 256 (the scale kernel strides) and N * C = 2 mod 4 (on its scalar route); computed once"""
    if not _stride_case:
        inp = LR.make_inputs(N_STRIDE, 2, seed=5)
        assert (N_STRIDE + 255) // 256 > 2048 and 3 * N_STRIDE > 4096 * 256 and N_STRIDE * 2 % 4 == 2
        _stride_case.update(inp=inp, got=run_fused(inp), ref=LR.run_ref(inp, W))
    return _stride_case


@gpu
def test_grid_stride():
    c = stride_case()
    within("N=%d C=2" % N_STRIDE, c["got"], LR.run_torch(c["inp"], W, "cuda"), c["ref"])


@gpu
def test_grid_stride_is_reproducible():
    c = stride_case()
    again = run_fused(c["inp"])
    for what, a, b in zip(NAMES, flat(c["got"]), flat(again)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what


@gpu
def test_finalize_edge():
    """nblk = 1025: thread 0 of the finalize kernel sums two partials, every other thread one"""
    n = 1024 * 256 + 1
    from minsu3d_amd import _lib
    import ctypes as C
    assert _lib.lib().ms3d_point_losses_blocks(C.c_long(n)) == 1025
    check("N=%d C=1" % n, LR.make_inputs(n, 1, seed=6))


# ------------------------------------------------------------------------------------------ crafted rows
@gpu
def test_exact_offsets():
    """ground-truth offset exactly zero (ng = 0), prediction equal to the ground truth (sign 0), both at once"""
    inp = LR.craft_offsets_exact(LR.make_inputs(300, 5, seed=2))
    _, _, go = check("exact offsets", inp)
    # row 4: the L1 term has gradient sign(0) = 0, the cosine is 1 and its gradient (I - u u^T) g / |p| vanishes up to rounding
    assert float(go[4].abs().max()) <= 1e-6 * float(go.abs().max())
    # row 3: cosine 0 whatever the prediction; what is left is the L1 sign times its weight over the count
    n_off = int((inp["instance_ids"] != -1).sum())
    assert torch.equal(go[3].abs(), torch.full((3,), np.float32(W[1]) * np.float32(1.0 / n_off)))
    assert float(go[5].abs().max()) == 0.0


@gpu
def test_eps_rows():
    """predictions of length 0, 0.5 eps, 2 eps: the clamp of F.normalize and its two Jacobians"""
    check("eps rows", LR.craft_eps_rows(LR.make_inputs(300, 5, seed=3)))


@gpu
def test_every_label_ignored():
    inp = LR.make_inputs(300, 7, seed=11, labelled=0.0)
    assert bool((inp["labels"] == -1).all())
    (sem, _, _), gs, _ = check("no label", inp)
    assert float(sem) == 0.0 and float(gs.abs().max()) == 0.0


@gpu
def test_no_point_in_an_instance():
    inp = LR.make_inputs(300, 7, seed=12, in_instance=0.0)
    assert bool((inp["instance_ids"] == -1).all())
    (_, norm_l, dir_l), _, go = check("no instance", inp)
    assert float(norm_l) == 0.0 and float(dir_l) == 0.0 and float(go.abs().max()) == 0.0


@gpu
def test_large_logits():
    inp = LR.make_inputs(300, 20, seed=13)
    inp["scores"] *= 1000.0
    assert float(inp["scores"].abs().max()) > 5000
    losses, gs, go = check("scores x 1000", inp)       # within() asserts that everything is finite
    assert float(losses[0]) > 100


@gpu
def test_no_rows():
    inp = LR.make_inputs(0, 4, seed=14)
    losses, gs, go = run_fused(inp)
    assert [float(v) for v in losses] == [0.0, 0.0, 0.0] and gs.shape == (0, 4) and go.shape == (0, 3)
    assert [float(v) for v in LR.run_torch(inp, W, "cuda")[0]] == [0.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------ autograd contract
@gpu
@pytest.mark.parametrize("only", [0, 1, 2])
def test_backward_through_one_loss(only):
    """set_materialize_grads(False): the two unused losses arrive as None = NULL in the scale kernel.  The gradient of the
    input the used loss does not depend on is exactly zero (the eps rows hold -g / eps ~ 1e7: 0 * that stays finite)"""
    inp = LR.craft_eps_rows(LR.make_inputs(777, 7, seed=20 + only))
    w = [0.0, 0.0, 0.0]
    w[only] = W[only]
    got = run_fused(inp, use=(only,))
    within("only loss %d" % only, got, LR.run_torch(inp, w, "cuda"), LR.run_ref(inp, w))
    _, gs, go = got
    assert bool(torch.isfinite(gs).all()) and bool(torch.isfinite(go).all())
    if only == 0:
        assert float(go.abs().max()) == 0.0 and float(gs.abs().max()) > 0
    else:
        assert float(gs.abs().max()) == 0.0 and float(go.abs().max()) > 0


@gpu
def test_second_backward_is_refused():
    from minsu3d_amd.loss.point_losses import point_losses
    inp = LR.make_inputs(257, 7, seed=30)
    s = inp["scores"].cuda().requires_grad_(True)
    p = inp["pred_offsets"].cuda().requires_grad_(True)
    total = sum(point_losses(s, p, inp["labels"].cuda(), inp["centre"].cuda(), inp["xyz"].cuda(), inp["instance_ids"].cuda()))
    total.backward(retain_graph=True)
    first = s.grad.clone()
    with pytest.raises(RuntimeError, match="scaled in place by the first backward pass"):
        total.backward()
    assert torch.equal(s.grad, first)


@gpu
def test_views_give_the_same_bytes():
    inp = LR.make_inputs(777, 7, seed=31)
    a, b = run_fused(inp), run_fused(inp, views=True)
    for what, x, y in zip(NAMES, flat(a), flat(b)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), what
