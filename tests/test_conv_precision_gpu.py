"""GPU: the sparse convolutions follow torch.set_float32_matmul_precision.

"highest" (the default) keeps every route float32 grade.  "high" / "medium" let the wide layers' bf16 kernels (forward /
backward-data with both sides >= 48 channels, backward-weight of the wide K = 27 layers) keep two / one of the three bf16
pieces x0 = bf16(x), x1 = bf16(x - x0) of each operand (include/minsu3d_hip.h, the *_p entry points).  Checked here:
the result IS the float64 product of the piece-reconstructed operands (and at "medium" is NOT float32 grade: the cheaper
kernel ran), every other route is byte-identical to "highest", no state sticks between settings, the forward's setting
governs its backward, a step is reproducible, and the models still compute and learn."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

from test_determinism_gpu import _cuda, _diff_report, _one_step, _softgroup_scores
from test_model_cpu import _build, small_batch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

BAR = 3e-6          # of the largest output: the float32-grade bar of test_bf16x3_wide_layers_are_float32_grade


@pytest.fixture(scope="module")
def be():
    from minsu3d_amd.backend import HipBackend
    return HipBackend()


@pytest.fixture(autouse=True)
def _restore_precision():
    prev = torch.get_float32_matmul_precision()
    yield
    torch.set_float32_matmul_precision(prev)


@pytest.fixture(scope="module")
def cm4():
    import bench
    from minsu3d_amd.MinkowskiEngine.tensor import CoordinateManager
    b = bench.make_batch([0, 1, 2, 3], torch.device("cuda", 0))
    return CoordinateManager(b["voxel_xyz"].int().contiguous(), spatial_sort=True)


def _ref_conv(a, W, nbr):
    """float64 gather-matmul: out[i] = sum_k a[nbr[k][i]] @ W[k] (absent neighbours skipped)"""
    out = torch.zeros(nbr.size(1), W.size(2), dtype=torch.float64, device=a.device)
    for k in range(W.size(0)):
        idx = nbr[k].long()
        m = idx >= 0
        out[m] += a[idx[m]] @ W[k]
    return out


def _pieces(t32, P):
    """the first P bf16 pieces of a float32 tensor, as float64 (x0 = bf16_rne(x), x1 = bf16_rne(x - x0), ...)"""
    out, r = [], t32.float()
    for _ in range(P):
        h = r.to(torch.bfloat16).float()
        out.append(h.double())
        r = r - h                               # exact in float32
    return out


def _piece_model(a32, W32, P, conv):
    """what a P-piece kernel computes, in float64: P = 2 -> a0w0 + a0w1 + a1w0, P = 1 -> a0w0"""
    a, w = _pieces(a32, P), _pieces(W32, P)
    terms = [(0, 0)] + ([(0, 1), (1, 0)] if P == 2 else [])
    return sum(conv(a[i], w[j]) for i, j in terms)


def _act32(x, scale, shift):
    """the fused prologue as the kernel computes it: fmaf(x, scale, shift) (one rounding: exact product + shift in float64,
    rounded to float32), then ReLU"""
    return torch.relu((x.double() * scale.double() + shift.double()).float())


@pytest.mark.parametrize("cin,cout,level", [(64, 64, 1), (96, 96, 2), (128, 128, 2), (64, 128, 2), (48, 48, 2), (96, 48, 2),
                                            (80, 80, 3), (112, 112, 3)])
def test_wide_layers_compute_the_piece_model(be, cm4, cin, cout, level):
    cm = cm4
    ts = 1
    for _ in range(level):
        cm.k2(ts); ts *= 2
    nbr, V, K = cm.k3(ts), cm.size(ts), 27
    assert [be.lib.ms3d_spconv_aux_kind_p(K, cin, cout, p) for p in (0, 1, 2)] == [2, 3, 4]
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(V, cin, device=dev, generator=g) * 2 + 0.5
    W = torch.randn(K, cin, cout, device=dev, generator=g) / (cin * 12) ** 0.5
    scale = torch.rand(cin, device=dev, generator=g) + 0.5
    shift = torch.randn(cin, device=dev, generator=g) * 0.3
    res = torch.randn(V, cout, device=dev, generator=g)
    dy = torch.randn(V, cout, device=dev, generator=g)
    act = _act32(x, scale, shift)
    Wt = W.flip(0).transpose(1, 2)
    fwd = lambda a, w: _ref_conv(a, w, nbr)
    exact = _ref_conv(act.double(), W.double(), nbr)
    bn = dict(scale=scale, shift=shift, mean=torch.zeros(cin, device=dev), invstd=torch.ones(cin, device=dev), relu=True,
              training=False)
    mask = (x.double() * scale.double() + shift.double() > 0) * scale.double()
    for prec, P in ((1, 2), (2, 1)):
        want = _piece_model(act, W, P, fwd)
        y, _, wf_buf = be.conv_layer_forward(x, W, nbr, V, K, cin, cout, True, (scale, shift), True, None, None, False,
                                             precision=prec)
        ref = want.abs().max()
        e = ((y.double() - want).abs().max() / ref).item()
        e_exact = ((y.double() - exact).abs().max() / ref).item()
        print(f"{cin}->{cout} rows={V} P={P}: forward vs piece model {e:.2e}, vs exact {e_exact:.2e}")
        assert e <= BAR
        if prec == 2:
            assert e_exact > BAR            # not float32 grade: the one-piece kernel ran
        # residual + output statistics in the epilogue, on the images laid out above
        y2, partial, _ = be.conv_layer_forward(x, None, nbr, V, K, cin, cout, True, (scale, shift), True, res, None, True,
                                               wf_ready=wf_buf, precision=prec)
        want2 = want + res.double()
        assert ((y2.double() - want2).abs().max() / want2.abs().max()).item() <= BAR
        st = partial.double().sum(0)
        assert torch.allclose(st[0], want2.sum(0), rtol=1e-5, atol=1e-5 * want2.abs().sum(0).max().item())
        # backward-data (fused BatchNorm-backward mask) and backward-weight
        dx, _, dW = be.conv_layer_backward(x, dy, wf_buf, nbr, nbr, V, V, K, cin, cout, bn, True, precision=prec)
        want_dx = _piece_model(dy, Wt, P, fwd) * mask
        e_dx = ((dx.double() - want_dx).abs().max() / want_dx.abs().max()).item()
        print(f"{cin}->{cout} P={P}: backward-data vs piece model {e_dx:.2e}")
        assert e_dx <= BAR
        # (the backend hands an offset list to the layers that take the exact offset-list kernel)
        wp = be.lib.ms3d_spconv_wgrad_pieces(V, K, cin, cout, int(be.offsetlist(nbr, K, V)[0] is not None), prec)
        if wp:
            assert wp == P
            idx = [torch.where(nbr[k] >= 0, nbr[k], 0).long() for k in range(K)]
            m = [(nbr[k] >= 0)[:, None] for k in range(K)]
            wgrad = lambda a, d: torch.stack([(a[idx[k]] * m[k]).t() @ d for k in range(K)])
            want_dW = _piece_model(act, dy, P, wgrad)
            e_dW = ((dW.double() - want_dW).abs().max() / want_dW.abs().max()).item()
            print(f"{cin}->{cout} P={P}: backward-weight vs piece model {e_dW:.2e}")
            assert e_dW <= 1e-5


def _fwd_bwd(be, prec, x, W, nbr_f, nbr_b, vin, vout, K, cin, cout, mirror, pre):
    y, _, wf = be.conv_layer_forward(x, W, nbr_f, vout, K, cin, cout, mirror, pre, pre is not None, None, None, True,
                                     precision=prec)
    g = torch.Generator(device="cuda").manual_seed(11)
    dy = torch.randn(vout, cout, device="cuda", generator=g)
    bn = None if pre is None else dict(scale=pre[0], shift=pre[1], mean=torch.zeros(cin, device="cuda"),
                                       invstd=torch.ones(cin, device="cuda"), relu=True, training=False)
    dx, _, dW = be.conv_layer_backward(x, dy, wf, nbr_f, nbr_b, vin, vout, K, cin, cout, bn, True, precision=prec)
    torch.cuda.synchronize()
    return y, dx, dW


def test_other_routes_are_exact_at_every_precision(be, cm4):
    """pair-list, pair-stream, K = 1, K = 8 down / up and weight-stationary routes: "medium" gives the bytes of "highest" """
    cm = cm4
    down0, up0 = cm.k2(1)
    down2, up2 = cm.k2(4)
    cm.k2(2); cm.k2(8)
    V0, V1, V2, V3 = cm.size(1), cm.size(2), cm.size(4), cm.size(8)
    ident = be.identity_table(V1, torch.device("cuda"))
    cases = [  # (nbr_fwd, nbr_bwd, vin, vout, K, cin, cout, mirror)
        (cm.k3(1), cm.k3(1), V0, V0, 27, 16, 16, True),          # pair list
        (cm.k3(1), cm.k3(1), V0, V0, 27, 32, 32, True),          # pair list, 32-row tiles
        (cm.k3(1), cm.k3(1), V0, V0, 27, 32, 64, True),          # pair stream (rectangular)
        (ident, ident, V1, V1, 1, 64, 64, False),                 # K = 1
        (down0, up0, V0, V1, 8, 32, 64, False),                   # K = 8 down
        (up2, down2, V3, V2, 8, 64, 32, False),                   # K = 8 up (transposed)
        (cm.k3(8), cm.k3(8), V3, V3, 27, 320, 160, True),         # weight-stationary (no bf16 image beyond 256 channels)
    ]
    g = torch.Generator(device="cuda").manual_seed(5)
    for nf, nb, vin, vout, K, cin, cout, mirror in cases:
        assert be.lib.ms3d_spconv_aux_kind_p(K, cin, cout, 2) == be.lib.ms3d_spconv_aux_kind(K, cin, cout)
        x = torch.randn(vin, cin, device="cuda", generator=g)
        W = torch.randn(K, cin, cout, device="cuda", generator=g) / (cin * K) ** 0.5
        pre = (torch.rand(cin, device="cuda", generator=g) + 0.5, torch.randn(cin, device="cuda", generator=g) * 0.3)
        hi = _fwd_bwd(be, 0, x, W, nf, nb, vin, vout, K, cin, cout, mirror, pre)
        md = _fwd_bwd(be, 2, x, W, nf, nb, vin, vout, K, cin, cout, mirror, pre)
        for a, b, what in zip(hi, md, ("y", "dx", "dW")):
            assert torch.equal(a, b), (K, cin, cout, what)


def _small_net():
    import minsu3d_amd.MinkowskiEngine as ME
    torch.manual_seed(3)
    return torch.nn.Sequential(
        ME.MinkowskiConvolution(16, 64, kernel_size=3), ME.MinkowskiBatchNorm(64), ME.MinkowskiReLU(),
        ME.MinkowskiConvolution(64, 64, kernel_size=3), ME.MinkowskiBatchNorm(64), ME.MinkowskiReLU(),
        ME.MinkowskiConvolution(64, 64, kernel_size=3), ME.MinkowskiBatchNorm(64), ME.MinkowskiReLU(),
        ME.MinkowskiConvolution(64, 16, kernel_size=3)).cuda().train()


def _net_step(net, coords, feats, R, fwd_prec, bwd_prec=None, window=True):
    """forward at fwd_prec (inside a prepare_conv_weights window with deferred backward-weight, or without one), switch
    to bwd_prec, backward -> output and every gradient"""
    import minsu3d_amd.MinkowskiEngine as ME
    from minsu3d_amd.MinkowskiEngine import functional as Fn
    net.zero_grad(set_to_none=True)
    torch.set_float32_matmul_precision(fwd_prec)
    x = ME.SparseTensor(features=feats, coordinates=coords)
    if window:
        code = Fn.conv_precision()
        with Fn.pass_precision(code):
            ME.prepare_conv_weights(net, precision=code)
            try:
                y = net(x)
            finally:
                ME.release_conv_weights()
    else:
        y = net(x)
    torch.set_float32_matmul_precision(bwd_prec or fwd_prec)
    (y.F * R).sum().backward()
    torch.cuda.synchronize()
    return [y.F.detach().clone()] + [p.grad.detach().clone() for p in net.parameters()]


@pytest.fixture(scope="module")
def net_inputs():
    import bench
    b = bench.make_batch([0], torch.device("cuda", 0))
    coords = b["voxel_xyz"].int().contiguous()
    g = torch.Generator(device="cuda").manual_seed(9)
    feats = torch.randn(coords.size(0), 16, device="cuda", generator=g)
    R = torch.randn(coords.size(0), 16, device="cuda", generator=g)
    return coords, feats, R


@pytest.mark.parametrize("window", [True, False])
def test_no_sticky_state(be, net_inputs, window):
    from minsu3d_amd import backend
    backend.set_backend(be)
    net = _small_net()
    a = _net_step(net, *net_inputs, "highest", window=window)
    m = _net_step(net, *net_inputs, "medium", window=window)
    b = _net_step(net, *net_inputs, "highest", window=window)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert not all(torch.equal(u, v) for u, v in zip(a, m))     # "medium" did run something else


@pytest.mark.parametrize("window", [True, False])
def test_forward_decides_the_backward_precision(be, net_inputs, window):
    from minsu3d_amd import backend
    backend.set_backend(be)
    net = _small_net()
    mm = _net_step(net, *net_inputs, "medium", "medium", window=window)
    mh = _net_step(net, *net_inputs, "medium", "highest", window=window)
    hh = _net_step(net, *net_inputs, "highest", "highest", window=window)
    assert all(torch.equal(u, v) for u, v in zip(mm, mh))
    assert not all(torch.equal(u, v) for u, v in zip(mm[1:], hh[1:]))


def _model_and_batch(name, seed=4, m=16):
    if m == 16:
        model = _build(name, seed=seed)
    else:
        from minsu3d_amd.config import load_config
        import minsu3d_amd.model as M
        torch.manual_seed(seed)
        cfg = load_config([f"model={name}", "model.network.blocks=[1,2,3]", f"model.network.m={m}"])
        model = getattr(M, cfg.model.network.module)(cfg)
        model.current_epoch = cfg.model.network.prepare_epochs + 1
    model.hparams.cfg.data.point_num_avg = [-1, -1] + [400.0] * 18
    model.hparams.cfg.data.radius_avg = [-1.0, -1.0] + [0.3] * 18
    model = model.cuda()
    model.voxelization_rand = (torch.tensor([0.3, 0.6, 0.9]).cuda(), torch.tensor([0.1, 0.2, 0.3]).cuda())
    batch = small_batch((41, 42))
    if name == "softgroup":
        batch = _softgroup_scores(batch)
    return model, _cuda(batch)


def test_medium_training_step_is_reproducible(be):
    from minsu3d_amd import backend
    backend.set_backend(be)
    torch.set_float32_matmul_precision("medium")
    model, batch = _model_and_batch("hais")
    first = _one_step(model, batch)
    again = _one_step(model, batch)
    assert again.keys() == first.keys()
    n_bad, worst = _diff_report(again, first)
    assert n_bad == 0, worst


# |loss(medium) - loss(highest)| / max(|loss(highest)|, 1), m = 32 models on two small scenes: measured 1.7e-4 (PointGroup),
# 5.8e-5 (HAIS, SoftGroup); "high" 2.0e-6 at most.  The bound leaves a factor of ~10.
MEDIUM_LOSS_BOUND = 2e-3


@pytest.mark.parametrize("name", ["pointgroup", "hais", "softgroup"])
def test_models_at_lower_precision(be, name):
    from minsu3d_amd import backend
    backend.set_backend(be)
    model, batch = _model_and_batch(name, m=32)      # m = 32: levels of 64 and 96 channels take the bf16 kernels
    losses = {}
    for prec in ("highest", "high", "medium"):
        torch.set_float32_matmul_precision(prec)
        m = copy.deepcopy(model)
        m.voxelization_rand = model.voxelization_rand
        m.train()
        with torch.no_grad():
            out = m(batch)
            losses[prec] = {k: float(v) for k, v in m._loss(batch, out).items()}
    print(name, losses)
    rel = {s: max(abs(losses[s][k] - v) / max(abs(v), 1.0) for k, v in losses["highest"].items()) for s in ("high", "medium")}
    print(name, "largest relative loss change:", rel)
    assert rel["medium"] > 0                        # the lower setting did reach the kernels
    for k, ref in losses["highest"].items():
        assert abs(losses["high"][k] - ref) <= 1e-3 * max(abs(ref), 1e-6) + 1e-6, (k, ref, losses["high"][k])
        md = losses["medium"][k]
        assert np.isfinite(md) and abs(md - ref) <= MEDIUM_LOSS_BOUND * max(abs(ref), 1.0), (k, ref, md)


def test_pointgroup_learns_at_medium_precision():
    import convergence
    torch.set_float32_matmul_precision("medium")
    rec = convergence.run(steps=360, prepare=160)
    before, mid, end = rec["eval"]
    tot = [sum(l.get(k, 0.0) for k in ("semantic_loss", "offset_norm_loss", "offset_dir_loss")) for l in rec["loss"]]
    win = [float(np.mean(tot[i:i + 40])) for i in range(0, len(tot), 40)]
    print("point-loss window means:", [round(w, 3) for w in win])
    print("eval:", before, mid, end)
    assert before["semantic_mIoU"] < 20.0 and before["AP50"] < 0.05
    assert all(b <= a + 0.02 for a, b in zip(win, win[1:])), win
    assert win[-1] < win[0] - 2.0
    assert mid["semantic_mIoU"] > 85.0 and end["semantic_mIoU"] > 92.0
    assert end["AP50"] > 0.7 and end["AP25"] > 0.8 and end["AP"] > 0.5, end
    assert end["AP"] > mid["AP"] + 0.2
    assert end["predicted_instances"] <= 2 * end["gt_instances"]
    score = [l["score_loss"] for l in rec["loss"] if "score_loss" in l]
    assert len(score) == 200 and np.mean(score[-40:]) < np.mean(score[:40])
