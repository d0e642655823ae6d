"""GPU: layers that create and drop coordinates -- ms3d_coords_expand / ms3d_coords_prune, MinkowskiGenerativeConvolutionTranspose,
MinkowskiPruning, SparseTensor.coordinate_rows / features_at_coordinates.

Coordinate sets, row maps, pruned features and their gradients are compared EXACTLY (they are copies): against the numpy
restatements of tests/generative_ref.py, which tests/test_generative_cpu.py pins to dense torch.  Values of the convolutions:
dense F.conv_transpose3d in float64 on the CPU with the padding / crop convention of test_geometry_gpu._transpose_case (small
clouds), a float64 gather-GEMM over a host-built table (large ones); bound 1e-4 of the largest magnitude (RTOL of
test_geometry_gpu, the project's bar for sparse-convolution activations), dgamma / dbeta of a fused BatchNorm 1e-3 as there.
features_at_coordinates' gradient is compared exactly with queries that name a row at most twice: a + b = b + a in floating
point, so the comparison does not depend on the order either side sums in."""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from generative_ref import (GEOMS, downsample_np, expand_np, expand_offsets_np, member_np, offsets_np, rows_np, strides_for,
                            transpose_front_pad)
from sparse_ref import random_sparse, ref_conv
from test_geometry_gpu import RTOL, check, dense_weight, densify64, manager_at, rel_err, sorted_map

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ME():
    import minsu3d_amd.MinkowskiEngine as me
    return me


@pytest.fixture(scope="module")
def be():
    from minsu3d_amd.backend import get_backend
    return get_backend()


@pytest.fixture(autouse=True)
def _restore_precision():
    prev = torch.get_float32_matmul_precision()
    yield
    torch.set_float32_matmul_precision(prev)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def at_stride(fine, ts):
    c, t = fine, 1
    while t < ts:
        t *= 2
        c = downsample_np(c, t)
    return c


# ---------------------------------------------------------------------------------------------- 1. coords_expand
@pytest.mark.parametrize("variant", ["plain", "negative", "shuffled"])
@pytest.mark.parametrize("ks,stride,dil", GEOMS)
def test_coords_expand_exact(be, ks, stride, dil, variant):
    rng = np.random.default_rng(7)
    fine, _ = random_sparse(rng, B=2, grid=12, n=400, C=1)
    for ts in strides_for(stride):
        c = at_stride(fine, ts).copy()
        if variant == "negative":
            c[:, 1:] -= 9 * ts
        elif variant == "shuffled":
            rng.shuffle(c)
        off = offsets_np(ks, dil, ts // stride)
        got = be.coords_expand(dev(c), torch.from_numpy(off.astype(np.int32))).cpu().numpy()
        want = expand_np(c, ks, stride, dil, ts)
        assert got.shape == want.shape and np.array_equal(got, want), (ks, stride, dil, ts, variant)


def test_coords_expand_repeated_rows_empty_and_range(be):
    from minsu3d_amd._lib import HipLibraryError
    rng = np.random.default_rng(9)
    c, _ = random_sparse(rng, B=2, grid=12, n=300, C=1)
    rep = np.concatenate([c[:120], c[40:90], c[120:], c[:7]])            # rows that occur two and three times
    for ks, dil in ((3, 1), (2, 1), (5, 1)):
        off = offsets_np(ks, dil, 1)
        got = be.coords_expand(dev(rep), torch.from_numpy(off.astype(np.int32))).cpu().numpy()
        assert np.array_equal(got, expand_offsets_np(rep, off)), ks
        assert np.array_equal(got, expand_offsets_np(c, off)), ks          # ... and the repeats change nothing here
    empty = be.coords_expand(torch.empty((0, 4), dtype=torch.int32, device="cuda"), torch.zeros((27, 3), dtype=torch.int32))
    assert tuple(empty.shape) == (0, 4) and empty.dtype == torch.int32
    # a cloud touching +16383: a +1 offset leaves the packable range -> MS3D_E_UNSUPPORTED (10002), not a wrapped row
    hi = c.copy()
    hi[:, 1:] += 16383 - c[:, 1:].max(0)
    off = offsets_np(3, 1, 1).astype(np.int32)
    with pytest.raises(HipLibraryError, match="10002"):
        be.coords_expand(dev(hi), torch.from_numpy(off))
    lo = c.copy()
    lo[:, 1:] += -16384 - c[:, 1:].min(0)
    with pytest.raises(HipLibraryError, match="10002"):
        be.coords_expand(dev(lo), torch.from_numpy(off))
    inward = off[(off >= 0).all(1)] * -1                                     # offsets that stay inside from the upper corner
    got = be.coords_expand(dev(hi), torch.from_numpy(np.ascontiguousarray(inward))).cpu().numpy()
    assert np.array_equal(got, expand_offsets_np(hi, inward.astype(np.int64)))
    with pytest.raises(HipLibraryError, match="10002"):                      # more than 2^31 - 1 candidates
        be.coords_expand(torch.zeros((1 << 20, 4), dtype=torch.int32, device="cuda"), torch.zeros((2048, 3), dtype=torch.int32))


# ---------------------------------------------------------------------------------------------- 2. against dense float64
def _gen_case(ME, ks, stride, dil, cin, cout, ts, pending=False, B=2, G=12, n=400, seed=23):
    rng = np.random.default_rng(seed + 100 * ks + 10 * stride + dil + cin)
    fine, _ = random_sparse(rng, B=B, grid=G, n=n, C=1)
    cm = manager_at(ME, fine, ts)
    in_coords = cm.coords[ts].cpu().numpy()
    out_ts = ts // stride
    feats = rng.standard_normal((in_coords.shape[0], cin)).astype(np.float32)
    conv = ME.MinkowskiGenerativeConvolutionTranspose(cin, cout, kernel_size=ks, stride=stride, dilation=dil, bias=True,
                                                      dimension=3).cuda().train()
    xf = dev(feats).requires_grad_(True)
    xin = ME.SparseTensor(xf, coordinate_manager=cm, tensor_stride=ts)
    x64 = torch.from_numpy(feats).double().requires_grad_(True)
    a64 = x64
    if pending:
        bn = ME.MinkowskiBatchNorm(cin).cuda().train()
        with torch.no_grad():
            bn.bn.weight.uniform_(0.5, 1.5)
            bn.bn.bias.uniform_(-0.3, 0.3)
        xin = ME.MinkowskiReLU()(bn(xin))
        assert xin._pending is not None and xin._pending["relu"]
        g64 = bn.bn.weight.detach().double().cpu().requires_grad_(True)
        b64 = bn.bn.bias.detach().double().cpu().requires_grad_(True)
        a64 = torch.relu(F.batch_norm(x64, None, None, g64, b64, True, 0.1, 1e-5))
    y = conv(xin)
    assert y.tensor_stride == out_ts and y.coordinate_manager is not cm
    out_coords = y.C.cpu().numpy()
    assert np.array_equal(out_coords, expand_np(in_coords, ks, stride, dil, ts))
    if pending:
        assert torch.is_tensor(y._stats) and y._stats.numel() > 0        # epilogue statistics for a following BatchNorm
    W64 = conv.kernel.detach().double().cpu().requires_grad_(True)
    bias64 = conv.bias.detach().double().cpu().requires_grad_(True)
    # out[stride * i + k * dil - p] += x[i] W[k] in units of the output tensor stride (_transpose_case's convention: p cells
    # of a centred kernel lie in front of the first input cell); nothing is cropped, so every reachable voxel is in the grid
    d = densify64(in_coords, a64, B, G // ts, ts)
    yd = F.conv_transpose3d(d, dense_weight(W64, ks).transpose(0, 1), stride=stride, dilation=dil)
    p = transpose_front_pad(ks, dil)
    oc = torch.from_numpy(out_coords).long()
    ix = (oc[:, 0], slice(None), oc[:, 1] // out_ts + p, oc[:, 2] // out_ts + p, oc[:, 3] // out_ts + p)
    outside = torch.ones(yd.shape[0], 1, *yd.shape[2:], dtype=torch.bool)
    outside[ix[0], 0, ix[2], ix[3], ix[4]] = False
    assert float((yd.detach().abs() * outside).max()) == 0.0, "the dense operator reaches a voxel the generated set lacks"
    want = yd[ix] + bias64
    tag = f"generative k{ks} s{stride} d{dil} ts{ts} {cin}->{cout}" + (" bn+relu" if pending else "")
    check(tag + " forward", y._F, want, RTOL)
    g = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y._F.backward(dev(g))
    want.backward(torch.from_numpy(g).double())
    check(tag + " backward-data", xf.grad, x64.grad, RTOL)
    check(tag + " backward-weight", conv.kernel.grad, W64.grad, RTOL)
    check(tag + " bias gradient", conv.bias.grad, bias64.grad.view(1, -1), RTOL)
    if pending:
        check(tag + " dgamma", bn.bn.weight.grad, g64.grad, 1e-3)
        check(tag + " dbeta", bn.bn.bias.grad, b64.grad, 1e-3)


@pytest.mark.parametrize("cin,cout", [(6, 16), (16, 32), (32, 48)])
@pytest.mark.parametrize("ks,stride,dil", GEOMS)
def test_generative_against_dense(ME, ks, stride, dil, cin, cout):
    _gen_case(ME, ks, stride, dil, cin, cout, ts=2 if stride == 2 else 1)


@pytest.mark.parametrize("ks,stride,dil", [(2, 2, 1), (3, 2, 1), (3, 1, 1)])
def test_generative_against_dense_other_tensor_stride(ME, ks, stride, dil):
    _gen_case(ME, ks, stride, dil, 16, 32, ts=4 if stride == 2 else 2, n=900, G=16)


@pytest.mark.parametrize("ks,stride,dil", GEOMS)
def test_generative_pending_bn_relu(ME, ks, stride, dil):
    _gen_case(ME, ks, stride, dil, 16, 32, ts=2 if stride == 2 else 1, pending=True)


def test_generated_set_is_cached_and_shared(ME):
    rng = np.random.default_rng(3)
    fine, _ = random_sparse(rng, B=2, grid=12, n=300, C=1)
    cm = manager_at(ME, fine, 2)
    x = ME.SparseTensor(torch.randn(cm.size(2), 16, device="cuda"), coordinate_manager=cm, tensor_stride=2)
    a = ME.MinkowskiGenerativeConvolutionTranspose(16, 16, kernel_size=3, stride=2, dimension=3).cuda()
    b = ME.MinkowskiGenerativeConvolutionTranspose(16, 32, kernel_size=3, stride=2, dimension=3).cuda()
    c = ME.MinkowskiGenerativeConvolutionTranspose(16, 16, kernel_size=2, stride=2, dimension=3).cuda()
    ya, yb, yc = a(x), b(x), c(x)
    assert ya.coordinate_manager is yb.coordinate_manager and ya.coordinate_manager is not yc.coordinate_manager
    assert cm.generate(2, 3, 2, 1) is cm.generate(2, 3, 2, 1)
    z = ME.cat(ya, yb)
    assert z.F.shape == (ya.F.size(0), 48) and torch.equal(z.F[:, :16], ya.F) and torch.equal(z.C, ya.C)
    assert 1 in cm.coords and cm.coords[1].size(0) == 300            # the manager's own finer set is untouched


def test_generative_stride_1_on_a_morton_sorted_manager(ME):
    """>= 100 000 rows at tensor stride 1: the manager holds its rows in Morton order.  The generated set must still be in
    first-occurrence order over the rows the CALLER sees (x.coordinates), and the values those of the caller's features."""
    rng = np.random.default_rng(29)
    n, G = 110000, 80
    flat = rng.choice(2 * G ** 3, n, replace=False)
    coords = np.stack([flat // G ** 3, flat // G ** 2 % G, flat // G % G, flat % G], 1).astype(np.int32)
    feats = rng.standard_normal((n, 4)).astype(np.float32)
    xf = dev(feats).requires_grad_(True)
    x = ME.SparseTensor(xf, dev(coords))
    assert x.coordinate_manager.perm is not None
    conv = ME.MinkowskiGenerativeConvolutionTranspose(4, 8, kernel_size=3, stride=1, dimension=3).cuda()
    y = conv(x)
    want_set = expand_np(coords, 3, 1, 1, 1)
    got = y.C.cpu().numpy()
    assert got.shape == want_set.shape and np.array_equal(got, want_set)
    nbr = torch.from_numpy(sorted_map(coords, want_set, -offsets_np(3, 1, 1)))
    x64 = torch.from_numpy(feats).double().requires_grad_(True)
    W64 = conv.kernel.detach().double().cpu().requires_grad_(True)
    want = ref_conv(x64, W64, nbr)
    check(f"generative k3 s1 4->8 on {n} Morton-sorted rows -> {len(got)}: forward", y.F, want, RTOL)
    g = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y.F.backward(dev(g))
    want.backward(torch.from_numpy(g).double())
    check("... backward-data (caller's row order)", xf.grad, x64.grad, RTOL)
    check("... backward-weight", conv.kernel.grad, W64.grad, RTOL)


# ---------------------------------------------------------------------------------------------- 3. wide K = 27
def _pieces(t32, P):
    out, r = [], t32.float()
    for _ in range(P):
        h = r.to(torch.bfloat16).float()
        out.append(h.double())
        r = r - h
    return out


def _two_piece(a32, w32, f):
    """what a two-piece bf16 kernel computes, in float64 (tests/test_conv_precision_gpu.py): a0 w0 + a0 w1 + a1 w0"""
    a, w = _pieces(a32, 2), _pieces(w32, 2)
    return f(a[0], w[0]) + f(a[0], w[1]) + f(a[1], w[0])


@pytest.mark.parametrize("precision", ["highest", "high"])
def test_generative_wide_k27_stays_off_the_submanifold_route(ME, be, precision):
    """64 -> 64, kernel 3, stride 1, generative: K = 27 with Vin != Vout and enough output rows that the backward-weight route
    of the wide SUBMANIFOLD layers would be chosen by shape alone.  "highest": 1e-4 against the float64 gather-GEMM.  "high":
    the wide layers' kernels may keep two bf16 pieces per operand; the existing precision tests hold such a result to 3e-6
    of the float64 product of the piece-reconstructed operands, every other route to float32 grade -- each of the three
    results must meet that bar against one of the two, and the 1e-4 bar against the exact product either way."""
    rng = np.random.default_rng(5)
    coords, _ = random_sparse(rng, B=1, grid=32, n=3000, C=1)
    cm = manager_at(ME, coords, 1)
    feats = rng.standard_normal((3000, 64)).astype(np.float32)
    xf = dev(feats).requires_grad_(True)
    conv = ME.MinkowskiGenerativeConvolutionTranspose(64, 64, kernel_size=3, stride=1, dimension=3).cuda()
    torch.set_float32_matmul_precision(precision)
    y = conv(ME.SparseTensor(xf, coordinate_manager=cm))
    out = y.C.cpu().numpy()
    vout = out.shape[0]
    assert np.array_equal(out, expand_np(coords, 3, 1, 1, 1)) and vout >= 13000, vout
    lib = be.lib
    assert lib.ms3d_spconv_wgrad_is_bf16x3(vout, 27, 64, 64, 0) == 1, vout      # what K == 27 alone would pick
    assert lib.ms3d_spconv_wgrad_is_bf16x3_g(vout, 27, 64, 64, 0, 0) == 0
    off = offsets_np(3, 1, 1)
    nbr = sorted_map(coords, out, -off)
    gen = cm.generate(1, 3, 1, 1)
    assert np.array_equal(gen[1].cpu().numpy(), nbr)
    inv = np.full((27, 3000), -1, np.int32)
    kk, oo = np.nonzero(nbr >= 0)
    inv[kk, nbr[kk, oo]] = oo
    assert np.array_equal(gen[2].cpu().numpy(), inv)
    g = rng.standard_normal((vout, 64)).astype(np.float32)
    y._F.backward(dev(g))
    torch.cuda.synchronize()
    x64 = torch.from_numpy(feats).double().requires_grad_(True)
    W64 = conv.kernel.detach().double().cpu().requires_grad_(True)
    nbr_t = torch.from_numpy(nbr)
    want = ref_conv(x64, W64, nbr_t)
    want.backward(torch.from_numpy(g).double())
    tag = f"generative k3 s1 64->64, {vout} rows, {precision}"
    got = {"forward": y._F, "backward-data": xf.grad, "backward-weight": conv.kernel.grad}
    exact = {"forward": want, "backward-data": x64.grad, "backward-weight": W64.grad}
    for name in got:
        check(f"{tag} {name}", got[name], exact[name], RTOL)
    if precision == "high":
        x32, W32, g32 = torch.from_numpy(feats), conv.kernel.detach().cpu(), torch.from_numpy(g)
        inv_t = torch.from_numpy(inv)
        idx = torch.where(nbr_t < 0, torch.full_like(nbr_t, 3000), nbr_t).long()

        def wgrad(a, d):
            ap = torch.cat([a, a.new_zeros(1, a.size(1))])
            return torch.stack([ap[idx[k]].t() @ d for k in range(27)])
        model = {"forward": _two_piece(x32, W32, lambda a, w: ref_conv(a, w, nbr_t)),
                 "backward-data": _two_piece(g32, W32, lambda d, w: ref_conv(d, w.transpose(1, 2), inv_t)),
                 "backward-weight": _two_piece(x32, g32, wgrad)}
        for name in got:
            e_exact, e_model = rel_err(got[name], exact[name]), rel_err(got[name], model[name])
            print(f"{tag} {name}: vs exact {e_exact:.2e}, vs two-piece model {e_model:.2e} (bound 3e-06 on one of them)")
            assert min(e_exact, e_model) <= 3e-6, (name, e_exact, e_model)


# ---------------------------------------------------------------------------------------------- 4. same function
@pytest.mark.parametrize("ks,dil", [(2, 1), (3, 1), (4, 1), (2, 2)])
def test_same_function_as_the_transposed_convolution(ME, ks, dil):
    rng = np.random.default_rng(31 + ks)
    fine, _ = random_sparse(rng, B=2, grid=12, n=400, C=1)
    cm = manager_at(ME, fine, 2)
    feats = torch.randn(cm.size(2), 16, device="cuda")
    old = ME.MinkowskiConvolutionTranspose(16, 32, kernel_size=ks, stride=2, dilation=dil, dimension=3).cuda()
    gen = ME.MinkowskiGenerativeConvolutionTranspose(16, 32, kernel_size=ks, stride=2, dilation=dil, dimension=3).cuda()
    with torch.no_grad():
        gen.kernel.copy_(old.kernel)
    yo = old(ME.SparseTensor(feats, coordinate_manager=cm, tensor_stride=2))
    yg = gen(ME.SparseTensor(feats, coordinate_manager=cm, tensor_stride=2))
    assert yo.tensor_stride == 1 and yg.tensor_stride == 1
    fine_rows, gen_rows = cm.coords[1].cpu().numpy(), yg.C.cpu().numpy()
    reach = expand_np(cm.coords[2].cpu().numpy(), ks, 2, dil, 2)                # every voxel the kernel reaches
    reached = member_np(fine_rows, reach)
    where = rows_np(fine_rows, gen_rows)                                       # fine row -> generated row (Python dict)
    # (not vacuous: even the sparsest case, kernel 2 with dilation 2, reaches the all-even eighth of the 400 finer rows)
    assert reached.sum() > 20 and (where[reached] >= 0).all(), "the generated set misses a reached finer row"
    assert not (where[~reached] >= 0).any()
    fo = yo.F.detach().cpu()
    assert float(fo[torch.from_numpy(~reached)].abs().max() if (~reached).any() else 0.0) == 0.0      # never fed: exactly zero
    common = torch.from_numpy(np.nonzero(reached)[0])
    check(f"generative vs transposed k{ks} d{dil} on the common rows", yg.F.detach().cpu()[torch.from_numpy(where[reached]).long()],
          fo[common], RTOL)


# ---------------------------------------------------------------------------------------------- 5. pruning
def _masks(rng, n):
    return {"random": rng.random(n) < 0.4, "all-true": np.ones(n, bool), "all-false": np.zeros(n, bool)}


def _prune_case(ME, make, rng, tag):
    """make() -> (a fresh SparseTensor, the leaf its features derive from by a row permutation at most)"""
    x, _ = make()
    feats, coords = x.F.detach().clone(), x.C.clone()
    n, c = feats.shape
    for name, m in _masks(rng, n).items():
        x, xf = make()                      # (a backward pass frees the graph between the leaf and the engine's row order)
        mask = dev(m)
        y = ME.MinkowskiPruning()(x, mask)
        assert y.tensor_stride == x.tensor_stride and y.coordinate_manager is not x.coordinate_manager
        assert y.coordinate_manager.perm is None and list(y.coordinate_manager.coords) == [x.tensor_stride]
        assert tuple(y.F.shape) == (int(m.sum()), c) and torch.equal(y.F, feats[mask]), (tag, name)
        assert y.C.dtype == torch.int32 and torch.equal(y.C, coords[mask]), (tag, name)
        g = torch.randn(int(m.sum()), c, device="cuda")
        y.F.backward(g)
        want = torch.zeros(n, c, device="cuda")
        want[mask] = g
        # (xf is in the caller's order, as the mask is)
        assert torch.equal(xf.grad, want), (tag, name)


def test_pruning_small(ME):
    rng = np.random.default_rng(41)
    for n, C_ in ((400, 16), (333, 5)):                                       # (5 floats: rows that are no multiple of 16 bytes)
        coords, feats = random_sparse(rng, B=2, grid=12, n=n, C=C_)

        def make():
            xf = dev(feats).requires_grad_(True)
            return ME.SparseTensor(xf, dev(coords)), xf
        _prune_case(ME, make, rng, f"{n} rows x {C_}")


def test_pruning_morton_sorted_stride_1(ME):
    rng = np.random.default_rng(43)
    n, G = 125000, 96
    flat = rng.choice(2 * G ** 3, n, replace=False)
    coords = np.stack([flat // G ** 3, flat // G ** 2 % G, flat // G % G, flat % G], 1).astype(np.int32)
    feats = torch.randn(n, 16, device="cuda")

    def make():
        xf = feats.clone().requires_grad_(True)
        x = ME.SparseTensor(xf, dev(coords))
        assert x.coordinate_manager.perm is not None, "the Morton-sorted manager is what this test is about"
        assert not torch.equal(x.coordinate_manager.perm, torch.arange(n, device="cuda"))
        return x, xf
    _prune_case(ME, make, rng, "125k rows, Morton sorted")
    # behind a layer (the features are then only held in the engine's order) and behind a pending BatchNorm + ReLU
    x, _ = make()
    conv = ME.MinkowskiConvolution(16, 16, kernel_size=3, dimension=3).cuda()
    bn = ME.MinkowskiBatchNorm(16).cuda().train()
    h = ME.MinkowskiReLU()(bn(conv(x)))
    assert h._pending is not None
    m = dev(rng.random(n) < 0.5)
    y = ME.MinkowskiPruning()(h, m)
    assert torch.equal(y.F, h.F[m]) and torch.equal(y.C, x.C[m])


def test_pruning_stride_2(ME):
    rng = np.random.default_rng(47)
    fine, _ = random_sparse(rng, B=2, grid=16, n=1500, C=1)
    cm = manager_at(ME, fine, 2)
    feats = torch.randn(cm.size(2), 32, device="cuda")

    def make():
        xf = feats.clone().requires_grad_(True)
        return ME.SparseTensor(xf, coordinate_manager=cm, tensor_stride=2), xf
    _prune_case(ME, make, rng, "stride 2")
    x, _ = make()
    # a pruned stride-2 tensor is a full citizen: k3 convolution, strided convolution and its transpose back
    y = ME.MinkowskiPruning()(x, dev(rng.random(cm.size(2)) < 0.6))
    pc = y.C.cpu().numpy()
    c3 = ME.MinkowskiConvolution(32, 16, kernel_size=3, dimension=3).cuda()
    z = c3(y)
    nbr = sorted_map(pc, pc, offsets_np(3, 1, 2))
    want = ref_conv(y.F.detach().double().cpu(), c3.kernel.detach().double().cpu(), torch.from_numpy(nbr))
    check("k3 on a pruned stride-2 tensor", z.F, want, RTOL)
    down = ME.MinkowskiConvolution(16, 16, kernel_size=2, stride=2, dimension=3).cuda()
    up = ME.MinkowskiConvolutionTranspose(16, 16, kernel_size=2, stride=2, dimension=3).cuda()
    d = down(z)
    u = up(d)
    assert d.tensor_stride == 4 and np.array_equal(d.C.cpu().numpy(), downsample_np(pc, 4))
    assert u.tensor_stride == 2 and torch.equal(u.C, y.C) and u.F.shape == (pc.shape[0], 16)
    with pytest.raises(NotImplementedError, match="generating new coordinates is not supported"):
        up(y)                                     # nothing finer than the root of a pruned tensor: the old refusal stands
    gp = ME.MinkowskiGlobalAvgPooling()(z)
    b = torch.from_numpy(pc[:, 0]).long()
    want = torch.stack([z.F.detach().double().cpu()[b == i].mean(0) for i in sorted(set(b.tolist()))])
    check("global average pooling on a pruned tensor", gp.F, want, 1e-5)


# ---------------------------------------------------------------------------------------------- 6. lookup
def _lookup_case(x, rng, tag):
    coords = x.C.cpu().numpy()
    n = coords.shape[0]
    present = coords[rng.integers(0, n, 300)]                                   # with repeats
    absent = present.copy()
    absent[:, 1 + rng.integers(0, 3)] += 1000
    other_batch = present[:20].copy()
    other_batch[:, 0] += 50
    far = np.array([[0, 20000, 0, 0], [0, 0, -20000, 0], [-1, 0, 0, 0]], np.int32)        # outside what a key can hold
    q = np.concatenate([present, absent, other_batch, far, present[:40]]).astype(np.int32)
    rng.shuffle(q)
    got = x.coordinate_rows(dev(q))
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(q),)
    want = rows_np(q, coords)
    assert (want >= 0).sum() >= 340 and (want < 0).sum() >= 300
    assert np.array_equal(got.cpu().numpy(), want), tag
    assert x.coordinate_rows(torch.empty((0, 4), dtype=torch.int32, device="cuda")).numel() == 0
    assert np.array_equal(x.coordinate_rows(dev(q.astype(np.int64))).cpu().numpy(), want)          # int64 queries


def test_coordinate_rows(ME):
    rng = np.random.default_rng(53)
    coords, feats = random_sparse(rng, B=2, grid=12, n=400, C=8)
    _lookup_case(ME.SparseTensor(dev(feats), dev(coords)), rng, "400 rows")
    n, G = 125000, 96
    flat = rng.choice(2 * G ** 3, n, replace=False)
    big = np.stack([flat // G ** 3, flat // G ** 2 % G, flat // G % G, flat % G], 1).astype(np.int32)
    x = ME.SparseTensor(torch.randn(n, 4, device="cuda"), dev(big))
    assert x.coordinate_manager.perm is not None
    _lookup_case(x, rng, "125k rows, Morton sorted")
    cm = manager_at(ME, coords, 2)
    _lookup_case(ME.SparseTensor(torch.randn(cm.size(2), 4, device="cuda"), coordinate_manager=cm, tensor_stride=2), rng, "stride 2")
    gen = ME.MinkowskiGenerativeConvolutionTranspose(4, 4, kernel_size=3, stride=2, dimension=3).cuda()
    _lookup_case(gen(ME.SparseTensor(torch.randn(cm.size(2), 4, device="cuda"), coordinate_manager=cm, tensor_stride=2)), rng,
                 "generated")


def test_features_at_coordinates(ME):
    rng = np.random.default_rng(59)
    for n, G, C_ in ((400, 12, 16), (125000, 96, 8)):
        flat = rng.choice(2 * G ** 3, n, replace=False)
        coords = np.stack([flat // G ** 3, flat // G ** 2 % G, flat // G % G, flat % G], 1).astype(np.int32)
        xf = torch.randn(n, C_, device="cuda").requires_grad_(True)
        x = ME.SparseTensor(xf, dev(coords))
        pick = rng.permutation(n)[:200]
        absent = coords[pick[:80]].copy()
        absent[:, 2] += 500
        q = np.concatenate([coords[pick], coords[pick[:60]], absent]).astype(np.int32)          # 60 rows asked for twice
        rng.shuffle(q)
        rows = torch.from_numpy(rows_np(q, coords)).cuda().long()
        y = x.features_at_coordinates(dev(q))
        ref_leaf = xf.detach().clone().requires_grad_(True)
        want = torch.where((rows >= 0)[:, None], ref_leaf[rows.clamp(min=0)], torch.zeros((), device="cuda"))
        assert torch.equal(y, want), n
        g = torch.randn(len(q), C_, device="cuda")
        y.backward(g)
        want.backward(g)
        assert torch.equal(xf.grad, ref_leaf.grad), n
        assert tuple(x.features_at_coordinates(torch.empty((0, 4), dtype=torch.int32, device="cuda")).shape) == (0, C_)


# ---------------------------------------------------------------------------------------------- 7. a completion-shaped network
class _CompletionNet(torch.nn.Module):
    """two strided encoder blocks; generative k2 s2 -> BN -> ReLU -> prune -> k3 convolution; generative k3 s2 -> BN -> ReLU ->
    prune -> 1x1 head.  The pruning targets are the ground-truth voxels at tensor stride 2 and 1."""

    def __init__(self, ME, cin=6, c=16, ncls=3):
        super().__init__()
        self.ME = ME
        conv, bn, gen = ME.MinkowskiConvolution, ME.MinkowskiBatchNorm, ME.MinkowskiGenerativeConvolutionTranspose
        self.enc1 = conv(cin, c, kernel_size=2, stride=2, dimension=3)
        self.bn1 = bn(c)
        self.enc2 = conv(c, 2 * c, kernel_size=3, stride=2, dimension=3)
        self.bn2 = bn(2 * c)
        self.gen2 = gen(2 * c, c, kernel_size=2, stride=2, dimension=3)
        self.bn_g2 = bn(c)
        self.mid = conv(c, c, kernel_size=3, dimension=3)
        self.bn_mid = bn(c)
        self.gen1 = gen(c, c, kernel_size=3, stride=2, dimension=3)
        self.bn_g1 = bn(c)
        self.head = conv(c, ncls, kernel_size=1, bias=True, dimension=3)
        self.prune = ME.MinkowskiPruning()

    @staticmethod
    def keep(x, target):
        rows = x.coordinate_rows(target)
        mask = torch.zeros(x.C.size(0), dtype=torch.bool, device=rows.device)
        mask[rows[rows >= 0].long()] = True
        return mask

    def forward(self, x, target2, target1):
        relu = self.ME.MinkowskiReLU()
        sets = {}
        h = self.enc2(relu(self.bn1(self.enc1(x))))                    # stride 4
        sets["s4"] = h.C
        g2 = relu(self.bn_g2(self.gen2(relu(self.bn2(h)))))           # stride 2, generated
        sets["g2"] = g2.C
        p2 = self.prune(g2, self.keep(g2, target2))
        sets["p2"] = p2.C
        m = self.mid(p2)
        g1 = relu(self.bn_g1(self.gen1(relu(self.bn_mid(m)))))        # stride 1, generated
        sets["g1"] = g1.C
        p1 = self.prune(g1, self.keep(g1, target1))
        sets["p1"] = p1.C
        assert (h.tensor_stride, g2.tensor_stride, m.tensor_stride, p1.tensor_stride) == (4, 2, 2, 1)
        return self.head(p1), sets


def _completion_step(ME, net, coords, feats, t2, t1):
    net.zero_grad(set_to_none=True)
    xf = dev(feats).requires_grad_(True)
    z, sets = net(ME.SparseTensor(xf, dev(coords)), dev(t2), dev(t1))
    loss = (z.F * z.F).mean()
    loss.backward()
    torch.cuda.synchronize()
    res = {"z": z.F.detach().clone(), "dx": xf.grad.clone()}
    res.update({"set/" + k: v.clone() for k, v in sets.items()})
    res.update({"grad/" + n: p.grad.clone() for n, p in net.named_parameters()})
    return res


def test_completion_network_sets_gradients_and_reproducibility(ME):
    torch.manual_seed(0)
    rng = np.random.default_rng(83)
    truth, _ = random_sparse(rng, B=2, grid=16, n=1800, C=1)             # the complete shape; the input sees 60 % of it
    coords = truth[rng.random(len(truth)) < 0.6]
    feats = rng.standard_normal((len(coords), 6)).astype(np.float32)
    t1, t2 = truth, downsample_np(truth, 2)
    net = _CompletionNet(ME).cuda().train()
    a = _completion_step(ME, net, coords, feats, t2, t1)
    b = _completion_step(ME, net, coords, feats, t2, t1)
    diff = [k for k in a if not torch.equal(a[k], b[k])]
    assert not diff, f"not bit-reproducible: {diff}"
    s4 = downsample_np(downsample_np(coords, 2), 4)
    g2 = expand_np(s4, 2, 2, 1, 4)
    p2 = g2[member_np(g2, t2)]
    g1 = expand_np(p2, 3, 2, 1, 2)
    p1 = g1[member_np(g1, t1)]
    for name, want in (("s4", s4), ("g2", g2), ("p2", p2), ("g1", g1), ("p1", p1)):
        got = a["set/" + name].cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), name
    assert 0 < len(p2) < len(g2) and 0 < len(p1) < len(g1) and a["z"].shape == (len(p1), 3)
    for n, p in net.named_parameters():
        g = a["grad/" + n]
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0, n
    assert torch.isfinite(a["dx"]).all() and float(a["dx"].abs().max()) > 0 and torch.isfinite(a["z"]).all()


# ---------------------------------------------------------------------------------------------- 8. not a toy
def _ms(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


@pytest.mark.parametrize("ks", [2, 3])
def test_generative_50k_rows(ME, be, ks):
    rng = np.random.default_rng(97)
    n, G = 50000, 64
    flat = rng.choice(G ** 3, n, replace=False)
    coords = (np.stack([flat * 0, flat // G ** 2, flat // G % G, flat % G], 1) * np.array([1, 2, 2, 2])).astype(np.int32)
    cm = ME.CoordinateManager.rooted(dev(coords), 2)
    off = torch.from_numpy(offsets_np(ks, 1, 1).astype(np.int32)).cuda()
    got = be.coords_expand(cm.coords[2], off).cpu().numpy()
    want = expand_np(coords, ks, 2, 1, 2)
    assert got.shape == want.shape and np.array_equal(got, want)
    t_expand = _ms(lambda: be.coords_expand(cm.coords[2], off))
    feats = rng.standard_normal((n, 16)).astype(np.float32)
    xf = dev(feats).requires_grad_(True)
    conv = ME.MinkowskiGenerativeConvolutionTranspose(16, 16, kernel_size=ks, stride=2, dimension=3).cuda()
    x = ME.SparseTensor(xf, coordinate_manager=cm, tensor_stride=2)
    y = conv(x)
    assert y.tensor_stride == 1 and np.array_equal(y.C.cpu().numpy(), want)
    nbr = sorted_map(coords, want, -offsets_np(ks, 1, 1))
    ref = ref_conv(torch.from_numpy(feats).double(), conv.kernel.detach().double().cpu(), torch.from_numpy(nbr))
    check(f"generative k{ks} s2 16->16, {n} -> {len(want)} rows, forward", y._F, ref, RTOL)
    g = torch.randn(len(want), 16, device="cuda")
    t_fwd = _ms(lambda: conv(x))                           # (set and tables are cached: the convolution alone)

    def step():
        xf.grad = None
        conv.kernel.grad = None
        conv(x)._F.backward(g)
    t_step = _ms(step)
    print(f"generative k{ks} s2 16->16 at tensor stride 2: rows in {n}, rows out {len(want)}, coords_expand {t_expand:.3f} ms, "
          f"layer forward {t_fwd:.3f} ms, forward + backward {t_step:.3f} ms (backward {t_step - t_fwd:.3f} ms)")
