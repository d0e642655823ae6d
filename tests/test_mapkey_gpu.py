"""GPU: coordinate map keys, layers onto coordinates the caller names (`coordinates=`), expand_coordinates, and the validating
entry point ms3d_coords_check.

The yardstick for values is never this engine: a float64 gather-matmul-sum (sparse_ref.ref_conv on the CPU) over a table
built by Python dict lookup, dense float64 conv3d for the expanded convolution, numpy for sets and sums.  Bounds are the
project's: 1e-4 of the tensor's largest magnitude for convolutions at the default "highest" precision; max pooling forward
exact; sums of at most 27 floats (sum / average pooling, pooling backward) 1e-6 relative; the channel-wise convolution is
held to the convolutions' bound, as its own suite holds it; copies and permutations bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from generative_ref import expand_offsets_np, offsets_np
from sparse_ref import random_sparse, ref_conv

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = 1e-4
STOL = 1e-6


@pytest.fixture(scope="module")
def ME():
    import minsu3d_amd.MinkowskiEngine as me
    return me


@pytest.fixture(scope="module")
def be():
    from minsu3d_amd.backend import get_backend
    return get_backend()


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def check(name, got, want, tol):
    assert tuple(got.shape) == tuple(want.shape), (name, tuple(got.shape), tuple(want.shape))
    e = rel_err(got, want)
    print(f"{name}: rel err {e:.3e} (bound {tol:.0e})")
    assert e <= tol, (name, e)


def same(a, b):
    return a.shape == b.shape and torch.equal(a.detach().cpu(), b.detach().cpu())


# ---------------------------------------------------------------------------------------------- host restatements
def dict_map(in_coords, out_coords, offsets):
    """nbr [K, Vout] by Python dict lookup: nbr[k][o] = row of in_coords at out_coords[o] + offsets[k], or -1"""
    table = {}
    for r, c in enumerate(in_coords.tolist()):
        table.setdefault(tuple(c), r)
    out = np.full((len(offsets), len(out_coords)), -1, np.int32)
    oc = out_coords.tolist()
    for k, (dx, dy, dz) in enumerate(offsets.tolist()):
        for o, (b, x, y, z) in enumerate(oc):
            out[k, o] = table.get((b, x + dx, y + dy, z + dz), -1)
    return out


def invert_np(nbr, vin):
    inv = np.full((nbr.shape[0], vin), -1, np.int32)
    kk, oo = np.nonzero(nbr >= 0)
    inv[kk, nbr[kk, oo]] = oo
    return inv


def floor_set(coords, q):
    c = coords.copy()
    c[:, 1:] = np.floor_divide(c[:, 1:], q) * q
    _, first = np.unique(c, axis=0, return_index=True)
    return c[np.sort(first)]


def make_target(rng, natural, out_ts, n=200, grid=12):
    """n distinct rows on the out_ts lattice: half are rows of `natural` (the set the layer would land on: they hold input),
    a quarter are other lattice cells in and around the cloud (empty neighbours), a quarter lie 2048 voxels away (no kernel
    offset reaches them); shuffled"""
    half, quarter = n // 2, n // 4
    held = natural[rng.permutation(len(natural))[:half]]
    have = {tuple(r) for r in natural.tolist()}
    # every lattice cell of a box three cells wider than the cloud on each side that `natural` lacks (the box is wider than
    # any set a kernel of size 3 reaches from the cloud, so free cells always exist), a random quarter of them
    cells = range(-3 * out_ts, grid + 3 * out_ts, out_ts)
    free = np.array([(b, x, y, z) for b in range(2) for x in cells for y in cells for z in cells if (b, x, y, z) not in have],
                    np.int32).reshape(-1, 4)
    assert len(free) >= quarter
    near = free[rng.permutation(len(free))[:quarter]]
    far = natural[rng.permutation(len(natural))[:n - half - quarter]].copy()
    far[:, 1] += 2048
    t = np.concatenate([held, near, far]).astype(np.int32)
    t = t[rng.permutation(len(t))]
    assert len(np.unique(t, axis=0)) == len(t)
    return t, (t[:, 1] >= 1024)


def sparse_input(ME, rng, cin, ts=1, n=300, grad=True):
    """(SparseTensor at tensor stride ts, leaf features, held input coordinates as numpy)"""
    coords, _ = random_sparse(rng, B=2, grid=12, n=n, C=1)
    cm = ME.CoordinateManager(torch.from_numpy(coords).to(DEV))
    t = 1
    while t < ts:
        cm.k2(t)
        t *= 2
    cin_np = cm.coords[ts].cpu().numpy()
    xf = torch.from_numpy(rng.standard_normal((len(cin_np), cin)).astype(np.float32)).to(DEV).requires_grad_(grad)
    return ME.SparseTensor(xf, coordinate_manager=cm, tensor_stride=ts), xf, cin_np


def conv_oracle(x_np, W, bias, nbr):
    """float64 leaves and y = sum_k x[nbr[k]] W[k] + bias"""
    x64 = torch.from_numpy(x_np).double().requires_grad_(True)
    W64 = W.detach().double().cpu().reshape(nbr.shape[0], x_np.shape[1], -1).requires_grad_(True)
    b64 = None if bias is None else bias.detach().double().cpu().requires_grad_(True)
    y = ref_conv(x64, W64, torch.from_numpy(nbr))
    if b64 is not None:
        y = y + b64
    return y, x64, W64, b64


# ---------------------------------------------------------------------------------------------- 1. key round trip
@pytest.mark.parametrize("case", ["small", "morton", "stride2"])
def test_key_round_trip(ME, case, monkeypatch):
    from minsu3d_amd.MinkowskiEngine import tensor as T
    rng = np.random.default_rng(5)
    if case == "morton":
        monkeypatch.setattr(T, "_SORT_MIN_ROWS", 4096)
        coords, feats = random_sparse(rng, B=2, grid=24, n=5000, C=6)
    else:
        coords, feats = random_sparse(rng, B=2, grid=12, n=300, C=6)
    c = torch.from_numpy(coords).to(DEV)
    xf = torch.from_numpy(feats).to(DEV).requires_grad_(True)
    x = ME.SparseTensor(xf, coordinates=c)
    assert (x.coordinate_manager.perm is not None) == (case == "morton")
    ts = 1
    if case == "stride2":
        down = ME.MinkowskiConvolution(6, 6, kernel_size=2, stride=2, dimension=3).to(DEV)
        x = down(x)
        ts = 2
    assert x.tensor_stride == ts
    z = ME.SparseTensor(x.F * 2, coordinate_map_key=x.coordinate_map_key, coordinate_manager=x.coordinate_manager)
    assert z.coordinate_manager is x.coordinate_manager and z.tensor_stride == ts
    assert z.coordinate_map_key == x.coordinate_map_key
    assert same(z.C, x.C) and same(z.F, 2 * x.F)
    assert same(x.coordinate_manager.get_coordinates(x.coordinate_map_key), x.C)
    # a convolution of z against the same layer on a tensor built fresh from (2 x.F, x.C)
    conv = ME.MinkowskiConvolution(6, 7, kernel_size=3, bias=True, dimension=3).to(DEV)
    ff = (2 * x.F).detach().clone().requires_grad_(True)
    if ts == 1:
        fresh = ME.SparseTensor(ff, coordinates=x.C.clone())
        assert (fresh.coordinate_manager.perm is not None) == (case == "morton")
    else:
        fresh = ME.SparseTensor(ff, coordinate_manager=ME.CoordinateManager.rooted(x.C.clone(), ts), tensor_stride=ts)
    y, y2 = conv(z), conv(fresh)
    assert same(y.C, y2.C) and same(y.F, y2.F)
    # gradients: through the key constructor's gather, exactly
    g = torch.from_numpy(rng.standard_normal(tuple(y.F.shape)).astype(np.float32)).to(DEV)
    if ts == 1:
        (gx,) = torch.autograd.grad((y.F * g).sum(), xf, retain_graph=True)      # (x.F is one cached node, used again below)
        (gf,) = torch.autograd.grad((y2.F * g).sum(), ff)
        assert same(gx, 2 * gf)
        w = torch.from_numpy(rng.standard_normal(tuple(xf.shape)).astype(np.float32)).to(DEV)
        z1 = ME.SparseTensor(x.F * 2, coordinate_map_key=x.coordinate_map_key)
        (gx,) = torch.autograd.grad((z1.F * w).sum(), xf)
        assert same(gx, 2 * w)
    else:
        xl = x.F.detach().clone().requires_grad_(True)
        z1 = ME.SparseTensor(xl * 2, coordinate_map_key=x.coordinate_map_key)
        y1 = conv(z1)
        assert same(y1.F, y2.F)
        (gx,) = torch.autograd.grad((y1.F * g).sum(), xl)
        (gf,) = torch.autograd.grad((y2.F * g).sum(), ff)
        assert same(gx, 2 * gf)


# ---------------------------------------------------------------------------------------------- 2. convolution onto a tensor
CONV_GEOMS = [(3, 1, 1), (5, 1, 1), (3, 1, 2), (1, 1, 1), (3, 2, 1), (2, 2, 1), (4, 2, 1)]


def _conv_onto(ME, ks, stride, dil, cin, cout, target_fn, seed=3):
    rng = np.random.default_rng(seed + 100 * ks + 10 * stride + dil + cin)
    x, xf, cin_np = sparse_input(ME, rng, cin)
    out_ts = stride
    natural = cin_np if stride == 1 else floor_set(cin_np, 2)
    tgt, far = target_fn(rng, natural, out_ts)
    conv = ME.MinkowskiConvolution(cin, cout, kernel_size=ks, stride=stride, dilation=dil, bias=True, dimension=3).to(DEV)
    conv.train()
    T = torch.from_numpy(tgt).long()          # any integer dtype, any device: a CPU int64 tensor
    y = conv(x, coordinates=T)
    assert y.tensor_stride == out_ts and y.coordinate_manager is not x.coordinate_manager
    assert y.C.dtype == torch.int32 and np.array_equal(y.C.cpu().numpy(), tgt)
    want_nbr = dict_map(cin_np, tgt, offsets_np(ks, dil, 1))
    table = x.coordinate_manager.target_map(1, y.coordinate_map_key, ks, stride, dil)
    if len(tgt):
        assert np.array_equal(table[0].cpu().numpy(), want_nbr)
        assert np.array_equal(table[1].cpu().numpy(), invert_np(want_nbr, len(cin_np)))
    assert table[2:] == (len(cin_np), len(tgt), ks ** 3)
    want, x64, W64, b64 = conv_oracle(xf.detach().cpu().numpy(), conv.kernel, conv.bias, want_nbr)
    tag = f"k{ks} s{stride} d{dil} {cin}->{cout} onto {len(tgt)} rows"
    assert tuple(y.F.shape) == (len(tgt), cout)
    if len(tgt):
        check(tag + " forward", y.F, want, RTOL)
        if far.any():
            assert (want_nbr[:, far] == -1).all()
            assert same(y.F[torch.from_numpy(far).to(DEV)], conv.bias.detach().expand(int(far.sum()), cout))
    g = rng.standard_normal((len(tgt), cout)).astype(np.float32)
    y.F.backward(torch.from_numpy(g).to(DEV))
    want.backward(torch.from_numpy(g).double())
    if len(tgt) and not far.all():
        check(tag + " backward-data", xf.grad, x64.grad, RTOL)
        check(tag + " backward-weight", conv.kernel.grad, W64.grad.view_as(conv.kernel), RTOL)
        check(tag + " bias gradient", conv.bias.grad, b64.grad, RTOL)
    else:          # nothing reaches a row: exact zeros (and the column sum of g for the bias)
        assert xf.grad is None or not xf.grad.any()
        assert not conv.kernel.grad.any()
        if len(tgt):
            check(tag + " bias gradient", conv.bias.grad, b64.grad, STOL)
        else:
            assert not conv.bias.grad.any()


@pytest.mark.parametrize("cin,cout", [(5, 7), (16, 32)])
@pytest.mark.parametrize("ks,stride,dil", CONV_GEOMS)
def test_conv_onto_tensor_target(ME, ks, stride, dil, cin, cout):
    _conv_onto(ME, ks, stride, dil, cin, cout, make_target)


@pytest.mark.parametrize("ks,stride", [(3, 1), (2, 2)])
def test_conv_onto_empty_target(ME, ks, stride):
    _conv_onto(ME, ks, stride, 1, 5, 7, lambda rng, nat, ts: (np.zeros((0, 4), np.int32), np.zeros(0, bool)))


@pytest.mark.parametrize("ks,stride", [(3, 1), (3, 2)])
def test_conv_onto_unreached_target(ME, ks, stride):
    def far_only(rng, nat, ts):
        t = nat[:64].copy()
        t[:, 2] -= 4096
        return t.astype(np.int32), np.ones(len(t), bool)
    _conv_onto(ME, ks, stride, 1, 16, 32, far_only)


# ---------------------------------------------------------------------------------------------- 3. the three target forms
def test_target_forms_agree_and_share_managers(ME):
    rng = np.random.default_rng(17)
    x, xf, cin_np = sparse_input(ME, rng, 16, grad=False)
    tgt, _ = make_target(rng, cin_np, 1)
    T = torch.from_numpy(tgt).to(DEV)
    t = ME.SparseTensor(torch.from_numpy(rng.standard_normal((len(tgt), 32)).astype(np.float32)).to(DEV), coordinates=T.clone())
    conv = ME.MinkowskiConvolution(16, 32, kernel_size=3, bias=True, dimension=3).to(DEV)
    pool = ME.MinkowskiSumPooling(3, dimension=3)
    a, b, c = conv(x, coordinates=T), conv(x, coordinates=t.coordinate_map_key), conv(x, coordinates=t)
    assert same(a.F, b.F) and same(b.F, c.F) and same(a.C, b.C) and same(b.C, t.C)
    # a key target lives on the key's manager: arithmetic and cat with tensors of that set need no union
    assert b.coordinate_manager is t.coordinate_manager and c.coordinate_manager is t.coordinate_manager
    s = b + t
    assert s.coordinate_manager is t.coordinate_manager and same(s.F, b.F + t.F)
    assert ME.cat(b, t).coordinate_manager is t.coordinate_manager and tuple(ME.cat(b, t).F.shape) == (len(tgt), 64)
    # the same tensor object twice, by two layers: ONE rooted manager; an in-place edit: a new one
    a2, p = conv(x, coordinates=T), pool(x, T)
    assert a2.coordinate_manager is a.coordinate_manager and p.coordinate_manager is a.coordinate_manager
    assert same(a2.F, a.F)
    first = T[0].clone()
    T[0, 1] += 4096
    a3 = conv(x, coordinates=T)
    assert a3.coordinate_manager is not a.coordinate_manager and same(a3.C, T) and same(a.C[0], first)
    assert same(a3.F[1:], a.F[1:]) and same(a3.F[0], conv.bias.detach()[0])


@pytest.mark.parametrize("ks,stride", [(3, 1), (5, 1), (2, 2), (3, 2)])
def test_natural_target_takes_the_ordinary_path(ME, ks, stride):
    rng = np.random.default_rng(19)
    x, xf, _ = sparse_input(ME, rng, 16, grad=False)
    conv = ME.MinkowskiConvolution(16, 32, kernel_size=ks, stride=stride, bias=True, dimension=3).to(DEV)
    plain = conv(x)
    onto = conv(x, coordinates=plain.coordinate_map_key)
    assert onto.coordinate_manager is x.coordinate_manager and onto.tensor_stride == stride
    assert same(onto.F, plain.F) and same(conv(x, coordinates=plain).F, plain.F)
    assert "_target_maps" not in x.coordinate_manager.__dict__          # no table of its own was built
    for layer in (ME.MinkowskiMaxPooling(ks, stride=stride, dimension=3),
                  ME.MinkowskiChannelwiseConvolution(16, kernel_size=ks, stride=stride, dimension=3).to(DEV)):
        assert same(layer(x, plain.coordinate_map_key).F, layer(x).F)
    if stride == 2:          # ... and back: the cached finer set of a transposed layer
        up = ME.MinkowskiConvolutionTranspose(32, 16, kernel_size=ks, stride=2, dimension=3).to(DEV)
        back = up(plain, x.coordinate_map_key)
        assert back.coordinate_manager is x.coordinate_manager and same(back.F, up(plain).F) and same(up(plain, x).F, back.F)
        pt = ME.MinkowskiPoolingTranspose(ks, 2, dimension=3)
        assert same(pt(plain, x).F, pt(plain).F)
        assert "_target_maps" not in x.coordinate_manager.__dict__


# ---------------------------------------------------------------------------------------------- 4. Morton-sorted target
def test_morton_sorted_key_target(ME, monkeypatch):
    from minsu3d_amd.MinkowskiEngine import tensor as T
    monkeypatch.setattr(T, "_SORT_MIN_ROWS", 4096)
    rng = np.random.default_rng(23)
    big, bf = random_sparse(rng, B=2, grid=24, n=5000, C=7)
    t = ME.SparseTensor(torch.from_numpy(bf).to(DEV), coordinates=torch.from_numpy(big).to(DEV))
    assert t.coordinate_manager.perm is not None
    x, xf, cin_np = sparse_input(ME, rng, 5)
    assert x.coordinate_manager.perm is None
    conv = ME.MinkowskiConvolution(5, 7, kernel_size=3, bias=True, dimension=3).to(DEV)
    y = conv(x, coordinates=t.coordinate_map_key)
    assert y.coordinate_manager is t.coordinate_manager and same(y.C, t.C) and np.array_equal(y.C.cpu().numpy(), big)
    want_nbr = dict_map(cin_np, big, offsets_np(3, 1, 1))          # rows as the CALLER sees them
    want, x64, W64, b64 = conv_oracle(xf.detach().cpu().numpy(), conv.kernel, conv.bias, want_nbr)
    check("Morton target forward", y.F, want, RTOL)
    s = y + t          # same set: row by row, in the caller's order
    assert s.coordinate_manager is t.coordinate_manager and same(s.F, y.F + t.F)
    g = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y.F.backward(torch.from_numpy(g).to(DEV))
    want.backward(torch.from_numpy(g).double())
    check("Morton target backward-data", xf.grad, x64.grad, RTOL)
    check("Morton target backward-weight", conv.kernel.grad, W64.grad, RTOL)


# ---------------------------------------------------------------------------------------------- 5. transposed convolution
@pytest.mark.parametrize("ks,stride", [(2, 2), (3, 2), (4, 2), (3, 1)])
def test_transposed_conv_onto_uncached_set(ME, ks, stride):
    rng = np.random.default_rng(29 + ks + stride)
    ts = 2
    x, xf, cin_np = sparse_input(ME, rng, 16, ts=ts)          # the stride-2 set a strided layer lands on
    out_ts = ts // stride
    reach = expand_offsets_np(cin_np, offsets_np(ks, 1, out_ts))
    tgt, far = make_target(rng, reach, out_ts)
    up = ME.MinkowskiConvolutionTranspose(16, 32, kernel_size=ks, stride=stride, bias=True, dimension=3).to(DEV)
    y = up(x, torch.from_numpy(tgt).to(DEV))          # second positional, as MinkowskiEngine takes it
    assert y.tensor_stride == out_ts and np.array_equal(y.C.cpu().numpy(), tgt)
    want_nbr = dict_map(cin_np, tgt, -offsets_np(ks, 1, out_ts))          # y[o] = sum_k x[o - off_k] W[k]
    table = x.coordinate_manager.target_map(ts, y.coordinate_map_key, ks, stride, 1, transposed=True)
    assert np.array_equal(table[0].cpu().numpy(), want_nbr)
    assert np.array_equal(table[1].cpu().numpy(), invert_np(want_nbr, len(cin_np)))
    want, x64, W64, b64 = conv_oracle(xf.detach().cpu().numpy(), up.kernel, up.bias, want_nbr)
    tag = f"transposed k{ks} s{stride}"
    check(tag + " forward", y.F, want, RTOL)
    assert same(y.F[torch.from_numpy(far).to(DEV)], up.bias.detach().expand(int(far.sum()), 32))
    g = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y.F.backward(torch.from_numpy(g).to(DEV))
    want.backward(torch.from_numpy(g).double())
    check(tag + " backward-data", xf.grad, x64.grad, RTOL)
    check(tag + " backward-weight", up.kernel.grad, W64.grad, RTOL)
    check(tag + " bias gradient", up.bias.grad, b64.grad, RTOL)


# ---------------------------------------------------------------------------------------------- 6. pooling, channel-wise
def pool_oracle(x_np, nbr, mode):
    x64 = torch.from_numpy(x_np).double().requires_grad_(True)
    idx = torch.from_numpy(nbr).long()
    present = (idx >= 0)
    rows = torch.cat([x64, x64.new_zeros(1, x64.size(1))])[torch.where(present, idx, torch.full_like(idx, x64.size(0)))]
    if mode == "max":
        y = torch.where(present[..., None], rows, rows.new_full((), -float("inf"))).max(0).values
        y = torch.where(present.any(0)[:, None], y, torch.zeros_like(y))
    else:
        y = rows.sum(0)
        if mode == "avg":
            y = y / present.sum(0).clamp_min(1)[:, None]
    return y, x64


@pytest.mark.parametrize("C_", [5, 16])
@pytest.mark.parametrize("ks,stride", [(3, 1), (2, 2), (3, 2)])
@pytest.mark.parametrize("mode", ["max", "avg", "sum"])
def test_pooling_onto_target(ME, mode, ks, stride, C_):
    rng = np.random.default_rng(31 + ks + stride + C_)
    x, xf, cin_np = sparse_input(ME, rng, C_)
    natural = cin_np if stride == 1 else floor_set(cin_np, 2)
    tgt, far = make_target(rng, natural, stride)
    layer = {"max": ME.MinkowskiMaxPooling, "avg": ME.MinkowskiAvgPooling, "sum": ME.MinkowskiSumPooling}[mode](
        ks, stride=stride, dimension=3)
    y = layer(x, torch.from_numpy(tgt).to(DEV))
    assert y.tensor_stride == stride and np.array_equal(y.C.cpu().numpy(), tgt)
    want_nbr = dict_map(cin_np, tgt, offsets_np(ks, 1, 1))
    want, x64 = pool_oracle(xf.detach().cpu().numpy(), want_nbr, mode)
    if mode == "max":
        assert same(y.F, want.float())
    else:
        check(f"{mode} pooling onto target forward", y.F, want, STOL)
    assert not y.F[torch.from_numpy(far).to(DEV)].any()
    g = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y.F.backward(torch.from_numpy(g).to(DEV))
    want.backward(torch.from_numpy(g).double())
    check(f"{mode} pooling onto target backward", xf.grad, x64.grad, STOL)


@pytest.mark.parametrize("ks,stride", [(2, 2), (3, 2), (3, 1)])
def test_pooling_transpose_onto_target(ME, ks, stride):
    rng = np.random.default_rng(37 + ks + stride)
    ts = 2
    x, xf, cin_np = sparse_input(ME, rng, 5, ts=ts)
    out_ts = ts // stride
    tgt, far = make_target(rng, expand_offsets_np(cin_np, offsets_np(ks, 1, out_ts)), out_ts)
    y = ME.MinkowskiPoolingTranspose(ks, stride, dimension=3)(x, coordinates=torch.from_numpy(tgt).to(DEV))
    assert y.tensor_stride == out_ts and np.array_equal(y.C.cpu().numpy(), tgt)
    want_nbr = dict_map(cin_np, tgt, -offsets_np(ks, 1, out_ts))
    want, x64 = pool_oracle(xf.detach().cpu().numpy(), want_nbr, "sum")
    check("pooling transpose onto target forward", y.F, want, STOL)
    assert not y.F[torch.from_numpy(far).to(DEV)].any()
    g = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y.F.backward(torch.from_numpy(g).to(DEV))
    want.backward(torch.from_numpy(g).double())
    check("pooling transpose onto target backward", xf.grad, x64.grad, STOL)


@pytest.mark.parametrize("C_", [5, 16])
@pytest.mark.parametrize("ks,stride", [(3, 1), (3, 2)])
def test_channelwise_onto_target(ME, ks, stride, C_):
    rng = np.random.default_rng(41 + ks + stride + C_)
    x, xf, cin_np = sparse_input(ME, rng, C_)
    natural = cin_np if stride == 1 else floor_set(cin_np, 2)
    tgt, far = make_target(rng, natural, stride)
    layer = ME.MinkowskiChannelwiseConvolution(C_, kernel_size=ks, stride=stride, bias=True, dimension=3).to(DEV)
    y = layer(x, torch.from_numpy(tgt).to(DEV))
    assert y.tensor_stride == stride and np.array_equal(y.C.cpu().numpy(), tgt)
    nbr = torch.from_numpy(dict_map(cin_np, tgt, offsets_np(ks, 1, 1))).long()
    x64 = xf.detach().double().cpu().requires_grad_(True)
    w64 = layer.kernel.detach().double().cpu().requires_grad_(True)
    b64 = layer.bias.detach().double().cpu().requires_grad_(True)
    rows = torch.cat([x64, x64.new_zeros(1, C_)])[torch.where(nbr >= 0, nbr, torch.full_like(nbr, x64.size(0)))]
    want = (rows * w64[:, None, :]).sum(0) + b64
    # (a convolution: the convolutions' bound, as tests/test_channelwise_gpu.py holds this layer to)
    check("channel-wise onto target forward", y.F, want, RTOL)
    assert same(y.F[torch.from_numpy(far).to(DEV)], layer.bias.detach().expand(int(far.sum()), C_))
    g = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y.F.backward(torch.from_numpy(g).to(DEV))
    want.backward(torch.from_numpy(g).double())
    check("channel-wise onto target backward-data", xf.grad, x64.grad, RTOL)
    check("channel-wise onto target backward-weight", layer.kernel.grad, w64.grad, RTOL)
    check("channel-wise onto target bias gradient", layer.bias.grad, b64.grad, RTOL)


# ---------------------------------------------------------------------------------------------- 7. ms3d_coords_check
def _flags(be, rows, lattice=1):
    return be.coords_check(torch.tensor(rows, dtype=torch.int32).reshape(-1, 4).to(DEV), lattice)


def test_coords_check_flags(be):
    rng = np.random.default_rng(43)
    base, _ = random_sparse(rng, B=2, grid=12, n=700, C=1)          # three blocks of 256 threads
    base = base.astype(np.int64)
    assert _flags(be, base) == 0
    assert be.coords_check(torch.empty((0, 4), dtype=torch.int32, device=DEV), 1) == 0          # V = 0
    assert be.coords_check(torch.empty((0, 4), dtype=torch.int32, device=DEV), 4) == 0
    # the boundary values are accepted ...
    edge = np.array([[524287, -16384, 16383, 0], [0, 16383, -16384, -16384], [1, 0, 0, 16383]], np.int64)
    assert _flags(be, np.concatenate([base, edge])) == 0
    # ... one past them raises bit 0, and only bit 0
    for bad in ([0, 16384, 0, 1], [0, 1, -16385, 0], [1, 0, 1, 16384], [524288, 0, 0, 1], [-1, 0, 0, 1]):
        assert _flags(be, np.concatenate([base, [bad]])) == 1, bad
        assert _flags(be, [bad]) == 1, bad
    # bit 1: off the lattice, negative coordinates included (floor arithmetic: -4 is on the lattice of 4, -3 is not)
    for lattice in (1, 2, 4):
        on = base.copy()
        on[:, 1:] = (on[:, 1:] - 6) * lattice
        assert _flags(be, on, lattice) == 0, lattice
        if lattice > 1:
            for axis in (1, 2, 3):
                off = on.copy()
                off[-1, axis] = -lattice - 1
                assert _flags(be, off, lattice) == 2, (lattice, axis)
            off = on.copy()
            off[0, 3] += 1
            assert _flags(be, off, lattice) == 2, lattice
            assert _flags(be, on, 2 * lattice) == 2          # odd multiples exist among 700 rows
    odd_batch = base.copy()
    odd_batch[:, 1:] *= 2
    assert _flags(be, odd_batch, 2) == 0          # the batch index is not on any lattice
    # bit 2: a repeat -- in the last two rows, and far apart
    assert _flags(be, np.concatenate([base, base[-1:]])) == 4
    assert _flags(be, np.concatenate([base[:1], base])) == 4
    assert _flags(be, [[0, 1, 2, 3], [0, 1, 2, 3]]) == 4
    assert _flags(be, [[0, -1, -2, -3], [1, -1, -2, -3]]) == 0          # another batch index is another coordinate
    # all together
    every = np.concatenate([base * np.array([1, 2, 2, 2]), [[0, 16384, 0, 0]], [[0, 3, 0, 0]], [[1, 8, 8, 8]], [[1, 8, 8, 8]]])
    assert _flags(be, every, 2) == 7
    assert _flags(be, np.concatenate([base, [[0, 16384, 0, 1]], base[:1]])) == 5
    assert _flags(be, [[0, 1, 0, 0], [0, 1, 0, 0]], 2) == 6


def test_layers_name_the_reason(ME):
    rng = np.random.default_rng(47)
    x, _, cin_np = sparse_input(ME, rng, 5, grad=False)
    conv = ME.MinkowskiConvolution(5, 7, kernel_size=3, dimension=3).to(DEV)
    down = ME.MinkowskiConvolution(5, 7, kernel_size=2, stride=2, dimension=3).to(DEV)
    pool = ME.MinkowskiMaxPooling(2, stride=2, dimension=3)
    good = torch.from_numpy(cin_np[:50]).to(DEV)
    with pytest.raises(ValueError, match="occurs twice"):
        conv(x, coordinates=torch.cat([good, good[-1:]]))
    outside = good.clone()
    outside[3, 2] = 16384
    with pytest.raises(ValueError, match="outside the packable range"):
        conv(x, coordinates=outside)
    odd = good.clone() * 2
    odd[7, 3] += 1
    for layer in (down, pool):
        with pytest.raises(ValueError, match="not a multiple of the output tensor stride 2"):
            layer(x, coordinates=odd)
    up = ME.MinkowskiConvolutionTranspose(7, 5, kernel_size=2, stride=2, dimension=3).to(DEV)
    x4 = ME.SparseTensor(torch.zeros((50, 7), device=DEV), coordinate_manager=ME.CoordinateManager.rooted(good * 4, 4),
                         tensor_stride=4)
    with pytest.raises(ValueError, match="not a multiple of the output tensor stride 2"):
        up(x4, odd)
    # nothing was cached for a refused tensor: mended in place it is checked again and accepted
    odd[7, 3] -= 1
    assert tuple(down(x, coordinates=odd).F.shape) == (50, 7)
    # a key target is not checked, only its stride must be the layer's output stride
    with pytest.raises(ValueError, match="tensor stride 4, the layer's output tensor stride is 2"):
        down(x, coordinates=x4)


# ---------------------------------------------------------------------------------------------- 8. expand_coordinates
@pytest.mark.parametrize("ks", [3, 5])
def test_expand_convolution(ME, ks):
    rng = np.random.default_rng(53 + ks)
    B, G, cin, cout = 2, 12, 5, 7
    x, xf, cin_np = sparse_input(ME, rng, cin)
    conv = ME.MinkowskiConvolution(cin, cout, kernel_size=ks, bias=True, dimension=3, expand_coordinates=True).to(DEV)
    y = conv(x)
    want_set = expand_offsets_np(cin_np, -offsets_np(ks, 1, 1))          # first occurrence, input row major, offset minor
    assert y.tensor_stride == 1 and y.coordinate_manager is not x.coordinate_manager
    assert np.array_equal(y.C.cpu().numpy(), want_set)
    assert conv(x).coordinate_manager is y.coordinate_manager          # cached per (ts, geometry)
    # dense float64 conv3d on a grid padded by the reach of the kernel on every side, read at the expanded set
    r = ks // 2
    x64 = xf.detach().double().cpu().requires_grad_(True)
    W64 = conv.kernel.detach().double().cpu().requires_grad_(True)
    b64 = conv.bias.detach().double().cpu().requires_grad_(True)
    ci = torch.from_numpy(cin_np).long()
    d = torch.zeros((B, G + 2 * r, G + 2 * r, G + 2 * r, cin), dtype=torch.float64)
    d = d.index_put((ci[:, 0], ci[:, 1] + r, ci[:, 2] + r, ci[:, 3] + r), x64).permute(0, 4, 1, 2, 3)
    Wd = W64.view(ks, ks, ks, cin, cout).permute(4, 3, 2, 1, 0)          # k = ix + ks iy + ks^2 iz -> [Cout, Cin, x, y, z]
    dense = F.conv3d(d, Wd, b64.view(-1), padding=r)
    co = torch.from_numpy(want_set).long()
    want = dense[co[:, 0], :, co[:, 1] + r, co[:, 2] + r, co[:, 3] + r]
    check(f"expand k{ks} forward", y.F, want, RTOL)
    g = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y.F.backward(torch.from_numpy(g).to(DEV))
    want.backward(torch.from_numpy(g).double())
    check(f"expand k{ks} backward-data", xf.grad, x64.grad, RTOL)
    check(f"expand k{ks} backward-weight", conv.kernel.grad, W64.grad, RTOL)
    check(f"expand k{ks} bias gradient", conv.bias.grad, b64.grad.view(1, -1), RTOL)


@pytest.mark.parametrize("ks,stride", [(3, 1), (2, 2)])
def test_expand_transposed_convolution_is_the_generative_layer(ME, ks, stride):
    rng = np.random.default_rng(59 + ks)
    x, xf, _ = sparse_input(ME, rng, 16, ts=2)
    gen = ME.MinkowskiGenerativeConvolutionTranspose(16, 32, kernel_size=ks, stride=stride, bias=True, dimension=3).to(DEV)
    exp = ME.MinkowskiConvolutionTranspose(16, 32, kernel_size=ks, stride=stride, bias=True, dimension=3,
                                           expand_coordinates=True).to(DEV)
    exp.load_state_dict(gen.state_dict())
    a, b = gen(x), exp(x)
    assert b.coordinate_manager is a.coordinate_manager and b.tensor_stride == a.tensor_stride == 2 // stride
    assert same(a.F, b.F) and same(a.C, b.C)
    g = torch.from_numpy(rng.standard_normal(tuple(a.F.shape)).astype(np.float32)).to(DEV)
    ga = torch.autograd.grad((a.F * g).sum(), [xf, gen.kernel, gen.bias])
    gb = torch.autograd.grad((b.F * g).sum(), [xf, exp.kernel, exp.bias])
    for u, v in zip(ga, gb):
        assert same(u, v)


@pytest.mark.parametrize("ks,stride", [(3, 1), (2, 2), (3, 2)])
def test_expand_pooling_transpose(ME, ks, stride):
    rng = np.random.default_rng(61 + ks + stride)
    ts = 2
    x, xf, cin_np = sparse_input(ME, rng, 5, ts=ts)
    out_ts = ts // stride
    y = ME.MinkowskiPoolingTranspose(ks, stride, dimension=3, expand_coordinates=True)(x)
    off = offsets_np(ks, 1, out_ts)
    want_set = expand_offsets_np(cin_np, off)
    assert y.tensor_stride == out_ts and np.array_equal(y.C.cpu().numpy(), want_set)
    # numpy: every input row adds itself to the K cells it reaches
    xs = xf.detach().cpu().numpy().astype(np.float64)
    row_of = {tuple(c): i for i, c in enumerate(want_set.tolist())}
    want = np.zeros((len(want_set), 5))
    g = rng.standard_normal(want.shape).astype(np.float32)
    want_dx = np.zeros_like(xs)
    for i, c in enumerate(cin_np.tolist()):
        for o in off.tolist():
            r = row_of[(c[0], c[1] + o[0], c[2] + o[1], c[3] + o[2])]
            want[r] += xs[i]
            want_dx[i] += g[r]
    check("expanding pooling transpose forward", y.F, torch.from_numpy(want), STOL)
    y.F.backward(torch.from_numpy(g).to(DEV))
    check("expanding pooling transpose backward", xf.grad, torch.from_numpy(want_dx), STOL)


# ---------------------------------------------------------------------------------------------- 9. the weight-image window
def test_target_convolution_inside_a_prepare_window(ME):
    """a k3 s1 convolution called onto a target must not pick up the MIRRORED backward-data image (or the deferred-reduction
    stamp) that prepare_conv_weights lays out for its static geometry: output, dx and both dW inside a window, in training
    mode, are the bytes of the same call outside it"""
    rng = np.random.default_rng(67)
    x0, _, cin_np = sparse_input(ME, rng, 16, grad=False)
    tgt, _ = make_target(rng, cin_np, 1)
    T = torch.from_numpy(tgt).to(DEV)
    feats = x0.F.detach()

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.onto = ME.MinkowskiConvolution(16, 16, kernel_size=3, dimension=3)
            self.same = ME.MinkowskiConvolution(16, 32, kernel_size=3, dimension=3)

        def forward(self, x):
            return self.same(self.onto(x, coordinates=T))

    net = Net().to(DEV).train()
    g = torch.from_numpy(rng.standard_normal((len(tgt), 32)).astype(np.float32)).to(DEV)

    def step(window):
        net.zero_grad(set_to_none=True)
        xf = feats.clone().requires_grad_(True)
        x = ME.SparseTensor(xf, coordinate_manager=x0.coordinate_manager)
        if window:
            ME.prepare_conv_weights(net)
            try:
                y = net(x)
            finally:
                ME.release_conv_weights()
        else:
            y = net(x)
        (y.F * g).sum().backward()
        return [t.detach().clone() for t in (y.F, xf.grad, net.onto.kernel.grad, net.same.kernel.grad)]

    outside, inside = step(False), step(True)
    for name, a, b in zip(("output", "dx", "dW onto", "dW same"), outside, inside):
        assert same(a, b), name
    # and the values are right (a mirrored image would show in dx alone)
    nbr1 = dict_map(cin_np, tgt, offsets_np(3, 1, 1))
    nbr2 = dict_map(tgt, tgt, offsets_np(3, 1, 1))
    x64 = feats.double().cpu().requires_grad_(True)
    y1 = ref_conv(x64, net.onto.kernel.detach().double().cpu(), torch.from_numpy(nbr1))
    y2 = ref_conv(y1, net.same.kernel.detach().double().cpu(), torch.from_numpy(nbr2))
    y2.backward(g.double().cpu())
    check("window output", inside[0], y2, RTOL)
    check("window dx", inside[1], x64.grad, RTOL)
