"""GPU: kernel regions (RegionType / KernelGenerator) -- the tables of ms3d_kmap_region and of the strided / target / generated
routes, and every layer that takes `kernel_generator=` on them.

Yardsticks (tests/region_ref.py): tables against a Python dictionary map and its numpy inverse, exactly, and against
backend.kmap_general / kmap_invert over the same list; convolution values against float64 dense torch (F.conv3d /
F.conv_transpose3d) of the region kernel EMBEDDED in the cube (2r + 1)^3 it fits in, zeros elsewhere, on the sparse input
scattered into a grid [B, C, x, y, z]; channel-wise convolution and pooling against a float64 gather over the dictionary map.
Bounds are the ones the cube geometries are held to: convolutions and the channel-wise layer 1e-4 of the tensor's largest
magnitude (tests/test_geometry_gpu.py, tests/test_channelwise_gpu.py; dgamma / dbeta of a pending BatchNorm 1e-3, for the
reason given there), max pooling forward exact, sums of a few floats (average / sum pooling, pooling backward, pooling
transpose) 1e-6 relative.  A HYPER_CUBE generator and the weight-image window are compared byte for byte.

R1 cross 3 (K = 7); R2 cross 5 dilation 2 (K = 13); R3 the axis kernel (-1, 0, +1 in x); R4 a centre, one partnered pair and
two unpartnered offsets; R5 one shift; R6 the 27 cube offsets shifted by +1 in x; R7 the 8 offsets of the k2 cell, at stride 1."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from region_ref import cross_offsets, cube_offsets, custom_offsets, dict_map, invert_np, expand_np, reach, embed
from sparse_ref import random_sparse, ref_conv

pytestmark = pytest.mark.gpu
RTOL = 1e-4
STOL = 1e-6
DEV = "cuda"

R3 = [(-1, 0, 0), (0, 0, 0), (1, 0, 0)]
R4 = [(0, 0, 0), (1, 0, 0), (0, 2, -1), (-1, 0, 0), (3, 3, 3)]
R5 = [(1, 0, 0)]
R6 = (cube_offsets(3, 1, 1) + np.array([1, 0, 0])).tolist()
R7 = cube_offsets(2, 1, 1).tolist()
CUSTOM = {"R3": R3, "R4": R4, "R5": R5, "R6": R6, "R7": R7}
NAMES = ("R1", "R2", "R3", "R4", "R5", "R6", "R7")


@pytest.fixture(scope="module")
def ME():
    import minsu3d_amd.MinkowskiEngine as me
    return me


@pytest.fixture(scope="module")
def be():
    from minsu3d_amd.backend import get_backend
    return get_backend()


def gen(ME, name, stride=1, **kw):
    if name == "R1":
        return ME.KernelGenerator(3, stride, region_type=ME.RegionType.HYPER_CROSS, dimension=3, **kw)
    if name == "R2":
        return ME.KernelGenerator(5, stride, 2, region_type=ME.RegionType.HYPER_CROSS, dimension=3, **kw)
    return ME.KernelGenerator(stride=stride, region_type=ME.RegionType.CUSTOM,
                              region_offsets=torch.tensor(CUSTOM[name], dtype=torch.int32), dimension=3, **kw)


def unit_offsets(name):
    """the region's offsets in units of the tensor stride, restated"""
    if name == "R1":
        return cross_offsets(3, 1, 1)
    if name == "R2":
        return cross_offsets(5, 2, 1)
    return custom_offsets(CUSTOM[name], 1)


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


def manager_at(ME, coords, ts):
    cm = ME.CoordinateManager(torch.from_numpy(np.ascontiguousarray(coords)).to(DEV))
    t = 1
    while t < ts:
        cm.k2(t)
        t *= 2
    return cm


def densify64(coords, feats, B, G, unit):
    d = torch.zeros((B, feats.shape[1], G, G, G), dtype=torch.float64)
    c = torch.as_tensor(coords).long()
    d[c[:, 0], :, c[:, 1] // unit, c[:, 2] // unit, c[:, 3] // unit] = feats
    return d


def read_dense(d, coords, unit, shift=0):
    c = torch.as_tensor(coords).long()
    return d[c[:, 0], :, c[:, 1] // unit + shift, c[:, 2] // unit + shift, c[:, 3] // unit + shift]


def extreme_cloud(c):
    """part of the cloud pushed against +16383, part against -16384, in ONE coordinate set, lined up so that `high + 1`
    wrapped around lands exactly on rows of the low part: a shifted coordinate that leaves the packable range must give -1,
    a wrapped key would find a row"""
    hi = c.copy()
    hi[:, 1:] += 16383 - c[:, 1:].max(0)
    lo = c.copy()
    lo[:, 1:] += -16384 - c[:, 1:].min(0)
    wrapped = hi.copy()
    wrapped[:, 1:] -= 32767
    wrapped = wrapped[(wrapped[:, 1:] >= -16384).all(1)]
    return np.unique(np.concatenate([hi, lo, wrapped]), axis=0).astype(np.int32)


# ---------------------------------------------------------------------------------------------- 1. tables
@pytest.mark.parametrize("shift", ["none", "negative", "extreme"])
@pytest.mark.parametrize("ts", [1, 2])
def test_region_tables_exact(ME, be, ts, shift):
    rng = np.random.default_rng(7)
    c, _ = random_sparse(rng, B=2, grid=12, n=400, C=1)
    if shift == "negative":
        c = c.copy()
        c[:, 1:] -= 9
    elif shift == "extreme":
        c = extreme_cloud(c)
        rng.shuffle(c)
    cm, again = manager_at(ME, c, ts), manager_at(ME, c, ts)
    held = cm.coords[ts]
    cin = held.cpu().numpy()
    V = cin.shape[0]
    for name in NAMES:
        g = gen(ME, name)
        offs = unit_offsets(name) * ts
        K = offs.shape[0]
        assert np.array_equal(g.offsets(ts), offs) and g.kernel_volume == K
        nbr_fwd, nbr_bwd, vin, vout, k, out_ts, mirror = cm.kernel_map(ts, g.kernel_size, 1, g.dilation, region=g)
        assert (vin, vout, k, out_ts, mirror) == (V, V, K, ts, False) and nbr_bwd is not nbr_fwd
        assert tuple(nbr_fwd.shape) == (K, V) and tuple(nbr_bwd.shape) == (K, V)
        want = dict_map(cin, cin, offs)
        inv = invert_np(want, V)
        assert np.array_equal(nbr_fwd.cpu().numpy(), want), name
        assert np.array_equal(nbr_bwd.cpu().numpy(), inv), name
        general = be.kmap_general(held, held, torch.from_numpy(offs.astype(np.int32)))
        assert torch.equal(nbr_fwd, general) and torch.equal(nbr_bwd, be.kmap_invert(general, K, V, V)), name
        assert cm.kernel_map(ts, g.kernel_size, 1, g.dilation, region=gen(ME, name))[0] is nbr_fwd           # cached, by value
        assert cm.kernel_map_inverse(ts, g.kernel_size, 1, g.dilation, region=g) is nbr_bwd
        twice = again.kernel_map(ts, g.kernel_size, 1, g.dilation, region=g)                 # the same bytes on every run
        assert torch.equal(twice[0], nbr_fwd) and torch.equal(twice[1], nbr_bwd), name
    cout = cm.coords[2 * ts].cpu().numpy() if 2 * ts in cm.coords else None
    for name in ("R1", "R3", "R4"):
        g = gen(ME, name, stride=2)
        offs = unit_offsets(name) * ts
        nbr_fwd, nbr_bwd, vin, vout, k, out_ts, mirror = cm.kernel_map(ts, g.kernel_size, 2, g.dilation, region=g)
        cout = cm.coords[2 * ts].cpu().numpy()
        assert (vin, vout, k, out_ts, mirror) == (V, cout.shape[0], offs.shape[0], 2 * ts, False)
        want = dict_map(cin, cout, offs)
        assert np.array_equal(nbr_fwd.cpu().numpy(), want), name
        assert np.array_equal(nbr_bwd.cpu().numpy(), invert_np(want, V)), name
        assert cm.kernel_map(ts, g.kernel_size, 2, g.dilation, region=g)[0] is nbr_fwd
        assert cm.kernel_map(ts, g.kernel_size, 1, g.dilation, region=g)[0] is not nbr_fwd        # the stride is in the key
    # the cube routes are where they were
    assert cm.kernel_map(ts, 3, 1, 1)[0] is cm.k3(ts) and cm.kernel_map(ts, 2, 2, 1)[0] is cm.k2(ts)[0]


def test_region_tables_one_row_and_none(ME, be):
    one = ME.CoordinateManager(torch.tensor([[0, 5, -3, 7]], dtype=torch.int32, device=DEV))
    for name in NAMES:
        g = gen(ME, name)
        offs = unit_offsets(name)
        fwd, inv, vin, vout, K, _, _ = one.kernel_map(1, g.kernel_size, 1, g.dilation, region=g)
        zero = [int(not any(o)) - 1 for o in offs.tolist()]          # row 0 under the zero offset, -1 elsewhere
        assert (vin, vout) == (1, 1) and fwd.view(-1).tolist() == zero and inv.view(-1).tolist() == zero, name
    none = ME.CoordinateManager(torch.empty((0, 4), dtype=torch.int32, device=DEV))
    for name in ("R1", "R4"):
        g = gen(ME, name)
        fwd, inv, vin, vout, K, _, _ = none.kernel_map(1, g.kernel_size, 1, g.dilation, region=g)
        assert (vin, vout, K) == (0, 0, g.kernel_volume) and fwd.size(0) == K and inv.size(0) == K
        assert int(fwd.max()) == -1 and int(inv.max()) == -1


@pytest.mark.parametrize("stray", [False, True])
def test_kmap_region_with_repeated_rows(ME, be, stray):
    """rows that repeat (and, `stray`, a row outside the packable range, which turns the mirrored stores off): nbr_fwd is
    kmap_general's table -- the first occurrence of a coordinate is named -- and both tables are the same bytes on every run"""
    rng = np.random.default_rng(13)
    c, _ = random_sparse(rng, B=2, grid=12, n=400, C=1)
    c = np.concatenate([c, c[:50], c[10:30], c[390:]])
    if stray:
        c = np.concatenate([c, np.array([[0, 20000, 3, 3], [1, 2, -17000, 5]], np.int32)])
    rng.shuffle(c)
    t = torch.from_numpy(np.ascontiguousarray(c)).to(DEV)
    for name in NAMES:
        offs = unit_offsets(name).astype(np.int32)
        fwd, inv = be.kmap_region(t, offs)
        assert torch.equal(fwd, be.kmap_general(t, t, torch.from_numpy(offs))), name
        if not stray:
            assert np.array_equal(fwd.cpu().numpy(), dict_map(c, c, offs)), name
        fwd2, inv2 = be.kmap_region(t, offs)
        assert torch.equal(fwd, fwd2) and torch.equal(inv, inv2), name
        assert int(inv.min()) >= -1 and int(inv.max()) < c.shape[0]


# ---------------------------------------------------------------------------------------------- 2. convolutions
def dense_region_conv(coords, x, W, bias, name, stride, ts, out_coords, B, G):
    offs = unit_offsets(name)
    r = reach(offs)
    y = F.conv3d(densify64(coords, x, B, G, ts), embed(W, offs, r), None if bias is None else bias.view(-1), stride=stride,
                 padding=r)
    return read_dense(y, out_coords, ts * stride)


def _conv_case(ME, name, stride, cin, cout, ts=1, pending=False, B=2, G=12, n=400, seed=11, twice=False):
    rng = np.random.default_rng(seed + 10 * stride + cin + sum(map(ord, name)))
    coords, _ = random_sparse(rng, B=B, grid=G, n=n, C=1)
    cm = manager_at(ME, coords, ts)
    in_coords = cm.coords[ts].cpu().numpy()
    feats = rng.standard_normal((in_coords.shape[0], cin)).astype(np.float32)
    g = gen(ME, name, stride)
    conv = ME.MinkowskiConvolution(cin, cout, kernel_generator=g, bias=True, dimension=3).to(DEV)
    conv.train()
    assert tuple(conv.kernel.shape) == (g.kernel_volume, cin, cout)
    gy = None
    runs = []
    for _ in range(2 if twice else 1):
        conv.zero_grad(set_to_none=True)
        xf = torch.from_numpy(feats).to(DEV).requires_grad_(True)
        xin = ME.SparseTensor(xf, coordinate_manager=cm, tensor_stride=ts)
        if pending:
            bn = ME.MinkowskiBatchNorm(cin).to(DEV).train()
            with torch.no_grad():
                bn.bn.weight.uniform_(0.5, 1.5)
                bn.bn.bias.uniform_(-0.3, 0.3)
            xin = ME.MinkowskiReLU()(bn(xin))
            assert xin._pending is not None and xin._pending["relu"]
        y = conv(xin)
        out_ts = ts * stride
        assert y.tensor_stride == out_ts and y.coordinate_manager is cm
        if gy is None:
            gy = rng.standard_normal(tuple(y._F.shape)).astype(np.float32)
        y._F.backward(torch.from_numpy(gy).to(DEV))
        runs.append([t.detach().clone() for t in (y._F, xf.grad, conv.kernel.grad, conv.bias.grad)])
    if twice:
        for what, a, b in zip(("output", "dx", "dW", "dbias"), *runs):
            assert same(a, b), (name, what)
    out_coords = cm.coords[out_ts].cpu().numpy()
    x64 = torch.from_numpy(feats).double().requires_grad_(True)
    a64 = x64
    if pending:
        g64 = bn.bn.weight.detach().double().cpu().requires_grad_(True)
        b64 = bn.bn.bias.detach().double().cpu().requires_grad_(True)
        a64 = torch.relu(F.batch_norm(x64, None, None, g64, b64, True, 0.1, 1e-5))
    W64 = conv.kernel.detach().double().cpu().requires_grad_(True)
    bias64 = conv.bias.detach().double().cpu().requires_grad_(True)
    want = dense_region_conv(in_coords, a64, W64, bias64, name, stride, ts, out_coords, B, G // ts)
    tag = f"{name} s{stride} ts{ts} {cin}->{cout}" + (" bn+relu" if pending else "")
    got_y, got_dx, got_dw, got_db = runs[-1]
    check(tag + " forward", got_y, want, RTOL)
    want.backward(torch.from_numpy(gy).double())
    check(tag + " backward-data", got_dx, x64.grad, RTOL)
    check(tag + " backward-weight", got_dw, W64.grad, RTOL)
    check(tag + " bias gradient", got_db, bias64.grad.view(1, -1), RTOL)
    if pending:
        check(tag + " dgamma", bn.bn.weight.grad, g64.grad, 1e-3)
        check(tag + " dbeta", bn.bn.bias.grad, b64.grad, 1e-3)


@pytest.mark.parametrize("cin,cout", [(6, 16), (16, 32), (32, 32)])
@pytest.mark.parametrize("name,stride", [("R1", 1), ("R1", 2), ("R2", 1), ("R3", 1), ("R4", 1), ("R5", 1), ("R4", 2)])
def test_conv_against_dense(ME, name, stride, cin, cout):
    _conv_case(ME, name, stride, cin, cout)


def test_conv_on_tensor_stride_2(ME):
    _conv_case(ME, "R1", 1, 16, 32, ts=2, n=900, G=16)


def test_conv_pending_bn_relu(ME):
    _conv_case(ME, "R1", 1, 16, 32, pending=True)


@pytest.mark.parametrize("name", ["R6", "R7"])
def test_conv_27_and_8_offsets_stay_off_the_tuned_routes(ME, name):
    """a CUSTOM list of exactly 27 / 8 offsets at 64 -> 64 is neither the 3x3x3 submanifold map nor the k2 map"""
    _conv_case(ME, name, 1, 64, 64)


@pytest.mark.parametrize("name", ["R6", "R7"])
def test_conv_27_and_8_offsets_many_rows(ME, name):
    """the same with enough rows (40 000 in 48^3) that pair lists and the wide backward-weight routes are chosen by shape;
    yardstick: the float64 gather over the dictionary map"""
    rng = np.random.default_rng(5)
    coords, _ = random_sparse(rng, B=1, grid=48, n=40000, C=1)
    cm = manager_at(ME, coords, 1)
    feats = rng.standard_normal((40000, 64)).astype(np.float32)
    xf = torch.from_numpy(feats).to(DEV).requires_grad_(True)
    conv = ME.MinkowskiConvolution(64, 64, kernel_generator=gen(ME, name), dimension=3).to(DEV).train()
    y = conv(ME.SparseTensor(xf, coordinate_manager=cm))
    nbr = dict_map(coords, coords, unit_offsets(name))
    assert np.array_equal(cm.kernel_map(1, -1, 1, 1, region=gen(ME, name))[0].cpu().numpy(), nbr)
    x64 = torch.from_numpy(feats).double().requires_grad_(True)
    W64 = conv.kernel.detach().double().cpu().requires_grad_(True)
    want = ref_conv(x64, W64, torch.from_numpy(nbr))
    check(name + " 40k rows forward", y._F, want, RTOL)
    g = rng.standard_normal((40000, 64)).astype(np.float32)
    y._F.backward(torch.from_numpy(g).to(DEV))
    want.backward(torch.from_numpy(g).double())
    check(name + " 40k rows backward-data", xf.grad, x64.grad, RTOL)
    check(name + " 40k rows backward-weight", conv.kernel.grad, W64.grad, RTOL)


# ---------------------------------------------------------------------------------------------- 7. the same bytes twice
@pytest.mark.parametrize("name,stride", [("R1", 1), ("R4", 1), ("R4", 2)])
def test_conv_same_bytes_twice(ME, name, stride):
    _conv_case(ME, name, stride, 16, 32, twice=True)


# ---------------------------------------------------------------------------------------------- 3. a cube generator
@pytest.mark.parametrize("ks,stride,dil", [(3, 1, 1), (2, 2, 1), (5, 1, 1)])
def test_cube_generator_is_the_plain_layer(ME, ks, stride, dil):
    rng = np.random.default_rng(29 + ks)
    coords, feats = random_sparse(rng, B=2, grid=12, n=400, C=16)
    cm = manager_at(ME, coords, 1)
    plain = ME.MinkowskiConvolution(16, 32, kernel_size=ks, stride=stride, dilation=dil, bias=True, dimension=3).to(DEV).train()
    g = ME.KernelGenerator(ks, stride, dil, region_type=ME.RegionType.HYPER_CUBE, dimension=3)
    byg = ME.MinkowskiConvolution(16, 32, kernel_generator=g, bias=True, dimension=3).to(DEV).train()
    byg.load_state_dict(plain.state_dict())
    gy = None
    res = []
    for layer in (plain, byg):
        xf = torch.from_numpy(feats).to(DEV).requires_grad_(True)
        y = layer(ME.SparseTensor(xf, coordinate_manager=cm))
        if gy is None:
            gy = torch.from_numpy(rng.standard_normal(tuple(y._F.shape)).astype(np.float32)).to(DEV)
        y._F.backward(gy)
        res.append((y._F.detach(), xf.grad, layer.kernel.grad, layer.bias.grad, y.tensor_stride))
    for what, a, b in zip(("output", "dx", "dW", "dbias"), res[0], res[1]):
        assert same(a, b), what
    assert res[0][4] == res[1][4] == stride


# ---------------------------------------------------------------------------------------------- 4. transposed, generated
def test_transposed_onto_the_cached_set(ME):
    B, G = 2, 12
    rng = np.random.default_rng(23)
    coords, feats = random_sparse(rng, B=B, grid=G, n=400, C=16)
    cm = manager_at(ME, coords, 1)
    g = gen(ME, "R1", stride=2)
    enc = ME.MinkowskiConvolution(16, 16, kernel_generator=g, dimension=3).to(DEV)
    mid = enc(ME.SparseTensor(torch.from_numpy(feats).to(DEV), coordinate_manager=cm))
    assert mid.tensor_stride == 2
    xc = mid._F.detach().cpu().numpy()
    xf = torch.from_numpy(xc).to(DEV).requires_grad_(True)
    up = ME.MinkowskiConvolutionTranspose(16, 32, kernel_generator=gen(ME, "R1", stride=2, is_transpose=True), bias=True,
                                          dimension=3).to(DEV)
    y = up(ME.SparseTensor(xf, coordinate_manager=cm, tensor_stride=2))
    assert y.tensor_stride == 1 and y.coordinate_manager is cm and y._F.size(0) == 400
    offs = unit_offsets("R1")
    r = reach(offs)
    x64 = torch.from_numpy(xc).double().requires_grad_(True)
    W64 = up.kernel.detach().double().cpu().requires_grad_(True)
    b64 = up.bias.detach().double().cpu().requires_grad_(True)
    # out[2 q + off_k] += x[q] W[k]: the transpose of the strided convolution; what reaches beyond the fine grid is never read
    d = densify64(cm.coords[2].cpu().numpy(), x64, B, G // 2, 2)
    yd = F.conv_transpose3d(d, embed(W64, offs, r).transpose(0, 1), b64.view(-1), stride=2)[..., r:r + G, r:r + G, r:r + G]
    want = read_dense(yd, coords, 1)
    check("transposed R1 forward", y._F, want, RTOL)
    gy = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y._F.backward(torch.from_numpy(gy).to(DEV))
    want.backward(torch.from_numpy(gy).double())
    check("transposed R1 backward-data", xf.grad, x64.grad, RTOL)
    check("transposed R1 backward-weight", up.kernel.grad, W64.grad, RTOL)
    check("transposed R1 bias gradient", up.bias.grad, b64.grad.view(1, -1), RTOL)


def _onto_case(ME, layer, name, x, xf, feats, coords, want_set, transposed, B, G, tag, rng, call=None):
    """a layer onto a generated / expanded / named set: the set, the values and the gradients against the dense reference,
    read at the set's coordinates shifted by r into a grid padded by r on every side"""
    y = layer(x) if call is None else call(x)
    assert np.array_equal(y.C.cpu().numpy(), want_set), tag + ": the output set"
    offs = unit_offsets(name)
    r = reach(offs)
    x64 = torch.from_numpy(feats).double().requires_grad_(True)
    W64 = layer.kernel.detach().double().cpu().requires_grad_(True)
    b64 = layer.bias.detach().double().cpu().requires_grad_(True)
    d = densify64(coords, x64, B, G, 1)
    if transposed:       # out[c + off_k] += x[c] W[k]
        yd = F.conv_transpose3d(d, embed(W64, offs, r).transpose(0, 1), b64.view(-1))
    else:                # out[o] = sum_k x[o + off_k] W[k]
        yd = F.conv3d(d, embed(W64, offs, r), b64.view(-1), padding=2 * r)
    want = read_dense(yd, want_set, 1, shift=r)
    check(tag + " forward", y.F, want, RTOL)
    gy = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y.F.backward(torch.from_numpy(gy).to(DEV))
    want.backward(torch.from_numpy(gy).double())
    check(tag + " backward-data", xf.grad, x64.grad, RTOL)
    check(tag + " backward-weight", layer.kernel.grad, W64.grad, RTOL)
    check(tag + " bias gradient", layer.bias.grad, b64.grad.view(1, -1), RTOL)
    return y


def _input(ME, rng, C, B=2, G=12, n=400):
    coords, feats = random_sparse(rng, B=B, grid=G, n=n, C=C)
    xf = torch.from_numpy(feats).to(DEV).requires_grad_(True)
    return coords, feats, xf, ME.SparseTensor(xf, coordinate_manager=manager_at(ME, coords, 1))


def test_generative_transpose_with_a_cross(ME):
    rng = np.random.default_rng(31)
    coords, feats, xf, x = _input(ME, rng, 16)
    layer = ME.MinkowskiGenerativeConvolutionTranspose(16, 32, kernel_generator=gen(ME, "R1"), bias=True, dimension=3).to(DEV)
    y = _onto_case(ME, layer, "R1", x, xf, feats, coords, expand_np(coords, unit_offsets("R1")), True, 2, 12, "generative R1",
                   rng)
    assert y.coordinate_manager is not x.coordinate_manager and y.tensor_stride == 1


def test_expand_coordinates_with_a_custom_list(ME):
    rng = np.random.default_rng(37)
    coords, feats, xf, x = _input(ME, rng, 16)
    layer = ME.MinkowskiConvolution(16, 32, kernel_generator=gen(ME, "R4", expand_coordinates=True), bias=True,
                                    dimension=3).to(DEV)
    assert layer.expand_coordinates
    _onto_case(ME, layer, "R4", x, xf, feats, coords, expand_np(coords, -unit_offsets("R4")), False, 2, 12, "expanding R4", rng)


def test_cross_onto_given_coordinates(ME):
    rng = np.random.default_rng(41)
    coords, feats, xf, x = _input(ME, rng, 16)
    offs = unit_offsets("R1")
    cells = {(int(rng.integers(0, 2)), *(int(v) for v in rng.integers(-1, 13, 3))) for _ in range(300)}
    tgt = np.array(sorted(cells), np.int32)
    rng.shuffle(tgt)
    lonely = np.nonzero((dict_map(coords, tgt, offs) < 0).all(0))[0]
    assert lonely.size > 0, "the target needs a row no input reaches"
    layer = ME.MinkowskiConvolution(16, 32, kernel_generator=gen(ME, "R1"), bias=True, dimension=3).to(DEV)
    T = torch.from_numpy(tgt).to(DEV)
    y = _onto_case(ME, layer, "R1", x, xf, feats, coords, tgt, False, 2, 12, "R1 onto a target", rng,
                   call=lambda t: layer(t, coordinates=T))
    assert torch.equal(y.F.detach()[torch.from_numpy(lonely).to(DEV)], layer.bias.detach().expand(lonely.size, 32))


# ---------------------------------------------------------------------------------------------- 5. channel-wise, pooling
def gather64(x64, nbr, fill=0.0):
    """[K, Vout, C]: the input row under every offset, `fill` where there is none"""
    xp = torch.cat([x64, torch.full((1, x64.size(1)), fill, dtype=torch.float64)])
    idx = torch.from_numpy(nbr).long()
    return xp[torch.where(idx < 0, torch.full_like(idx, x64.size(0)), idx)]


@pytest.mark.parametrize("C_", [5, 16, 33])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("name", ["R1", "R4"])
def test_channelwise_against_gather(ME, name, stride, C_):
    rng = np.random.default_rng(50 + C_ + stride)
    coords, feats = random_sparse(rng, B=2, grid=12, n=400, C=C_)
    cm = manager_at(ME, coords, 1)
    xf = torch.from_numpy(feats).to(DEV).requires_grad_(True)
    layer = ME.MinkowskiChannelwiseConvolution(C_, kernel_generator=gen(ME, name, stride), bias=True, dimension=3).to(DEV)
    y = layer(ME.SparseTensor(xf, coordinate_manager=cm))
    assert y.tensor_stride == stride
    nbr = dict_map(coords, cm.coords[stride].cpu().numpy(), unit_offsets(name))
    x64 = torch.from_numpy(feats).double().requires_grad_(True)
    W64 = layer.kernel.detach().double().cpu().requires_grad_(True)
    b64 = layer.bias.detach().double().cpu().requires_grad_(True)
    want = (gather64(x64, nbr) * W64[:, None, :]).sum(0) + b64
    tag = f"channel-wise {name} s{stride} C{C_}"
    check(tag + " forward", y._F, want, RTOL)
    gy = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y._F.backward(torch.from_numpy(gy).to(DEV))
    want.backward(torch.from_numpy(gy).double())
    check(tag + " backward-data", xf.grad, x64.grad, RTOL)
    check(tag + " backward-weight", layer.kernel.grad, W64.grad, RTOL)
    check(tag + " bias gradient", layer.bias.grad, b64.grad, RTOL)


@pytest.mark.parametrize("C_", [5, 16, 33])
@pytest.mark.parametrize("name", ["R1", "R4"])
@pytest.mark.parametrize("mode", ["max", "avg", "sum"])
def test_pooling_against_gather(ME, mode, name, C_):
    """(both regions hold the centre, so every output row has an input present)"""
    rng = np.random.default_rng(60 + C_)
    coords, feats = random_sparse(rng, B=2, grid=12, n=400, C=C_)
    cm = manager_at(ME, coords, 1)
    xf = torch.from_numpy(feats).to(DEV).requires_grad_(True)
    cls = {"max": ME.MinkowskiMaxPooling, "avg": ME.MinkowskiAvgPooling, "sum": ME.MinkowskiSumPooling}[mode]
    y = cls(3, kernel_generator=gen(ME, name), dimension=3)(ME.SparseTensor(xf, coordinate_manager=cm))
    nbr = dict_map(coords, coords, unit_offsets(name))
    x64 = torch.from_numpy(feats).double().requires_grad_(True)
    if mode == "max":
        vals = gather64(x64, nbr, -np.inf)
        assert int((vals == vals.max(0).values).sum(0).max()) == 1, "a tie in a max: the draw is not what it should be"
        want = vals.max(0).values
    else:
        want = gather64(x64, nbr).sum(0)
        if mode == "avg":
            cnt = torch.from_numpy((nbr >= 0).sum(0)).double().view(-1, 1)         # the inputs PRESENT
            assert float(cnt.min()) >= 1 and float(cnt.max()) > float(cnt.min())
            want = want / cnt
    tag = f"{mode} pool {name} C{C_}"
    if mode == "max":
        assert torch.equal(y._F.detach().cpu(), want.detach().float()), tag
    else:
        check(tag + " forward", y._F, want, STOL)
    gy = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y._F.backward(torch.from_numpy(gy).to(DEV))
    want.backward(torch.from_numpy(gy).double())
    check(tag + " backward", xf.grad, x64.grad, STOL)


@pytest.mark.parametrize("name,stride", [("R1", 1), ("R1", 2), ("R4", 1)])
def test_pooling_transpose(ME, name, stride):
    """out[o] = sum_k x[o - off_k]: at stride 1 on the set itself (R4 has offsets without a partner: the inverse table, not
    the forward one), at stride 2 from the coarse set onto the cached fine one"""
    rng = np.random.default_rng(70 + stride)
    coords, _ = random_sparse(rng, B=2, grid=12, n=400, C=1)
    cm = manager_at(ME, coords, stride)
    cin = cm.coords[stride].cpu().numpy()
    feats = rng.standard_normal((cin.shape[0], 16)).astype(np.float32)
    xf = torch.from_numpy(feats).to(DEV).requires_grad_(True)
    layer = ME.MinkowskiPoolingTranspose(3, stride, kernel_generator=gen(ME, name, stride), dimension=3)
    y = layer(ME.SparseTensor(xf, coordinate_manager=cm, tensor_stride=stride))
    assert y.tensor_stride == 1 and y._F.size(0) == 400
    nbr = dict_map(cin, coords, -unit_offsets(name))
    x64 = torch.from_numpy(feats).double().requires_grad_(True)
    want = gather64(x64, nbr).sum(0)
    tag = f"pooling transpose {name} s{stride}"
    check(tag + " forward", y._F, want, STOL)
    gy = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y._F.backward(torch.from_numpy(gy).to(DEV))
    want.backward(torch.from_numpy(gy).double())
    check(tag + " backward", xf.grad, x64.grad, STOL)


# ---------------------------------------------------------------------------------------------- 6. the weight-image window
def test_region_layers_inside_a_prepare_window(ME):
    """cube 3 -> BN -> ReLU -> R1 -> R4: one training step inside a prepare_conv_weights window and one outside it give the
    same bytes -- loss and every gradient (the level tests/test_mapkey_gpu.py holds the `coordinates=` layers to): a region
    layer is laid out like a two-set layer, with no mirrored backward-data image"""
    rng = np.random.default_rng(67)
    coords, feats = random_sparse(rng, B=2, grid=12, n=400, C=16)
    cm = manager_at(ME, coords, 1)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.cube = ME.MinkowskiConvolution(16, 16, kernel_size=3, dimension=3)
            self.bn = ME.MinkowskiBatchNorm(16)
            self.relu = ME.MinkowskiReLU()
            self.cross = ME.MinkowskiConvolution(16, 32, kernel_generator=gen(ME, "R1"), dimension=3)
            self.custom = ME.MinkowskiConvolution(32, 16, kernel_generator=gen(ME, "R4"), bias=True, dimension=3)

        def forward(self, x):
            return self.custom(self.cross(self.relu(self.bn(self.cube(x)))))

    torch.manual_seed(0)
    net = Net().to(DEV).train()
    assert net.cube._image_mirror() and not net.cross._image_mirror() and not net.custom._image_mirror()
    gy = torch.from_numpy(rng.standard_normal((400, 16)).astype(np.float32)).to(DEV)

    def step(window):
        net.zero_grad(set_to_none=True)
        xf = torch.from_numpy(feats).to(DEV).requires_grad_(True)
        x = ME.SparseTensor(xf, coordinate_manager=cm)
        if window:
            ME.prepare_conv_weights(net)
            try:
                y = net(x)
            finally:
                ME.release_conv_weights()
        else:
            y = net(x)
        loss = (y.F * gy).sum()
        loss.backward()
        out = {"loss": loss.detach().clone(), "y": y.F.detach().clone(), "dx": xf.grad.clone()}
        out.update({n: p.grad.clone() for n, p in net.named_parameters()})
        return out

    outside, inside = step(False), step(True)
    assert set(outside) == set(inside) and len(outside) == 3 + 6
    for k in outside:
        assert same(outside[k], inside[k]), k
    # and the values are right (a mirrored image would show in dx)
    P = {n: p.detach().double().cpu() for n, p in net.named_parameters()}
    x64 = torch.from_numpy(feats).double().requires_grad_(True)
    h = ref_conv(x64, P["cube.kernel"], torch.from_numpy(dict_map(coords, coords, cube_offsets(3, 1, 1))))
    h = torch.relu(F.batch_norm(h, None, None, P["bn.bn.weight"], P["bn.bn.bias"], True, 0.1, 1e-5))
    h = ref_conv(h, P["cross.kernel"], torch.from_numpy(dict_map(coords, coords, unit_offsets("R1"))))
    h = ref_conv(h, P["custom.kernel"], torch.from_numpy(dict_map(coords, coords, unit_offsets("R4")))) + P["custom.bias"]
    h.backward(gy.double().cpu())
    check("window output", inside["y"], h, RTOL)
    check("window dx", inside["dx"], x64.grad, RTOL)
