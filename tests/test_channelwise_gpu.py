"""GPU: MinkowskiChannelwiseConvolution (csrc/chconv.hip) -- forward, backward-data (the forward kernel through the inverse
table), the two-stage backward-weight reduction and the bias gradient.

The yardstick for values is dense torch in float64 on the CPU, never this engine: the sparse input is scattered into a dense
grid [B, C, x, y, z], the kernel W [K, C] with k = ix + ks iy + ks^2 iz becomes the depthwise dense weight
W.view(ks, ks, ks, C).permute(3, 2, 1, 0).unsqueeze(1) of F.conv3d(groups=C), and the result is read at the output
coordinates.  Padding: odd kernels dilation * (ks - 1) / 2 on both sides, even kernels none in front and the reach of the
kernel behind.  Gradients come from autograd through that float64 graph.  Bound: the project's bar, 1e-4 of the reference
tensor's largest magnitude, for the output, din, dW and dbias alike.  The small helpers (cloud, densify, read, pad) are this
file's own copies.  Every weight-reduction size here (at most 2r + 1 = 257 rows) fits a 16^3 grid, so the dense reference
serves them all and no table-walking restatement is needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
RTOL = 1e-4
GEOMS = [(3, 1, 1), (3, 1, 2), (5, 1, 1), (2, 2, 1), (3, 2, 1), (4, 2, 1)]


@pytest.fixture(scope="module")
def ME():
    import minsu3d_amd.MinkowskiEngine as me
    return me


@pytest.fixture(scope="module")
def be():
    from minsu3d_amd.backend import get_backend
    return get_backend()


@pytest.fixture(scope="module")
def rows_per_part(be):
    return int(be.lib.ms3d_chconv_wgrad_rows_per_part())


# ---------------------------------------------------------------------------------------------- helpers (own copies)
def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def check(name, got, want, tol=RTOL):
    assert tuple(got.shape) == tuple(want.shape), (name, tuple(got.shape), tuple(want.shape))
    e = rel_err(got, want)
    print(f"{name}: rel err {e:.3e} (bound {tol:.0e})")
    assert e <= tol, (name, e)


def cloud(rng, B, G, n):
    """n distinct (b, x, y, z) rows of a B x G^3 grid in random order"""
    cells = rng.choice(B * G ** 3, size=n, replace=False)
    b, rest = np.divmod(cells, G ** 3)
    x, rest = np.divmod(rest, G * G)
    y, z = np.divmod(rest, G)
    return np.stack([b, x, y, z], 1).astype(np.int32)


def densify64(coords, feats, B, G, unit):
    d = torch.zeros((B, feats.shape[1], G, G, G), dtype=torch.float64)
    c = torch.as_tensor(coords).long()
    d[c[:, 0], :, c[:, 1] // unit, c[:, 2] // unit, c[:, 3] // unit] = feats
    return d


def read_dense(d, coords, unit):
    c = torch.as_tensor(coords).long()
    return d[c[:, 0], :, c[:, 1] // unit, c[:, 2] // unit, c[:, 3] // unit]


def pad_for(ks, dil):
    """(F.pad tuple behind the three spatial axes or None, symmetric conv padding) of a kernel"""
    if ks % 2:
        return None, dil * (ks - 1) // 2
    r = dil * (ks - 1)
    return (0, r, 0, r, 0, r), 0


def dense_chconv(coords, x, W, bias, ks, stride, dil, ts, out_coords, B, G):
    """x [V, C], W [K, C], bias [1, C] or None (float64, autograd) -> rows at out_coords"""
    C = W.shape[1]
    d = densify64(coords, x, B, G, ts)
    padt, p = pad_for(ks, dil)
    if padt is not None:
        d = F.pad(d, padt)
    w = W.view(ks, ks, ks, C).permute(3, 2, 1, 0).unsqueeze(1)
    y = F.conv3d(d, w, None if bias is None else bias.view(-1), stride=stride, padding=p, dilation=dil, groups=C)
    return read_dense(y, out_coords, ts * stride)


def _coordinate_order(coords):
    c = np.asarray(coords).astype(np.int64)
    return np.argsort(((c[:, 0] * 64 + c[:, 1]) * 64 + c[:, 2]) * 64 + c[:, 3])


def manager_of(ME, coords, kind="plain"):
    c = torch.from_numpy(np.ascontiguousarray(coords)).cuda()
    if kind == "rooted":
        return ME.CoordinateManager.rooted(c, 1)
    if kind == "sorted":
        cm = ME.CoordinateManager(c, spatial_sort=True)
        assert cm.perm is not None, "the cloud is too small to be Morton-sorted"
        return cm
    return ME.CoordinateManager(c)


def run_case(ME, coords, ks, stride, dil, C, bias, B, G, kind="plain", seed=0, tag=None, needs=(True, True)):
    """the layer on `coords` (caller order) against the dense float64 graph: forward and every gradient asked for.
    -> dict of the engine's results with rows in CALLER order (stride-2 outputs: with their coordinates)"""
    rng = np.random.default_rng(1000 * ks + 100 * stride + 10 * dil + C + seed)
    V = coords.shape[0]
    feats = rng.standard_normal((V, C)).astype(np.float32)
    torch.manual_seed(seed + ks + C)
    layer = ME.MinkowskiChannelwiseConvolution(C, kernel_size=ks, stride=stride, dilation=dil, bias=bias, dimension=3).cuda()
    x_grad, w_grad = needs
    layer.kernel.requires_grad_(w_grad)
    cm = manager_of(ME, coords, kind)
    xf = torch.from_numpy(feats).cuda().requires_grad_(x_grad)
    xin = ME.SparseTensor(xf if cm.perm is None else xf[cm.perm], coordinate_manager=cm, tensor_stride=1)
    y = layer(xin)
    assert y.tensor_stride == stride and y.coordinate_manager is cm
    out_coords = y.coordinates.cpu().numpy()
    x64 = torch.from_numpy(feats).double().requires_grad_(True)
    W64 = layer.kernel.detach().double().cpu().requires_grad_(True)
    b64 = layer.bias.detach().double().cpu().requires_grad_(True) if bias else None
    want = dense_chconv(coords, x64, W64, b64, ks, stride, dil, 1, out_coords, B, G)
    tag = tag or f"k{ks} s{stride} d{dil} C{C} V{V} {kind}" + (" bias" if bias else "")
    yf = y.features
    assert yf.dtype == torch.float32
    check(tag + " forward", yf, want)
    # (dout is dealt out by output COORDINATE, so that two managers that order a stride-2 set differently see the same one)
    g = np.empty(tuple(want.shape), np.float32)
    g[_coordinate_order(out_coords)] = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    yf.backward(torch.from_numpy(g).cuda())
    want.backward(torch.from_numpy(g).double())
    res = dict(y=yf.detach(), out_coords=out_coords, layer=layer, want_dx=x64.grad, want_dw=W64.grad)
    if x_grad:
        check(tag + " backward-data", xf.grad, x64.grad)
        res["dx"] = xf.grad
    else:
        assert xf.grad is None
    if w_grad:
        assert tuple(layer.kernel.grad.shape) == (ks ** 3, C)
        check(tag + " backward-weight", layer.kernel.grad, W64.grad)
        res["dw"] = layer.kernel.grad
    else:
        assert layer.kernel.grad is None
    if bias:
        check(tag + " bias gradient", layer.bias.grad, b64.grad.view(1, -1))
        res["db"] = layer.bias.grad
    return res


# ---------------------------------------------------------------------------------------------- 1. geometries
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("ks,stride,dil", GEOMS)
def test_geometries_against_dense(ME, ks, stride, dil, bias):
    coords = cloud(np.random.default_rng(11), 2, 12, 300)
    run_case(ME, coords, ks, stride, dil, 20, bias, 2, 12)


def _by_coordinate(rows, coords):
    return rows[torch.from_numpy(_coordinate_order(coords)).to(rows.device)]


@pytest.mark.parametrize("ks,stride,dil", GEOMS)
def test_rooted_and_morton_sorted_managers_agree(ME, ks, stride, dil):
    """a manager made by CoordinateManager.rooted (rows stay as given) and a Morton-sorted one (4200 rows: the engine sorts
    from 4096 rows on) hold the dense reference each, and give the same rows in caller order: the forward and backward-data
    sums run over ascending k whatever the row order, so those are equal bit for bit (stride-2 outputs are matched by their
    coordinates, each manager orders that set its own way); dW is summed over the rows in engine order and is held to the
    reference on both"""
    coords = cloud(np.random.default_rng(13), 2, 16, 4200)
    a = run_case(ME, coords, ks, stride, dil, 20, True, 2, 16, kind="rooted")
    b = run_case(ME, coords, ks, stride, dil, 20, True, 2, 16, kind="sorted")
    assert torch.equal(a["layer"].kernel, b["layer"].kernel)
    if stride == 1:
        assert np.array_equal(a["out_coords"], coords) and np.array_equal(b["out_coords"], coords)
        assert torch.equal(a["y"], b["y"])
    else:
        assert torch.equal(_by_coordinate(a["y"], a["out_coords"]), _by_coordinate(b["y"], b["out_coords"]))
    assert torch.equal(a["dx"], b["dx"])


# ---------------------------------------------------------------------------------------------- 2. lane-layout edges
@pytest.mark.parametrize("V", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("C", [1, 3, 4, 64, 68])
def test_lane_layout_edges(ME, C, V):
    """C = 1, 3: scalar lanes; 4: one 16-byte lane per row; 64: a full tile of 16 lanes; 68: two tiles of 9 and 8 lanes (a
    lane count per row that is no power of two).  V = 1: a single voxel that only its centre offset finds."""
    coords = cloud(np.random.default_rng(17 + V), 2, 12, V)
    run_case(ME, coords, 3, 1, 1, C, True, 2, 12)


def test_isolated_rows_at_dilation_2(ME):
    coords = cloud(np.random.default_rng(19), 2, 12, 120)
    cm = manager_of(ME, coords)
    nbr = cm.kernel_map(1, 3, 1, 2)[0].cpu().numpy()
    found = (nbr >= 0).sum(0)
    assert (found == 1).any() and (found > 1).any(), "the cloud must hold isolated rows and connected ones"
    for C in (3, 20):
        run_case(ME, coords, 3, 1, 2, C, True, 2, 12)


# ---------------------------------------------------------------------------------------------- 3. weight-reduction edges
@pytest.mark.parametrize("C", [4, 3])
@pytest.mark.parametrize("dv", ["r-1", "r", "r+1", "2r+1"])
def test_weight_reduction_edges(ME, rows_per_part, C, dv):
    r = rows_per_part
    V = {"r-1": r - 1, "r": r, "r+1": r + 1, "2r+1": 2 * r + 1}[dv]
    B = 1
    while B * 16 ** 3 < 4 * V:          # keep the cloud sparse enough to have absent neighbours
        B *= 2
    coords = cloud(np.random.default_rng(23 + V), B, 16, V)
    res = run_case(ME, coords, 3, 1, 1, C, True, B, 16)
    assert "dw" in res and "db" in res


def test_weight_reduction_strided_output_crosses_a_part(ME, rows_per_part):
    """(2, 2, 1): the parts are runs of OUTPUT rows -- r + 1 coarse cells, one to three fine voxels in each"""
    r = rows_per_part
    rng = np.random.default_rng(29)
    B = 1
    while B * 8 ** 3 < 2 * (r + 1):
        B *= 2
    coarse = cloud(rng, B, 8, r + 1)
    fine = []
    for b, x, y, z in coarse.tolist():
        kids = rng.choice(8, size=int(rng.integers(1, 4)), replace=False)
        fine += [(b, 2 * x + (k & 1), 2 * y + ((k >> 1) & 1), 2 * z + (k >> 2)) for k in kids.tolist()]
    coords = np.array(fine, np.int32)
    rng.shuffle(coords)
    for C in (4, 3):
        res = run_case(ME, coords, 2, 2, 1, C, True, B, 16)
        assert res["y"].size(0) == r + 1


# ---------------------------------------------------------------------------------------------- 4. unaligned rows
def test_unaligned_rows_take_the_scalar_route(ME, be):
    """rows carved one float into a buffer are 4-byte but not 16-byte aligned: the scalar kernel runs, same bits"""
    rng = np.random.default_rng(31)
    coords = cloud(rng, 2, 12, 300)
    cm = manager_of(ME, coords)
    nbr, _, vin, vout, K, _, _ = cm.kernel_map(1, 3, 1, 1)
    x = torch.from_numpy(rng.standard_normal((vin, 4)).astype(np.float32)).cuda()
    w = torch.from_numpy(rng.standard_normal((K, 4)).astype(np.float32)).cuda()
    bias = torch.from_numpy(rng.standard_normal((1, 4)).astype(np.float32)).cuda()
    flat = torch.zeros(vin * 4 + 1, dtype=torch.float32, device="cuda")
    xu = flat[1:].view(vin, 4)
    xu.copy_(x)
    assert x.data_ptr() % 16 == 0 and xu.data_ptr() % 16 == 4 and xu.is_contiguous()
    ya = be.chconv_forward(x, w, bias, nbr, vout, K)
    yu = be.chconv_forward(xu, w, bias, nbr, vout, K)
    assert torch.equal(ya, yu)
    want = dense_chconv(coords, x.double().cpu(), w.double().cpu(), bias.double().cpu(), 3, 1, 1, 1, coords, 2, 12)
    check("unaligned forward", yu, want)


# ---------------------------------------------------------------------------------------------- 5. bit-reproducibility
def test_bit_reproducible(ME, rows_per_part):
    V = 2 * rows_per_part + 1
    coords = cloud(np.random.default_rng(37), 1, 16, V)
    a = run_case(ME, coords, 3, 1, 1, 20, True, 1, 16, seed=5)
    b = run_case(ME, coords, 3, 1, 1, 20, True, 1, 16, seed=5)
    assert torch.equal(a["layer"].kernel, b["layer"].kernel)
    for name in ("y", "dx", "dw", "db"):
        assert a[name].cpu().numpy().tobytes() == b[name].cpu().numpy().tobytes(), name


# ---------------------------------------------------------------------------------------------- 6. needs_input_grad
def test_frozen_kernel_and_input_without_grad(ME):
    coords = cloud(np.random.default_rng(41), 2, 12, 300)
    res = run_case(ME, coords, 3, 1, 1, 20, False, 2, 12, needs=(True, False))
    assert "dx" in res and res["layer"].kernel.grad is None
    res = run_case(ME, coords, 3, 2, 1, 20, False, 2, 12, needs=(False, True))
    assert "dw" in res and "dx" not in res


# ---------------------------------------------------------------------------------------------- 7. pending BatchNorm
def test_pending_batchnorm_relu_in_front(ME):
    """MinkowskiBatchNorm -> MinkowskiReLU leave the normalisation pending; the layer materialises it (x._raw()) and gives
    exactly what it gives on the materialised rows, and the dense float64 graph's values"""
    rng = np.random.default_rng(43)
    C, B, G = 20, 2, 12
    coords = cloud(rng, B, G, 300)
    feats = rng.standard_normal((300, C)).astype(np.float32)
    cm = manager_of(ME, coords)
    bn = ME.MinkowskiBatchNorm(C).cuda().train()
    with torch.no_grad():
        bn.bn.weight.uniform_(0.5, 1.5)
        bn.bn.bias.uniform_(-0.3, 0.3)
    layer = ME.MinkowskiChannelwiseConvolution(C, kernel_size=3, bias=True, dimension=3).cuda()
    xf = torch.from_numpy(feats).cuda().requires_grad_(True)
    t = ME.MinkowskiReLU()(bn(ME.SparseTensor(xf, coordinate_manager=cm)))
    assert t._pending is not None and t._pending["relu"]
    y = layer(t)
    assert y._pending is None
    with torch.no_grad():
        t2 = ME.MinkowskiReLU()(bn(ME.SparseTensor(xf.detach(), coordinate_manager=cm)))
        rows = t2._raw()
        y2 = layer(ME.SparseTensor(rows, coordinate_manager=cm))
    assert torch.equal(y._F.detach(), y2._F)
    x64 = torch.from_numpy(feats).double().requires_grad_(True)
    g64 = bn.bn.weight.detach().double().cpu()
    b64 = bn.bn.bias.detach().double().cpu()
    W64 = layer.kernel.detach().double().cpu().requires_grad_(True)
    bias64 = layer.bias.detach().double().cpu().requires_grad_(True)
    a64 = torch.relu(F.batch_norm(x64, None, None, g64, b64, True, 0.1, 1e-5))
    want = dense_chconv(coords, a64, W64, bias64, 3, 1, 1, 1, coords, B, G)
    check("bn+relu forward", y._F, want)
    g = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y._F.backward(torch.from_numpy(g).cuda())
    want.backward(torch.from_numpy(g).double())
    check("bn+relu backward-data", xf.grad, x64.grad)
    check("bn+relu backward-weight", layer.kernel.grad, W64.grad)
    check("bn+relu bias gradient", layer.bias.grad, bias64.grad.view(1, -1))


# ---------------------------------------------------------------------------------------------- 8. composed block
def test_depthwise_separable_residual_block(ME):
    """x + pointwise(relu(bn(depthwise 3^3 (x)))), then a stride-2 depthwise downsample, against the same block made of dense
    float64 torch operators: conv3d(groups=C), batch_norm over the occupied voxels only (the rows read back from the grid),
    conv3d 1x1x1"""
    rng = np.random.default_rng(47)
    C, B, G, V = 16, 2, 12, 400
    coords = cloud(rng, B, G, V)
    feats = rng.standard_normal((V, C)).astype(np.float32)
    cm = manager_of(ME, coords)
    # (no bias on the depthwise layer: a training-mode BatchNorm behind it removes the mean, its gradient is identically zero)
    dw = ME.MinkowskiChannelwiseConvolution(C, kernel_size=3, dimension=3).cuda()
    bn = ME.MinkowskiBatchNorm(C).cuda().train()
    pw = ME.MinkowskiConvolution(C, C, kernel_size=1, dimension=3).cuda().train()
    down = ME.MinkowskiChannelwiseConvolution(C, kernel_size=2, stride=2, dimension=3).cuda()
    with torch.no_grad():
        bn.bn.weight.uniform_(0.5, 1.5)
        bn.bn.bias.uniform_(-0.3, 0.3)
    xf = torch.from_numpy(feats).cuda().requires_grad_(True)
    x = ME.SparseTensor(xf, coordinate_manager=cm)
    y = down(x + pw(ME.MinkowskiReLU()(bn(dw(x)))))
    assert y.tensor_stride == 2
    out_coords = y.coordinates.cpu().numpy()

    def p64(t):
        return t.detach().double().cpu().requires_grad_(True)
    x64, Wd, gam, bet, Wp, Wdn = (p64(t) for t in (xf, dw.kernel, bn.bn.weight, bn.bn.bias, pw.kernel, down.kernel))
    h = dense_chconv(coords, x64, Wd, None, 3, 1, 1, 1, coords, B, G)
    h = torch.relu(F.batch_norm(h, None, None, gam, bet, True, 0.1, 1e-5))
    h = read_dense(F.conv3d(densify64(coords, h, B, G, 1), Wp.t().reshape(C, C, 1, 1, 1)), coords, 1)
    want = dense_chconv(coords, x64 + h, Wdn, None, 2, 2, 1, 1, out_coords, B, G)
    check("block forward", y._F, want)
    g = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y._F.backward(torch.from_numpy(g).cuda())
    want.backward(torch.from_numpy(g).double())
    check("block dx", xf.grad, x64.grad)
    check("block depthwise dW", dw.kernel.grad, Wd.grad)
    check("block dgamma", bn.bn.weight.grad, gam.grad)
    check("block dbeta", bn.bn.bias.grad, bet.grad)
    check("block pointwise dW", pw.kernel.grad, Wp.grad)
    check("block downsample dW", down.kernel.grad, Wdn.grad)


# ---------------------------------------------------------------------------------------------- 9. argument checks
def test_argument_checks(be):
    from minsu3d_amd._lib import HipLibraryError, E_UNSUPPORTED
    V = 5
    x = torch.zeros((V, 4), dtype=torch.float32, device="cuda")
    none255 = torch.full((255, V), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(HipLibraryError, match=str(E_UNSUPPORTED)):
        be.chconv_forward(x, torch.zeros((255, 4), device="cuda"), None, none255, V, 255)
    with pytest.raises(HipLibraryError, match=str(E_UNSUPPORTED)):
        be.chconv_backward_weight(x, x, none255, V, 255)
    none27 = torch.full((27, V), -1, dtype=torch.int32, device="cuda")
    x0 = torch.zeros((V, 0), dtype=torch.float32, device="cuda")
    with pytest.raises(HipLibraryError, match=str(E_UNSUPPORTED)):
        be.chconv_forward(x0, torch.zeros((27, 0), device="cuda"), None, none27, V, 27)
    with pytest.raises(HipLibraryError, match=str(E_UNSUPPORTED)):
        be.chconv_backward_weight(x0, x0, none27, V, 27)
    empty = torch.zeros((27, 0), dtype=torch.int32, device="cuda")
    y = be.chconv_forward(x, torch.ones((27, 4), device="cuda"), None, empty, 0, 27)
    assert tuple(y.shape) == (0, 4) and y.dtype == torch.float32
    dW = be.chconv_backward_weight(x, y, empty, 0, 27)
    assert tuple(dW.shape) == (27, 4) and not dW.any()
    torch.cuda.synchronize()
    # a table without a single present input: the bias alone
    bias = torch.arange(4, dtype=torch.float32, device="cuda").view(1, 4)
    y = be.chconv_forward(x, torch.ones((27, 4), device="cuda"), bias, none27, V, 27)
    assert torch.equal(y, bias.expand(V, 4))
