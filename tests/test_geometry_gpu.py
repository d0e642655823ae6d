"""GPU: general sparse geometries -- kernel maps of any kernel size / dilation at stride 1 or 2, convolutions with bias over
them (forward, backward-data, backward-weight, bias gradient), transposed convolutions onto a cached coordinate set, sparse
and global pooling.

The yardstick for values is dense torch in float64 on the CPU, never this engine: the sparse input is scattered into a dense
grid laid out [B, C, x, y, z] (as sparse_ref.densify does), so a weight W[k], k = ix + ks iy + ks^2 iz, becomes the dense
kernel [Cout, Cin, kx, ky, kz]; F.conv3d / F.conv_transpose3d / F.max_pool3d / F.avg_pool3d run on it, and the result is
read at the output coordinates.  Padding: odd kernels dilation * (ks - 1) / 2 on both sides, even kernels none in front and
the reach of the kernel behind.  Bound for convolutions: the project's bar, 1e-4 of the tensor's largest magnitude, at the
default "highest" precision.  Pooling: a max and a copy do not round, so max forward is compared exactly; sums of at most 27
floats (average / sum pooling, and every pooling BACKWARD whose kernels overlap -- an input row that is the maximum of
several outputs collects several gradients) to 1e-6 relative; the backward of a non-overlapping max pooling (kernel 2, stride
2) is a copy again and is compared exactly.  The one table too large for a dense grid (40 000 rows in 64^3) is checked with
sparse_ref.ref_conv in float64 over a table built by sorted-key lookup on the host."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sparse_ref import random_sparse, ref_conv

pytestmark = pytest.mark.gpu
RTOL = 1e-4


@pytest.fixture(scope="module")
def ME():
    import minsu3d_amd.MinkowskiEngine as me
    return me


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def check(name, got, want, tol):
    assert tuple(got.shape) == tuple(want.shape), (name, tuple(got.shape), tuple(want.shape))
    e = rel_err(got, want)
    print(f"{name}: rel err {e:.3e} (bound {tol:.0e})")
    assert e <= tol, (name, e)


# ---------------------------------------------------------------------------------------------- host restatements
def offsets_np(ks, dil, ts):
    i = np.arange(ks) - ((ks - 1) // 2 if ks % 2 else 0)
    return np.array([(x, y, z) for z in i for y in i for x in i], np.int64) * dil * ts


def dict_map(in_coords, out_coords, offsets):
    """nbr [K, Vout] by Python dict lookup (first occurrence of a coordinate wins)"""
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


def sorted_map(in_coords, out_coords, offsets):
    """the same table for large clouds: int64 keys, one searchsorted per offset"""
    def key(c):
        c = c.astype(np.int64)
        return (c[:, 0] << 48) | ((c[:, 1] + 32768) << 32) | ((c[:, 2] + 32768) << 16) | (c[:, 3] + 32768)
    kin = key(in_coords)
    order = np.argsort(kin, kind="stable")
    ks = kin[order]
    out = np.full((len(offsets), len(out_coords)), -1, np.int32)
    for k, off in enumerate(offsets):
        q = out_coords.astype(np.int64).copy()
        q[:, 1:] += off
        kq = key(q)
        pos = np.searchsorted(ks, kq)
        pos[pos >= len(ks)] = 0
        hit = ks[pos] == kq
        out[k, hit] = order[pos[hit]]
    return out


def dense_weight(W, ks):
    """W [K, Cin, Cout] with k = ix + ks iy + ks^2 iz -> [Cout, Cin, kx, ky, kz]"""
    cin, cout = W.shape[1], W.shape[2]
    return W.view(ks, ks, ks, cin, cout).permute(4, 3, 2, 1, 0).contiguous()


def densify64(coords, feats, B, G, unit, fill=0.0):
    d = torch.full((B, feats.shape[1], G, G, G), fill, dtype=torch.float64)
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


def dense_conv(coords, x, W, bias, ks, stride, dil, ts, out_coords, B, G):
    d = densify64(coords, x, B, G, ts)
    padt, p = pad_for(ks, dil)
    if padt is not None:
        d = F.pad(d, padt)
    y = F.conv3d(d, dense_weight(W, ks), None if bias is None else bias.view(-1), stride=stride, padding=p, dilation=dil)
    return read_dense(y, out_coords, ts * stride)


def manager_at(ME, coords, ts):
    cm = ME.CoordinateManager(torch.from_numpy(np.ascontiguousarray(coords)).cuda())
    t = 1
    while t < ts:
        cm.k2(t)
        t *= 2
    return cm


GEOMS = [(3, 1, 1), (3, 1, 2), (3, 1, 3), (5, 1, 1), (3, 2, 1), (2, 2, 1), (2, 2, 2), (4, 2, 1), (3, 2, 2)]


# ---------------------------------------------------------------------------------------------- 4. kernel maps
def _extreme_cloud(c):
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


@pytest.mark.parametrize("shift", ["none", "negative", "extreme"])
@pytest.mark.parametrize("ts", [1, 2])
def test_kernel_maps_exact(ME, ts, shift):
    rng = np.random.default_rng(7)
    c, _ = random_sparse(rng, B=2, grid=12, n=400, C=1)
    if shift == "negative":
        c = c.copy()
        c[:, 1:] -= 9
    elif shift == "extreme":
        c = _extreme_cloud(c)
        rng.shuffle(c)
    cm = manager_at(ME, c, ts)
    cin = cm.coords[ts].cpu().numpy()
    for ks, stride, dil in GEOMS:
        nbr_fwd, nbr_bwd, vin, vout, K, out_ts, mirror = cm.kernel_map(ts, ks, stride, dil)
        assert (vin, K, out_ts) == (cin.shape[0], ks ** 3, ts * stride)
        cout = cm.coords[out_ts].cpu().numpy()
        assert vout == cout.shape[0] and tuple(nbr_fwd.shape) == (K, vout)
        if stride == 2:      # the output set: floor to multiples of 2 ts, first-occurrence order
            q = cin.copy()
            q[:, 1:] = np.floor_divide(q[:, 1:], 2 * ts) * (2 * ts)
            _, first = np.unique(q, axis=0, return_index=True)
            assert np.array_equal(cout, q[np.sort(first)])
        want = dict_map(cin, cout, offsets_np(ks, dil, ts))
        assert np.array_equal(nbr_fwd.cpu().numpy(), want), (ks, stride, dil)
        inv = invert_np(want, vin)
        if stride == 1:
            assert mirror and nbr_bwd is nbr_fwd
            assert np.array_equal(want[::-1], inv)           # a submanifold map is its own inverse with mirrored offsets
        else:
            assert not mirror and tuple(nbr_bwd.shape) == (K, vin)
            assert np.array_equal(nbr_bwd.cpu().numpy(), inv), (ks, stride, dil)
        assert cm.kernel_map(ts, ks, stride, dil)[0] is nbr_fwd      # cached
        assert np.array_equal(cm.kernel_map_inverse(ts, ks, stride, dil).cpu().numpy(), inv)   # what a pooling backward walks
    assert cm.kernel_map(ts, 3, 1, 1)[0] is cm.k3(ts)
    down, up = cm.k2(ts)
    km = cm.kernel_map(ts, 2, 2, 1)
    assert km[0] is down and km[1] is up
    assert cm.kernel_map(ts, 1, 1, 1)[0] is cm.identity(ts)


def test_kernel_map_refusals(ME):
    rng = np.random.default_rng(3)
    c, _ = random_sparse(rng, B=2, grid=12, n=100, C=1)
    cm = manager_at(ME, c, 1)
    for ks, stride in ((2, 1), (3, 3), (4, 1)):
        with pytest.raises(NotImplementedError, match=f"kernel_size={ks}, stride={stride}"):
            cm.kernel_map(1, ks, stride, 1)


# ---------------------------------------------------------------------------------------------- 5. convolutions
def _conv_case(ME, ks, stride, dil, cin, cout, ts=1, seed=11, pending=False, B=2, G=12, n=400, coords=None):
    rng = np.random.default_rng(seed + 100 * ks + 10 * stride + dil + cin)
    if coords is None:
        coords, _ = random_sparse(rng, B=B, grid=G, n=n, C=1)
    cm = manager_at(ME, coords, ts)
    in_coords = cm.coords[ts].cpu().numpy()
    feats = rng.standard_normal((in_coords.shape[0], cin)).astype(np.float32)
    conv = ME.MinkowskiConvolution(cin, cout, kernel_size=ks, stride=stride, dilation=dil, bias=True, dimension=3).cuda()
    conv.train()
    xf = torch.from_numpy(feats).cuda().requires_grad_(True)
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
    out_ts = ts * stride
    assert y.tensor_stride == out_ts
    out_coords = cm.coords[out_ts].cpu().numpy()
    W64 = conv.kernel.detach().double().cpu().requires_grad_(True)
    bias64 = conv.bias.detach().double().cpu().requires_grad_(True)
    want = dense_conv(in_coords, a64, W64, bias64, ks, stride, dil, ts, out_coords, B, G // ts)
    tag = f"k{ks} s{stride} d{dil} ts{ts} {cin}->{cout}" + (" bn+relu" if pending else "")
    check(tag + " forward", y._F, want, RTOL)
    g = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y._F.backward(torch.from_numpy(g).cuda())
    want.backward(torch.from_numpy(g).double())
    check(tag + " backward-data", xf.grad, x64.grad, RTOL)
    check(tag + " backward-weight", conv.kernel.grad, W64.grad, RTOL)
    check(tag + " bias gradient", conv.bias.grad, bias64.grad.view(1, -1), RTOL)
    if pending:
        # (the BatchNorm parameters' own gradients are sums over all rows of products with the normalised activations, whose
        # float32 statistics differ from float64 ones: held to 1e-3, as the existing fused BatchNorm-backward checks hold them)
        check(tag + " dgamma", bn.bn.weight.grad, g64.grad, 1e-3)
        check(tag + " dbeta", bn.bn.bias.grad, b64.grad, 1e-3)


@pytest.mark.parametrize("cin,cout", [(6, 16), (16, 32), (32, 32)])
@pytest.mark.parametrize("ks,stride,dil", GEOMS)
def test_conv_against_dense(ME, ks, stride, dil, cin, cout):
    _conv_case(ME, ks, stride, dil, cin, cout)


@pytest.mark.parametrize("ks,stride,dil", [(3, 1, 2), (3, 2, 1), (5, 1, 1), (2, 2, 2)])
def test_conv_against_dense_tensor_stride_2(ME, ks, stride, dil):
    _conv_case(ME, ks, stride, dil, 16, 32, ts=2, n=900, G=16)


@pytest.mark.parametrize("ks,stride,dil", [(3, 2, 1), (3, 1, 2), (5, 1, 1)])
def test_conv_pending_bn_relu(ME, ks, stride, dil):
    _conv_case(ME, ks, stride, dil, 16, 32, pending=True)


def test_conv_wide_k3_s2_stays_off_the_submanifold_route(ME):
    """64 -> 64, kernel 3, stride 2, with enough output rows that the backward-weight route of the wide SUBMANIFOLD layers
    (three-piece bf16 operands: it splits Vout rows of the input) would be chosen by shape alone"""
    from minsu3d_amd.backend import get_backend
    lib = get_backend().lib
    rng = np.random.default_rng(5)
    G = 48
    coords, _ = random_sparse(rng, B=1, grid=G, n=40000, C=1)
    cm = manager_at(ME, coords, 1)
    vout = cm.kernel_map(1, 3, 2, 1)[3]
    assert lib.ms3d_spconv_wgrad_is_bf16x3(vout, 27, 64, 64, 0) == 1, vout      # what K == 27 alone would pick
    assert lib.ms3d_spconv_wgrad_is_bf16x3_g(vout, 27, 64, 64, 0, 0) == 0
    assert lib.ms3d_spconv_wgrad_is_bf16x3_g(vout, 27, 64, 64, 0, 1) == 1
    _conv_case(ME, 3, 2, 1, 64, 64, B=1, G=G, coords=coords)


# ---------------------------------------------------------------------------------------------- 6. large K
def _transpose_case(ME, ks, dil, cin, cout, B=2, G=12, n=400, seed=23):
    rng = np.random.default_rng(seed + ks + cin)
    coords, _ = random_sparse(rng, B=B, grid=G, n=n, C=1)
    cm = manager_at(ME, coords, 2)
    vc = cm.size(2)
    feats = rng.standard_normal((vc, cin)).astype(np.float32)
    xf = torch.from_numpy(feats).cuda().requires_grad_(True)
    conv = ME.MinkowskiConvolutionTranspose(cin, cout, kernel_size=ks, stride=2, dilation=dil, dimension=3).cuda()
    y = conv(ME.SparseTensor(xf, coordinate_manager=cm, tensor_stride=2))
    assert y.tensor_stride == 1 and y._F.size(0) == coords.shape[0]
    x64 = torch.from_numpy(feats).double().requires_grad_(True)
    W64 = conv.kernel.detach().double().cpu().requires_grad_(True)
    # out[2c + i * dil - p] += x[c] W[i]: the transpose of the strided convolution with front padding p; an even kernel has
    # none, and what reaches beyond the fine grid is never read
    d = densify64(cm.coords[2].cpu().numpy(), x64, B, G // 2, 2)
    _, p = pad_for(ks, dil)
    yd = F.conv_transpose3d(d, dense_weight(W64, ks).transpose(0, 1), stride=2, dilation=dil)[..., p:p + G, p:p + G, p:p + G]
    want = read_dense(yd, coords, 1)
    tag = f"transposed k{ks} s2 d{dil} {cin}->{cout}"
    check(tag + " forward", y._F, want, RTOL)
    g = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y._F.backward(torch.from_numpy(g).cuda())
    want.backward(torch.from_numpy(g).double())
    check(tag + " backward-data", xf.grad, x64.grad, RTOL)
    check(tag + " backward-weight", conv.kernel.grad, W64.grad, RTOL)


@pytest.mark.parametrize("cin,cout", [(16, 16), (32, 48)])
def test_large_k_dense(ME, cin, cout):
    _conv_case(ME, 5, 1, 1, cin, cout, seed=31)
    _transpose_case(ME, 4, 1, cin, cout)
    _transpose_case(ME, 2, 1, cin, cout)
    _transpose_case(ME, 3, 1, cin, cout)


def test_large_k_large_table(ME):
    """40 000 rows in a 64^3 grid: above the row count where K <= 27 tables get pair lists -- K = 125 / 64 must fall through
    to the table walk.  Yardstick: ref_conv in float64 over a host-built table."""
    rng = np.random.default_rng(41)
    coords, _ = random_sparse(rng, B=1, grid=64, n=40000, C=1)
    cm = manager_at(ME, coords, 2)
    feats = rng.standard_normal((40000, 16)).astype(np.float32)
    xf = torch.from_numpy(feats).cuda().requires_grad_(True)
    conv = ME.MinkowskiConvolution(16, 16, kernel_size=5, dimension=3).cuda()
    y = conv(ME.SparseTensor(xf, coordinate_manager=cm))
    nbr = sorted_map(coords, coords, offsets_np(5, 1, 1))
    assert np.array_equal(cm.kernel_map(1, 5, 1, 1)[0].cpu().numpy(), nbr)
    x64 = torch.from_numpy(feats).double().requires_grad_(True)
    W64 = conv.kernel.detach().double().cpu().requires_grad_(True)
    want = ref_conv(x64, W64, torch.from_numpy(nbr))
    check("k5 40k rows forward", y._F, want, RTOL)
    g = rng.standard_normal((40000, 16)).astype(np.float32)
    y._F.backward(torch.from_numpy(g).cuda())
    want.backward(torch.from_numpy(g).double())
    check("k5 40k rows backward-data", xf.grad, x64.grad, RTOL)
    check("k5 40k rows backward-weight", conv.kernel.grad, W64.grad, RTOL)
    # transposed kernel 4, stride 2, 32 -> 48, onto the 40 000 fine rows
    cc = cm.coords[2].cpu().numpy()
    up = invert_np(sorted_map(coords, cc, offsets_np(4, 1, 1)), 40000)       # inverse of the strided map fine -> coarse
    feats = rng.standard_normal((cc.shape[0], 32)).astype(np.float32)
    xf = torch.from_numpy(feats).cuda().requires_grad_(True)
    conv = ME.MinkowskiConvolutionTranspose(32, 48, kernel_size=4, stride=2, dimension=3).cuda()
    y = conv(ME.SparseTensor(xf, coordinate_manager=cm, tensor_stride=2))
    x64 = torch.from_numpy(feats).double().requires_grad_(True)
    W64 = conv.kernel.detach().double().cpu().requires_grad_(True)
    want = ref_conv(x64, W64, torch.from_numpy(up))
    check("transposed k4 40k rows forward", y._F, want, RTOL)
    g = rng.standard_normal((40000, 48)).astype(np.float32)
    y._F.backward(torch.from_numpy(g).cuda())
    want.backward(torch.from_numpy(g).double())
    check("transposed k4 40k rows backward-data", xf.grad, x64.grad, RTOL)
    check("transposed k4 40k rows backward-weight", conv.kernel.grad, W64.grad, RTOL)


# ---------------------------------------------------------------------------------------------- 7. pooling
@pytest.mark.parametrize("C_", [5, 16, 33])
@pytest.mark.parametrize("ks,stride", [(2, 2), (3, 2), (3, 1)])
@pytest.mark.parametrize("mode", ["max", "avg", "sum"])
def test_pooling_against_dense(ME, mode, ks, stride, C_):
    B, G = 2, 12
    rng = np.random.default_rng(50 + ks + stride + C_)
    coords, _ = random_sparse(rng, B=B, grid=G, n=400, C=1)
    feats = rng.standard_normal((400, C_)).astype(np.float32)
    cm = manager_at(ME, coords, 1)
    xf = torch.from_numpy(feats).cuda().requires_grad_(True)
    layer = {"max": ME.MinkowskiMaxPooling, "avg": ME.MinkowskiAvgPooling, "sum": ME.MinkowskiSumPooling}[mode](
        kernel_size=ks, stride=stride, dimension=3)
    y = layer(ME.SparseTensor(xf, coordinate_manager=cm))
    assert y.tensor_stride == stride
    out_coords = cm.coords[stride].cpu().numpy()
    x64 = torch.from_numpy(feats).double().requires_grad_(True)
    p = (ks - 1) // 2 if ks % 2 else 0
    if mode == "max":
        nbr = cm.kernel_map(1, ks, stride, 1)[0].long().cpu()
        vals = torch.cat([x64.detach(), torch.full((1, C_), -np.inf, dtype=torch.float64)])[nbr]      # [K, Vout, C]
        assert int((vals == vals.max(0).values).sum(0).max()) == 1, "a tie in a max: the draw is not what it should be"
        d = densify64(coords, x64, B, G, 1, fill=-np.inf)
        want = read_dense(F.max_pool3d(d, ks, stride=stride, padding=p), out_coords, stride)
    else:
        d = densify64(coords, x64, B, G, 1)
        want = read_dense(F.avg_pool3d(d, ks, stride=stride, padding=p, divisor_override=1), out_coords, stride)
        if mode == "avg":
            occ = densify64(coords, torch.ones(400, 1, dtype=torch.float64), B, G, 1)
            cnt = read_dense(F.avg_pool3d(occ, ks, stride=stride, padding=p, divisor_override=1), out_coords, stride)
            assert float(cnt.min()) >= 1
            want = want / cnt
    tag = f"{mode} pool k{ks} s{stride} C{C_}"
    if mode == "max":
        assert torch.equal(y._F.detach().cpu(), want.detach().float()), tag
    else:
        check(tag + " forward", y._F, want, 1e-6)
    g = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y._F.backward(torch.from_numpy(g).cuda())
    want.backward(torch.from_numpy(g).double())
    if mode == "max" and (ks, stride) == (2, 2):
        assert torch.equal(xf.grad.cpu(), x64.grad.float()), tag
    else:
        check(tag + " backward", xf.grad, x64.grad, 1e-6)


def test_pooling_materialises_pending(ME):
    rng = np.random.default_rng(61)
    coords, feats = random_sparse(rng, B=2, grid=12, n=400, C=16)
    x = ME.SparseTensor(torch.from_numpy(feats).cuda(), torch.from_numpy(coords).cuda())
    bn = ME.MinkowskiBatchNorm(16).cuda().train()
    h = ME.MinkowskiReLU()(bn(x))
    assert h._pending is not None
    y = ME.MinkowskiMaxPooling(kernel_size=2, stride=2, dimension=3)(h)
    a = torch.relu(F.batch_norm(torch.from_numpy(feats).double(), None, None, bn.bn.weight.detach().double().cpu(),
                                bn.bn.bias.detach().double().cpu(), True, 0.1, 1e-5))
    d = densify64(coords, a, 2, 12, 1, fill=-np.inf)
    want = read_dense(F.max_pool3d(d, 2, stride=2), x.coordinate_manager.coords[2].cpu().numpy(), 2)
    check("max pool behind a pending BN+ReLU", y._F, want, 1e-5)


@pytest.mark.parametrize("C_", [5, 16])
@pytest.mark.parametrize("mode", ["max", "avg", "sum"])
def test_global_pooling(ME, mode, C_):
    rng = np.random.default_rng(70 + C_)
    coords, _ = random_sparse(rng, B=3, grid=12, n=500, C=1)      # shuffled: rows are NOT batch-contiguous
    coords[:, 0] *= 2                                           # batch indices 0, 2, 4: only the present ones give a row
    feats = rng.standard_normal((500, C_)).astype(np.float32)
    xf = torch.from_numpy(feats).cuda().requires_grad_(True)
    layer = {"max": ME.MinkowskiGlobalMaxPooling, "avg": ME.MinkowskiGlobalAvgPooling,
             "sum": ME.MinkowskiGlobalSumPooling}[mode]()
    y = layer(ME.SparseTensor(xf, torch.from_numpy(coords).cuda()))
    x64 = torch.from_numpy(feats).double().requires_grad_(True)
    b = torch.from_numpy(coords[:, 0]).long()
    rows = []
    for bi in (0, 2, 4):
        seg = x64[b == bi]
        rows.append(seg.max(0).values if mode == "max" else seg.mean(0) if mode == "avg" else seg.sum(0))
    want = torch.stack(rows)
    assert y.C[:, 0].tolist() == [0, 2, 4]
    if mode == "max":
        assert torch.equal(y.F.detach().cpu(), want.detach().float())
    else:
        check(f"global {mode} forward", y.F, want, 1e-5)
    g = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y.F.backward(torch.from_numpy(g).cuda())
    want.backward(torch.from_numpy(g).double())
    check(f"global {mode} backward", xf.grad, x64.grad, 1e-5)


# ---------------------------------------------------------------------------------------------- 8 / 9. a network
class _Net(torch.nn.Module):
    """5x5x5 stem, two dilated residual blocks, a k3 s2 step, max pooling, transposed k2 s2 (twice, back to stride 1), ME.cat
    with the stem's output, 1x1 head with bias, global average pooling"""

    def __init__(self, ME, cin=6, c=16, ncls=5):
        super().__init__()
        self.ME = ME
        conv, bn = ME.MinkowskiConvolution, ME.MinkowskiBatchNorm
        self.stem = conv(cin, c, kernel_size=5, dimension=3)
        self.blocks = torch.nn.ModuleList()
        for dil in (2, 3):
            self.blocks.append(torch.nn.ModuleList([bn(c), conv(c, c, kernel_size=3, dilation=dil, dimension=3),
                                                    bn(c), conv(c, c, kernel_size=3, dilation=dil, dimension=3)]))
        self.bn_down = bn(c)
        self.down = conv(c, 2 * c, kernel_size=3, stride=2, dimension=3)
        self.pool = ME.MinkowskiMaxPooling(kernel_size=2, stride=2, dimension=3)
        self.bn_up1 = bn(2 * c)
        self.up1 = ME.MinkowskiConvolutionTranspose(2 * c, 2 * c, kernel_size=2, stride=2, dimension=3)
        self.bn_up0 = bn(2 * c)
        self.up0 = ME.MinkowskiConvolutionTranspose(2 * c, c, kernel_size=2, stride=2, dimension=3)
        self.bn_head = bn(2 * c)
        self.head = conv(2 * c, ncls, kernel_size=1, bias=True, dimension=3)
        self.gpool = ME.MinkowskiGlobalAvgPooling()

    def forward(self, x):
        ME, relu = self.ME, self.ME.MinkowskiReLU()
        s = self.stem(x)
        h = s
        for bn0, c0, bn1, c1 in self.blocks:
            h = h + c1(relu(bn1(c0(relu(bn0(h))))))
        d = self.down(relu(self.bn_down(h)))                 # stride 2
        p = self.pool(d)                                     # stride 4
        u = self.up1(relu(self.bn_up1(p)))                   # stride 2
        u = self.up0(relu(self.bn_up0(u + d)))               # stride 1
        z = self.head(relu(self.bn_head(ME.cat(u, s))))
        return z, self.gpool(z)

    def reference(self, feats, cm):
        """the same network layer by layer in float64: ref_conv / F.batch_norm over the engine's OWN tables"""
        P = {n: p.detach().double().cpu() for n, p in self.named_parameters()}

        def conv(name, x, ts, ks, stride=1, dil=1, transpose=False):
            nbr = cm.kernel_map(ts // 2, ks, 2, dil)[1] if transpose else cm.kernel_map(ts, ks, stride, dil)[0]
            W = P[name + ".kernel"]
            y = ref_conv(x, W.view(nbr.size(0), W.shape[-2], W.shape[-1]), nbr.cpu())
            return y + P[name + ".bias"] if name + ".bias" in P else y

        def bnrelu(name, x):
            return torch.relu(F.batch_norm(x, None, None, P[name + ".bn.weight"], P[name + ".bn.bias"], True, 0.1, 1e-5))

        s = conv("stem", feats.double(), 1, 5)
        h = s
        for i, dil in enumerate((2, 3)):
            t = conv(f"blocks.{i}.1", bnrelu(f"blocks.{i}.0", h), 1, 3, dil=dil)
            h = h + conv(f"blocks.{i}.3", bnrelu(f"blocks.{i}.2", t), 1, 3, dil=dil)
        d = conv("down", bnrelu("bn_down", h), 1, 3, stride=2)
        nbr = cm.kernel_map(2, 2, 2, 1)[0].long().cpu()
        p = torch.cat([d, torch.full((1, d.size(1)), -np.inf, dtype=torch.float64)])[nbr].max(0).values
        u = conv("up1", bnrelu("bn_up1", p), 4, 2, transpose=True)
        u = conv("up0", bnrelu("bn_up0", u + d), 2, 2, transpose=True)
        z = conv("head", bnrelu("bn_head", torch.cat([u, s], 1)), 1, 1)
        b = cm.coords[1][:, 0].long().cpu()
        return z, torch.stack([z[b == i].mean(0) for i in sorted(set(b.tolist()))])


def _net_step(ME, net, coords, feats):
    net.zero_grad(set_to_none=True)
    xf = torch.from_numpy(feats).cuda().requires_grad_(True)
    x = ME.SparseTensor(xf, torch.from_numpy(coords).cuda())
    z, gp = net(x)
    loss = (z.F * z.F).mean() + gp.F.sum()
    loss.backward()
    torch.cuda.synchronize()
    res = {"z": z.F.detach().clone(), "gp": gp.F.detach().clone(), "dx": xf.grad.clone()}
    res.update({"grad/" + n: p.grad.clone() for n, p in net.named_parameters()})
    return res, x.coordinate_manager


def test_network_reproducible_and_composed(ME):
    torch.manual_seed(0)
    rng = np.random.default_rng(81)
    coords, feats = random_sparse(rng, B=2, grid=16, n=1500, C=6)
    net = _Net(ME).cuda().train()
    a, cm = _net_step(ME, net, coords, feats)
    b, _ = _net_step(ME, net, coords, feats)
    diff = [k for k in a if not torch.equal(a[k], b[k])]
    assert not diff, f"not bit-reproducible: {diff}"
    for n, p in net.named_parameters():
        g = a["grad/" + n]
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0, n
    assert torch.isfinite(a["dx"]).all() and float(a["dx"].abs().max()) > 0
    z64, gp64 = net.reference(torch.from_numpy(feats), cm)
    check("network output", a["z"], z64, RTOL)
    check("network global average", a["gp"], gp64, RTOL)
