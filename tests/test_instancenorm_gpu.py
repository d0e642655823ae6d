"""GPU: MinkowskiInstanceNorm / MinkowskiStableInstanceNorm (csrc/inorm.hip) -- the segmented statistics, the row pass and the
backward, and the activation table behind them.

The yardstick for values is never this engine: torch.nn.functional.instance_norm in float64 on the CPU, applied per batch
index to x_b.T[None] with the same float32-rounded inputs, the layer's eps, weight and bias; gradients come from autograd
through that graph under a random dy.  (A batch index with ONE row is outside what torch's operator accepts; there the graph
is its limit, y = 0 * x * weight + bias: variance 0, xhat = 0.)  Bound: the project's bar, 1e-4 of the reference tensor's largest
magnitude, for y, dx, dweight and dbias alike; the measured error of every comparison is printed.  The small helpers (cloud,
densify, dense convolution) are this file's own copies.

Two rows in a segment are why the kernels sum and normalise in float64 (rows stay float32): there xhat = +-(1 - d) with
d = 2 eps / (x1 - x2)^2 and the true dx is about 1e-8 of the two terms it is the difference of, which float32 statistics
cannot resolve (measured with float32 arithmetic on the GPU: 1.4e-1 of the reference at C = 1).  The bound is the same 1e-4."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
RTOL = 1e-4
CHANNELS = [1, 3, 4, 20, 64, 66, 132]


@pytest.fixture(scope="module")
def ME():
    import minsu3d_amd.MinkowskiEngine as me
    return me


@pytest.fixture(scope="module")
def be():
    from minsu3d_amd.backend import get_backend
    return get_backend()


@pytest.fixture(scope="module")
def S(be):
    return int(be.lib.ms3d_inorm_slices())


# ---------------------------------------------------------------------------------------------- helpers (own copies)
def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def check(name, got, want, tol=RTOL):
    assert tuple(got.shape) == tuple(want.shape), (name, tuple(got.shape), tuple(want.shape))
    e = rel_err(got, want)
    print(f"{name}: rel err {e:.3e} (bound {tol:.0e})")
    assert e <= tol, (name, e)


def cloud(rng, lengths, batch_ids=None, G=16):
    """sum(lengths) distinct (b, x, y, z) rows, lengths[i] of them in the G^3 grid of batch index batch_ids[i], handed over in
    random order (interleaved across the batch indices)"""
    batch_ids = list(range(len(lengths))) if batch_ids is None else batch_ids
    rows = []
    for b, n in zip(batch_ids, lengths):
        cells = rng.choice(G ** 3, size=n, replace=False)
        x, rest = np.divmod(cells, G * G)
        y, z = np.divmod(rest, G)
        rows.append(np.stack([np.full(n, b), x, y, z], 1))
    rows = np.concatenate(rows).astype(np.int32)
    return rows[rng.permutation(rows.shape[0])]


def reference(x64, batch, eps, w64, b64):
    """float64 rows [V, C] (autograd), batch index per row -> instance_norm per batch index, rows where they were"""
    batch = torch.as_tensor(np.asarray(batch)).long()
    pieces, where = [], []
    for b in torch.unique(batch).tolist():
        idx = torch.nonzero(batch == b).view(-1)
        xb = x64[idx]
        if idx.numel() == 1:
            yb = 0.0 * xb * w64.view(1, -1) + b64.view(1, -1)
        else:
            yb = F.instance_norm(xb.t()[None], weight=w64.view(-1), bias=b64.view(-1), use_input_stats=True, eps=eps)[0].t()
        pieces.append(yb)
        where.append(idx)
    inv = torch.empty(batch.numel(), dtype=torch.long)
    inv[torch.cat(where)] = torch.arange(batch.numel())
    return torch.cat(pieces)[inv]


def manager_of(ME, coords, kind="plain"):
    c = torch.from_numpy(np.ascontiguousarray(coords)).cuda()
    if kind == "rooted":
        return ME.CoordinateManager.rooted(c, 1)
    if kind == "sorted":
        cm = ME.CoordinateManager(c, spatial_sort=True)
        assert cm.perm is not None, "the cloud is too small to be Morton-sorted"
        return cm
    return ME.CoordinateManager(c)


def make_layer(ME, C, cls="MinkowskiInstanceNorm", eps=None, seed=0):
    layer = getattr(ME, cls)(C) if eps is None else getattr(ME, cls)(C, eps=eps)
    g = torch.Generator().manual_seed(100 + seed)
    with torch.no_grad():
        layer.weight.copy_(torch.rand((1, C), generator=g) + 0.5)
        layer.bias.copy_(torch.rand((1, C), generator=g) * 0.6 - 0.3)
    return layer.cuda()


def features(rng, V, C, mean=0.0):
    return (mean + rng.standard_normal((V, C))).astype(np.float32)


def run_case(ME, coords, C, cls="MinkowskiInstanceNorm", eps=None, kind="plain", seed=0, tag=None, needs=(True, True),
             mean=0.0, only=("y", "dx", "dw", "db")):
    """the layer on `coords` (caller order) against the float64 graph: forward and every gradient asked for
    -> dict of the engine's results, rows in CALLER order"""
    rng = np.random.default_rng(7 * C + seed)
    V = coords.shape[0]
    feats = features(rng, V, C, mean)
    layer = make_layer(ME, C, cls, eps, seed)
    x_grad, p_grad = needs
    layer.weight.requires_grad_(p_grad)
    layer.bias.requires_grad_(p_grad)
    cm = manager_of(ME, coords, kind)
    xf = torch.from_numpy(feats).cuda().requires_grad_(x_grad)
    xin = ME.SparseTensor(xf if cm.perm is None else xf[cm.perm], coordinate_manager=cm, tensor_stride=1)
    y = layer(xin)
    assert y.tensor_stride == 1 and y.coordinate_manager is cm and y._pending is None
    yf = y.features
    assert yf.dtype == torch.float32 and tuple(yf.shape) == (V, C)
    x64 = torch.from_numpy(feats).double().requires_grad_(True)
    w64 = layer.weight.detach().double().cpu().requires_grad_(True)
    b64 = layer.bias.detach().double().cpu().requires_grad_(True)
    want = reference(x64, coords[:, 0], layer.eps, w64, b64)
    tag = tag or f"{cls} C{C} V{V} {kind}"
    if "y" in only:
        check(tag + " forward", yf, want)
    g = rng.standard_normal((V, C)).astype(np.float32)
    res = dict(y=yf.detach(), layer=layer, feats=feats, dy=g)
    if not (x_grad or p_grad):
        return res
    yf.backward(torch.from_numpy(g).cuda())
    want.backward(torch.from_numpy(g).double())
    res.update(want_y=want.detach(), want_dx=x64.grad, want_dw=w64.grad, want_db=b64.grad)
    if x_grad:
        if "dx" in only:
            check(tag + " dx", xf.grad, x64.grad)
        res["dx"] = xf.grad
    else:
        assert xf.grad is None
    if p_grad:
        assert tuple(layer.weight.grad.shape) == (1, C) and tuple(layer.bias.grad.shape) == (1, C)
        if "dw" in only:
            check(tag + " dweight", layer.weight.grad, w64.grad)
        if "db" in only:
            check(tag + " dbias", layer.bias.grad, b64.grad)
        res["dw"], res["db"] = layer.weight.grad, layer.bias.grad
    else:
        assert layer.weight.grad is None and layer.bias.grad is None
    return res


def seg_length(name, S):
    return {"1": 1, "2": 2, "S-1": S - 1, "S": S, "S+1": S + 1, "2S+1": 2 * S + 1, "3000": 3000}[name]


# ---------------------------------------------------------------------------------------------- 1. lengths x channels
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("n", ["1", "2", "S-1", "S", "S+1", "2S+1", "3000"])
def test_one_batch_segment_lengths(ME, S, n, C):
    """B = 1.  1, 2, S - 1: empty slices and one-row slices; S, S + 1, 2S + 1: full, ragged last slice (S + 1 rows make
    slices of 2 rows, most of them empty); 3000: several rows per thread on the wide rows.  C = 1, 3: a partly filled lane;
    4, 20, 64: 16-byte lanes; 66: guarded lanes, 17 per row; 132: two column passes."""
    V = seg_length(n, S)
    coords = cloud(np.random.default_rng(11 + V), [V])
    res = run_case(ME, coords, C)
    if V == 1:
        assert torch.equal(res["y"], res["layer"].bias.detach())
        assert bool((res["dx"] == 0).all())


@pytest.mark.parametrize("C", CHANNELS)
def test_three_batches_unequal_interleaved(ME, S, C):
    """batch indices 0, 2, 5 (not consecutive), S + 1, 1 and 700 rows, handed over interleaved; the one-row segment gives
    y = bias and dx = 0 exactly"""
    coords = cloud(np.random.default_rng(13), [S + 1, 1, 700], [0, 2, 5])
    assert not np.all(np.diff(coords[:, 0]) >= 0), "the rows must not be batch-contiguous"
    res = run_case(ME, coords, C)
    lone = int(np.nonzero(coords[:, 0] == 2)[0][0])
    assert torch.equal(res["y"][lone], res["layer"].bias.detach().view(-1))
    assert bool((res["dx"][lone] == 0).all())
    assert bool((res["dx"] != 0).any())


# ---------------------------------------------------------------------------------------------- 2. unaligned rows
def test_unaligned_rows_take_the_scalar_route(ME, be, S):
    """C = 4 rows carved 8 bytes into a buffer are contiguous but not 16-byte aligned: the guarded 4-byte route runs and gives
    the bits of the 16-byte one, forward and backward"""
    rng = np.random.default_rng(17)
    coords = cloud(rng, [S + 1, 1, 700], [0, 2, 5])
    V = coords.shape[0]
    cm = manager_of(ME, coords)
    group = cm.batch_group(1)
    x = torch.from_numpy(features(rng, V, 4)).cuda()
    dy = torch.from_numpy(features(rng, V, 4)).cuda()
    w = torch.from_numpy(features(rng, 1, 4)).cuda()
    b = torch.from_numpy(features(rng, 1, 4)).cuda()
    flat = torch.zeros(V * 4 + 2, dtype=torch.float32, device="cuda")
    xu = flat[2:].view(V, 4)
    xu.copy_(x)
    assert x.data_ptr() % 16 == 0 and xu.data_ptr() % 16 == 8 and xu.is_contiguous()
    ya, ma, ia = be.inorm_forward(x, group, 1e-5, w, b)
    yu, mu, iu = be.inorm_forward(xu, group, 1e-5, w, b)
    assert torch.equal(ya, yu) and torch.equal(ma, mu) and torch.equal(ia, iu)
    ga = be.inorm_backward(dy, x, group, ma, ia, w)
    gu = be.inorm_backward(dy, xu, group, mu, iu, w)
    for a, u in zip(ga, gu):
        assert torch.equal(a, u)
    x64 = x.double().cpu().requires_grad_(True)
    want = reference(x64, coords[:, 0], 1e-5, w.double().cpu(), b.double().cpu())
    check("unaligned forward", yu, want)
    want.backward(dy.double().cpu())
    check("unaligned dx", gu[0], x64.grad)


# ---------------------------------------------------------------------------------------------- 3. managers
@pytest.mark.parametrize("kind", ["plain", "sorted", "rooted"])
def test_managers(ME, kind):
    """4200 rows over the batch indices 0 and 3 (the engine Morton-sorts from 4096 rows on; the sorted manager holds the rows
    in its own order, the results are compared in the caller's)"""
    coords = cloud(np.random.default_rng(19), [2300, 1900], [0, 3])
    run_case(ME, coords, 20, kind=kind)


def _norm_alone(ME, layer, t, batch, tag, rng):
    """the layer on the engine's own rows of `t` (a leaf made of them) against the float64 graph of those rows"""
    rows = t._raw().detach().clone().requires_grad_(True)
    y = layer(t._like(rows))
    assert y.tensor_stride == t.tensor_stride and y.coordinate_manager is t.coordinate_manager
    x64 = rows.detach().double().cpu().requires_grad_(True)
    w64 = layer.weight.detach().double().cpu().requires_grad_(True)
    b64 = layer.bias.detach().double().cpu().requires_grad_(True)
    want = reference(x64, batch, layer.eps, w64, b64)
    check(tag + " forward", y._F, want)
    g = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y._F.backward(torch.from_numpy(g).cuda())
    want.backward(torch.from_numpy(g).double())
    check(tag + " dx", rows.grad, x64.grad)
    check(tag + " dweight", layer.weight.grad, w64.grad)
    check(tag + " dbias", layer.bias.grad, b64.grad)
    return y


def test_behind_a_stride_2_convolution(ME):
    """tensor stride 2: the grouping of the coarse set.  The float64 reference takes the engine's own input rows to the norm
    layer (the norm alone is under test)."""
    rng = np.random.default_rng(23)
    coords = cloud(rng, [500, 300, 40], [0, 1, 4])
    cm = manager_of(ME, coords)
    conv = ME.MinkowskiConvolution(6, 20, kernel_size=2, stride=2, dimension=3).cuda()
    x = ME.SparseTensor(torch.from_numpy(features(rng, coords.shape[0], 6)).cuda(), coordinate_manager=cm)
    with torch.no_grad():
        h = conv(x)
    assert h.tensor_stride == 2
    batch = cm.coords[2][:, 0].cpu().numpy()
    y = _norm_alone(ME, make_layer(ME, 20), h, batch, "behind stride 2", rng)
    assert y.tensor_stride == 2 and torch.equal(y.coordinates, h.coordinates)


def test_pending_batchnorm_relu_in_front(ME):
    """MinkowskiBatchNorm -> MinkowskiReLU leave the normalisation pending; the layer materialises it (x._raw()) and gives
    exactly what it gives on the materialised rows, which are held to the float64 graph"""
    rng = np.random.default_rng(29)
    C = 20
    coords = cloud(rng, [400, 250], [0, 1])
    cm = manager_of(ME, coords)
    bn = ME.MinkowskiBatchNorm(C).cuda().train()
    with torch.no_grad():
        bn.bn.weight.uniform_(0.5, 1.5)
        bn.bn.bias.uniform_(-0.3, 0.3)
    layer = make_layer(ME, C)
    xf = torch.from_numpy(features(rng, coords.shape[0], C)).cuda()
    with torch.no_grad():
        t = ME.MinkowskiReLU()(bn(ME.SparseTensor(xf, coordinate_manager=cm)))
        assert t._pending is not None and t._pending["relu"]
        y = layer(t)
        assert y._pending is None
        t2 = ME.MinkowskiReLU()(bn(ME.SparseTensor(xf, coordinate_manager=cm)))
        rows = t2._raw()
    y2 = _norm_alone(ME, layer, t2._like(rows), coords[:, 0], "behind bn+relu", rng)
    assert torch.equal(y._F, y2._F.detach())


# ---------------------------------------------------------------------------------------------- 4. offset inputs
@pytest.mark.parametrize("C", [4, 3])
@pytest.mark.parametrize("n", ["S+1", "3000"])
def test_offset_inputs(ME, S, n, C):
    """mean 100, standard deviation 1 per channel: E[x^2] - E[x]^2 of the raw float32 values misses the bound by more than
    10x here; the shifted slice sums merged by Chan's formula must hold it, forward and dx"""
    V = seg_length(n, S)
    coords = cloud(np.random.default_rng(31 + V), [V])
    run_case(ME, coords, C, mean=100.0, tag=f"offset C{C} V{V}", only=("y", "dx"))


# ---------------------------------------------------------------------------------------------- 5. the two classes, eps
@pytest.mark.parametrize("cls,eps", [("MinkowskiInstanceNorm", None), ("MinkowskiStableInstanceNorm", None),
                                     ("MinkowskiInstanceNorm", 1e-2), ("MinkowskiStableInstanceNorm", 0.5)])
def test_classes_and_eps(ME, cls, eps):
    coords = cloud(np.random.default_rng(37), [300, 200], [0, 1])
    res = run_case(ME, coords, 20, cls=cls, eps=eps)
    want_eps = eps if eps is not None else {"MinkowskiInstanceNorm": 1e-8, "MinkowskiStableInstanceNorm": 1e-6}[cls]
    assert res["layer"].eps == want_eps
    if eps is not None:
        # a non-default eps is visible: the same rows under the default differ by far more than the bound
        other = run_case(ME, coords, 20, cls=cls, only=())
        assert rel_err(other["y"], res["want_y"]) > 10 * RTOL


def test_train_and_eval_give_the_same_bytes(ME):
    coords = cloud(np.random.default_rng(41), [300, 200], [0, 1])
    cm = manager_of(ME, coords)
    layer = make_layer(ME, 20)
    x = ME.SparseTensor(torch.from_numpy(features(np.random.default_rng(43), 500, 20)).cuda(), coordinate_manager=cm)
    with torch.no_grad():
        a = layer.train()(x)._F
        b = layer.eval()(x)._F
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- 6. needs_input_grad
def test_frozen_affine_and_input_without_grad(ME, S):
    coords = cloud(np.random.default_rng(47), [S + 1, 1, 700], [0, 2, 5])
    full = run_case(ME, coords, 20)
    frozen = run_case(ME, coords, 20, needs=(True, False))
    assert "dw" not in frozen and frozen["layer"].weight.grad is None and frozen["layer"].bias.grad is None
    assert torch.equal(frozen["dx"], full["dx"])
    no_dx = run_case(ME, coords, 20, needs=(False, True))
    assert "dx" not in no_dx
    assert torch.equal(no_dx["dw"], full["dw"]) and torch.equal(no_dx["db"], full["db"])


# ---------------------------------------------------------------------------------------------- 7. bit-reproducibility
def test_bit_reproducible(ME, S):
    coords = cloud(np.random.default_rng(53), [2 * S + 1, 1, 3000], [0, 2, 5])
    a = run_case(ME, coords, 20, seed=5)
    b = run_case(ME, coords, 20, seed=5)
    for name in ("y", "dx", "dw", "db"):
        assert torch.equal(a[name], b[name]), name


# ---------------------------------------------------------------------------------------------- 8. many rows per thread
@pytest.mark.parametrize("C", [132, 8])
def test_long_segments_through_the_backend(be, S, C):
    """20000 and 9000 rows in two interleaved segments, straight through the backend (no coordinates are needed for the
    grouping): on 132 channels a thread walks more rows than it keeps in flight, so the row loop comes round again"""
    from minsu3d_amd.backend import BatchGroup
    rng = np.random.default_rng(59 + C)
    batch = np.concatenate([np.zeros(20000, np.int64), np.ones(9000, np.int64)])
    rng.shuffle(batch)
    V = batch.size
    bt = torch.from_numpy(batch).cuda()
    order = torch.sort(bt, stable=True).indices
    offsets = torch.tensor([0, 20000, V], dtype=torch.int32, device="cuda")
    group = BatchGroup.from_tensors(order, offsets, bt.to(torch.int32))
    x = torch.from_numpy(features(rng, V, C)).cuda()
    dy = torch.from_numpy(features(rng, V, C)).cuda()
    w = torch.from_numpy(features(rng, 1, C)).cuda()
    b = torch.from_numpy(features(rng, 1, C)).cuda()
    y, mean, invstd = be.inorm_forward(x, group, 1e-5, w, b)
    dx, dw, db = be.inorm_backward(dy, x, group, mean, invstd, w)
    x64 = x.double().cpu().requires_grad_(True)
    w64, b64 = w.double().cpu().requires_grad_(True), b.double().cpu().requires_grad_(True)
    want = reference(x64, batch, 1e-5, w64, b64)
    want.backward(dy.double().cpu())
    tag = f"long segments C{C}"
    check(tag + " forward", y, want)
    check(tag + " dx", dx, x64.grad)
    check(tag + " dweight", dw.view(1, -1), w64.grad)
    check(tag + " dbias", db.view(1, -1), b64.grad)
    # no affine: weight 1, bias 0
    y1, _, _ = be.inorm_forward(x, group, 1e-5, None, None)
    one, zero = torch.ones(1, C, dtype=torch.float64), torch.zeros(1, C, dtype=torch.float64)
    check(tag + " forward without affine", y1, reference(x.double().cpu(), batch, 1e-5, one, zero))


# ---------------------------------------------------------------------------------------------- 9. the composed formulation
def composed_instance_norm(ME, x, weight, bias, eps):
    """the layer's arithmetic from the existing layers: global average pooling, broadcast addition / multiplication"""
    pool, add, mul = ME.MinkowskiGlobalAvgPooling(), ME.MinkowskiBroadcastAddition(), ME.MinkowskiBroadcastMultiplication()
    mean = pool(x)
    centred = add(x, mean._like(-mean._F))
    var = pool(centred._like(centred._F * centred._F))
    normed = mul(centred, var._like(torch.rsqrt(var._F + eps)))
    return normed._like(normed._F * weight + bias)


def test_against_the_composed_layers(ME):
    """secondary (consistency, not the yardstick): the same bound between the layer and the composition"""
    rng = np.random.default_rng(61)
    C = 20
    coords = cloud(rng, [600, 350, 50], [0, 2, 5])
    cm = manager_of(ME, coords)
    layer = make_layer(ME, C)
    feats = torch.from_numpy(features(rng, coords.shape[0], C)).cuda()
    g = torch.from_numpy(features(rng, coords.shape[0], C)).cuda()
    xa = feats.clone().requires_grad_(True)
    ya = layer(ME.SparseTensor(xa, coordinate_manager=cm))._F
    ya.backward(g)
    got = (ya.detach(), xa.grad, layer.weight.grad.clone(), layer.bias.grad.clone())
    layer.zero_grad(set_to_none=True)
    xb = feats.clone().requires_grad_(True)
    yb = composed_instance_norm(ME, ME.SparseTensor(xb, coordinate_manager=cm), layer.weight, layer.bias, layer.eps)._F
    yb.backward(g)
    for name, a, b in zip(("forward", "dx", "dweight", "dbias"), got, (yb, xb.grad, layer.weight.grad, layer.bias.grad)):
        check("composed " + name, a, b)


# ---------------------------------------------------------------------------------------------- 10. one composed block
def dense_weight(W, ks):
    """W [K, Cin, Cout] with k = ix + ks iy + ks^2 iz -> [Cout, Cin, kx, ky, kz]"""
    cin, cout = W.shape[1], W.shape[2]
    return W.view(ks, ks, ks, cin, cout).permute(4, 3, 2, 1, 0).contiguous()


def densify64(coords, feats, B, G):
    d = torch.zeros((B, feats.shape[1], G, G, G), dtype=torch.float64)
    c = torch.as_tensor(coords).long()
    d[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]] = feats
    return d


def read_dense(d, coords):
    c = torch.as_tensor(coords).long()
    return d[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]]


def dense_conv3(coords, x, W, B, G):
    """3x3x3 submanifold convolution of the rows x [V, Cin] (float64, autograd) -> rows at the same coordinates"""
    return read_dense(F.conv3d(densify64(coords, x, B, G), dense_weight(W, 3), padding=1), coords)


def test_conv_instancenorm_elu_conv_block(ME):
    """conv -> instance norm -> MinkowskiELU -> conv on a small cloud against the dense float64 graph (conv3d over the
    occupied grid, instance_norm over the occupied voxels of a batch index, elu): forward and all parameter gradients"""
    rng = np.random.default_rng(67)
    cin, C, B, G = 6, 16, 2, 12
    coords = cloud(rng, [260, 180], [0, 1], G=G)
    V = coords.shape[0]
    cm = manager_of(ME, coords)
    torch.manual_seed(71)
    conv1 = ME.MinkowskiConvolution(cin, C, kernel_size=3, dimension=3).cuda()
    norm = make_layer(ME, C, "MinkowskiStableInstanceNorm")
    act = ME.MinkowskiELU(alpha=0.8)
    conv2 = ME.MinkowskiConvolution(C, C, kernel_size=3, dimension=3).cuda()
    feats = features(rng, V, cin)
    xf = torch.from_numpy(feats).cuda().requires_grad_(True)
    y = conv2(act(norm(conv1(ME.SparseTensor(xf, coordinate_manager=cm)))))

    def p64(t):
        return t.detach().double().cpu().requires_grad_(True)
    x64, W1, w64, b64, W2 = (p64(t) for t in (xf, conv1.kernel, norm.weight, norm.bias, conv2.kernel))
    h = dense_conv3(coords, x64, W1, B, G)
    h = F.elu(reference(h, coords[:, 0], norm.eps, w64, b64), alpha=0.8)
    want = dense_conv3(coords, h, W2, B, G)
    check("block forward", y._F, want)
    g = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    y._F.backward(torch.from_numpy(g).cuda())
    want.backward(torch.from_numpy(g).double())
    check("block dx", xf.grad, x64.grad)
    check("block conv1 dW", conv1.kernel.grad, W1.grad)
    check("block norm dweight", norm.weight.grad, w64.grad)
    check("block norm dbias", norm.bias.grad, b64.grad)
    check("block conv2 dW", conv2.kernel.grad, W2.grad)


# ---------------------------------------------------------------------------------------------- 11. argument contracts
def test_argument_contracts(be):
    from minsu3d_amd._lib import HipLibraryError, E_UNSUPPORTED
    from minsu3d_amd.backend import BatchGroup
    dev = "cuda"
    order = torch.arange(5, dtype=torch.int64, device=dev)
    offsets = torch.tensor([0, 5], dtype=torch.int32, device=dev)
    seg = torch.zeros(5, dtype=torch.int32, device=dev)
    x0 = torch.zeros((5, 0), dtype=torch.float32, device=dev)
    with pytest.raises(HipLibraryError, match=str(E_UNSUPPORTED)):
        be.inorm_forward(x0, BatchGroup.from_tensors(order, offsets, seg), 1e-5, None, None)
    # 65536 segments are refused before any pointer is looked at (asked of the library itself: nothing is allocated for it)
    import ctypes as C
    null = C.c_void_p(0)
    assert be.lib.ms3d_inorm_forward(null, C.c_long(5), 4, null, null, 65536, null, C.c_float(1e-5), null, null, null, null,
                                     null, null, C.c_size_t(0), null) == E_UNSUPPORTED
    assert be.lib.ms3d_inorm_backward(null, null, C.c_long(5), 4, null, null, 65536, null, null, null, null, null, null, null,
                                      null, C.c_size_t(0), null) == E_UNSUPPORTED
    # a workspace that is too small is refused before anything is launched
    x = torch.zeros((5, 4), dtype=torch.float32, device=dev)
    stat = torch.zeros((1, 4), dtype=torch.float64, device=dev)
    small = torch.zeros(16, dtype=torch.uint8, device=dev)

    def ptr(t):
        return C.c_void_p(t.data_ptr())
    assert be.lib.ms3d_inorm_forward(ptr(x), C.c_long(5), 4, ptr(order), ptr(offsets), 1, ptr(seg), C.c_float(1e-5), null, null,
                                     ptr(stat), ptr(stat), ptr(x), ptr(small), C.c_size_t(16), null) == 10001
    # no rows: nothing is launched, empty results, zero parameter gradients
    e64, e32 = order[:0], seg[:0]
    none = torch.zeros(1, dtype=torch.int32, device=dev)
    xe = torch.zeros((0, 4), dtype=torch.float32, device=dev)
    empty = BatchGroup.from_tensors(e64, none, e32)
    y, mean, invstd = be.inorm_forward(xe, empty, 1e-5, None, None)
    assert tuple(y.shape) == (0, 4) and tuple(mean.shape) == (0, 4) and tuple(invstd.shape) == (0, 4)
    dx, dw, db = be.inorm_backward(xe, xe, empty, mean, invstd, None)
    assert tuple(dx.shape) == (0, 4) and not dw.any() and not db.any()
    torch.cuda.synchronize()
