"""GPU: points in, points out -- TensorField quantisation (four modes), slice / cat_slice (on the field's own tensor and across
coordinate sets), trilinear interpolation (map, values, gradient), MinkowskiPoolingTranspose, and a point -> voxel -> point
network step.

Yardsticks: tests/field_ref.py (numpy; pinned against float64 grid_sample / index_add_ in tests/test_field_cpu.py) and dense
float64 torch.  Bars: everything integer is exact (sets, inverse maps, interpolation rows); so is everything that is a fixed
chain of float32 operations the restatement repeats in the same order (interpolation weights, voxel features of every mode,
their gradient, slice and its gradient); interpolated values, their gradient, pooling transpose and the composed step are
within RTOL = 1e-4 of the largest magnitude of the float64 result, BatchNorm parameters within 1e-3 as in
test_generative_gpu.py.

Every comparison prints its error (pytest -s); the recorded figures are in DESIGN section 4.2."""
import functools
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import field_ref as R
from sparse_ref import random_sparse, ref_conv
from test_geometry_gpu import RTOL, check, densify64, invert_np, manager_at, offsets_np, read_dense, rel_err, sorted_map

pytestmark = pytest.mark.gpu
CHANNELS = (1, 6, 16, 33, 64)


@pytest.fixture(scope="module")
def ME():
    import minsu3d_amd.MinkowskiEngine as me
    return me


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def modes_of(ME):
    q = ME.SparseTensorQuantizationMode
    return {R.AVG: q.UNWEIGHTED_AVERAGE, R.SUM: q.UNWEIGHTED_SUM, R.MAX: q.MAX_POOL, R.FIRST: q.RANDOM_SUBSAMPLE}


def uniform_points(rng, n, B, lo, hi):
    p = np.empty((n, 4), np.float32)
    p[:, 0] = rng.integers(0, B, n)
    p[:, 1:] = rng.uniform(lo, hi, (n, 3))
    return p


# ---------------------------------------------------------------------------------------------- 1. quantisation
@functools.lru_cache(maxsize=None)
def quant_case(ts):
    """3000 points of 3 batches in [-6, 6) cells, 300 of them on exact integer coordinates, then 400 jittered copies of one
    point (one voxel holds over 400 points) -> (points, (coords, inverse, first) of field_ref.quantize_np).  Shared, read only."""
    rng = np.random.default_rng(100 + ts)
    p = uniform_points(rng, 3000, 3, -6 * ts, 6 * ts)
    p[:300, 1:] = np.round(p[:300, 1:])
    crowd = np.tile(np.array([[1, 2.5 * ts, -3.5 * ts, 0.5 * ts]], np.float32), (400, 1))
    crowd[:, 1:] += rng.uniform(-0.4 * ts, 0.4 * ts, (400, 3)).astype(np.float32)
    p = np.concatenate([p, crowd]).astype(np.float32)
    q = R.quantize_np(p, ts)
    assert np.bincount(q[1]).max() >= 400
    p.setflags(write=False)
    return p, q


@pytest.mark.parametrize("ts", [1, 2, 4])
def test_quantize_set_inverse_and_order(ME, ts):
    pts, (coords, inverse, first) = quant_case(ts)
    field = ME.TensorField(torch.ones(len(pts), 1).cuda(), dev(pts))
    x = field.sparse(tensor_stride=ts)
    assert x.tensor_stride == ts and x.C.dtype == torch.int32
    assert np.array_equal(x.C.cpu().numpy(), coords)
    assert field.inverse_mapping.dtype == torch.int64 and np.array_equal(field.inverse_mapping.cpu().numpy(), inverse)
    assert np.array_equal(x.F.cpu().numpy(), np.ones((len(coords), 1), np.float32))


@pytest.mark.parametrize("mode", [R.AVG, R.SUM, R.MAX, R.FIRST])
@pytest.mark.parametrize("ts", [1, 2, 4])
def test_quantize_features_and_gradient_exact(ME, ts, mode):
    pts, (coords, inverse, first) = quant_case(ts)
    v = len(coords)
    rng = np.random.default_rng(7 * ts + mode)
    points = dev(pts)
    for C in CHANNELS:
        feats = rng.standard_normal((len(pts), C)).astype(np.float32)
        if mode == R.MAX:
            feats[rng.integers(0, len(pts), 600)] = feats[3000]          # ties inside the crowded voxel and elsewhere
        want, arg, count = R.reduce_np(mode, feats, inverse, v)
        dvox = rng.standard_normal((v, C)).astype(np.float32)
        runs = []
        for _ in range(2):
            leaf = dev(feats).requires_grad_(True)
            x = ME.TensorField(leaf, points, quantization_mode=modes_of(ME)[mode]).sparse(tensor_stride=ts)
            x.F.backward(dev(dvox))
            runs.append((x.F.detach(), leaf.grad))
        got, grad = runs[0]
        assert np.array_equal(got.cpu().numpy(), want), (mode, C)
        if mode == R.FIRST:
            g = np.zeros_like(feats)
            g[first] = dvox
        else:
            g = R.reduce_backward_np(mode, dvox, inverse, arg, count)
        assert np.array_equal(grad.cpu().numpy(), g), (mode, C)
        assert torch.equal(runs[1][0], got) and torch.equal(runs[1][1], grad)
    # the mode of .sparse() overrides the field's
    f = ME.TensorField(dev(feats), points)
    assert f.quantization_mode is ME.SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE
    assert np.array_equal(f.sparse(ts, quantization_mode=modes_of(ME)[mode]).F.cpu().numpy(), want)


def test_quantize_empty(ME):
    for mode in modes_of(ME).values():
        x = ME.TensorField(torch.zeros((0, 6)).cuda(), torch.zeros((0, 4)).cuda(), quantization_mode=mode).sparse()
        assert tuple(x.F.shape) == (0, 6) and tuple(x.C.shape) == (0, 4)


# ---------------------------------------------------------------------------------------------- 2. the models' route
def test_same_as_sparse_quantize_and_slice(ME):
    """RANDOM_SUBSAMPLE is the route the models take (ME.utils.sparse_quantize + features[inverse]): the same set, features
    and inverse map; slice is X.features[inverse] and its gradient a serial scatter-add in ascending point index"""
    pts, (coords, inverse, first) = quant_case(1)
    rng = np.random.default_rng(5)
    feats = rng.standard_normal((len(pts), 6)).astype(np.float32)
    points, f = dev(pts), dev(feats)
    field = ME.TensorField(f, points, quantization_mode=ME.SparseTensorQuantizationMode.RANDOM_SUBSAMPLE)
    x = field.sparse()
    c2, f2, inv2 = ME.utils.sparse_quantize(points, f, return_inverse=True, quantization_size=1)
    assert torch.equal(x.C, c2) and torch.equal(x.F, f2) and torch.equal(field.inverse_mapping, inv2)
    vox = rng.standard_normal((len(coords), 16)).astype(np.float32)
    dpt = rng.standard_normal((len(pts), 16)).astype(np.float32)
    acc = np.zeros_like(vox)
    for n, r in enumerate(inverse):
        acc[r] += dpt[n]
    for _ in range(2):
        leaf = dev(vox).requires_grad_(True)
        y = ME.SparseTensor(leaf, coordinate_manager=x.coordinate_manager)
        sl = field.slice(y)
        assert isinstance(sl, ME.TensorField) and sl.C is points
        assert torch.equal(sl.F, leaf.detach()[field.inverse_mapping]) and torch.equal(y.slice(field).F, sl.F)
        assert torch.equal(field.cat_slice(y).F, torch.cat([f, sl.F], 1)) and torch.equal(y.cat_slice(field).F, field.cat_slice(y).F)
        sl.F.backward(dev(dpt))
        assert np.array_equal(leaf.grad.cpu().numpy(), acc)


# ---------------------------------------------------------------------------------------------- 3. interpolation
@functools.lru_cache(maxsize=None)
def interp_case(ts):
    """B = 2, a 6^3 window shifted by -3, ~60 % of the cells occupied, at tensor stride ts; queries: 2000 uniform points in the
    window, the set's own coordinates, 16 points 100 cells away, 8 points of a batch index the set lacks -> (cells, coords,
    points, rows, weights); the conditions that keep the comparisons from passing vacuously are asserted here"""
    B, G = 2, 6
    rng = np.random.default_rng(200 + ts)
    cells, _ = random_sparse(rng, B=B, grid=G, n=int(0.6 * B * G ** 3), C=1)
    cells = cells.copy()
    cells[:, 1:] -= 3
    coords = cells.copy()
    coords[:, 1:] *= ts
    far = uniform_points(rng, 16, B, 100 * ts, 101 * ts)
    alien = uniform_points(rng, 8, 1, -3 * ts, 3 * ts)
    alien[:, 0] = B + 1
    pts = np.concatenate([uniform_points(rng, 2000, B, -3 * ts, 3 * ts), coords.astype(np.float32), far, alien]).astype(np.float32)
    rows, weights = R.interp_map_np(coords, pts, ts)
    assert 0.2 <= (rows < 0).mean() <= 0.8
    assert (rows >= 0).all(0).sum() >= 10 and (rows < 0).all(0).sum() >= 16
    for a in (cells, coords, pts, rows, weights):
        a.setflags(write=False)
    return cells, coords, pts, rows, weights


@pytest.mark.parametrize("ts", [1, 2, 4])
def test_interpolation_map_values_gradient(ME, ts):
    cells, coords, pts, rows, weights = interp_case(ts)
    v, n = len(coords), len(pts)
    on = slice(2000, 2000 + v)
    none = (rows < 0).all(0)
    cm = ME.CoordinateManager.rooted(dev(coords), ts)
    points = dev(pts)
    got_rows, got_w, (entry_sorted, seg_start) = cm.interpolation_map(ts, points)
    assert got_rows.dtype == torch.int32 and np.array_equal(got_rows.cpu().numpy(), rows)
    assert got_w.dtype == torch.float32 and np.array_equal(got_w.cpu().numpy(), weights)
    assert cm.interpolation_map(ts, points)[0] is got_rows                         # cached per points tensor
    e = entry_sorted.cpu().numpy()
    seg = seg_start.cpu().numpy()
    assert seg[0] == 0 and seg[-1] == len(e) == (rows >= 0).sum()
    of_row = rows.T.reshape(-1)[e]
    assert np.array_equal(of_row, np.sort(of_row)) and np.array_equal(np.bincount(of_row, minlength=v), np.diff(seg))
    assert all(np.all(np.diff(e[seg[r]:seg[r + 1]]) > 0) for r in range(v))        # ascending point inside a row
    rng = np.random.default_rng(ts)
    field = ME.TensorField(torch.zeros(n, 1).cuda(), points)
    worst = [0.0, 0.0]
    for C in CHANNELS:
        x = rng.standard_normal((v, C)).astype(np.float32)
        dout = rng.standard_normal((n, C)).astype(np.float32)
        want = R.interp_np(x, rows, weights)
        gwant = R.interp_backward_np(dout, rows, weights, v)
        runs = []
        for _ in range(2):
            leaf = dev(x).requires_grad_(True)
            X = ME.SparseTensor(leaf, coordinate_manager=cm, tensor_stride=ts)
            out = X.interpolate(field)
            assert isinstance(out, ME.TensorField) and out.C is points
            out.F.backward(dev(dout))
            runs.append((out.F.detach(), leaf.grad))
        got, grad = runs[0]
        worst[0] = max(worst[0], rel_err(got, torch.from_numpy(want)))
        worst[1] = max(worst[1], rel_err(grad, torch.from_numpy(gwant)))
        check(f"interpolation ts {ts} C {C} forward", got, torch.from_numpy(want), RTOL)
        check(f"interpolation ts {ts} C {C} gradient", grad, torch.from_numpy(gwant), RTOL)
        assert torch.equal(got[on], dev(x))                       # weights (1, 0, ..., 0): the voxel's own row, bit for bit
        assert not got[dev(none)].any()
        assert torch.equal(runs[1][0], got) and torch.equal(runs[1][1], grad)
        layer = ME.MinkowskiInterpolation(return_kernel_map=True, return_weights=True)
        o2, kmap, w2 = layer(ME.SparseTensor(dev(x), coordinate_manager=cm, tensor_stride=ts), points)
        assert torch.equal(o2, got) and np.array_equal(kmap.cpu().numpy(), rows) and np.array_equal(w2.cpu().numpy(), weights)
        assert torch.equal(ME.MinkowskiInterpolation()(X, points), got)
    print(f"interpolation ts {ts}: worst forward {worst[0]:.3e}, worst gradient {worst[1]:.3e}")


def test_interpolation_edges(ME):
    """floor, not truncation; non-finite points and corners outside the packable range name no row and give zeros"""
    coords = np.array([[0, -1, 0, 0], [0, 0, 0, 0], [0, 16383, 0, 0]], np.int32)
    pts = np.array([[0, -0.5, 0, 0], [0, np.nan, 0, 0], [0, np.inf, 0, 0], [0, 16383.5, 0, 0], [0, 1e30, 0, 0],
                    [-1, 0, 0, 0], [0, -16384.5, 0, 0]], np.float32)
    rows, weights = R.interp_map_np(coords, pts, 1)
    x = ME.SparseTensor(dev(np.array([[1.0, 2.0], [3.0, 5.0], [7.0, 11.0]], np.float32)), coordinates=dev(coords))
    out, kmap, w = ME.MinkowskiInterpolation(return_kernel_map=True, return_weights=True)(x, dev(pts))
    assert np.array_equal(kmap.cpu().numpy(), rows) and np.array_equal(w.cpu().numpy(), weights)
    assert out.cpu().tolist() == [[2.0, 3.5], [0, 0], [0, 0], [3.5, 5.5], [0, 0], [0, 0], [0, 0]]


# ---------------------------------------------------------------------------------------------- 4. dense pin
def test_interpolation_against_grid_sample(ME):
    ts, C, B, G = 2, 6, 2, 6
    cells, coords, pts, rows, weights = interp_case(ts)
    rng = np.random.default_rng(9)
    x = rng.standard_normal((len(coords), C)).astype(np.float32)
    dout = rng.standard_normal((len(pts), C)).astype(np.float32)
    leaf64 = torch.from_numpy(x).double().requires_grad_(True)
    shifted = cells.copy()
    shifted[:, 1:] = (shifted[:, 1:] + 4) * ts             # cell -3 sits at index 1: one empty cell of margin on every side
    want = R.grid_sample64(densify64(shifted, leaf64, B, G + 2, ts), -4, pts, ts)
    want.backward(torch.from_numpy(dout).double())
    leaf = dev(x).requires_grad_(True)
    X = ME.SparseTensor(leaf, coordinate_manager=ME.CoordinateManager.rooted(dev(coords), ts), tensor_stride=ts)
    out = ME.MinkowskiInterpolation()(X, dev(pts))
    out.backward(dev(dout))
    check("interpolation against grid_sample, forward", out, want.detach(), RTOL)
    check("interpolation against grid_sample, gradient", leaf.grad, leaf64.grad, RTOL)


# ---------------------------------------------------------------------------------------------- 5. slice across sets
def _lookup(set_coords, query):
    table = {tuple(c): r for r, c in reversed(list(enumerate(set_coords.tolist())))}
    return np.array([table.get(tuple(q), -1) for q in query.tolist()], np.int64)


def test_slice_across_coordinate_sets(ME):
    pts, (coords, inverse, first) = quant_case(1)
    rng = np.random.default_rng(31)
    feats = rng.standard_normal((len(pts), 4)).astype(np.float32)
    field = ME.TensorField(dev(feats), dev(pts))
    x = field.sparse()
    torch.manual_seed(3)

    def expect(t, ts):
        r = _lookup(t.C.cpu().numpy(), R.voxel_of(pts, ts))
        padded = torch.cat([t.F.detach(), t.F.new_zeros((1, t.F.size(1)))])
        return r, padded[dev(np.where(r < 0, t.F.size(0), r))]
    # the output of a generative layer: a superset on a manager of its own
    gen = ME.MinkowskiGenerativeConvolutionTranspose(4, 8, kernel_size=3, stride=1, dimension=3).cuda()(x)
    assert gen.coordinate_manager is not x.coordinate_manager
    r, want = expect(gen, 1)
    assert (r >= 0).all() and torch.equal(field.slice(gen).F, want)
    # a pruned tensor: points whose voxel was dropped get zeros
    mask = dev(rng.random(len(coords)) < 0.5)
    pruned = ME.MinkowskiPruning()(x, mask)
    r, want = expect(pruned, 1)
    got = field.slice(pruned).F
    assert (r < 0).any() and (r >= 0).any() and torch.equal(got, want) and not got[dev(r < 0)].any()
    assert np.array_equal(r >= 0, mask.cpu().numpy()[inverse])
    # a coarser level of the field's own manager
    down = ME.MinkowskiConvolution(4, 8, kernel_size=2, stride=2, dimension=3).cuda()(x)
    assert down.tensor_stride == 2 and down.coordinate_manager is x.coordinate_manager
    r, want = expect(down, 2)
    assert (r >= 0).all() and len(np.unique(r)) == down.F.size(0) and torch.equal(down.slice(field).F, want)
    assert torch.equal(field.cat_slice(down).F, torch.cat([field.F, want], 1))
    assert field._rows_in(down) is field._rows_in(down)              # looked up once per (manager, tensor stride)
    # the gradient reaches the sliced tensor's features: per row the sum over its points, zero for rows no point names
    leaf = pruned.F.detach().clone().requires_grad_(True)
    t = ME.SparseTensor(leaf, coordinate_manager=pruned.coordinate_manager)
    dpt = rng.standard_normal((len(pts), 4)).astype(np.float32)
    field.slice(t).F.backward(dev(dpt))
    r = _lookup(pruned.C.cpu().numpy(), R.voxel_of(pts, 1))
    acc = np.zeros((leaf.size(0), 4), np.float32)
    for n, row in enumerate(r):
        if row >= 0:
            acc[row] += dpt[n]
    assert np.array_equal(leaf.grad.cpu().numpy(), acc)


# ---------------------------------------------------------------------------------------------- 6. pooling transpose
@pytest.mark.parametrize("ks,stride", [(2, 2), (3, 2), (3, 1)])
def test_pooling_transpose_against_dense(ME, ks, stride):
    """dense float64 conv_transpose3d with an all-ones depthwise kernel, read at the target set"""
    B, G, C = 2, 12, 6
    rng = np.random.default_rng(60 + ks + stride)
    fine, _ = random_sparse(rng, B=B, grid=G, n=400, C=1)
    ts = stride                                             # the input lives at tensor stride 2 (-> 1) or 1 (stays)
    cm = manager_at(ME, fine, ts)
    cin = cm.coords[ts].cpu().numpy()
    x = rng.standard_normal((len(cin), C)).astype(np.float32)
    leaf = dev(x).requires_grad_(True)
    y = ME.MinkowskiPoolingTranspose(ks, stride, dimension=3)(ME.SparseTensor(leaf, coordinate_manager=cm, tensor_stride=ts))
    assert y.tensor_stride == 1 and y.coordinate_manager is cm
    target = y.C.cpu().numpy()
    assert np.array_equal(np.unique(target, axis=0), np.unique(fine, axis=0))
    leaf64 = torch.from_numpy(x).double().requires_grad_(True)
    d = densify64(cin, leaf64, B, G // ts, ts)
    ones = torch.ones((C, 1, ks, ks, ks), dtype=torch.float64)
    pad = 1 if ks == 3 else 0
    dense = F.conv_transpose3d(d, ones, stride=stride, padding=pad, output_padding=1 if (ks == 3 and stride == 2) else 0,
                               groups=C)
    assert tuple(dense.shape[2:]) == (G, G, G)
    want = read_dense(dense, target, 1)
    dout = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    want.backward(torch.from_numpy(dout).double())
    y.F.backward(dev(dout))
    check(f"pooling transpose k{ks} s{stride} forward", y.F, want.detach(), RTOL)
    check(f"pooling transpose k{ks} s{stride} gradient", leaf.grad, leaf64.grad, RTOL)
    if (ks, stride) == (2, 2):                              # every fine voxel copies its parent
        parent = _lookup(cin, R.voxel_of(target, 2))
        assert torch.equal(y.F.detach(), dev(x)[dev(parent)])


def test_pooling_transpose_needs_a_cached_target(ME):
    coords = dev(np.array([[0, 0, 0, 0], [0, 8, 0, 0], [1, 4, 2, 0]], np.int32))
    x = ME.SparseTensor(torch.ones(3, 4).cuda(), coordinate_manager=ME.CoordinateManager.rooted(coords, 2), tensor_stride=2)
    for ks in (2, 3):
        with pytest.raises(NotImplementedError, match="cached finer coordinate set"):
            ME.MinkowskiPoolingTranspose(ks, 2, dimension=3)(x)
    y = ME.MinkowskiPoolingTranspose(3, 1, dimension=3)(x)           # stride 1 stays on the set
    assert y.tensor_stride == 2 and torch.equal(y.F, x.F)            # (no two of these voxels are neighbours)


# ---------------------------------------------------------------------------------------------- 7. composed
class _PointNet(torch.nn.Module):
    C0, C1, C2, C3 = 4, 8, 16, 5

    def __init__(self, ME):
        super().__init__()
        self.conv1 = ME.MinkowskiConvolution(self.C0, self.C1, kernel_size=3, dimension=3)
        self.bn = ME.MinkowskiBatchNorm(self.C1)
        self.relu = ME.MinkowskiReLU()
        self.down = ME.MinkowskiConvolution(self.C1, self.C2, kernel_size=2, stride=2, dimension=3)
        self.up = ME.MinkowskiConvolutionTranspose(self.C2, self.C1, kernel_size=2, stride=2, dimension=3)
        self.head = ME.MinkowskiConvolution(2 * self.C1, self.C3, kernel_size=1, dimension=3)
        self.cat = ME.cat
        with torch.no_grad():
            self.bn.bn.weight.uniform_(0.5, 1.5)
            self.bn.bn.bias.uniform_(-0.3, 0.3)

    def forward(self, field):
        x = field.sparse()
        h = self.relu(self.bn(self.conv1(x)))
        u = self.up(self.down(h))
        return self.head(self.cat(h, u)).slice(field), x


def _composed_reference(net, pts, feats, target):
    """the same step in float64 torch over tables built on the host"""
    coords, inverse, _ = _quantize_big(pts)
    v = len(coords)
    p64 = {n: p.detach().double().cpu().requires_grad_(True) for n, p in net.named_parameters()}
    f64 = torch.from_numpy(feats).double().requires_grad_(True)
    inv = torch.from_numpy(inverse)
    cnt = torch.bincount(inv, minlength=v).double()
    x = torch.zeros((v, feats.shape[1]), dtype=torch.float64).index_add(0, inv, f64) / cnt[:, None]
    k3 = torch.from_numpy(sorted_map(coords, coords, offsets_np(3, 1, 1)))
    h = ref_conv(x, p64["conv1.kernel"], k3)
    h = torch.relu(F.batch_norm(h, None, None, p64["bn.bn.weight"], p64["bn.bn.bias"], True, 0.1, 1e-5))
    q = coords.copy()
    q[:, 1:] = np.floor_divide(q[:, 1:], 2) * 2
    coarse = np.unique(q, axis=0).astype(np.int32)                  # (the order of the coarse rows does not reach the loss)
    down = sorted_map(coords, coarse, offsets_np(2, 1, 1))
    c = ref_conv(h, p64["down.kernel"], torch.from_numpy(down))
    u = ref_conv(c, p64["up.kernel"], torch.from_numpy(invert_np(down, v)))
    out = torch.cat([h, u], 1) @ p64["head.kernel"]
    loss = ((out[inv] - torch.from_numpy(target).double()) ** 2).mean()
    loss.backward()
    return loss.detach(), f64.grad, {n: p.grad for n, p in p64.items()}, coords, inverse, out.detach()


def _quantize_big(pts):
    """field_ref.quantize_np for clouds too large for a Python loop: first-occurrence order through np.unique"""
    q = R.voxel_of(pts, 1)
    _, first, inverse = np.unique(q, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return q[first[order]].astype(np.int32), rank[inverse.reshape(-1)], first[order]


@pytest.mark.parametrize("size", ["small", "morton"])
def test_composed_point_voxel_point_step(ME, size):
    from minsu3d_amd.MinkowskiEngine import tensor as T
    rng = np.random.default_rng(77)
    if size == "small":
        pts = uniform_points(rng, 3000, 2, -6, 6)
    else:
        pts = uniform_points(rng, 170000, 2, 0, 64)
    if size == "small":      # (the fast restatement of the set itself)
        assert all(np.array_equal(a, b) for a, b in zip(_quantize_big(pts), R.quantize_np(pts, 1)))
    feats = rng.standard_normal((len(pts), _PointNet.C0)).astype(np.float32)
    target = rng.standard_normal((len(pts), _PointNet.C3)).astype(np.float32)
    torch.manual_seed(11)
    net = _PointNet(ME).cuda().train()
    loss64, df64, g64, coords, inverse, out64 = _composed_reference(net, pts, feats, target)
    assert (len(coords) >= T._SORT_MIN_ROWS) == (size == "morton")
    points, tgt = dev(pts), dev(target)
    runs = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        leaf = dev(feats).requires_grad_(True)
        field = ME.TensorField(leaf, points)
        out, x = net(field)
        loss = ((out.F - tgt) ** 2).mean()
        loss.backward()
        runs.append((loss.detach(), leaf.grad, {n: p.grad.clone() for n, p in net.named_parameters()}))
    assert (x.coordinate_manager.perm is not None) == (size == "morton")      # the Morton composition ran
    assert np.array_equal(x.C.cpu().numpy(), coords) and np.array_equal(field.inverse_mapping.cpu().numpy(), inverse)
    loss, df, grads = runs[0]
    check(f"composed {size} loss", loss.view(1), loss64.view(1), RTOL)
    check(f"composed {size} d features", df, df64, RTOL)
    for n, g in grads.items():
        check(f"composed {size} d {n}", g, g64[n], 1e-3 if n.startswith("bn.") else RTOL)
    assert torch.equal(runs[1][0], loss) and torch.equal(runs[1][1], df)
    for n, g in grads.items():
        assert torch.equal(runs[1][2][n], g), n
    # interpolation on the same (possibly Morton-sorted) manager: the map names the rows the caller sees
    sub = dev(pts[:4000])
    y = ME.SparseTensor(dev(out64.float().numpy()), coordinates=x.C) if size == "small" else \
        ME.SparseTensor(dev(out64.float().numpy())[x.coordinate_manager.perm], coordinate_manager=x.coordinate_manager)
    val, kmap, w = ME.MinkowskiInterpolation(return_kernel_map=True, return_weights=True)(y, sub)
    rows, weights = R.interp_map_np(coords, pts[:4000], 1)
    assert np.array_equal(kmap.cpu().numpy(), rows) and np.array_equal(w.cpu().numpy(), weights)
    check(f"composed {size} interpolation", val, torch.from_numpy(R.interp_np(out64.float().numpy(), rows, weights)), RTOL)


# ---------------------------------------------------------------------------------------------- 8. size (printed only)
# ------------------------------------------------------------------------------------------------ the scalar route
def off_by_one_float(a):
    """the same values in storage that starts one float behind a 16-byte boundary (a slice of a larger buffer)"""
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    t = buf[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert buf.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 4 and t.is_contiguous() and t.contiguous().data_ptr() == t.data_ptr()
    return t


def same_bits(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


def test_misaligned_rows_take_the_scalar_route():
    """C = 8 would take four floats per lane (130 points: 260 threads, two blocks); features and upstream gradients one float
    off the alignment take one, and give the same bytes in interpolation and in all three reductions, both directions, and
    for max the same winners"""
    from minsu3d_amd.backend import get_backend
    be = get_backend()
    rng = np.random.default_rng(131)
    N, V, C = 130, 40, 8
    # points -> voxels: every voxel holds a point, some hold many; the stable sort of the map and its segments
    inverse = np.concatenate([np.arange(V), rng.integers(0, V // 4, N - V)]).astype(np.int32)
    rng.shuffle(inverse)
    order = np.argsort(inverse, kind="stable").astype(np.int64)
    seg_start = np.concatenate([[0], np.cumsum(np.bincount(inverse, minlength=V))]).astype(np.int32)
    feats = rng.standard_normal((N, C)).astype(np.float32)
    feats[:, 0] = np.round(feats[:, 0])                            # ties for max: the first point of the voxel wins
    dvox = rng.standard_normal((V, C)).astype(np.float32)
    for mode in (R.AVG, R.SUM, R.MAX):
        a, aarg = be.field_reduce(mode, dev(feats), dev(order), dev(seg_start), V)
        b, barg = be.field_reduce(mode, off_by_one_float(feats), dev(order), dev(seg_start), V)
        assert same_bits(a, b), mode
        if mode == R.MAX:
            assert torch.equal(aarg, barg)
            w = aarg.cpu().numpy()
            assert np.array_equal(inverse[w], np.tile(np.arange(V)[:, None], (1, C)))
            assert np.array_equal(a.cpu().numpy(), feats[w, np.arange(C)[None, :]])
        else:
            assert aarg is None and barg is None
        da = be.field_reduce_backward(mode, dev(dvox), dev(inverse), dev(seg_start), aarg)
        db = be.field_reduce_backward(mode, off_by_one_float(dvox), dev(inverse), dev(seg_start), barg)
        assert same_bits(da, db), mode
        if mode == R.SUM:
            assert np.array_equal(da.cpu().numpy(), dvox[inverse])

    # voxels -> points: eight corners per point, a third of them absent; the table sorted by voxel row, entry = 8 * point + corner
    rows = rng.integers(0, V, (8, N)).astype(np.int32)
    rows[rng.random((8, N)) < 0.33] = -1
    rows[:, 5] = -1                                                # a point without corners
    weights = rng.random((8, N)).astype(np.float32)
    flat = rows.T.reshape(-1)
    e = np.nonzero(flat >= 0)[0]
    entry_sorted = e[np.argsort(flat[e], kind="stable")].astype(np.int64)
    eseg = np.concatenate([[0], np.cumsum(np.bincount(flat[e], minlength=V))]).astype(np.int32)
    x = rng.standard_normal((V, C)).astype(np.float32)
    dout = rng.standard_normal((N, C)).astype(np.float32)
    a = be.interp_forward(dev(x), dev(rows), dev(weights))
    b = be.interp_forward(off_by_one_float(x), dev(rows), dev(weights))
    want = sum(np.where(rows[j][:, None] >= 0, weights[j].astype(np.float64)[:, None] * x[np.maximum(rows[j], 0)], 0.0) for j in range(8))
    assert np.allclose(a.cpu().numpy(), want, rtol=0, atol=1e-5 * np.abs(want).max()) and not a[5].any()
    assert same_bits(a, b)
    a = be.interp_backward(dev(dout), dev(weights), dev(entry_sorted), dev(eseg), V)
    b = be.interp_backward(off_by_one_float(dout), dev(weights), dev(entry_sorted), dev(eseg), V)
    want = np.zeros((V, C))
    np.add.at(want, flat[e], weights.T.reshape(-1)[e].astype(np.float64)[:, None] * dout[e // 8])
    assert np.allclose(a.cpu().numpy(), want, rtol=0, atol=1e-5 * np.abs(want).max())
    assert same_bits(a, b)


def _ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def test_field_200k_points_times_printed(ME):
    """200 000 points over ~60 000 voxels at C = 32: the kernels beside the torch-composed formulation on the same inputs.
    Nothing about speed is asserted."""
    from minsu3d_amd.backend import get_backend
    be = get_backend()
    rng = np.random.default_rng(123)
    n, C = 200000, 32
    pts = uniform_points(rng, n, 1, 0, 40)
    points, feats = dev(pts), torch.randn(n, C, device="cuda")
    field = ME.TensorField(feats, points)
    x = field.sparse()
    v = x.F.size(0)
    inv = field.inverse_mapping
    order = torch.sort(inv, stable=True).indices.contiguous()
    seg = torch.zeros(v + 1, dtype=torch.int32, device="cuda")
    seg[1:] = torch.cumsum(torch.bincount(inv, minlength=v), 0)
    inv32 = inv.to(torch.int32)
    counts = torch.bincount(inv, minlength=v).float()[:, None]
    t_reduce = _ms(lambda: be.field_reduce(0, feats, order, seg, v))
    t_reduce_t = _ms(lambda: torch.zeros(v, C, device="cuda").index_add_(0, inv, feats) / counts)
    dvox = torch.randn(v, C, device="cuda")
    t_rbwd = _ms(lambda: be.field_reduce_backward(0, dvox, inv32, seg, None))
    t_rbwd_t = _ms(lambda: (dvox / counts)[inv])
    cm = x.coordinate_manager
    coords = cm.coords[1]
    rows, weights = be.interp_map(coords, points, 1)
    t_map = _ms(lambda: be.interp_map(coords, points, 1))

    def grouping():
        flat = rows.t().reshape(-1)
        valid = torch.nonzero(flat >= 0).view(-1)
        return valid[torch.sort(flat[valid].long(), stable=True).indices]
    t_sort = _ms(grouping)
    _, _, (entry_sorted, seg_start) = cm.interpolation_map(1, points)
    xv, dout = torch.randn(v, C, device="cuda"), torch.randn(n, C, device="cuda")
    t_fwd = _ms(lambda: be.interp_forward(xv, rows, weights))
    t_bwd = _ms(lambda: be.interp_backward(dout, weights, entry_sorted, seg_start, v))
    xpad = torch.cat([xv, xv.new_zeros(1, C)])
    idx = torch.where(rows < 0, torch.full_like(rows, v), rows).long()

    def torch_fwd():
        out = torch.zeros(n, C, device="cuda")
        for j in range(8):
            out = out + weights[j][:, None] * xpad.index_select(0, idx[j])
        return out

    def torch_bwd():
        din = torch.zeros(v + 1, C, device="cuda")
        for j in range(8):
            din.index_put_((idx[j],), weights[j][:, None] * dout, accumulate=True)
        return din[:v]
    t_fwd_t, t_bwd_t = _ms(torch_fwd), _ms(torch_bwd)
    check("200k interpolation forward vs torch", be.interp_forward(xv, rows, weights), torch_fwd(), RTOL)
    check("200k interpolation backward vs torch", be.interp_backward(dout, weights, entry_sorted, seg_start, v), torch_bwd(), RTOL)
    check("200k reduce vs torch", be.field_reduce(0, feats, order, seg, v)[0],
          torch.zeros(v, C, device="cuda").index_add_(0, inv, feats) / counts, RTOL)
    print(f"field 200k: points {n}, voxels {v}, C {C}, corner entries present {int((rows >= 0).sum())}\n"
          f"  field_reduce (average) {t_reduce:.3f} ms | torch index_add_ + divide {t_reduce_t:.3f} ms\n"
          f"  field_reduce_backward  {t_rbwd:.3f} ms | torch divide + index    {t_rbwd_t:.3f} ms\n"
          f"  interp_map             {t_map:.3f} ms\n"
          f"  grouping sort          {t_sort:.3f} ms (once per map)\n"
          f"  interp_forward         {t_fwd:.3f} ms | torch 8 x index_select + multiply-add {t_fwd_t:.3f} ms\n"
          f"  interp_backward        {t_bwd:.3f} ms | torch 8 x index_put_(accumulate)      {t_bwd_t:.3f} ms")
