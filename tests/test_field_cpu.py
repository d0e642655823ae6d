"""Points in, points out (TensorField, MinkowskiInterpolation, MinkowskiPoolingTranspose): what can be checked without a GPU
-- the exported names, the header, the host-decided contracts of the entry points, the refusals on a backend without the
kernels, the engine's own plumbing (cached maps, the Morton composition, the autograd functions) over a numpy backend, and the
expectation itself: the numpy restatements of tests/field_ref.py, which the GPU tests compare the engine against, are checked
here against float64 torch (grid_sample on the densified tensor, index_add_)."""
import os
import re

import numpy as np
import pytest
import torch

import minsu3d_amd.MinkowskiEngine as ME
import field_ref as R
from sparse_ref import random_sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("TensorField", "SparseTensorQuantizationMode", "MinkowskiInterpolation", "MinkowskiPoolingTranspose")
SYMBOLS = ("ms3d_interp_map", "ms3d_interp_forward", "ms3d_interp_backward", "ms3d_field_reduce", "ms3d_field_reduce_backward")
EPS = float(np.finfo(np.float32).eps)
QM = ME.SparseTensorQuantizationMode
MODES = {R.AVG: QM.UNWEIGHTED_AVERAGE, R.SUM: QM.UNWEIGHTED_SUM, R.MAX: QM.MAX_POOL, R.FIRST: QM.RANDOM_SUBSAMPLE}


def test_new_names_exported():
    for name in NEW:
        assert isinstance(getattr(ME, name), type), name
    for method in ("slice", "cat_slice", "interpolate"):
        assert callable(getattr(ME.SparseTensor, method)), method
    for method in ("sparse", "slice", "cat_slice"):
        assert callable(getattr(ME.TensorField, method)), method
    assert callable(ME.CoordinateManager.interpolation_map)
    assert {m.name for m in QM} >= {"UNWEIGHTED_AVERAGE", "UNWEIGHTED_SUM", "MAX_POOL", "RANDOM_SUBSAMPLE"}
    import minsu3d_amd.dropin.MinkowskiEngine as dropin
    for name in NEW:
        assert getattr(dropin, name) is getattr(ME, name) and name in dropin.__all__, name
    for word in NEW:
        assert word in ME.__doc__, word
    unsupported = ME.__doc__.split("Not supported")[1]
    for word in ("MinkowskiPoolingTranspose", "MinkowskiInterpolation", "TensorField"):
        assert word not in unsupported, word
    assert "quantization_mode" in unsupported and "coordinates" in unsupported


def test_header_declares_new_symbols():
    """(tests/test_abi_cpu.py then proves that the cross-compiled library exports them)"""
    text = open(os.path.join(ROOT, "include", "minsu3d_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b" + sym + r"\s*\(", text), sym


def test_entry_points_decide_their_contracts_on_the_host():
    """unknown modes, tensor strides that are no power of two, row counts beyond 2^31 - 1 and null pointers: MS3D_E_UNSUPPORTED;
    zero rows: 0 -- all decided before anything is launched, so this runs without a GPU"""
    import ctypes as C
    from minsu3d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    null, L, bad = C.c_void_p(0), C.c_long, _lib.E_UNSUPPORTED
    big = 2 ** 31

    def imap(vin, n, ts):
        return lib.ms3d_interp_map(null, vin, null, L(n), ts, null, null, null, C.c_size_t(0), null)
    for ts in (0, -2, 3, 6, 12):
        assert imap(10, 10, ts) == bad and imap(0, 0, ts) == bad, ts
    for ts in (1, 2, 4, 1024):
        assert imap(10, 0, ts) == 0 and imap(0, 10, ts) == 0 and imap(0, 0, ts) == 0, ts
        assert imap(10, 10, ts) == bad                       # null pointers
    assert imap(10, (big - 1) // 8 + 1, 1) == bad            # 8 N entries no longer fit an int
    assert imap(10, -1, 1) == bad

    fwd = lambda n, c: lib.ms3d_interp_forward(null, null, null, L(n), c, null, null)
    assert fwd(0, 4) == 0 and fwd(10, 4) == bad and fwd(10, 0) == bad and fwd((big - 1) // 8 + 1, 4) == bad
    bwd = lambda vin, n, c: lib.ms3d_interp_backward(null, null, null, null, L(vin), L(n), c, null, null)
    assert bwd(0, 10, 4) == 0 and bwd(0, 0, 4) == 0 and bwd(10, 10, 4) == bad and bwd(10, 10, 0) == bad
    assert bwd(big, 10, 4) == bad and bwd(10, (big - 1) // 8 + 1, 4) == bad

    red = lambda mode, v, c: lib.ms3d_field_reduce(mode, null, null, null, L(v), c, null, null, null)
    rbw = lambda mode, n, c: lib.ms3d_field_reduce_backward(mode, null, null, null, null, L(n), c, null, null)
    for fn in (red, rbw):
        for mode in (0, 1, 2):
            assert fn(mode, 0, 4) == 0 and fn(mode, 10, 4) == bad and fn(mode, big, 4) == bad and fn(mode, 10, 0) == bad
        for mode in (-1, 3, 7):
            assert fn(mode, 0, 4) == bad and fn(mode, 10, 4) == bad


def _tensor(coords, feats, ts=1):
    coords = torch.as_tensor(coords)
    cm = ME.CoordinateManager(coords) if ts == 1 else ME.CoordinateManager.rooted(coords, ts)
    return ME.SparseTensor(torch.as_tensor(feats), coordinate_manager=cm, tensor_stride=ts)


def test_layers_name_the_hip_backend_when_it_lacks_them():
    from minsu3d_amd import backend

    class Bare:
        pass

    class QuantizeOnly:
        def sparse_quantize(self, coords):
            raise AssertionError("a refused mode must not reach the backend")
    pts = torch.tensor([[0, 0.5, 0.5, 0.5], [0, 1.5, 0.5, 0.5], [1, 0.25, 0, 2]])
    field = ME.TensorField(torch.ones(3, 4), pts)
    x = _tensor(np.array([[0, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 2]], np.int32), np.ones((3, 4), np.float32))
    backend.set_backend(Bare())           # (tests/conftest.py restores the backend)
    with pytest.raises(NotImplementedError, match=r"HIP backend \(ms3d_sparse_quantize\)"):
        field.sparse()
    with pytest.raises(NotImplementedError, match=r"HIP backend \(ms3d_interp_map\)"):
        x.interpolate(field)
    with pytest.raises(NotImplementedError, match=r"HIP backend \(ms3d_interp_map\)"):
        ME.MinkowskiInterpolation()(x, pts)
    with pytest.raises(NotImplementedError, match="HIP backend"):
        field.slice(x)                    # another manager: the lookup of SparseTensor.coordinate_rows
    backend.set_backend(QuantizeOnly())
    for mode in (QM.UNWEIGHTED_AVERAGE, QM.UNWEIGHTED_SUM, QM.MAX_POOL):
        with pytest.raises(NotImplementedError, match=r"HIP backend \(ms3d_field_reduce\)"):
            field.sparse(quantization_mode=mode)


def test_refusals():
    pts = torch.tensor([[0, 0.5, 0.5, 0.5], [0, 1.5, 0.5, 0.5]])
    field = ME.TensorField(torch.ones(2, 4), pts)
    for ts in (0, 3, 6, (2, 2, 2), 2.0):
        with pytest.raises(NotImplementedError, match="power of two"):
            field.sparse(tensor_stride=ts)
    with pytest.raises(NotImplementedError, match="quantization_mode"):
        ME.TensorField(torch.ones(2, 4), pts, quantization_mode=1)
    with pytest.raises(ValueError, match="coordinates"):
        ME.TensorField(torch.ones(2, 4), pts[:, 1:])
    with pytest.raises(ValueError, match="sparse"):
        field.inverse_mapping
    for geom in ((2, 3), (2, 4), (2, 1)):
        with pytest.raises(NotImplementedError):
            ME.MinkowskiPoolingTranspose(*geom)
    # a stride-2 pooling transpose needs the cached finer set: a tensor that was never downsampled has none
    x = _tensor(np.array([[0, 0, 0, 0], [0, 2, 0, 0]], np.int32), np.ones((2, 4), np.float32), ts=2)
    with pytest.raises(NotImplementedError, match="cached finer coordinate set"):
        ME.MinkowskiPoolingTranspose(2, 2)(x)
    with pytest.raises(NotImplementedError, match="cached finer coordinate set"):
        ME.MinkowskiPoolingTranspose(3, 2)(_tensor(np.array([[0, 0, 0, 0]], np.int32), np.ones((1, 4), np.float32)))


# ------------------------------------------------------------------------------------------ the yardstick itself, pinned
def _points(rng, n, B, lo, hi):
    p = np.empty((n, 4), np.float32)
    p[:, 0] = rng.integers(0, B, n)
    p[:, 1:] = rng.uniform(lo, hi, (n, 3))
    return p


@pytest.mark.parametrize("ts", [1, 2, 4])
def test_interp_np_is_grid_sample(ts):
    """values and feature gradient of the restatement against float64 grid_sample on the densified tensor (zeros padding,
    align_corners): negative coordinates, points on the lattice, points far outside and points of a batch the set lacks"""
    B, G, C, NQ = 2, 6, 5, 1500
    rng = np.random.default_rng(40 + ts)
    cells, x = random_sparse(rng, B=B, grid=G, n=int(0.6 * B * G ** 3), C=C)
    cells = cells.copy()
    cells[:, 1:] -= 3
    coords = cells.copy()
    coords[:, 1:] *= ts
    pts = np.concatenate([_points(rng, NQ, B, -3 * ts, 3 * ts), coords.astype(np.float32),
                          _points(rng, 8, B, 100 * ts, 101 * ts), _points(rng, 8, 1, -3 * ts, 3 * ts) + [B + 1, 0, 0, 0]])
    pts = pts.astype(np.float32)
    rows, weights = R.interp_map_np(coords, pts, ts)
    absent = (rows < 0).mean()
    assert 0.2 <= absent <= 0.8 and ((rows >= 0).all(0)).sum() >= 10 and ((rows < 0).all(0)).sum() >= 16
    assert weights.dtype == np.float32 and np.abs(weights.astype(np.float64).sum(0)[:-16] - 1).max() <= 4 * EPS
    got = R.interp_np(x, rows, weights)
    # dense: one cell of margin on every side of the 6^3 window that starts at cell -3
    leaf = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    c = torch.as_tensor(cells).long()
    dense = torch.zeros((B, G + 2, G + 2, G + 2, C), dtype=torch.float64)
    dense = dense.index_put((c[:, 0], c[:, 1] + 4, c[:, 2] + 4, c[:, 3] + 4), leaf).permute(0, 4, 1, 2, 3)
    want = R.grid_sample64(dense, -4, pts, ts)
    scale = want.detach().abs().max().item()
    assert scale > 0.5 and np.abs(got - want.detach().numpy()).max() <= 8 * EPS * scale
    assert not got[-16:].any()
    on = slice(NQ, NQ + len(coords))
    assert np.array_equal(rows[0, on], np.arange(len(coords))) and np.array_equal(got[on], x.astype(np.float64))
    dout = rng.standard_normal(got.shape)
    want.backward(torch.as_tensor(dout))
    g = R.interp_backward_np(dout, rows, weights, len(coords))
    assert np.abs(g - leaf.grad.numpy()).max() <= 8 * EPS * np.abs(g).max()


def test_interp_map_np_edges():
    """-0.5 lies in cell -1 (floor, not truncation); non-finite points and corners outside the packable range name no row"""
    coords = np.array([[0, -1, 0, 0], [0, 0, 0, 0], [0, 16383, 0, 0]], np.int32)
    pts = np.array([[0, -0.5, 0, 0], [0, np.nan, 0, 0], [0, np.inf, 0, 0], [0, 16383.5, 0, 0], [0, 1e30, 0, 0],
                    [-1, 0, 0, 0], [0, -16384.5, 0, 0]], np.float32)
    rows, weights = R.interp_map_np(coords, pts, 1)
    assert rows[:, 0].tolist() == [0, 1, -1, -1, -1, -1, -1, -1] and weights[:2, 0].tolist() == [0.5, 0.5]
    assert (rows[:, 1:3] == -1).all() and not weights[:, 1:3].any()
    assert rows[:, 3].tolist() == [2] + [-1] * 7 and weights[1, 3] == 0.5
    assert (rows[:, 4:] == -1).all() and np.isfinite(weights).all()


@pytest.mark.parametrize("ts", [1, 2])
def test_quantize_np_matches_index_add(ts):
    B, C = 3, 5
    rng = np.random.default_rng(50 + ts)
    pts = np.concatenate([_points(rng, 600, B, -6 * ts, 6 * ts), np.array([[1, -0.5, 0.0, 2.0], [1, -1.0, 0.0, 2.0]], np.float32)])
    feats = rng.standard_normal((len(pts), C)).astype(np.float32)
    coords, inverse, first = R.quantize_np(pts, ts)
    assert coords.dtype == np.int32 and (coords[:, 1:] % ts == 0).all()
    assert np.array_equal(coords[inverse[-2]], [1, -ts, 0, 2]) and inverse[-1] == inverse[-2]      # floor: -0.5 -> -ts
    # the set is the set of floored points, in first-occurrence order
    want = np.floor(pts[:, 1:].astype(np.float64) / ts).astype(np.int64) * ts
    assert np.array_equal(coords[inverse][:, 1:], want) and np.array_equal(coords[inverse][:, 0], pts[:, 0].astype(np.int64))
    assert np.array_equal(first, np.sort(first)) and np.array_equal(inverse[first], np.arange(len(first)))
    assert len(np.unique(coords, axis=0)) == len(coords) and np.bincount(inverse).max() > 1
    v = len(coords)
    acc = torch.zeros((v, C), dtype=torch.float64).index_add_(0, torch.as_tensor(inverse), torch.as_tensor(feats).double())
    cnt = np.bincount(inverse, minlength=v)
    s, _, count = R.reduce_np(R.SUM, feats, inverse, v)
    a, _, _ = R.reduce_np(R.AVG, feats, inverse, v)
    m, arg, _ = R.reduce_np(R.MAX, feats, inverse, v)
    f, _, _ = R.reduce_np(R.FIRST, feats, inverse, v)
    assert np.array_equal(count, cnt) and s.dtype == a.dtype == np.float32
    bound = cnt.max() * EPS * np.abs(feats).max() * cnt.max()
    assert np.abs(s - acc.numpy()).max() <= bound and np.abs(a - acc.numpy() / cnt[:, None]).max() <= bound
    for r in range(v):
        assert np.array_equal(m[r], feats[inverse == r].max(0)) and np.array_equal(f[r], feats[first[r]])
    assert np.array_equal(np.take_along_axis(feats, arg[inverse], 0)[first], m)
    # gradients: autograd on the same float64 expressions
    dvox = rng.standard_normal((v, C)).astype(np.float32)
    for mode in (R.SUM, R.AVG, R.MAX):
        leaf = torch.tensor(feats, dtype=torch.float64, requires_grad=True)
        idx = torch.as_tensor(inverse)
        if mode == R.MAX:
            y = torch.stack([leaf[idx == r].max(0).values for r in range(v)])
        else:
            y = torch.zeros((v, C), dtype=torch.float64).index_add(0, idx, leaf)
            if mode == R.AVG:
                y = y / torch.as_tensor(cnt).double()[:, None]
        y.backward(torch.as_tensor(dvox).double())
        g = R.reduce_backward_np(mode, dvox, inverse, arg, count)
        assert g.dtype == np.float32 and np.abs(g - leaf.grad.numpy()).max() <= 2 * EPS * np.abs(dvox).max()


# ------------------------------------------------------------------------------------------ plumbing over a numpy backend
class NumpyBackend:
    """the backend methods the new layers call, served by the restatements on CPU tensors: lets the engine's own plumbing run
    without a GPU.  spatial_order hands out a fixed shuffle, so a "sorted" manager holds its rows in another order than the
    caller sees and every composed map is exercised."""

    def spatial_order(self, coords):
        return torch.from_numpy(np.random.default_rng(len(coords)).permutation(len(coords)))

    def sparse_quantize(self, coords):
        _, inverse, first = R.quantize_np(coords.numpy(), 1)
        return torch.from_numpy(first.astype(np.int32)), torch.from_numpy(inverse.astype(np.int32))

    def kmap_general(self, in_coords, out_coords, offsets):
        table = {tuple(c): r for r, c in reversed(list(enumerate(in_coords.tolist())))}
        out = np.full((len(offsets), max(len(out_coords), 1)), -1, np.int32)
        for k, (dx, dy, dz) in enumerate(offsets.tolist()):
            for o, (b, x, y, z) in enumerate(out_coords.tolist()):
                out[k, o] = table.get((b, x + dx, y + dy, z + dz), -1)
        return torch.from_numpy(out)

    def scatter_add_rows(self, src, idx, n_rows, max_dup=None, sorted_=None):
        out = np.zeros((n_rows, src.size(1)), np.float32)
        for i, r in enumerate(idx.tolist()):
            out[r] += src[i].numpy()
        return torch.from_numpy(out)

    def field_reduce(self, mode, feats, order, seg_start, v):
        inverse = np.empty(len(order), np.int64)
        seg = seg_start.numpy()
        for r in range(v):
            pts = order[seg[r]:seg[r + 1]].numpy()
            assert np.array_equal(pts, np.sort(pts))
            inverse[pts] = r
        out, arg, _ = R.reduce_np(mode, feats.detach().numpy(), inverse, v)
        return torch.from_numpy(out), (torch.from_numpy(arg.astype(np.int32)) if mode == R.MAX else None)

    def field_reduce_backward(self, mode, dvox, inverse, seg_start, arg):
        count = np.diff(seg_start.numpy()).astype(np.int64)
        return torch.from_numpy(R.reduce_backward_np(mode, dvox.numpy(), inverse.numpy().astype(np.int64),
                                                     None if arg is None else arg.numpy().astype(np.int64), count))

    def interp_map(self, coords, points, ts):
        rows, weights = R.interp_map_np(coords.numpy(), points.numpy(), ts)
        return torch.from_numpy(rows), torch.from_numpy(weights)

    def interp_forward(self, x, rows, weights):
        return torch.from_numpy(R.interp_np(x.detach().numpy(), rows.numpy(), weights.numpy()).astype(np.float32))

    def interp_backward(self, dout, weights, entry_sorted, seg_start, vin):
        e, seg, w = entry_sorted.numpy(), seg_start.numpy(), weights.numpy()
        din = np.zeros((vin, dout.size(1)), np.float64)
        for r in range(vin):
            mine = e[seg[r]:seg[r + 1]]
            assert np.array_equal(mine, np.sort(mine)) and len(np.unique(mine >> 3)) == len(mine)
            for ent in mine:
                din[r] += float(w[ent & 7, ent >> 3]) * dout[ent >> 3].double().numpy()
        return torch.from_numpy(din.astype(np.float32))


@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("mode", [R.AVG, R.SUM, R.MAX, R.FIRST])
def test_engine_plumbing_over_a_numpy_backend(mode, sort, monkeypatch):
    from minsu3d_amd import backend
    from minsu3d_amd.MinkowskiEngine import tensor as T
    backend.set_backend(NumpyBackend())
    if sort:
        monkeypatch.setattr(T, "_SORT_MIN_ROWS", 10)
    rng = np.random.default_rng(60 + mode)
    B, C = 2, 4
    pts = _points(rng, 300, B, -3, 3)
    pts[:40, 1:] = np.round(pts[:40, 1:])                    # points with exact integer coordinates
    feats = rng.standard_normal((300, C)).astype(np.float32)
    leaf = torch.tensor(feats, requires_grad=True)
    points = torch.from_numpy(pts)
    field = ME.TensorField(leaf, points, quantization_mode=MODES[mode])
    x = field.sparse()
    coords, inverse, first = R.quantize_np(pts, 1)
    v = len(coords)
    assert (x.coordinate_manager.perm is not None) == sort
    want, arg, count = R.reduce_np(mode, feats, inverse, v)
    assert np.array_equal(x.C.numpy(), coords) and np.array_equal(field.inverse_mapping.numpy(), inverse)
    assert np.array_equal(x.F.detach().numpy(), want)
    dvox = rng.standard_normal((v, C)).astype(np.float32)
    x.F.backward(torch.from_numpy(dvox))
    if mode == R.FIRST:
        g = np.zeros_like(feats)
        g[first] = dvox
    else:
        g = R.reduce_backward_np(mode, dvox, inverse, arg, count)
    assert np.array_equal(leaf.grad.numpy(), g)
    # slice on the field's own tensor, and its gradient: a serial scatter-add in ascending point index
    xl = torch.tensor(want, requires_grad=True)
    y = ME.SparseTensor(xl[x.coordinate_manager.perm] if sort else xl, coordinate_manager=x.coordinate_manager)
    sl = field.slice(y)
    assert isinstance(sl, ME.TensorField) and sl.C is points and np.array_equal(sl.F.detach().numpy(), want[inverse])
    cs = y.cat_slice(field)
    assert np.array_equal(cs.F.detach().numpy(), np.concatenate([feats, want[inverse]], 1))
    dpt = rng.standard_normal((300, C)).astype(np.float32)
    sl.F.backward(torch.from_numpy(dpt), retain_graph=True)
    acc = np.zeros((v, C), np.float32)
    for n, r in enumerate(inverse):
        acc[r] += dpt[n]
    assert np.array_equal(xl.grad.numpy(), acc)
    # slice through a tensor on ANOTHER manager (half of the voxels, shuffled): absent voxels give the zero row
    keep = rng.permutation(v)[:v // 2]
    other = _tensor(coords[keep], want[keep])
    lookup = np.full(v, -1)
    lookup[keep] = np.arange(len(keep))
    got = field.slice(other).F.numpy()
    hit = lookup[inverse] >= 0
    assert hit.any() and (~hit).any() and np.array_equal(got[hit], want[keep][lookup[inverse][hit]]) and not got[~hit].any()
    assert field._rows_in(other) is field._rows_in(other)
    # interpolation on the (possibly re-ordered) manager: the map names the rows the caller sees, values and gradient follow
    xl.grad = None
    out, kmap, w = ME.MinkowskiInterpolation(return_kernel_map=True, return_weights=True)(y, points)
    rows, weights = R.interp_map_np(coords, pts, 1)
    assert np.array_equal(kmap.numpy(), rows) and np.array_equal(w.numpy(), weights)
    ref = R.interp_np(want, rows, weights)
    assert np.abs(out.detach().numpy() - ref).max() <= 4 * EPS * np.abs(ref).max()
    assert torch.equal(y.interpolate(field).F, out)
    cm = y.coordinate_manager
    assert cm.interpolation_map(1, points)[0] is cm.interpolation_map(1, points)[0]
    out.backward(torch.from_numpy(dpt))
    gref = R.interp_backward_np(dpt, rows, weights, v)
    assert np.abs(xl.grad.numpy() - gref).max() <= 4 * EPS * np.abs(gref).max()
    # an empty field
    empty = ME.TensorField(torch.zeros((0, C)), torch.zeros((0, 4))).sparse()
    assert tuple(empty.F.shape) == (0, C) and tuple(empty.C.shape) == (0, 4)
