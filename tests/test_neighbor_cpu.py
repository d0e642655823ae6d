"""Pooling and weighted sums over a neighbour index (ME.knn_map / NeighborMap, neighbor_pool, neighbor_sum, knn_interpolate;
csrc/neighbor.hip): what can be checked without a GPU -- the exports and the documents, the record (its translation into held
rows and its transposed table), the CPU path (the rules as torch expressions) against the serial numpy reference of
tests/neighbor_ref.py, torch.equal where the rule is a float32 chain and the project's bar of 1e-4 of the largest magnitude of
the float64 result otherwise, gradcheck in float64, every refusal, empty maps, and the host side of the library through ctypes
on the cross-compiled library: the getters, the workspace size and the return codes, all decided before a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import minsu3d_amd.MinkowskiEngine as ME
from fps_ref import random_voxels
from neighbor_ref import feature_grad_ref, idw_ref, pool_ref, table_ref, weight_grad_ref, wsum_ref
from test_knn_cpu import Shuffling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-4                                        # the project's bar: of the largest magnitude of the float64 result
SYMBOLS = ("ms3d_nbr_chunk_entries", "ms3d_nbr_ws_bytes", "ms3d_nbr_pool_forward", "ms3d_nbr_wsum_forward", "ms3d_nbr_backward",
           "ms3d_nbr_wsum_backward_w")
E_WORKSPACE, E_UNSUPPORTED = 10001, 10002          # MS3D_E_* of include/minsu3d_hip.h
# 7 queries over 5 rows, k = 3: invalid slots in every position, an all-invalid query, a row named twice by one query
HAND = torch.tensor([[0, 1, -1], [2, -1, 2], [-1, -1, -1], [1, 0, 2], [4, 4, 4], [-1, 3, 0], [3, 2, 1]])


def close(got, want, name):
    want = torch.as_tensor(want)
    assert tuple(got.shape) == tuple(want.shape), (name, tuple(got.shape), tuple(want.shape))
    err = ((got.detach().double() - want).abs().max() / want.abs().max().clamp_min(1e-30)).item() if want.numel() else 0.0
    print(f"{name}: rel err {err:.3e} (bound {RTOL:.0e})")
    assert err <= RTOL, (name, err)


def check_ops(x, nmap, idx, feats, seed=0):
    """every op and gradient of the CPU path on one map against the reference over the caller-order rows `feats` and the
    caller-numbered index `idx` [N, k]; x: what the ops take (a tensor with requires_grad, or a tensor object whose
    features derive from the leaf `feats`)"""
    def rows(t):
        t = t if torch.is_tensor(t) else t.F
        return t.reshape(-1, t.size(-1))

    idx_np, f_np = idx.reshape(-1, idx.size(-1)).numpy(), feats.detach().numpy()
    N, V = idx_np.shape[0], f_np.shape[0]
    g = torch.Generator().manual_seed(seed)
    dout = torch.randn(N, f_np.shape[1], generator=g)
    for mode in ("sum", "avg", "max"):
        want, arg = pool_ref(f_np, idx_np, mode)
        out = rows(ME.neighbor_pool(x, nmap, mode))
        assert torch.equal(out, torch.from_numpy(want)), mode
        feats.grad = None
        out.backward(dout, retain_graph=True)
        close(feats.grad, feature_grad_ref(dout.numpy(), idx_np, V, mode, arg=arg), f"d{mode}")
    w = torch.randn(idx.shape, generator=g).requires_grad_()
    with torch.no_grad():
        w[idx < 0] = float("nan")                   # the weight of an invalid slot is never read
    out = rows(ME.neighbor_sum(x, nmap, w))
    w_np = w.detach().reshape(N, -1).numpy()
    close(out, wsum_ref(f_np, idx_np, w_np), "wsum")
    feats.grad = None
    out.backward(dout, retain_graph=True)
    close(feats.grad, feature_grad_ref(dout.numpy(), idx_np, V, "weighted", w=np.nan_to_num(w_np)), "wsum dx")
    close(w.grad.reshape(N, -1), weight_grad_ref(dout.numpy(), f_np, idx_np), "wsum dw")
    assert bool((w.grad[idx < 0] == 0).all())           # an invalid slot receives a zero weight gradient
    if nmap.d2 is not None:
        close(rows(ME.knn_interpolate(x, nmap)), wsum_ref(f_np, idx_np, idw_ref(idx_np, nmap.d2.reshape(N, -1).numpy())), "idw")


def test_exported_and_documented():
    import minsu3d_amd.dropin.MinkowskiEngine as dropin
    from minsu3d_amd import backend
    for name in ("knn_map", "NeighborMap", "neighbor_pool", "neighbor_sum", "knn_interpolate", "MinkowskiKNNPooling",
                 "MinkowskiKNNInterpolation"):
        assert getattr(dropin, name) is getattr(ME, name) and name in dropin.__all__
    assert ME.NeighborMap is backend.NeighbourGroup
    doc = ME.__doc__
    line = "knn_map(x, k, queries=None, max_squared_distance=None) -> NeighborMap"
    assert doc.index("knn_query(x, k, queries=None") < doc.index(line) < doc.index("Not supported (each raises")
    assert doc.count("Not supported") == 1
    section = doc[doc.index(line):doc.index("Not supported (each raises")]
    for word in ("The rules, all of them", "lowest slot wins ties", "first slot", "fmaf", "bit for bit", "1 <= k <= 254", "idx_held",
                 "ms3d_nbr_chunk_entries", "ms3d_nbr_pool_forward", "Out of scope", "per-head", "float16", "from_index",
                 "MinkowskiKNNPooling", "MinkowskiKNNInterpolation", "not differentiable"):
        assert word in section, word
    assert "a fused neighbour gather" not in doc and "a fused neighbour gather" not in ME.knn_query.__doc__
    assert "neighbor_pool" in ME.knn_query.__doc__
    assert len(list(ME.MinkowskiKNNPooling(3).parameters())) == 0 == len(list(ME.MinkowskiKNNInterpolation().parameters()))
    for path in ("README.md", "DESIGN.md"):
        assert "neighbor_pool" in open(os.path.join(ROOT, path)).read(), path


def test_hand_made_map_record_and_ops():
    m = ME.NeighborMap.from_index(HAND, 5)
    assert (m.N, m.k, m.V, m.lead) == (7, 3, 5, (7,)) and m.d2 is None and m.idx is HAND
    assert torch.equal(m.idx_held, HAND) and m.valid.dtype == torch.int32 and m.valid.tolist() == [2, 2, 0, 3, 3, 2, 3]
    e, seg = m.entry_sorted.numpy(), m.seg_start.numpy()
    assert m.entry_sorted.dtype == torch.int64 and m.seg_start.dtype == torch.int32
    want_e, want_seg = table_ref(HAND.numpy(), 5)
    assert np.array_equal(e, want_e) and np.array_equal(seg, want_seg)
    assert m.table is m.table                                       # made once and kept
    feats = torch.randn(5, 6, requires_grad=True)
    check_ops(feats, m, HAND, feats)
    lead = ME.NeighborMap.from_index(HAND[:6].view(2, 3, 3), 5)      # leading shape [2, 3]
    out = ME.neighbor_pool(feats, lead, "sum")
    assert tuple(out.shape) == (2, 3, 6) and torch.equal(out.view(6, 6), ME.neighbor_pool(feats, m, "sum")[:6])


@pytest.mark.parametrize("V,N,k", [(1, 1, 1), (40, 33, 5), (9, 300, 16), (300, 7, 254)])
def test_table_invariants(V, N, k):
    rng = np.random.default_rng(V + N + k)
    idx = rng.integers(-V // 3 - 1, V, size=(N, k))
    m = ME.NeighborMap.from_index(torch.from_numpy(idx), V)
    e, seg = m.entry_sorted.numpy(), m.seg_start.numpy()
    of_row = idx.reshape(-1)[e]
    assert seg.shape == (V + 1,) and seg[0] == 0 and seg[-1] == len(e) == (idx >= 0).sum()
    assert np.array_equal(of_row, np.sort(of_row)) and np.array_equal(np.bincount(of_row, minlength=V), np.diff(seg))
    assert all(np.all(np.diff(e[seg[r]:seg[r + 1]]) > 0) for r in range(V))           # ascending entry inside a row
    assert np.array_equal(m.valid.numpy(), (idx >= 0).sum(1))


def test_max_ties_and_nan():
    feats = torch.tensor([[1.0, 5.0], [1.0, 7.0], [float("nan"), 2.0], [1.0, 7.0]], requires_grad=True)
    idx = torch.tensor([[0, 1, 3], [3, 1, 0], [2, 0, 1], [0, 2, 1], [-1, 1, 3]])
    m = ME.NeighborMap.from_index(idx, 4)
    out = ME.neighbor_pool(feats, m, "max")
    want, arg = pool_ref(feats.detach().numpy(), idx.numpy(), "max")
    assert torch.equal(torch.from_numpy(want).isnan(), out.isnan())
    assert torch.equal(torch.nan_to_num(out, nan=-1.0), torch.nan_to_num(torch.from_numpy(want), nan=-1.0))
    assert arg.tolist() == [[0, 1], [0, 0], [0, 2], [0, 2], [1, 1]]          # lowest slot on ties; a NaN only from slot 0
    assert np.isnan(want[2, 0]) and want[3, 0] == 1.0
    out.backward(torch.ones_like(out))
    close(feats.grad, feature_grad_ref(np.ones((5, 2)), idx.numpy(), 4, "max", arg=arg), "dmax on ties")


def test_single_weight_one_neighbour_is_a_copy():
    feats = torch.randn(6, 5)
    idx = torch.tensor([[-1, 4, -1], [2, -1, -1], [-1, -1, 0]])
    w = torch.full((3, 3), float("nan"))
    w[idx >= 0] = 1.0
    assert torch.equal(ME.neighbor_sum(feats, ME.NeighborMap.from_index(idx, 6), w), feats[[4, 2, 0]])


def test_gradcheck_float64():
    idx = torch.tensor([[0, 1, 2], [3, 4, 0], [1, -1, 3], [2, 2, 4], [4, 0, 1], [3, 1, 2], [0, 4, 3]])
    assert idx.shape == (7, 3) and int((idx < 0).sum()) == 1
    d2 = torch.rand(7, 3)
    m = ME.NeighborMap.from_index(idx, 5, d2)
    x = torch.randn(5, 4, dtype=torch.float64, requires_grad=True)
    w = torch.randn(7, 3, dtype=torch.float64, requires_grad=True)
    for mode in ("sum", "avg", "max"):
        assert torch.autograd.gradcheck(lambda t: ME.neighbor_pool(t, m, mode), (x,))
    assert torch.autograd.gradcheck(lambda t, u: ME.neighbor_sum(t, m, u), (x, w))
    assert torch.autograd.gradcheck(lambda t: ME.knn_interpolate(t, m), (x,))


def _sparse(coords, feats, **kw):
    c = torch.as_tensor(np.asarray(coords), dtype=torch.int32)
    cm = ME.CoordinateManager(c, **kw)
    return ME.SparseTensor(feats, coordinate_map_key=ME.CoordinateMapKey(cm, 1))      # features in the CALLER's order


@pytest.mark.parametrize("shuffled", [False, True])
def test_knn_made_maps_all_three_forms(shuffled):
    from minsu3d_amd import backend
    backend.set_backend(Shuffling())                 # with spatial_sort: held order != caller order (conftest restores it)
    c = random_voxels([30, 22], seed=4, side=6)
    feats = torch.randn(c.shape[0], 6, requires_grad=True)
    x = _sparse(c, feats, spatial_sort=shuffled)
    cm = x.coordinate_manager
    assert (cm.perm is not None) == shuffled
    # queries=None: the target is x's own set
    m = ME.knn_map(x, 4)
    idx, d2 = ME.knn_query(x, 4)
    assert torch.equal(m.idx, idx) and torch.equal(m.d2, d2) and (m.N, m.k, m.V) == (52, 4, 52)
    out = ME.neighbor_pool(x, m, "max")
    assert isinstance(out, ME.SparseTensor) and out.coordinate_manager is cm and out.tensor_stride == 1
    check_ops(x, m, idx, feats)
    if shuffled:                                     # the values are held rows, the rows in held order
        assert torch.equal(m.idx_held, cm.inv[idx][cm.perm])
        # the table: grouped by HELD support row; inside a row ascending in the CALLER's numbering of the queries
        e, seg = m.entry_sorted, m.seg_start.tolist()
        assert torch.equal(m.idx_held.view(-1)[e], torch.arange(52).repeat_interleave(m.seg_start.diff().long()))
        in_caller = cm.perm[e // 4] * 4 + e % 4
        want_e, want_seg = table_ref(idx.numpy(), 52)
        for v in range(52):
            r = int(cm.perm[v])
            assert in_caller[seg[v]:seg[v + 1]].tolist() == want_e[want_seg[r]:want_seg[r + 1]].tolist()
    # a capped map: trailing -1 slots
    capped = ME.knn_map(x, 3, max_squared_distance=1)
    assert int((capped.idx < 0).sum()) > 0
    check_ops(x, capped, capped.idx, feats, seed=1)
    # [B, M] picks: no target set, plain [B, M, C]
    picks = ME.farthest_point_sampling(x, 5)
    pm = ME.knn_map(x, 3, picks)
    out = ME.neighbor_pool(x, pm, "avg")
    assert torch.is_tensor(out) and tuple(out.shape) == (2, 5, 6)
    check_ops(x, pm, pm.idx, feats, seed=2)
    # y: another set (stride 2 of the same manager); both directions
    cm.k2(1)
    coarse_feats = torch.randn(cm.coords[2].size(0), 6, requires_grad=True)
    y = ME.SparseTensor(coarse_feats, coordinate_manager=cm, tensor_stride=2)
    down = ME.knn_map(x, 3, y)
    out = ME.neighbor_pool(x, down, "max")
    assert isinstance(out, ME.SparseTensor) and out.tensor_stride == 2 and out.coordinate_manager is cm
    check_ops(x, down, down.idx, feats, seed=3)
    up = ME.knn_map(y, 3, x)
    out = ME.knn_interpolate(y, up)
    assert isinstance(out, ME.SparseTensor) and out.tensor_stride == 1 and tuple(out.F.shape) == (52, 6)
    check_ops(y, up, up.idx, coarse_feats, seed=4)
    out = ME.MinkowskiKNNInterpolation(3)(y, x)
    assert torch.equal(out.F, ME.knn_interpolate(y, up).F)
    assert torch.equal(ME.MinkowskiKNNPooling(3, "max")(x, y).F, ME.neighbor_pool(x, down, "max").F)
    assert torch.equal(ME.MinkowskiKNNPooling(9, "max")(x, nmap=down).F, ME.neighbor_pool(x, down, "max").F)


def test_field_maps():
    rng = np.random.default_rng(5)
    p = np.concatenate([rng.integers(0, 2, (40, 1)), rng.random((40, 3)) * 4], 1).astype(np.float32)
    q = np.concatenate([rng.integers(0, 2, (11, 1)), rng.random((11, 3)) * 4], 1).astype(np.float32)
    feats = torch.randn(40, 3, requires_grad=True)
    x, y = ME.TensorField(feats, torch.from_numpy(p)), ME.TensorField(torch.zeros(11, 1), torch.from_numpy(q))
    m = ME.knn_map(x, 3, y, max_squared_distance=1.5)
    out = ME.knn_interpolate(x, m)
    assert isinstance(out, ME.TensorField) and out.C is y.C and tuple(out.F.shape) == (11, 3) and m.d2.dtype == torch.float32
    check_ops(x, m, m.idx, feats)
    with pytest.raises(ValueError, match="another set"):
        ME.neighbor_pool(y, m)


def test_refusals():
    with pytest.raises(ValueError, match="int64"):
        ME.NeighborMap.from_index(HAND.to(torch.int32), 5)
    with pytest.raises(ValueError, match="int64"):
        ME.NeighborMap.from_index(HAND.tolist(), 5)
    with pytest.raises(ValueError, match="no row of 4"):
        ME.NeighborMap.from_index(HAND, 4)
    with pytest.raises(ValueError, match="254"):
        ME.NeighborMap.from_index(torch.zeros((2, 255), dtype=torch.int64), 5)
    with pytest.raises(ValueError, match="k = 0"):
        ME.NeighborMap.from_index(torch.zeros((2, 0), dtype=torch.int64), 5)
    with pytest.raises(ValueError, match="shape of idx"):
        ME.NeighborMap.from_index(HAND, 5, d2=torch.zeros(7, 2))
    ME.NeighborMap.from_index(torch.zeros((2, 254), dtype=torch.int64), 5)
    m = ME.NeighborMap.from_index(HAND, 5)
    feats = torch.randn(5, 4)
    with pytest.raises(ValueError, match="mode"):
        ME.neighbor_pool(feats, m, "min")
    with pytest.raises(ValueError, match="5 rows"):
        ME.neighbor_pool(torch.randn(6, 4), m)
    with pytest.raises(ValueError, match=r"\[V, C\]"):
        ME.neighbor_pool(torch.randn(5), m)
    with pytest.raises(TypeError, match="NeighborMap"):
        ME.neighbor_pool(feats, HAND)
    with pytest.raises(TypeError, match="SparseTensor"):
        ME.neighbor_pool([1.0], m)
    for dtype in (torch.float16, torch.bfloat16, torch.int64):
        with pytest.raises(NotImplementedError, match="rows"):
            ME.neighbor_pool(feats.to(dtype), m)
    with pytest.raises(NotImplementedError, match="per-head"):
        ME.neighbor_sum(feats, m, torch.randn(7, 3, 2))
    with pytest.raises(ValueError, match="shape of the index"):
        ME.neighbor_sum(feats, m, torch.randn(7, 2))
    with pytest.raises(ValueError, match="float tensor"):
        ME.neighbor_sum(feats, m, HAND)
    with pytest.raises(ValueError, match="float64"):
        ME.neighbor_sum(feats, m, torch.randn(7, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="no distances"):
        ME.knn_interpolate(feats, m)
    # a map serves the set it was made for: another manager, another stride, plain rows
    c = random_voxels([20], seed=1, side=5)
    x = ME.SparseTensor(torch.randn(20, 4), coordinate_manager=ME.CoordinateManager(torch.from_numpy(c)))
    other = ME.SparseTensor(torch.randn(20, 4), coordinate_manager=ME.CoordinateManager(torch.from_numpy(c)))
    km = ME.knn_map(x, 2)
    ME.neighbor_pool(x._like(torch.randn(20, 4)), km)                         # the same set, other features: fine
    for wrong in (other, torch.randn(20, 4)):
        with pytest.raises(ValueError, match="another set"):
            ME.neighbor_pool(wrong, km)
    with pytest.raises(ValueError, match="another set"):
        ME.neighbor_pool(x, ME.NeighborMap.from_index(km.idx, 20))
    with pytest.raises(TypeError, match="mixed kinds"):
        ME.knn_map(x, 2, ME.TensorField(torch.zeros(3, 1), torch.zeros(3, 4)))
    with pytest.raises(ValueError, match="k must be"):
        ME.knn_map(x, 65)
    for bad in (0, True, 2.0):
        with pytest.raises(ValueError, match="k must be"):
            ME.MinkowskiKNNPooling(bad)
        with pytest.raises(ValueError, match="k must be"):
            ME.MinkowskiKNNInterpolation(bad)
    with pytest.raises(ValueError, match="mode"):
        ME.MinkowskiKNNPooling(3, "min")


def test_device_rows_without_the_kernels_name_the_entry_point(monkeypatch):
    """the refusal of a backend without ms3d_nbr_pool_forward, reached without a device: the ops look at is_cuda only"""
    from minsu3d_amd import backend
    from minsu3d_amd.MinkowskiEngine import functional as Fn

    class Rows:                                       # what _nbr_input reads of a device tensor
        is_cuda, dtype, device = True, torch.float32, torch.device("cpu")

        def dim(self):
            return 2

        def size(self, i):
            return (5, 4)[i]

        def is_floating_point(self):
            return True

    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, Rows)))
    backend.set_backend(Shuffling())
    with pytest.raises(NotImplementedError, match="ms3d_nbr_pool_forward"):
        Fn.neighbor_pool(Rows(), ME.NeighborMap.from_index(HAND, 5))


def test_empty_maps():
    feats = torch.randn(5, 4, requires_grad=True)
    m = ME.NeighborMap.from_index(torch.empty((0, 3), dtype=torch.int64), 5)                  # N == 0
    w = torch.randn(0, 3, requires_grad=True)
    for out in (ME.neighbor_pool(feats, m, "max"), ME.neighbor_pool(feats, m, "avg"), ME.neighbor_sum(feats, m, w)):
        assert tuple(out.shape) == (0, 4)
        feats.grad = None
        out.sum().backward()
        assert tuple(feats.grad.shape) == (5, 4) and not feats.grad.any()
    assert tuple(w.grad.shape) == (0, 3) and m.entry_sorted.numel() == 0 and m.seg_start.tolist() == [0] * 6
    m = ME.NeighborMap.from_index(torch.empty((2, 0, 3), dtype=torch.int64), 5)               # [B, 0, k]
    assert tuple(ME.neighbor_pool(feats, m, "sum").shape) == (2, 0, 4)
    none = torch.randn(0, 4, requires_grad=True)                                              # V == 0
    m = ME.NeighborMap.from_index(torch.full((3, 2), -1), 0)
    w = torch.randn(3, 2, requires_grad=True)
    for out in (ME.neighbor_pool(none, m, "max"), ME.neighbor_pool(none, m, "avg"), ME.neighbor_sum(none, m, w)):
        assert tuple(out.shape) == (3, 4) and not out.any()
        none.grad = None
        out.sum().backward()
        assert tuple(none.grad.shape) == (0, 4)
    assert tuple(w.grad.shape) == (3, 2) and not w.grad.any() and m.seg_start.tolist() == [0]
    x = ME.SparseTensor(torch.randn(0, 4), coordinate_manager=ME.CoordinateManager(torch.zeros((0, 4), dtype=torch.int32)))
    em = ME.knn_map(x, 2)
    out = ME.neighbor_pool(x, em, "max")
    assert isinstance(out, ME.SparseTensor) and tuple(out.F.shape) == (0, 4)


# ---------------------------------------------------------------------------------------------- the library's host side
@pytest.fixture(scope="module")
def lib():
    from minsu3d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    so.ms3d_nbr_ws_bytes.restype = ctypes.c_size_t
    return so


def test_header_and_library_surface(lib):
    text = open(os.path.join(ROOT, "include", "minsu3d_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", code), s
        assert hasattr(lib, s), s
    T = lib.ms3d_nbr_chunk_entries()
    assert T >= 64 and T & (T - 1) == 0
    assert lib.ms3d_nbr_ws_bytes(ctypes.c_long(0), 64) == 0 == lib.ms3d_nbr_ws_bytes(ctypes.c_long(5), 0)
    assert lib.ms3d_nbr_ws_bytes(ctypes.c_long(7), 33) == 7 * 33 * 4
    from minsu3d_amd import backend
    assert backend.get_backend().nbr_chunk_entries() == T and backend.NBR_MAX_K == 254


def test_return_codes_are_decided_before_a_launch(lib):
    L, P = ctypes.c_long, ctypes.c_void_p
    buf = ctypes.create_string_buffer(256)
    p = P((ctypes.addressof(buf) + 15) & ~15)                          # a non-NULL, 16-byte aligned host address; never followed
    null = P(0)

    def pool(mode=0, x=p, V=4, idx=p, N=3, k=2, C=4, out=p, arg=p):
        return lib.ms3d_nbr_pool_forward(mode, x, L(V), idx, L(N), k, C, out, arg, null)

    def wsum(x=p, V=4, idx=p, w=p, N=3, k=2, C=4, out=p):
        return lib.ms3d_nbr_wsum_forward(x, L(V), idx, w, L(N), k, C, out, null)

    def bwd(mode=2, dout=p, w=p, arg=p, valid=p, es=p, seg=p, cs=p, n_chunks=0, V=4, N=3, k=2, C=4, dx=p, ws=null, ws_bytes=0):
        return lib.ms3d_nbr_backward(mode, dout, w, arg, valid, es, seg, cs, L(n_chunks), L(V), L(N), k, C, dx, ws,
                                     ctypes.c_size_t(ws_bytes), null)

    def bww(dout=p, x=p, idx=p, N=3, k=2, C=4, dw=p):
        return lib.ms3d_nbr_wsum_backward_w(dout, x, idx, L(N), k, C, dw, null)

    for bad in (dict(mode=-1), dict(mode=3), dict(k=0), dict(k=255), dict(C=0), dict(N=-1), dict(V=-1), dict(V=2 ** 31),
                dict(N=2 ** 31), dict(N=2 ** 30, k=2), dict(idx=null), dict(out=null), dict(x=null), dict(arg=null)):
        assert pool(**bad) == E_UNSUPPORTED, bad
    assert pool(N=0, idx=null, out=null, x=null, arg=null) == 0         # zero output rows: nothing is launched or looked at
    assert pool(mode=2, N=0, k=254) == 0
    for bad in (dict(k=0), dict(k=255), dict(C=0), dict(N=-1), dict(N=2 ** 30), dict(idx=null), dict(w=null), dict(out=null),
                dict(x=null)):
        assert wsum(**bad) == E_UNSUPPORTED, bad
    assert wsum(N=0, idx=null, w=null, out=null) == 0
    for bad in (dict(mode=-1), dict(mode=4), dict(k=0), dict(k=255), dict(C=0), dict(V=-1), dict(N=-1), dict(n_chunks=-1),
                dict(n_chunks=2 ** 31), dict(seg=null), dict(cs=null), dict(dx=null), dict(dout=null), dict(es=null),
                dict(mode=3, w=null), dict(mode=0, arg=null), dict(mode=1, valid=null), dict(n_chunks=1, ws=null, ws_bytes=64),
                dict(n_chunks=1, ws=P(p.value + 4), ws_bytes=64)):
        assert bwd(**bad) == E_UNSUPPORTED, bad
    assert bwd(n_chunks=2, ws=p, ws_bytes=2 * 4 * 4 - 1) == E_WORKSPACE
    assert bwd(V=0, seg=null, cs=null, dx=null) == 0
    assert bwd(mode=2, w=null, arg=null, valid=null, V=0) == 0           # read for their mode only
    for bad in (dict(k=0), dict(k=255), dict(C=0), dict(N=-1), dict(dout=null), dict(x=null), dict(idx=null), dict(dw=null)):
        assert bww(**bad) == E_UNSUPPORTED, bad
    assert bww(N=0, dout=null, x=null, idx=null, dw=null) == 0
