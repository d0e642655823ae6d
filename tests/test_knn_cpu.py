"""k nearest neighbours per sample (ME.knn_query, csrc/knn.hip): what can be checked without a GPU -- the exports and the
documents, the CPU path (the rule as a torch expression) against the serial numpy reference of tests/knn_ref.py with
torch.equal on the rows AND the distances, every refusal, the caches, and the host side of the library through ctypes on the
cross-compiled library: the getters, the workspace size and every return code, which are all decided before a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import minsu3d_amd.MinkowskiEngine as ME
from fps_ref import lattice, random_voxels
from knn_ref import knn_forms, knn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ms3d_knn_max_k", "ms3d_knn_queries_per_group", "ms3d_knn_rows_per_tile", "ms3d_knn_ws_bytes", "ms3d_knn_i32",
           "ms3d_knn_f32")
E_WORKSPACE, E_UNSUPPORTED = 10001, 10002          # MS3D_E_* of include/minsu3d_hip.h
# batch indices 0, 2 and 5 (gaps), the rows of the samples interleaved
GAPS = random_voxels([9, 6, 12], seed=3, side=6, batch_indices=[0, 2, 5])


def _sparse(coords, **kw):
    c = torch.as_tensor(np.asarray(coords), dtype=torch.int32)
    return ME.SparseTensor(torch.randn(c.size(0), 3), coordinate_manager=ME.CoordinateManager(c, **kw))


def _field(points, dtype=torch.float32):
    c = torch.as_tensor(np.asarray(points)).to(dtype)
    return ME.TensorField(torch.randn(c.size(0), 2), c)


def _coords(t):
    return (t._points32() if isinstance(t, ME.TensorField) else t.C).numpy()


def _same(x, k, queries=None, cap=None):
    """the CPU path against the serial reference over the caller-order coordinates: rows and distances, bit for bit"""
    got_i, got_d = ME.knn_query(x, k, queries, cap)
    kw = {}
    if torch.is_tensor(queries):
        kw["rows"] = queries.numpy()
    elif queries is not None:
        kw["other"] = _coords(queries)
    want_i, want_d = knn_forms(_coords(x), k, cap=cap, **kw)
    assert got_i.dtype == torch.int64 and tuple(got_i.shape) == want_i.shape
    assert got_d.dtype == (torch.float32 if isinstance(x, ME.TensorField) else torch.int64) and tuple(got_d.shape) == want_d.shape
    assert torch.equal(got_i, torch.from_numpy(want_i))
    assert torch.equal(got_d, torch.from_numpy(want_d))
    return got_i, got_d


class Shuffling:
    """a backend that holds the rows in another order than the caller's (what the Morton sort does on the device), and makes
    the stride-2 set of a manager"""

    def spatial_order(self, coords):
        return torch.from_numpy(np.random.default_rng(11).permutation(coords.size(0)))

    def downsample(self, coords, ts):
        c = coords.numpy()
        q = np.concatenate([c[:, :1], c[:, 1:] // (2 * ts) * (2 * ts)], 1)
        _, first, parent = np.unique(q, axis=0, return_index=True, return_inverse=True)
        rank = np.argsort(np.argsort(first))                      # first-occurrence order
        return (torch.from_numpy(q[np.sort(first)]), torch.from_numpy(rank[parent.reshape(-1)].astype(np.int32)),
                torch.zeros(c.shape[0], dtype=torch.int32))

    def kmap_k2(self, parent, koff, vc):
        return None, None


def test_exported_from_the_package_and_the_dropin():
    import minsu3d_amd.dropin.MinkowskiEngine as dropin
    assert callable(ME.knn_query)
    assert dropin.knn_query is ME.knn_query and "knn_query" in dropin.__all__
    doc = ME.__doc__
    line = "knn_query(x, k, queries=None, max_squared_distance=None) -> (idx int64 [..., k], d2 [..., k])"
    assert line in doc
    assert doc.index("farthest_point_sampling(x, num_samples, start=None)") < doc.index(line) < doc.index("Not supported (each raises")
    assert doc.count("Not supported") == 1
    section = doc[doc.index(line):doc.index("Not supported (each raises")]
    for word in ("The rule, all of it", "lowest caller row", "3 221 028 867", "FMA", "mask before indexing", "boundary included",
                 "ms3d_knn_i32", "ms3d_knn_queries_per_group", "ms3d_knn_rows_per_tile", "[B, M, k]", "Out of scope", "TypeError"):
        assert word in section, word
    fps_section = doc[doc.index("farthest_point_sampling(x, num_samples"):doc.index(line)]
    assert "knn_query" in fps_section and "kNN or ball grouping" not in doc
    own = ME.knn_query.__doc__
    for word in ("The rule, all of it", "lowest caller row", "3 221 028 867", "FMA", "mask before indexing", "ValueError",
                 "TypeError", "[B, M, k]", "2^22", "not differentiable", "Out of scope", "farthest_point_sampling"):
        assert word in own, word
    assert "knn_query" in ME.farthest_point_sampling.__doc__ and "kNN or ball grouping" not in ME.farthest_point_sampling.__doc__
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "knn_query" in design and "csrc/knn.hip" in design
    assert design.index("csrc/fps.hip") < design.index("csrc/knn.hip")
    assert "knn_query" in open(os.path.join(ROOT, "README.md")).read()


def test_header_declares_the_symbols():
    text = open(os.path.join(ROOT, "include", "minsu3d_hip.h")).read()
    assert "csrc/knn.hip" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ms3d_[a-z0-9_]+)\s*\(", text))
    for s in SYMBOLS:
        assert s in declared, s


def test_hand_worked_example():
    """rows (0,0) (1,0) (5,0) (5,5) (2,2) (0,1) in the plane z = 0; from row 0 the squared distances are 0 1 25 50 8 1: itself,
    then rows 1 and 5 tie at 1 and the lower row comes first, then row 4 at 8"""
    c = [[0, 0, 0, 0], [0, 1, 0, 0], [0, 5, 0, 0], [0, 5, 5, 0], [0, 2, 2, 0], [0, 0, 1, 0]]
    idx, d2 = ME.knn_query(_sparse(c), 4)
    assert idx[0].tolist() == [0, 1, 5, 4] and d2[0].tolist() == [0, 1, 1, 8]
    assert idx[3].tolist() == [3, 4, 2, 1] and d2[3].tolist() == [0, 18, 25, 41]
    ri, rd = knn_ref(np.array(c), 4, np.array(c))
    assert ri[0].tolist() == [0, 1, 5, 4] and rd[3].tolist() == [0, 18, 25, 41]


@pytest.mark.parametrize("n,k", [(4, 7), (4, 64), (9, 16)])
def test_lattice_ties_on_both_manager_kinds(n, k):
    from minsu3d_amd import backend
    c = lattice(n, seed=5)
    plain = _same(_sparse(c, spatial_sort=False), k)
    backend.set_backend(Shuffling())                 # (tests/conftest.py restores the backend)
    x = _sparse(c, spatial_sort=True)
    cm = x.coordinate_manager
    assert cm.perm is not None and cm.caller_rows(1) is not None and not torch.equal(cm.coords[1], x.C)
    shuffled = _same(x, k)
    assert torch.equal(plain[0], shuffled[0]) and torch.equal(plain[1], shuffled[1])
    assert plain[0][:, 0].tolist() == list(range(n ** 3))          # every row finds itself first
    picks = torch.tensor([[5, 0, 5, n ** 3 - 1]])                   # a duplicate inside the row is legal
    rows = _same(x, k, picks)
    assert torch.equal(rows[0], plain[0][picks]) and torch.equal(rows[1], plain[1][picks])


@pytest.mark.parametrize("k", [1, 2, 3, 6])
def test_gaps_and_interleaved_rows(k):
    x = _sparse(GAPS)
    idx, _ = _same(x, k)                               # k = 6 is the whole sample of batch index 2, sorted
    batch = torch.from_numpy(GAPS[:, 0]).long()
    assert torch.equal(batch[idx], batch[:, None].expand(-1, k))
    rows = [np.flatnonzero(GAPS[:, 0] == b) for b in (0, 2, 5)]
    picks = torch.tensor([[rows[0][4], rows[0][0]], [rows[1][5], rows[1][5]], [rows[2][0], rows[2][11]]])
    got = _same(x, k, picks)
    assert tuple(got[0].shape) == (3, 2, k) and torch.equal(got[0], idx[picks])
    if k == 6:
        assert sorted(idx[rows[1][0]].tolist()) == rows[1].tolist()


def test_another_set_with_a_subset_of_the_batch_indices():
    """y holds batch indices 5 and 0 of x's 0, 2, 5, its rows in another order; sample 2 of x has no queries, so k may exceed it"""
    x = _sparse(GAPS)
    y = random_voxels([7, 4], seed=9, side=6, batch_indices=[5, 0])
    idx, d2 = _same(x, 8, _sparse(y))
    assert tuple(idx.shape) == (11, 8)
    assert torch.equal(torch.from_numpy(GAPS[:, 0]).long()[idx], torch.from_numpy(y[:, 0]).long()[:, None].expand(-1, 8))
    with pytest.raises(ValueError, match=r"k = 8 is larger than sample 1, which has 6 rows"):
        ME.knn_query(x, 8)
    absent = random_voxels([3, 2], seed=9, side=6, batch_indices=[5, 3])
    with pytest.raises(ValueError, match="batch index 3 is present in queries and absent from x"):
        ME.knn_query(x, 1, _sparse(absent))


def test_stride_two_set_and_rooted_manager():
    from minsu3d_amd import backend
    backend.set_backend(Shuffling())                 # (tests/conftest.py restores the backend)
    c = random_voxels([40, 25], seed=8, side=8)
    cm = ME.CoordinateManager(torch.from_numpy(c), spatial_sort=True)
    cm.k2(1)
    coarse = cm.coords[2]
    assert 0 < coarse.size(0) < c.shape[0] and cm.perm is not None
    fine = ME.SparseTensor(torch.randn(c.shape[0], 3), coordinate_manager=cm)
    x = ME.SparseTensor(torch.randn(coarse.size(0), 3), coordinate_manager=cm, tensor_stride=2)
    _same(x, 5)
    _same(x, 3, fine)                                  # every fine row finds its three nearest coarse rows
    _same(fine, 4, x)
    rooted = ME.SparseTensor(torch.randn(coarse.size(0), 3), coordinate_manager=ME.CoordinateManager.rooted(coarse, 2),
                             tensor_stride=2)
    a, b = _same(rooted, 3, fine), ME.knn_query(x, 3, fine)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_distances_above_two_to_the_31():
    """from row 0 the far corner is 3 * 32767^2 = 3 221 028 867 away, which as a signed 32-bit number is negative: signed
    arithmetic puts it before the origin (805 306 368 away)"""
    c = np.array([[0, -16384, -16384, -16384], [0, 0, 0, 0], [0, 16383, 16383, 16383]], np.int32)
    assert np.int32(np.uint32(3221028867)) < 3 * 16384 ** 2
    idx, d2 = _same(_sparse(c), 3)
    assert idx[0].tolist() == [0, 1, 2] and d2[0].tolist() == [0, 805306368, 3221028867]
    assert idx[2].tolist() == [2, 1, 0] and d2.dtype == torch.int64


def _points(shift=0.0, samples=2, n=200):
    parts = []
    for seed in range(samples):
        p = np.random.default_rng(seed).integers(0, 12, (n, 3)) * np.float32(0.1)
        parts.append(np.concatenate([np.full((n, 1), 2 * seed, np.float32), (p + np.float32(shift)).astype(np.float32)], 1))
    return np.concatenate(parts).astype(np.float32)


@pytest.mark.parametrize("shift", [0.0, 100.3])
def test_field_points_round_as_specified(shift):
    pts = _points(shift)
    f = _field(pts)
    idx, d2 = _same(f, 8)
    assert d2.dtype == torch.float32 and bool((d2[:, 0] == 0).all())
    picks = torch.tensor([[3, 150, 3], [399, 200, 250]])
    _same(f, 8, picks)
    _same(f, 3, _field(_points(shift, samples=1, n=50)))
    assert f._batch_group() is f._batch_group() and f._batch_indices() is f._batch_indices() == (0, 2)


def test_float64_and_integer_points_are_taken_to_float32():
    pts = _points()
    f = _field(pts.astype(np.float64) + 1e-9, torch.float64)
    assert f._points32().dtype == torch.float32
    _same(f, 5)
    g = _field(np.random.default_rng(1).integers(-9, 9, (60, 4)) * np.array([0, 1, 1, 1]), torch.int32)
    assert _same(g, 4)[1].dtype == torch.float32


def test_duplicated_points_come_in_row_order():
    pts = np.array([[0, 0.5, 0.5, 0.5], [0, 1.5, 0.5, 0.5], [0, 0.5, 0.5, 0.5], [0, 1.5, 0.5, 0.5], [0, 0.5, 0.5, 0.5]], np.float32)
    idx, d2 = _same(_field(pts), 4)
    assert idx[2].tolist() == [0, 2, 4, 1] and d2[2].tolist() == [0, 0, 0, 1]       # row 2 is not its own first neighbour


def test_the_cap():
    c = [[0, 0, 0, 0], [0, 1, 0, 0], [0, 5, 0, 0], [0, 5, 5, 0], [0, 2, 2, 0], [0, 0, 1, 0]]
    x = _sparse(c)
    idx, d2 = _same(x, 4, cap=8)                        # 8 occurs (row 0 to row 4): the boundary is included
    assert idx[0].tolist() == [0, 1, 5, 4] and d2[0].tolist() == [0, 1, 1, 8]
    idx, d2 = _same(x, 4, cap=7)
    assert idx[0].tolist() == [0, 1, 5, -1] and d2[0].tolist() == [0, 1, 1, -1]
    idx, d2 = _same(x, 3, cap=0)                        # only coincident rows: the row itself
    assert idx.tolist() == [[i, -1, -1] for i in range(6)]
    free = _same(x, 6)
    assert int(free[0].min()) >= 0 and int(free[1].min()) >= 0
    assert torch.equal(_same(x, 6, cap=2 ** 40)[0], free[0])
    pts = np.array([[0, 0.5, 0.5, 0.5], [0, 1.5, 0.5, 0.5], [0, 0.5, 0.5, 0.5], [0, 0.5, 0.5, 0.75]], np.float32)
    f = _field(pts)
    idx, d2 = _same(f, 3, cap=0.0625)                   # 0.25^2 occurs
    assert idx[0].tolist() == [0, 2, 3] and d2[0].tolist() == [0, 0, 0.0625]
    idx, d2 = _same(f, 3, cap=0.0)
    assert idx[0].tolist() == [0, 2, -1] and d2[0, 2].item() == float("inf") and idx[1].tolist() == [1, -1, -1]
    _same(f, 3, torch.tensor([[1, 3]]), cap=0.07)       # the cap is taken to float32


def test_refusals():
    x = _sparse(GAPS)
    for bad in (0, -1, 65, 2.5, True, None, torch.tensor(2)):
        with pytest.raises(ValueError, match="k must be a Python int with 1 <= k <= 64"):
            ME.knn_query(x, bad)
    with pytest.raises(ValueError, match=r"k = 7 is larger than sample 1, which has 6 rows"):
        ME.knn_query(x, 7)
    with pytest.raises(ValueError, match=r"k = 7 is larger than sample 1, which has 6 rows"):
        ME.knn_query(x, 7, max_squared_distance=3)                           # one rule, with a cap too
    with pytest.raises(TypeError, match="x must be a SparseTensor or a TensorField"):
        ME.knn_query(torch.zeros(4, 4), 2)
    f = _field(_points())
    with pytest.raises(TypeError, match="mixed kinds"):
        ME.knn_query(x, 2, f)
    with pytest.raises(TypeError, match="mixed kinds"):
        ME.knn_query(f, 2, x)
    for bad in (1.0, True, "1"):
        with pytest.raises(ValueError, match="max_squared_distance must be a Python int >= 0 for a SparseTensor"):
            ME.knn_query(x, 2, max_squared_distance=bad)
    for bad in (1, True, "1"):
        with pytest.raises(ValueError, match="max_squared_distance must be a Python float >= 0 for a TensorField"):
            ME.knn_query(f, 2, max_squared_distance=bad)
    with pytest.raises(ValueError, match="max_squared_distance must be >= 0"):
        ME.knn_query(x, 2, max_squared_distance=-1)
    for bad in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="max_squared_distance must be >= 0"):
            ME.knn_query(f, 2, max_squared_distance=bad)
    good = torch.tensor([[int(np.flatnonzero(GAPS[:, 0] == b)[0])] for b in (0, 2, 5)])
    assert tuple(ME.knn_query(x, 2, good)[0].shape) == (3, 1, 2)
    with pytest.raises(ValueError, match=r"queries must have shape \[B, M\] with B = 3"):
        ME.knn_query(x, 2, good[:2])                                         # another B
    with pytest.raises(ValueError, match=r"queries must have shape \[B, M\] with B = 3"):
        ME.knn_query(x, 2, good.view(3))
    with pytest.raises(ValueError, match="queries must be an int64 tensor"):
        ME.knn_query(x, 2, good.int())
    with pytest.raises(ValueError, match="queries must be None, an int64 tensor"):
        ME.knn_query(x, 2, good.tolist())
    swapped = good[[1, 0, 2]]
    with pytest.raises(ValueError, match=rf"queries\[0, 0\] = {int(swapped[0, 0])} is not a row of sample 0"):
        ME.knn_query(x, 2, swapped)
    for outside in (-1, GAPS.shape[0]):
        far = good.repeat(1, 2)
        far[2, 1] = outside
        with pytest.raises(ValueError, match=rf"queries\[2, 1\] = {outside} is not a row of sample 2"):
            ME.knn_query(x, 2, far)
    wide = np.array([[0, 0, 0, 0], [0, 16384, 0, 0]], np.int32)
    with pytest.raises(ValueError, match="packable range"):
        ME.knn_query(_sparse(wide), 1)
    with pytest.raises(ValueError, match="packable range"):
        ME.knn_query(_sparse(wide[:1]), 1, _sparse(wide))                    # both sets
    small = _field(np.array([[0, 0, 0, 0], [0, 1, 0, 0], [1, 2, 0, 0], [1, 3, 0, 0.]]))
    with pytest.raises(ValueError, match=r"k = 3 is larger than sample 0, which has 2 rows"):
        ME.knn_query(small, 3)


def test_more_samples_than_the_kernel_takes():
    n = 65536
    c = np.stack([np.arange(n), np.zeros(n), np.zeros(n), np.zeros(n)], 1).astype(np.int32)
    with pytest.raises(ValueError, match="B = 65536 is above the kernel's limit of 65535"):
        ME.knn_query(_sparse(c), 1)


def test_empty_inputs():
    x = ME.SparseTensor(torch.zeros(0, 3), coordinate_manager=ME.CoordinateManager(torch.zeros((0, 4), dtype=torch.int32)))
    for q in (None, x):
        idx, d2 = ME.knn_query(x, 7, q)
        assert idx.dtype == d2.dtype == torch.int64 and tuple(idx.shape) == tuple(d2.shape) == (0, 7)
    idx, d2 = ME.knn_query(x, 7, torch.zeros((0, 5), dtype=torch.int64))
    assert tuple(idx.shape) == tuple(d2.shape) == (0, 5, 7)
    full = _sparse(GAPS)
    idx, d2 = ME.knn_query(full, 2, torch.zeros((3, 0), dtype=torch.int64))
    assert idx.dtype == torch.int64 and tuple(idx.shape) == tuple(d2.shape) == (3, 0, 2)
    assert tuple(ME.knn_query(full, 2, x)[0].shape) == (0, 2)                 # no queries
    f = ME.TensorField(torch.zeros(0, 3), torch.zeros(0, 4))
    idx, d2 = ME.knn_query(f, 2)
    assert idx.dtype == torch.int64 and d2.dtype == torch.float32 and tuple(idx.shape) == tuple(d2.shape) == (0, 2)


def test_queries_go_in_bounded_chunks(monkeypatch):
    """the CPU path never holds a whole sample's [V_q, V_b] matrix: with the bound at 40 pairs a sample of 12 rows goes three
    queries at a time, one of 9 rows four at a time, and the result is the same"""
    from minsu3d_amd.MinkowskiEngine import tensor as T
    assert T._KNN_CHUNK == 2 ** 22
    x = _sparse(GAPS)
    want = ME.knn_query(x, 5)
    seen = []
    topk = torch.topk

    def spy(key, *a, **kw):
        seen.append(tuple(key.shape))
        return topk(key, *a, **kw)

    monkeypatch.setattr(T, "_KNN_CHUNK", 40)
    monkeypatch.setattr(torch, "topk", spy)
    got = ME.knn_query(x, 5)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert max(r * c for r, c in seen) <= 40 and (3, 12) in seen and (4, 9) in seen and (1, 9) in seen


def test_host_reads_are_made_once(monkeypatch):
    cm = ME.CoordinateManager(torch.from_numpy(GAPS))
    x = ME.SparseTensor(torch.randn(GAPS.shape[0], 3), coordinate_manager=cm)
    y = _sparse(random_voxels([7, 4], seed=9, side=6, batch_indices=[5, 0]))
    f = _field(_points())
    ME.knn_query(x, 2), ME.knn_query(x, 2, y), ME.knn_query(f, 2), ME.knn_query(f, 2, f)
    assert cm.batch_lengths(1) == (9, 6, 12) and cm.batch_lengths(1) is cm.batch_lengths(1)
    assert cm.batch_indices(1) == (0, 2, 5) and cm.batch_indices(1) is cm.batch_indices(1)
    reads = []
    tolist = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: reads.append(tuple(self.shape)) or tolist(self))
    ME.knn_query(x, 3), ME.knn_query(x, 3, y, 4), ME.knn_query(f, 3), ME.knn_query(f, 3, f, 0.5)
    assert reads == []                                  # lengths, batch indices and extent all come from the caches


def test_inverse_distance_unpooling_carries_gradients():
    fine = random_voxels([60, 45], seed=20, side=10, batch_indices=[1, 4])
    feats = torch.randn(fine.shape[0], 5)
    x = ME.SparseTensor(feats, coordinate_manager=ME.CoordinateManager(torch.from_numpy(fine)))
    picks = ME.farthest_point_sampling(x, 6)
    coarse_f = torch.randn(12, 5, requires_grad=True)
    coarse = ME.SparseTensor(coarse_f, coordinate_manager=ME.CoordinateManager(x.C[picks.reshape(-1)].contiguous()))
    idx, d2 = ME.knn_query(coarse, 3, x)
    assert tuple(idx.shape) == (105, 3) and not idx.requires_grad
    w = 1.0 / (d2.float() + 1e-8)
    w = w / w.sum(-1, keepdim=True)
    up = (coarse.F[idx] * w[..., None]).sum(-2)
    assert tuple(up.shape) == (105, 5) and bool(torch.isfinite(up).all())
    up.sum().backward()
    assert coarse_f.grad is not None and bool(torch.isfinite(coarse_f.grad).all()) and float(coarse_f.grad.abs().sum()) > 0
    at_pick = picks.reshape(-1)
    assert torch.allclose(up[at_pick], coarse_f.detach(), atol=1e-5)          # a pick gets its own features back


# ---- the host side of the library
def _library():
    from minsu3d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.ms3d_knn_ws_bytes.restype = ctypes.c_size_t
    return lib


def test_getters_and_sizes():
    from minsu3d_amd import _lib
    lib = _library()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert lib.ms3d_knn_max_k() == 64
    qpg, rpt = lib.ms3d_knn_queries_per_group(), lib.ms3d_knn_rows_per_tile()
    assert qpg >= 64 and qpg % 64 == 0 and rpt >= 64 and rpt % 64 == 0
    # a tile of 16-byte rows, a group's lists of 64 keys and its stashes stay below the 64 KiB a kernel gets without asking
    assert 16 * rpt + 8 * qpg * 64 < 64 * 1024
    assert _lib.lib().ms3d_knn_ws_bytes.restype is ctypes.c_size_t
    L = ctypes.c_long
    for v in (1, 2, 63, 64, 65, 1000, 400000, 2 ** 31 - 1):
        assert lib.ms3d_knn_ws_bytes(L(v)) == 16 * v                          # 16 B a row, no 32-bit wrap
    assert lib.ms3d_knn_ws_bytes(L(0)) == 0 and lib.ms3d_knn_ws_bytes(L(-3)) == 0


@pytest.mark.parametrize("entry", ["ms3d_knn_i32", "ms3d_knn_f32"])
def test_return_codes(entry):
    """every code is decided on the host before a launch, so HOST buffers stand in for the device's and nothing runs"""
    lib = _library()
    fn = getattr(lib, entry)
    V, B, NQ, K = 12, 2, 5, 3
    data = (ctypes.c_int * (4 * V))()
    order = (ctypes.c_longlong * V)(*range(V))
    seg = (ctypes.c_int * (B + 1))(0, 5, V)
    queries = (ctypes.c_int * (4 * NQ))()
    qstart = (ctypes.c_int * (B + 1))(0, 2, NQ)
    out = (ctypes.c_longlong * (NQ * K))()
    d2 = (ctypes.c_int * (NQ * K))()
    need = lib.ms3d_knn_ws_bytes(ctypes.c_long(V))
    raw = (ctypes.c_char * (need + 64))()
    ws = (ctypes.addressof(raw) + 15) & ~15                        # 16-byte aligned
    S = ctypes.c_size_t
    cap = ctypes.c_longlong(-1) if entry.endswith("i32") else ctypes.c_float(-1.0)

    def call(data=data, order=order, seg=seg, V=V, B=B, queries=queries, qstart=qstart, NQ=NQ, most=3, k=K, out=out, d2=d2,
             ws=ws, nbytes=need):
        return fn(data, order, seg, None, V, B, queries, qstart, NQ, most, k, cap, out, d2, ctypes.c_void_p(ws), S(nbytes), None)

    for bad in (dict(V=-1), dict(B=-1), dict(B=65536), dict(NQ=-1), dict(most=-1), dict(k=0), dict(k=-4), dict(k=65)):
        assert call(**bad) == E_UNSUPPORTED, bad
    assert call(V=0) == 0 and call(B=0) == 0 and call(NQ=0) == 0 and call(most=0) == 0
    assert call(NQ=0, data=None, order=None, seg=None, queries=None, qstart=None, out=None, d2=None, ws=None, nbytes=0) == 0
    assert call(V=0, k=0) == E_UNSUPPORTED                                          # the ranges come first
    for missing in ("data", "order", "seg", "queries", "qstart", "out", "d2", "ws"):
        assert call(**{missing: None}) == E_UNSUPPORTED, missing
    assert call(ws=ws + 4) == E_UNSUPPORTED                                         # not 16-byte aligned
    assert call(nbytes=need - 1) == E_WORKSPACE and call(nbytes=0) == E_WORKSPACE
