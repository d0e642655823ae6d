"""GPU: k nearest neighbours per sample (ME.knn_query; csrc/knn.hip).

The rule has one answer, so every comparison is torch.equal, on the rows AND on the distances: against tests/knn_ref.py (serial
numpy over the caller-order coordinates: int64 arithmetic for voxels, float32 operation by operation for points) and against the
package's own CPU path on the same input.  Support lengths sit at the edges of a wave and of the LDS tile
(ms3d_knn_rows_per_tile()), query counts at the edges of a group (ms3d_knn_queries_per_group()); the float cases are ones in
which a fused multiply-add changes the bits of 12 to 17 % of the distances."""
import numpy as np
import pytest
import torch

from fps_ref import lattice, random_voxels
from knn_ref import knn_forms

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ME():
    import minsu3d_amd.MinkowskiEngine as me
    return me


@pytest.fixture(scope="module")
def G():
    """(queries a group takes, rows of a tile)"""
    from minsu3d_amd.backend import get_backend
    be = get_backend()
    assert be.knn_max_k() == 64
    q, t = be.knn_geometry()
    assert q >= 64 and t >= 64
    return q, t


def _on_cpu(ME, t):
    if isinstance(t, ME.TensorField):
        return ME.TensorField(torch.zeros(t.C.size(0), 1), t._points32().cpu())
    c = t.C.cpu()
    return ME.SparseTensor(torch.zeros(c.size(0), 1), coordinate_manager=ME.CoordinateManager.rooted(c, t.tensor_stride),
                           tensor_stride=t.tensor_stride)


def _coords(ME, t):
    return (t._points32() if isinstance(t, ME.TensorField) else t.C).cpu().numpy()


def _check(ME, x, k, queries=None, cap=None, cpu_path=True):
    """x on the device: the kernel against the serial reference and against the CPU path over the caller's coordinates"""
    got_i, got_d = ME.knn_query(x, k, queries, cap)
    assert got_i.is_cuda and got_d.is_cuda and got_i.dtype == torch.int64
    assert got_d.dtype == (torch.float32 if isinstance(x, ME.TensorField) else torch.int64)
    kw, q_cpu = {}, None
    if torch.is_tensor(queries):
        kw["rows"], q_cpu = queries.cpu().numpy(), queries.cpu()
    elif queries is not None:
        kw["other"], q_cpu = _coords(ME, queries), _on_cpu(ME, queries)
    want_i, want_d = knn_forms(_coords(ME, x), k, cap=cap, **kw)
    assert tuple(got_i.shape) == want_i.shape and tuple(got_d.shape) == want_d.shape
    assert torch.equal(got_i.cpu(), torch.from_numpy(want_i))
    assert torch.equal(got_d.cpu(), torch.from_numpy(want_d))
    if cpu_path:
        cpu_i, cpu_d = ME.knn_query(_on_cpu(ME, x), k, q_cpu, cap)
        assert torch.equal(got_i.cpu(), cpu_i) and torch.equal(got_d.cpu(), cpu_d)
    return got_i, got_d


def _sparse(ME, coords, spatial_sort=False, channels=4):
    c = torch.as_tensor(np.asarray(coords), dtype=torch.int32).to(DEV)
    cm = ME.CoordinateManager(c, spatial_sort=spatial_sort)
    return ME.SparseTensor(torch.randn(c.size(0), channels, device=DEV), coordinate_manager=cm)


def _rows_of(coords, picks):
    """int64 [B, len(picks)]: for every sample (ascending batch index) its picks[j]-th row (modulo its length)"""
    b = np.asarray(coords)[:, 0]
    rows = [np.flatnonzero(b == v) for v in np.unique(b)]
    return torch.from_numpy(np.stack([r[np.asarray(picks) % r.size] for r in rows])).to(DEV)


def test_support_length_edges_in_one_launch(ME, G):
    T = G[1]
    lengths = [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3]
    c = random_voxels(lengths, seed=1)
    idx, d2 = _check(ME, _sparse(ME, c), 1)
    assert idx[:, 0].tolist() == list(range(c.shape[0])) and int(d2.max()) == 0          # every row finds itself
    _check(ME, _sparse(ME, random_voxels(lengths[1:], seed=2)), 2)


@pytest.mark.parametrize("k", [3, 16, 64])
def test_k_across_the_tile_edges(ME, G, k):
    T = G[1]
    _check(ME, _sparse(ME, random_voxels([64, 65, T - 1, T, T + 1, 2 * T + 3], seed=3 + k)), k)


def test_k_equal_to_the_length_returns_the_sample_sorted(ME):
    c = random_voxels([16, 40], seed=4, side=6)
    x = _sparse(ME, c)
    idx, d2 = _check(ME, x, 16)
    first = torch.from_numpy(np.flatnonzero(c[:, 0] == 0))
    assert torch.equal(idx.cpu()[first].sort(1).values, first[None, :].expand(16, -1))
    assert bool((d2[:, 1:] >= d2[:, :-1]).all())
    whole = _sparse(ME, random_voxels([64], seed=5, side=5))
    idx, _ = _check(ME, whole, 64)
    assert torch.equal(idx.sort(1).values.cpu(), torch.arange(64)[None, :].expand(64, -1))


def test_query_counts_at_the_group_edges(ME, G):
    Q = G[0]
    c = random_voxels([Q + 30, 2 * Q + 5, Q + 1], seed=6)
    x = _sparse(ME, c)
    every = ME.knn_query(x, 5)
    for M in (Q - 1, Q, Q + 1):
        picks = _rows_of(c, np.arange(M) * 7)               # duplicates inside a row where a sample is short
        idx, d2 = _check(ME, x, 5, picks)
        assert tuple(idx.shape) == (3, M, 5)
        assert torch.equal(idx, every[0][picks]) and torch.equal(d2, every[1][picks])
    y = _sparse(ME, random_voxels([Q - 1, Q, Q + 1], seed=7))
    assert tuple(_check(ME, x, 4, y)[0].shape) == (3 * Q, 4)


@pytest.mark.parametrize("spatial_sort", [False, True])
@pytest.mark.parametrize("n,k", [(4, 64), (9, 16)])
def test_lattice_ties_and_caller_numbering(ME, n, k, spatial_sort):
    c = lattice(n, seed=5)
    idx, d2 = _check(ME, _sparse(ME, c, spatial_sort=spatial_sort), k)
    assert idx[:, 0].tolist() == list(range(n ** 3))
    other = ME.knn_query(_sparse(ME, c, spatial_sort=not spatial_sort), k)
    assert torch.equal(idx, other[0]) and torch.equal(d2, other[1])


def test_morton_sorted_manager(ME, G):
    """enough rows for the manager to hold them in Morton order: the rows are read through batch_rows where they are held and
    named through caller_rows; two samples full of ties, the larger of many tiles"""
    big, small = lattice(22, seed=6, batch=3), lattice(9, seed=7, batch=1)
    assert big.shape[0] > 8 * G[1]
    c = np.concatenate([big, small])[np.random.default_rng(8).permutation(big.shape[0] + small.shape[0])]
    x = _sparse(ME, c, spatial_sort=True)
    cm = x.coordinate_manager
    assert cm.perm is not None and cm.caller_rows(1) is not None
    picks = ME.farthest_point_sampling(x, 40)
    idx, d2 = _check(ME, x, 32, picks)
    plain = _sparse(ME, c, spatial_sort=False)
    assert plain.coordinate_manager.perm is None
    every, every_plain = ME.knn_query(x, 32), ME.knn_query(plain, 32)
    assert torch.equal(every[0], every_plain[0]) and torch.equal(every[1], every_plain[1])
    assert torch.equal(idx, every[0][picks]) and torch.equal(d2, every[1][picks])            # form 2 = rows of form 1
    y = _sparse(ME, random_voxels([50, 70], seed=9, side=24, batch_indices=[3, 1]), spatial_sort=True)
    _check(ME, x, 7, y)


def test_gaps_and_interleaved_rows(ME):
    c = random_voxels([70, 9, 300], seed=9, side=12, batch_indices=[0, 2, 5])
    x = _sparse(ME, c)
    idx, _ = _check(ME, x, 9)
    batch = torch.from_numpy(c[:, 0]).long()
    assert torch.equal(batch[idx.cpu()], batch[:, None].expand(-1, 9))
    _check(ME, x, 9, _rows_of(c, [0, 8, 3, 8]))


def test_another_set_with_a_subset_of_the_batch_indices(ME):
    c = random_voxels([70, 9, 300], seed=9, side=12, batch_indices=[0, 2, 5])
    y = random_voxels([130, 20], seed=10, side=12, batch_indices=[5, 0])
    x = _sparse(ME, c)
    idx, _ = _check(ME, x, 12, _sparse(ME, y))                 # sample 1 of x (9 rows) has no queries
    assert torch.equal(torch.from_numpy(c[:, 0]).long()[idx.cpu()], torch.from_numpy(y[:, 0]).long()[:, None].expand(-1, 12))
    with pytest.raises(ValueError, match="batch index 3 is present in queries and absent from x"):
        ME.knn_query(x, 1, _sparse(ME, random_voxels([3, 2], seed=9, side=6, batch_indices=[5, 3])))


def test_stride_two_set_and_rooted_manager(ME):
    x = _sparse(ME, random_voxels([900, 500], seed=10, side=24))
    cm = x.coordinate_manager
    cm.k2(1)
    coarse = cm.coords[2]
    assert 0 < coarse.size(0) < 1400
    down = ME.SparseTensor(torch.randn(coarse.size(0), 4, device=DEV), coordinate_manager=cm, tensor_stride=2)
    _check(ME, down, 6)
    a = _check(ME, down, 3, x)                                 # every fine row finds its three nearest coarse rows
    _check(ME, x, 5, down)
    rooted = ME.SparseTensor(torch.randn(coarse.size(0), 4, device=DEV),
                             coordinate_manager=ME.CoordinateManager.rooted(coarse.clone(), 2), tensor_stride=2)
    b = _check(ME, rooted, 3, x)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_distances_above_two_to_the_31(ME):
    c = np.array([[0, -16384, -16384, -16384], [0, 0, 0, 0], [0, 16383, 16383, 16383]], np.int32)
    idx, d2 = _check(ME, _sparse(ME, c), 3)
    assert idx[0].tolist() == [0, 1, 2]                 # as a signed 32-bit number 3 221 028 867 is negative: row 2 before row 1
    assert d2.dtype == torch.int64 and d2[0].tolist() == [0, 805306368, 3221028867] and d2[2].tolist() == [0, 805208067, 3221028867]
    assert np.int32(np.uint32(3221028867)) < 0


def _points(shift=0.0):
    parts = []
    for seed in range(4):
        p = np.random.default_rng(seed).integers(0, 12, (600, 3)) * np.float32(0.1)
        parts.append(np.concatenate([np.full((600, 1), seed, np.float32), (p + np.float32(shift)).astype(np.float32)], 1))
    return np.concatenate(parts).astype(np.float32)


def _field(ME, pts, dtype=torch.float32):
    c = torch.from_numpy(pts).to(dtype).to(DEV)
    return ME.TensorField(torch.randn(c.size(0), 4, device=DEV), c)


@pytest.mark.parametrize("shift", [0.0, 100.3])
def test_float_points_round_as_specified(ME, shift):
    """a 12^3 lattice of step float32(0.1), 600 points a sample (many duplicates, many ties): a contracted distance differs in
    its bits for 17 % of the pairs (12 % with the shift) and changes the rows of 5 % of the queries (14 %)"""
    pts = _points(shift)
    assert pts.dtype == np.float32
    f = _field(ME, pts)
    idx, d2 = _check(ME, f, 8)
    assert tuple(idx.shape) == (2400, 8) and d2.dtype == torch.float32
    picks = _rows_of(pts, [5, 17, 5, 599])
    _check(ME, f, 8, picks)
    _check(ME, f, 3, _field(ME, _points(shift)[600:1500]))


def test_float64_points_are_taken_to_float32(ME):
    pts = _points()[:1200]
    f = _field(ME, pts.astype(np.float64) + 1e-9, torch.float64)
    _check(ME, f, 8)


def test_duplicated_points_come_in_row_order(ME):
    base = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 2.5, 0.5]], np.float32)
    pts = np.concatenate([np.zeros((30, 1), np.float32), np.tile(base, (10, 1))], 1)
    idx, d2 = _check(ME, _field(ME, pts), 12)
    assert idx[4].tolist()[:10] == list(range(1, 30, 3)) and d2[4].tolist()[:10] == [0.0] * 10       # ten copies, lowest row first


def test_the_cap(ME):
    c = random_voxels([200, 90], seed=11, side=8)
    x = _sparse(ME, c)
    free_i, free_d = _check(ME, x, 16)
    assert int(free_i.min()) >= 0 and int(free_d.min()) >= 0               # no cap: no -1
    cap = int(free_d[0, 9])                                                # a distance that occurs: the boundary is included
    idx, d2 = _check(ME, x, 16, cap=cap)
    assert int(idx[0, 9]) >= 0 and int(d2[0, 9]) == cap
    keep = free_d <= cap
    assert torch.equal(idx, torch.where(keep, free_i, -1)) and torch.equal(d2, torch.where(keep, free_d, -1))
    assert bool(((idx[:, 1:] < 0) | (idx[:, :-1] >= 0)).all())             # the -1 slots come last
    idx, d2 = _check(ME, x, 4, cap=0)                                      # only coincident rows: the row itself
    assert idx[:, 0].tolist() == list(range(290)) and int(idx[:, 1:].max()) == -1 and int(d2[:, 1:].max()) == -1
    _check(ME, x, 4, _rows_of(c, [1, 2, 3]), cap=3)
    f = _field(ME, _points()[:1200])
    free = _check(ME, f, 8)
    cap = float(free[1][3, 7])
    idx, d2 = _check(ME, f, 8, cap=cap)
    assert int(idx[3, 7]) >= 0 and bool(torch.isinf(d2[idx < 0]).all()) and bool((d2[idx >= 0] <= cap).all())
    idx, d2 = _check(ME, f, 8, cap=0.0)
    assert bool((d2[idx >= 0] == 0).all()) and bool((idx[:, 0] >= 0).all())


def test_dirty_workspace_and_same_bytes(ME, G):
    T = G[1]
    big = _sparse(ME, random_voxels([6 * T, 4 * T + 1], seed=30, side=64))
    picks = _rows_of(big.C.cpu().numpy(), np.arange(10) * 97)
    first = _check(ME, big, 20, picks)
    small = _sparse(ME, random_voxels([T + 1, 40], seed=31, side=64))       # the workspace holds the large call's words
    a = _check(ME, small, 10)
    b = ME.knn_query(small, 10)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    again = ME.knn_query(big, 20, picks)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    f = _field(ME, _points())
    a, b = ME.knn_query(f, 20), ME.knn_query(f, 20)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_refusals_on_the_device(ME):
    from minsu3d_amd import backend
    x = _sparse(ME, random_voxels([30, 12], seed=40))
    with pytest.raises(ValueError, match=r"k = 13 is larger than sample 1, which has 12 rows"):
        ME.knn_query(x, 13)
    with pytest.raises(ValueError, match="k must be a Python int with 1 <= k <= 64"):
        ME.knn_query(x, 65)
    rows = [int(np.flatnonzero(x.C[:, 0].cpu().numpy() == b)[0]) for b in (1, 0)]
    with pytest.raises(ValueError, match=r"queries\[0, 0\] = \d+ is not a row of sample 0"):
        ME.knn_query(x, 2, torch.tensor(rows, device=DEV).view(2, 1))
    with pytest.raises(ValueError, match="max_squared_distance must be a Python int"):
        ME.knn_query(x, 2, max_squared_distance=1.5)
    with pytest.raises(TypeError, match="mixed kinds"):
        ME.knn_query(x, 2, _field(ME, _points()[:100]))
    empty = ME.knn_query(x, 2, torch.zeros((2, 0), dtype=torch.int64, device=DEV))
    assert tuple(empty[0].shape) == (2, 0, 2) and empty[0].is_cuda

    class Bare:
        pass

    backend.set_backend(Bare())                        # (tests/conftest.py restores the backend)
    with pytest.raises(NotImplementedError, match="ms3d_knn_i32"):
        ME.knn_query(x, 2)


def test_inverse_distance_unpooling(ME):
    """carry the features of M picks back to all V rows: the three nearest picks of every row, weighted by 1 / d2"""
    torch.manual_seed(0)
    C, M = 8, 12
    x = _sparse(ME, random_voxels([200, 90], seed=50, side=12, batch_indices=[1, 4]), channels=C)
    picks = ME.farthest_point_sampling(x, M)
    feats = torch.randn(2 * M, C, device=DEV, requires_grad=True)
    coarse = ME.SparseTensor(feats, coordinate_manager=ME.CoordinateManager(x.C[picks.reshape(-1)].contiguous()))
    idx, d2 = _check(ME, coarse, 3, x)
    assert tuple(idx.shape) == (290, 3)
    w = 1.0 / (d2.float() + 1e-8)
    w = w / w.sum(-1, keepdim=True)
    up = (coarse.F[idx] * w[..., None]).sum(-2)
    assert tuple(up.shape) == (290, C) and bool(torch.isfinite(up).all())
    up.square().sum().backward()
    assert feats.grad is not None and bool(torch.isfinite(feats.grad).all()) and float(feats.grad.abs().sum()) > 0
    assert torch.allclose(up[picks.reshape(-1)], feats.detach(), atol=1e-5)                 # a pick gets its own features back
