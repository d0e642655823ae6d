"""GPU: farthest point sampling per sample (ME.farthest_point_sampling; csrc/fps.hip).

The rule has one answer, so every comparison is torch.equal: against tests/fps_ref.py (serial numpy over the caller-order
coordinates: int64 arithmetic for voxels, float32 operation by operation for points) and against the package's own CPU path on
the same input.  Segment lengths sit at the edges of a wave, of the workgroup and of the two bodies (ms3d_fps_resident_rows());
the float cases are ones in which a fused multiply-add or float64 arithmetic changes a pick well inside the steps they take."""
import numpy as np
import pytest
import torch

from fps_ref import fps_ref, lattice, random_voxels

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ME():
    import minsu3d_amd.MinkowskiEngine as me
    return me


@pytest.fixture(scope="module")
def R():
    from minsu3d_amd.backend import get_backend
    rows = get_backend().fps_resident_rows()
    assert rows >= 1024
    return rows


def _check(ME, x, M, start=None):
    """x on the device: the kernel against the serial reference and against the CPU path over the caller's coordinates"""
    got = ME.farthest_point_sampling(x, M, start=start)
    assert got.is_cuda and got.dtype == torch.int64
    c = x.C.cpu()
    if isinstance(x, ME.TensorField):
        c = x._points32().cpu()
        on_cpu = ME.TensorField(torch.zeros(c.size(0), 1), c)
    else:
        on_cpu = ME.SparseTensor(torch.zeros(c.size(0), 1), coordinate_manager=ME.CoordinateManager.rooted(c, x.tensor_stride),
                                 tensor_stride=x.tensor_stride)
    start_cpu = None if start is None else start.cpu()
    want = torch.from_numpy(fps_ref(c.numpy(), M, None if start is None else start_cpu.tolist()))
    assert tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got.cpu(), ME.farthest_point_sampling(on_cpu, M, start=start_cpu))
    return got


def _sparse(ME, coords, spatial_sort=False, channels=4):
    c = torch.as_tensor(np.asarray(coords), dtype=torch.int32).to(DEV)
    cm = ME.CoordinateManager(c, spatial_sort=spatial_sort)
    return ME.SparseTensor(torch.randn(c.size(0), channels, device=DEV), coordinate_manager=cm)


def test_segment_length_edges(ME):
    lengths = [1, 2, 63, 64, 65, 1023, 1024, 1025]
    got = _check(ME, _sparse(ME, random_voxels(lengths, seed=1)), 1)
    assert tuple(got.shape) == (8, 1)
    _check(ME, _sparse(ME, random_voxels(lengths[1:], seed=2)), 2)


def test_both_bodies_in_one_launch(ME, R):
    c = random_voxels([R - 1, R, R + 1, 3], seed=3, side=64)
    got = _check(ME, _sparse(ME, c), 3)
    assert tuple(got.shape) == (4, 3)


def test_streaming_body_many_picks(ME, R):
    """several sweep steps a thread (more than four rows a thread), a length that is no multiple of four, and enough picks for
    the minima to be rewritten many times"""
    _check(ME, _sparse(ME, random_voxels([4 * R + 1027, R + 2], seed=4, side=64)), 24)


@pytest.mark.parametrize("spatial_sort", [False, True])
def test_lattice_ties_and_caller_numbering(ME, spatial_sort):
    c = lattice(4, seed=5)
    got = _check(ME, _sparse(ME, c, spatial_sort=spatial_sort), 64)
    assert sorted(got[0].tolist()) == list(range(64))


@pytest.mark.parametrize("M,with_start", [(40, False), (7, True)])
def test_morton_sorted_manager(ME, R, M, with_start):
    """enough rows for the manager to hold them in Morton order: the rows are read through batch_rows where they are held and
    named through caller_rows; one sample in each body, full of ties"""
    big, small = lattice(22, seed=6, batch=3), lattice(9, seed=7, batch=1)
    assert big.shape[0] > R >= small.shape[0]
    c = np.concatenate([big, small])[np.random.default_rng(8).permutation(big.shape[0] + small.shape[0])]
    x = _sparse(ME, c, spatial_sort=True)
    cm = x.coordinate_manager
    assert cm.perm is not None and cm.caller_rows(1) is not None
    start = None
    if with_start:
        start = torch.tensor([np.flatnonzero(c[:, 0] == 1)[100], np.flatnonzero(c[:, 0] == 3)[5000]], device=DEV)
    got = _check(ME, x, M, start)
    assert torch.equal(got, ME.farthest_point_sampling(_sparse(ME, c, spatial_sort=False), M, start=start))


def test_gaps_and_interleaved_rows(ME):
    c = random_voxels([70, 9, 300], seed=9, side=12, batch_indices=[0, 2, 5])
    got = _check(ME, _sparse(ME, c), 9)
    assert torch.from_numpy(c[:, 0]).long()[got.cpu()].tolist() == [[0] * 9, [2] * 9, [5] * 9]
    assert sorted(got[1].tolist()) == np.flatnonzero(c[:, 0] == 2).tolist()          # M = V_b: every row once


def test_stride_two_set_and_rooted_manager(ME):
    x = _sparse(ME, random_voxels([900, 500], seed=10, side=24))
    cm = x.coordinate_manager
    cm.k2(1)
    coarse = cm.coords[2]
    assert 0 < coarse.size(0) < 1400
    _check(ME, ME.SparseTensor(torch.randn(coarse.size(0), 4, device=DEV), coordinate_manager=cm, tensor_stride=2), 30)
    rooted = ME.CoordinateManager.rooted(coarse.clone(), 2)
    _check(ME, ME.SparseTensor(torch.randn(coarse.size(0), 4, device=DEV), coordinate_manager=rooted, tensor_stride=2), 30)


def test_distances_above_two_to_the_31(ME):
    c = np.array([[0, -16384, -16384, -16384], [0, 0, 0, 0], [0, 16383, 16383, 16383]], np.int32)
    got = _check(ME, _sparse(ME, c), 3)
    assert got.tolist() == [[0, 2, 1]]                # signed 32-bit arithmetic gives [0, 1, 2]


def test_distances_above_two_to_the_31_streaming_body(ME, R):
    """the same corners inside a sample that takes the streaming body, whose coordinates are packed to 16 bits"""
    c = random_voxels([R + 9], seed=12, side=64)
    c[0, 1:], c[1, 1:], c[2, 1:] = -16384, 16383, (16383, -16384, 0)
    got = _check(ME, _sparse(ME, c), 4)
    assert got[0, :2].tolist() == [0, 1]


def test_start_given(ME, R):
    c = random_voxels([100, R + 50, 17], seed=13, side=64)
    start = torch.tensor([np.flatnonzero(c[:, 0] == b)[k] for b, k in ((0, 99), (1, R + 49), (2, 0))], device=DEV)
    got = _check(ME, _sparse(ME, c), 12, start)
    assert got[:, 0].tolist() == start.tolist()


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
    """a 12^3 lattice of step float32(0.1), 600 points a sample (many duplicates, many ties): a contracted distance changes a
    pick between step 21 and 27 for each of the four seeds (between 34 and 47 with the shift), float64 arithmetic by step 14"""
    pts = _points(shift)
    assert pts.dtype == np.float32
    got = _check(ME, _field(ME, pts), 64)
    assert tuple(got.shape) == (4, 64)


def test_float64_points_are_taken_to_float32(ME):
    pts = _points()
    f = _field(ME, pts.astype(np.float64) + 1e-9, torch.float64)
    _check(ME, f, 30)


def test_duplicated_points_repeat_the_lowest_row(ME):
    base = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 2.5, 0.5]], np.float32)
    pts = np.concatenate([np.zeros((30, 1), np.float32), np.tile(base, (10, 1))], 1)
    got = _check(ME, _field(ME, pts), 8)              # three distinct positions, eight picks
    assert got[0, 3:].tolist() == [0] * 5


def test_float_points_streaming_body(ME, R):
    rng = np.random.default_rng(20)
    n = [2 * R + 3, 50]
    pts = np.concatenate([np.concatenate([np.full((k, 1), b, np.float32),
                                          (rng.integers(0, 40, (k, 3)) * np.float32(0.1)).astype(np.float32)], 1)
                          for b, k in enumerate(n)])
    pts = pts[rng.permutation(pts.shape[0])]
    _check(ME, _field(ME, pts), 40)


def test_dirty_workspace_and_same_bytes(ME, R):
    big = _sparse(ME, random_voxels([3 * R, 2 * R + 1], seed=30, side=64))
    first = _check(ME, big, 6)
    small = _sparse(ME, random_voxels([R + 1, 40], seed=31, side=64))       # the workspace holds the large call's words
    a = _check(ME, small, 10)
    b = ME.farthest_point_sampling(small, 10)
    assert torch.equal(a, b)
    assert torch.equal(first, ME.farthest_point_sampling(big, 6))
    f = _field(ME, _points())
    assert torch.equal(ME.farthest_point_sampling(f, 20), ME.farthest_point_sampling(f, 20))


def test_refusals_on_the_device(ME):
    from minsu3d_amd import backend
    x = _sparse(ME, random_voxels([30, 12], seed=40))
    with pytest.raises(ValueError, match=r"num_samples = 13 is larger than sample 1, which has 12 rows"):
        ME.farthest_point_sampling(x, 13)
    bad = torch.tensor([int(np.flatnonzero(x.C[:, 0].cpu().numpy() == b)[0]) for b in (1, 0)], device=DEV)
    with pytest.raises(ValueError, match="is not a row of sample 0"):
        ME.farthest_point_sampling(x, 2, start=bad)

    class Bare:
        pass

    backend.set_backend(Bare())                        # (tests/conftest.py restores the backend)
    with pytest.raises(NotImplementedError, match="ms3d_fps_i32"):
        ME.farthest_point_sampling(x, 2)


def test_queries_for_query_attention(ME):
    torch.manual_seed(0)
    E, H, M = 16, 4, 10
    x = _sparse(ME, random_voxels([200, 90], seed=50, side=12, batch_indices=[1, 4]), channels=E)
    idx = ME.farthest_point_sampling(x, M)
    queries = x.F[idx]
    assert tuple(queries.shape) == (2, M, E)
    positions = x.C[idx][..., 1:]
    assert tuple(positions.shape) == (2, M, 3) and x.C[idx][..., 0].tolist() == [[1] * M, [4] * M]
    out = ME.MinkowskiQueryAttention(E, H).to(DEV)(queries, x)
    assert tuple(out.shape) == (2, M, E) and bool(torch.isfinite(out).all())
