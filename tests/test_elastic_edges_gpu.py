"""GPU parity of the elastic distortion (csrc/augment.hip) with the host restatement minsu3d_amd.util.transform
(blur_noise + trilinear) where random points never go: on the grid nodes (t integral, f = 0), on the inclusive upper
boundary t == n - 1 (the cell index is clamped to n - 2 and f == 1), on axes with the minimum of two nodes, a hair
outside the grid, and at point counts around the 256-thread block.  Points are float64; the bound is the 1e-9 voxels of
tests/test_dataset_gpu.py.  What is crafted is checked on the CPU first: trilinear() of a grid of ones is non-zero inside
and exactly 0 outside, so it tells how the host restatement itself classifies a point.

A hair outside.  One float64 below the lower boundary is outside.  One float64 above the upper boundary is NOT: x - lo is
twice the boundary coordinate, has twice its ulp, and the sum rounds (to even) back onto t == n - 1, so the restatement
and the kernel both sample it as the boundary node.  The first float the restatement calls outside is searched for on the
CPU (it is the second one above); the one in between is compared like every inside point."""
import numpy as np
import pytest
import torch

from minsu3d_amd.util import transform as T

gpu = pytest.mark.gpu
GRAN, MAG, TOL = 6.0, 40.0, 1e-9
SHAPES = [(2, 2, 2), (2, 5, 3), (7, 2, 4)]


@pytest.fixture(scope="module")
def be():
    from minsu3d_amd import backend as B
    return B.get_backend()


def noise_for(shape):
    return np.random.default_rng(sum(s * 10 ** i for i, s in enumerate(shape))).standard_normal((3,) + shape).astype(np.float32)


def host_inside(shape, pts):
    return T.trilinear(np.ones(shape, np.float32), GRAN, pts) != 0.0


def host(noise, pts, mag=MAG):
    return pts + np.hstack([T.trilinear(T.blur_noise(n), GRAN, pts)[:, None] for n in noise]) * mag


def hi_of(shape):
    return (np.array(shape, np.float64) - 1) * GRAN               # nodes: linspace(-hi, hi, n), spacing 2 * gran


def node_points(shape, boundary_only=False):
    idx = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3)
    if boundary_only:
        idx = idx[np.any((idx == 0) | (idx == np.array(shape) - 1), axis=1)]
    pts = -hi_of(shape) + idx * (2 * GRAN)
    t = (pts + hi_of(shape)) / (2 * GRAN)
    assert np.array_equal(t, idx) and host_inside(shape, pts).all()           # integral on all three axes, 0 and n - 1 included
    return idx, pts


def mid_cell(shape, m, rng):
    """m points strictly inside the grid, away from the nodes"""
    cell = np.stack([rng.integers(0, s - 1, m) for s in shape], 1)
    return -hi_of(shape) + (cell + rng.uniform(0.2, 0.8, (m, 3))) * (2 * GRAN)


def upper_face_points(shape, rng):
    """for each axis: t == n - 1 on it, mid-cell on the other two"""
    out = []
    for a in range(3):
        p = mid_cell(shape, 9, rng)
        p[:, a] = hi_of(shape)[a]
        out.append(p)
    pts = np.concatenate(out)
    assert host_inside(shape, pts).all()
    return pts


def first_outside_above(shape, a, others):
    x = hi_of(shape)[a]
    for steps in range(1, 4):
        x = np.nextafter(x, np.inf)
        p = others.copy()
        p[a] = x
        if not host_inside(shape, p[None])[0]:
            return x, steps
    raise AssertionError("no float within 3 of the boundary is outside")


def hair_points(shape, rng):
    """-> (outside points, the points one float above the upper boundary, which the restatement samples as t == n - 1)"""
    outside, on_edge = [], []
    for a in range(3):
        base = mid_cell(shape, 1, rng)[0]
        below = base.copy()
        below[a] = np.nextafter(-hi_of(shape)[a], -np.inf)
        above = base.copy()
        above[a], steps = first_outside_above(shape, a, base)
        assert steps == 2 and above[a] > hi_of(shape)[a]
        edge = base.copy()
        edge[a] = np.nextafter(hi_of(shape)[a], np.inf)
        outside += [below, above]
        on_edge.append(edge)
    outside, on_edge = np.array(outside), np.array(on_edge)
    assert not host_inside(shape, outside).any() and host_inside(shape, on_edge).all()
    return outside, on_edge


def run(be, noise, pts, mag=MAG):
    got = be.elastic(torch.from_numpy(pts).cuda(), torch.from_numpy(noise).cuda(), GRAN, mag)
    assert got.dtype == torch.float64 and tuple(got.shape) == pts.shape
    return got.cpu().numpy()


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_every_grid_node(be, shape):
    noise = noise_for(shape)
    idx, pts = node_points(shape)
    want = host(noise, pts)
    assert np.abs(want - pts).max() > 1e-3                     # the nodes do move: an all-zero sample would show
    assert np.abs(run(be, noise, pts) - want).max() < TOL


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_upper_boundary_is_inside(be, shape):
    noise = noise_for(shape)
    pts = upper_face_points(shape, np.random.default_rng(1))
    want = host(noise, pts)
    assert np.abs(want - pts).max(1).min() > 0.0               # inclusive: every one of them is displaced
    assert np.abs(run(be, noise, pts) - want).max() < TOL


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_a_hair_outside(be, shape):
    noise = noise_for(shape)
    outside, on_edge = hair_points(shape, np.random.default_rng(2))
    got = run(be, noise, outside)
    assert np.array_equal(got.view(np.int64), outside.view(np.int64))         # left where they are, bit for bit
    want = host(noise, on_edge)
    assert np.abs(want - on_edge).max(1).min() > 0.0
    assert np.abs(run(be, noise, on_edge) - want).max() < TOL


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_blurred_boundary_cells(be, shape):
    """at a node the trilinear weights are 0 and 1, so with mag = 1 the displacement IS the blurred grid's value there:
    the zero-padded taps of the six blur passes at the faces, edges and corners, read without the interpolation"""
    noise = noise_for(shape)
    idx, pts = node_points(shape, boundary_only=True)
    blurred = np.stack([T.blur_noise(n) for n in noise])                       # [3, bx, by, bz] float32
    want = pts + blurred[:, idx[:, 0], idx[:, 1], idx[:, 2]].T.astype(np.float64)
    assert np.abs(host(noise, pts, 1.0) - want).max() < TOL
    assert np.abs(run(be, noise, pts, 1.0) - want).max() < TOL


@gpu
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_point_counts_at_the_block_edge(be, n):
    shape = (2, 5, 3)
    noise = noise_for(shape)
    rng = np.random.default_rng(n)
    pts = rng.uniform(-1.1, 1.1, (n, 3)) * hi_of(shape)                       # some of them outside
    pts[-1:] = hi_of(shape)                                                   # the last thread: the far corner node
    got = run(be, noise, pts)
    if n:
        assert np.abs(got - host(noise, pts)).max() < TOL
    if n >= 255:
        inside = host_inside(shape, pts)
        assert inside.any() and not inside.all()
        assert np.array_equal(got[~inside], pts[~inside])


def test_crafted_points_are_what_they_claim():
    """the assertions inside the builders, on the CPU"""
    for shape in SHAPES:
        idx, pts = node_points(shape)
        assert pts.shape[0] == int(np.prod(shape)) and (idx == 0).any() and (idx == np.array(shape) - 1).any()
        node_points(shape, boundary_only=True)
        upper_face_points(shape, np.random.default_rng(1))
        outside, on_edge = hair_points(shape, np.random.default_rng(2))
        # what "inside" means for the one-float-above point: t is exactly n - 1
        t = (on_edge + hi_of(shape)) / (2 * GRAN)
        assert all(t[a, a] == shape[a] - 1 for a in range(3))
        assert np.array_equal(host(noise_for(shape), outside), outside)
