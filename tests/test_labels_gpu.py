"""GPU: ms3d_quantize_labels (csrc/labels.hip) through backend.quantize_labels and through ME.utils.sparse_quantize(labels=).

Yardstick: tests/labels_ref.py, the serial loop of the sequential rule; the kernel is handed the maps of that loop, so the
hash-based quantiser is not part of the kernel cases.  Shapes: the smallest at which the two launches can go wrong -- no row,
one row, a grid of several blocks with a ragged tail, a voxel of more rows than a wavefront whose one dissenter is the last
row or the first-occurrence row, no repeated voxel, one voxel only.  Every comparison is an exact integer comparison."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from labels_ref import quantize_labels_ref

pytestmark = pytest.mark.gpu
IGNORE = -100
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def be():
    from minsu3d_amd.backend import HipBackend
    return HipBackend()


def dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()


@functools.lru_cache(maxsize=None)
def kernel_case(name):
    """(labels [n], first-occurrence rows [m], voxel of every row [n], expected voxel labels [m]) from the serial loop.
    Shared, read only."""
    rng = np.random.default_rng(11)
    if name == "empty":
        coords, labels = np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
    elif name == "one_row":
        coords, labels = np.array([[3, 1, 2]]), np.array([6])
    elif name == "ragged_grid":                    # 256 * 3 + 1 rows (four blocks, the last holds one row) into <= 40 voxels
        n = 256 * 3 + 1
        vox = rng.integers(0, 40, n)
        coords = np.stack([vox % 4, (vox // 4) % 5, vox // 20], 1)
        labels = np.where(rng.random(n) < 0.02, rng.integers(0, 5, n), vox % 5)    # 2 % of the rows dissent
    elif name in ("crowd_last_dissents", "crowd_first_dissents", "crowd_agrees"):
        # one voxel of 200 rows (more than a wavefront) among 30 rows of other voxels
        coords = np.concatenate([np.tile([[7, 7, 7]], (200, 1)), rng.integers(0, 3, (30, 3))])
        labels = np.concatenate([np.full(200, 4), rng.integers(0, 2, 30)])
        if name == "crowd_last_dissents":
            order = np.concatenate([rng.permutation(229) + 1, [0]])               # a crowd row goes last ...
            coords, labels = coords[order], labels[order]
            labels[-1] = 9                                                          # ... and is the only one to differ
        elif name == "crowd_first_dissents":
            labels[0] = 9                                                           # the first-occurrence row is the odd one
    elif name == "all_single":                     # m == n
        coords = np.stack([np.arange(300), np.zeros(300, np.int64), np.zeros(300, np.int64)], 1)
        labels = rng.integers(0, 5, 300)
    elif name == "one_voxel_agrees":
        coords, labels = np.zeros((300, 3), np.int64), np.full(300, 3)
    elif name == "one_voxel_disagrees":
        coords, labels = np.zeros((300, 3), np.int64), np.full(300, 3)
        labels[157] = 2
    else:
        raise KeyError(name)
    _, want, first, inverse = quantize_labels_ref(coords, labels, IGNORE)
    return labels, first, inverse, want


KERNEL_CASES = ("empty", "one_row", "ragged_grid", "crowd_last_dissents", "crowd_first_dissents", "crowd_agrees", "all_single",
                "one_voxel_agrees", "one_voxel_disagrees")


def test_cases_are_what_they_claim():
    """the inputs, checked once on the CPU: the property each case is named for holds"""
    labels, first, inverse, want = kernel_case("ragged_grid")
    assert len(labels) == 769 and 30 <= len(first) <= 40 and (want == IGNORE).any() and (want != IGNORE).any()
    for name, odd_row in (("crowd_last_dissents", 229), ("crowd_first_dissents", None)):
        labels, first, inverse, want = kernel_case(name)
        crowd = inverse[odd_row] if odd_row is not None else 0
        rows = np.flatnonzero(inverse == crowd)
        assert len(rows) == 200 and want[crowd] == IGNORE
        odd = rows[labels[rows] != 4]
        assert odd.tolist() == [odd_row if odd_row is not None else first[crowd]]
    labels, first, inverse, want = kernel_case("crowd_agrees")
    assert want[0] == 4 and (inverse == 0).sum() == 200
    labels, first, inverse, want = kernel_case("all_single")
    assert len(first) == len(labels) == 300 and np.array_equal(want, labels)
    assert kernel_case("one_voxel_agrees")[3].tolist() == [3] and kernel_case("one_voxel_disagrees")[3].tolist() == [IGNORE]


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_kernel_matches_the_serial_rule(be, name):
    labels, first, inverse, want = kernel_case(name)
    out = be.quantize_labels(dev(labels), dev(first), dev(inverse), IGNORE)
    assert out.dtype == torch.int32 and out.is_cuda and tuple(out.shape) == (len(first),)
    assert np.array_equal(out.cpu().numpy(), want)
    again = be.quantize_labels(dev(labels), dev(first), dev(inverse), IGNORE)
    assert torch.equal(out, again)


@pytest.mark.parametrize("name", ("one_row", "ragged_grid", "crowd_last_dissents", "all_single"))
def test_guard_band(be, name):
    """`out` is the front of a larger allocation: 64 int32 of a sentinel behind its m entries stay untouched"""
    from minsu3d_amd import _lib
    labels, first, inverse, want = kernel_case(name)
    n, m = len(labels), len(first)
    l, u, i = dev(labels), dev(first), dev(inverse)
    buf = torch.full((m + 64,), SENTINEL, dtype=torch.int32, device="cuda")
    _lib.check(be.lib.ms3d_quantize_labels(_lib.ptr(l), _lib.ptr(u), _lib.ptr(i), n, m, IGNORE, _lib.ptr(buf),
                                           _lib.stream_handle()), "ms3d_quantize_labels")
    host = buf.cpu().numpy()
    assert np.array_equal(host[:m], want) and (host[m:] == SENTINEL).all()


def test_boundary_codes(be):
    """decided on the host before anything is launched"""
    from minsu3d_amd import _lib
    labels, first, inverse, want = kernel_case("ragged_grid")
    n, m = len(labels), len(first)
    l, u, i = dev(labels), dev(first), dev(inverse)
    buf = torch.full((m,), SENTINEL, dtype=torch.int32, device="cuda")
    call = lambda n_, m_: be.lib.ms3d_quantize_labels(_lib.ptr(l), _lib.ptr(u), _lib.ptr(i), n_, m_, IGNORE, _lib.ptr(buf),
                                                      _lib.stream_handle())
    assert call(0, 0) == 0 and call(n, 0) == 0 and call(0, m) == 0
    assert call(-1, m) == _lib.E_UNSUPPORTED and call(n, -1) == _lib.E_UNSUPPORTED and call(m - 1, m) == _lib.E_UNSUPPORTED
    null = ctypes.c_void_p(0)
    assert be.lib.ms3d_quantize_labels(null, _lib.ptr(u), _lib.ptr(i), n, m, IGNORE, _lib.ptr(buf),
                                       _lib.stream_handle()) == _lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == SENTINEL).all()                                     # none of them wrote


# ------------------------------------------------------------------------------------------------- the public call
@functools.lru_cache(maxsize=None)
def batch_case():
    """2 samples x 2000 points in an 8^3 grid of cells (4-column input), 5 classes that follow x with 10 % noise ->
    (points f32 [4000, 4], labels i64 [4000]).  Shared, read only."""
    rng = np.random.default_rng(21)
    n = 4000
    pts = np.empty((n, 4), np.float32)
    pts[:, 0] = np.repeat([0, 1], n // 2)
    pts[:, 1:] = rng.uniform(-4, 4, (n, 3))
    labels = np.clip(np.floor((pts[:, 1] + 4) / 8 * 5), 0, 4).astype(np.int64)
    noisy = rng.random(n) < 0.1
    labels[noisy] = rng.integers(0, 5, int(noisy.sum()))
    return pts, labels


def test_sparse_quantize_labels_gpu_equals_cpu_path():
    import minsu3d_amd.MinkowskiEngine as ME
    from minsu3d_amd import backend
    from oracle.oracle_backend import OracleBackend
    pts, labels = batch_case()
    cells = np.floor(pts).astype(np.int64)
    want_c, want_l, want_idx, want_inv = quantize_labels_ref(cells, labels, IGNORE)
    assert (want_l == IGNORE).any() and (want_l != IGNORE).any()                     # agreeing and disagreeing voxels occur
    assert (np.bincount(want_inv)[want_l != IGNORE] > 1).any()                       # some voxel of several points agrees
    assert len(np.unique(want_c[:, 0])) == 2

    hip = backend.HipBackend()
    prev = backend.set_backend(hip)
    try:
        gpu = ME.utils.sparse_quantize(torch.from_numpy(pts).cuda(), labels=torch.from_numpy(labels).cuda(), return_index=True,
                                       return_inverse=True, quantization_size=1, device="cuda")
        again = ME.utils.sparse_quantize(torch.from_numpy(pts).cuda(), labels=torch.from_numpy(labels).cuda(), return_index=True,
                                         return_inverse=True, quantization_size=1, device="cuda")
        backend.set_backend(OracleBackend())
        cpu = ME.utils.sparse_quantize(torch.from_numpy(pts), labels=torch.from_numpy(labels), return_index=True,
                                       return_inverse=True, quantization_size=1)
    finally:
        backend.set_backend(prev)
    assert len(gpu) == len(cpu) == 4
    for g, a, c, want in zip(gpu, again, cpu, (want_c, want_l, want_idx, want_inv)):
        assert g.is_cuda and not c.is_cuda and g.dtype == c.dtype
        assert torch.equal(g, a)                                                     # the same call twice: the same bytes
        assert torch.equal(g.cpu(), c) and np.array_equal(c.numpy(), want)
    assert gpu[1].dtype == torch.int64


def test_sparse_quantize_labels_gpu_dtypes_and_numpy_labels():
    """uint8 labels and an ndarray of labels beside device coordinates: tensors on the coordinates' device, own dtype"""
    import minsu3d_amd.MinkowskiEngine as ME
    from minsu3d_amd import backend
    pts, labels = batch_case()
    want_l = quantize_labels_ref(np.floor(pts).astype(np.int64), labels, 255)[1]
    prev = backend.set_backend(backend.HipBackend())
    try:
        for given in (torch.from_numpy(labels).to(torch.uint8).cuda(), labels.astype(np.uint8)):
            c, l = ME.utils.sparse_quantize(torch.from_numpy(pts).cuda(), labels=given, ignore_label=255, quantization_size=1)
            assert l.is_cuda and l.dtype == torch.uint8 and np.array_equal(l.cpu().numpy().astype(np.int64), want_l)
    finally:
        backend.set_backend(prev)
