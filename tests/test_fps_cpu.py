"""Farthest point sampling (ME.farthest_point_sampling, csrc/fps.hip): what can be checked without a GPU -- the exports and the
documents, the CPU path (the rule as a torch expression) against the serial numpy reference of tests/fps_ref.py, every refusal,
the caches, and the host side of the library through ctypes on the cross-compiled library: the sizes and every return code,
which are all decided before a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import minsu3d_amd.MinkowskiEngine as ME
from fps_ref import fps_ref, lattice, random_voxels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ms3d_fps_resident_rows", "ms3d_fps_ws_bytes", "ms3d_fps_i32", "ms3d_fps_f32")
E_WORKSPACE, E_UNSUPPORTED = 10001, 10002          # MS3D_E_* of include/minsu3d_hip.h
# batch indices 0, 2 and 5 (gaps), the rows of the samples interleaved
GAPS = random_voxels([9, 6, 12], seed=3, side=6, batch_indices=[0, 2, 5])


def _sparse(coords, **kw):
    c = torch.as_tensor(np.asarray(coords), dtype=torch.int32)
    return ME.SparseTensor(torch.randn(c.size(0), 3), coordinate_manager=ME.CoordinateManager(c, **kw))


def _same(got, coords, M, start=None):
    want = fps_ref(coords, M, None if start is None else start.tolist())
    assert got.dtype == torch.int64 and tuple(got.shape) == want.shape
    assert torch.equal(got, torch.from_numpy(want))


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
    assert callable(ME.farthest_point_sampling)
    assert dropin.farthest_point_sampling is ME.farthest_point_sampling and "farthest_point_sampling" in dropin.__all__
    doc = ME.__doc__
    assert "farthest_point_sampling(x, num_samples, start=None)" in doc
    assert doc.index("MinkowskiVoxelAttention(embed_dim") < doc.index("farthest_point_sampling(x, num_samples") \
        < doc.index("Not supported (each raises")
    assert doc.count("Not supported") == 1                       # the section says "Out of scope"
    section = doc[doc.index("farthest_point_sampling(x, num_samples"):doc.index("Not supported (each raises")]
    for word in ("Out of scope", "lowest caller row", "3 221 028 867", "FMA", "fminf", "ms3d_fps_i32", "ms3d_fps_resident_rows",
                 "[0, M]", "start"):
        assert word in section, word
    own = ME.farthest_point_sampling.__doc__
    for word in ("lowest caller row", "3 221 028 867", "FMA", "fminf", "ValueError", "[0, M]", "not differentiable",
                 "Out of scope", "MinkowskiQueryAttention"):
        assert word in own, word
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "farthest_point_sampling" in design and "csrc/fps.hip" in design
    assert design.index("csrc/vattn.hip") < design.index("csrc/fps.hip")


def test_header_declares_the_symbols():
    text = open(os.path.join(ROOT, "include", "minsu3d_hip.h")).read()
    assert "csrc/fps.hip" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ms3d_[a-z0-9_]+)\s*\(", text))
    for s in SYMBOLS:
        assert s in declared, s


def test_hand_worked_example():
    """rows (0,0) (1,0) (5,0) (5,5) (2,2) in the plane z = 0, from row 0:
    squared distances to row 0: 0 1 25 50 8                      -> row 3
    nearest of {0, 3}:          0 min(1,41) min(25,25) 0 min(8,18) = 0 1 25 0 8  -> row 2
    nearest of {0, 3, 2}:       0 min(1,16) 0 0 min(8,13)          = 0 1 0 0 8   -> row 4
    nearest of {0, 3, 2, 4}:    0 min(1,5) 0 0 0                   = 0 1 0 0 0   -> row 1"""
    c = [[0, 0, 0, 0], [0, 1, 0, 0], [0, 5, 0, 0], [0, 5, 5, 0], [0, 2, 2, 0]]
    got = ME.farthest_point_sampling(_sparse(c), 5)
    assert got.tolist() == [[0, 3, 2, 4, 1]]
    assert fps_ref(np.array(c), 5).tolist() == [[0, 3, 2, 4, 1]]


def test_lattice_ties_on_both_manager_kinds():
    from minsu3d_amd import backend
    c = lattice(4, seed=5)
    plain = ME.farthest_point_sampling(_sparse(c, spatial_sort=False), 64)
    backend.set_backend(Shuffling())                 # (tests/conftest.py restores the backend)
    x = _sparse(c, spatial_sort=True)
    cm = x.coordinate_manager
    assert cm.perm is not None and cm.caller_rows(1) is not None and not torch.equal(cm.coords[1], x.C)
    assert torch.equal(x.C, torch.from_numpy(c))
    shuffled = ME.farthest_point_sampling(x, 64)
    assert torch.equal(plain, shuffled)
    _same(plain, c, 64)
    assert sorted(plain[0].tolist()) == list(range(64))


def test_gaps_and_interleaved_rows():
    x = _sparse(GAPS)
    for M in (1, 4, 6):
        got = ME.farthest_point_sampling(x, M)
        _same(got, GAPS, M)
        batch_of = torch.from_numpy(GAPS[:, 0]).long()[got]
        assert batch_of.tolist() == [[0] * M, [2] * M, [5] * M]


def test_one_pick_and_every_row_of_the_smallest_sample():
    x = _sparse(GAPS)
    first = ME.farthest_point_sampling(x, 1)
    assert first.tolist() == [[int(np.flatnonzero(GAPS[:, 0] == b)[0])] for b in (0, 2, 5)]     # the lowest caller row
    got = ME.farthest_point_sampling(x, 6)            # the sample of batch index 2 has exactly 6 rows
    assert sorted(got[1].tolist()) == np.flatnonzero(GAPS[:, 0] == 2).tolist()
    _same(got, GAPS, 6)


def test_stride_two_set():
    from minsu3d_amd import backend
    backend.set_backend(Shuffling())                 # (tests/conftest.py restores the backend)
    c = random_voxels([40, 25], seed=8, side=8)
    cm = ME.CoordinateManager(torch.from_numpy(c))
    cm.k2(1)
    coarse = cm.coords[2]
    assert 0 < coarse.size(0) < c.shape[0] and int((coarse[:, 1:] % 2).abs().sum()) == 0
    x = ME.SparseTensor(torch.randn(coarse.size(0), 3), coordinate_manager=cm, tensor_stride=2)
    M = int(torch.bincount(coarse[:, 0].long()).min())
    _same(ME.farthest_point_sampling(x, M), coarse.numpy(), M)
    rooted = ME.SparseTensor(torch.randn(coarse.size(0), 3), coordinate_manager=ME.CoordinateManager.rooted(coarse, 2),
                             tensor_stride=2)
    _same(ME.farthest_point_sampling(rooted, 3), coarse.numpy(), 3)


def test_start_given():
    x = _sparse(GAPS)
    rows = [np.flatnonzero(GAPS[:, 0] == b) for b in (0, 2, 5)]
    start = torch.tensor([rows[0][4], rows[1][-1], rows[2][0]])
    got = ME.farthest_point_sampling(x, 5, start=start)
    assert got[:, 0].tolist() == start.tolist()
    _same(got, GAPS, 5, start)
    assert not torch.equal(got, ME.farthest_point_sampling(x, 5))


def test_distances_above_two_to_the_31():
    """from row 0 the far corner is 3 * 32767^2 = 3 221 028 867 away, which as a signed 32-bit number is negative: signed
    arithmetic picks the origin (805 306 368 away) instead"""
    c = np.array([[0, -16384, -16384, -16384], [0, 0, 0, 0], [0, 16383, 16383, 16383]], np.int32)
    assert 3 * 32767 ** 2 == 3221028867 and 2 ** 31 < 3221028867 < 2 ** 32
    assert np.int32(np.uint32(3221028867)) < 3 * 16384 ** 2
    got = ME.farthest_point_sampling(_sparse(c), 3)
    assert got.tolist() == [[0, 2, 1]]
    _same(got, c, 3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int32])
def test_field_points(dtype):
    rng = np.random.default_rng(0)
    pts = rng.integers(0, 12, (300, 3)) * np.float32(0.1)
    b = rng.integers(0, 3, (300, 1)) * 2
    if dtype == torch.int32:
        pts = rng.integers(-9, 9, (300, 3))
    c = np.concatenate([b, pts], 1)
    f = ME.TensorField(torch.randn(300, 2), torch.as_tensor(c).to(dtype))
    as32 = f._points32().numpy()
    assert as32.dtype == np.float32
    M = 40
    got = ME.farthest_point_sampling(f, M)
    _same(got, as32, M)
    start = torch.from_numpy(np.array([np.flatnonzero(b[:, 0] == v)[3] for v in (0, 2, 4)]))
    _same(ME.farthest_point_sampling(f, M, start=start), as32, M, start)
    assert f._batch_group() is f._batch_group() and f._like(f.F * 2)._batch_group() is f._batch_group()


def test_duplicated_points_repeat_the_lowest_row():
    pts = np.array([[0, 0.5, 0.5, 0.5], [0, 1.5, 0.5, 0.5], [0, 0.5, 0.5, 0.5], [0, 1.5, 0.5, 0.5], [0, 0.5, 0.5, 0.5]], np.float32)
    f = ME.TensorField(torch.randn(5, 2), torch.from_numpy(pts))
    got = ME.farthest_point_sampling(f, 5)
    assert got.tolist() == [[0, 1, 0, 0, 0]]          # two distinct positions; then every distance is 0
    _same(got, pts, 5)


def test_refusals():
    x = _sparse(GAPS)
    for bad in (0, -1, 2.5, True, None, torch.tensor(2)):
        with pytest.raises(ValueError, match="num_samples must be a Python int >= 1"):
            ME.farthest_point_sampling(x, bad)
    with pytest.raises(ValueError, match=r"num_samples = 7 is larger than sample 1, which has 6 rows"):
        ME.farthest_point_sampling(x, 7)
    with pytest.raises(TypeError, match="SparseTensor or a TensorField"):
        ME.farthest_point_sampling(torch.zeros(4, 4), 2)
    good = torch.tensor([int(np.flatnonzero(GAPS[:, 0] == b)[0]) for b in (0, 2, 5)])
    assert ME.farthest_point_sampling(x, 2, start=good)[:, 0].tolist() == good.tolist()
    with pytest.raises(ValueError, match=r"start must have shape \[B\] = \[3\]"):
        ME.farthest_point_sampling(x, 2, start=good[:2])                      # another B
    with pytest.raises(ValueError, match=r"start must have shape \[B\] = \[3\]"):
        ME.farthest_point_sampling(x, 2, start=good.view(3, 1))
    with pytest.raises(ValueError, match="start must be an int64 tensor"):
        ME.farthest_point_sampling(x, 2, start=good.int())
    with pytest.raises(ValueError, match="start must be an int64 tensor"):
        ME.farthest_point_sampling(x, 2, start=good.tolist())
    swapped = good[[1, 0, 2]]
    with pytest.raises(ValueError, match=rf"start\[0\] = {int(swapped[0])} is not a row of sample 0"):
        ME.farthest_point_sampling(x, 2, start=swapped)
    for outside in (-1, GAPS.shape[0]):
        far = good.clone()
        far[2] = outside
        with pytest.raises(ValueError, match=rf"start\[2\] = {outside} is not a row of sample 2"):
            ME.farthest_point_sampling(x, 2, start=far)
    wide = np.array([[0, 0, 0, 0], [0, 16384, 0, 0]], np.int32)
    with pytest.raises(ValueError, match="packable range"):
        ME.farthest_point_sampling(_sparse(wide), 1)
    f = ME.TensorField(torch.randn(4, 2), torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0], [1, 2, 0, 0], [1, 3, 0, 0.]]))
    with pytest.raises(ValueError, match=r"num_samples = 3 is larger than sample 0, which has 2 rows"):
        ME.farthest_point_sampling(f, 3)
    with pytest.raises(ValueError, match=r"start\[1\] = 1 is not a row of sample 1"):
        ME.farthest_point_sampling(f, 2, start=torch.tensor([0, 1]))


def test_empty_input():
    x = ME.SparseTensor(torch.zeros(0, 3), coordinate_manager=ME.CoordinateManager(torch.zeros((0, 4), dtype=torch.int32)))
    got = ME.farthest_point_sampling(x, 7)
    assert got.dtype == torch.int64 and tuple(got.shape) == (0, 7)
    f = ME.TensorField(torch.zeros(0, 3), torch.zeros(0, 4))
    got = ME.farthest_point_sampling(f, 2, start=torch.zeros(0, dtype=torch.int64))
    assert got.dtype == torch.int64 and tuple(got.shape) == (0, 2)


def test_segment_lengths_are_read_once():
    cm = ME.CoordinateManager(torch.from_numpy(GAPS))
    assert cm.batch_lengths(1) == (9, 6, 12) and cm.batch_lengths(1) is cm.batch_lengths(1)


def test_result_carries_no_gradient_but_the_gather_does():
    c = torch.from_numpy(GAPS)
    feats = torch.randn(c.size(0), 4, requires_grad=True)
    x = ME.SparseTensor(feats, coordinate_manager=ME.CoordinateManager(c))
    idx = ME.farthest_point_sampling(x, 3)
    assert not idx.requires_grad
    q = x.F[idx]
    assert tuple(q.shape) == (3, 3, 4)
    q.sum().backward()
    want = torch.zeros(c.size(0))
    want[idx.reshape(-1)] = 1
    assert torch.equal(feats.grad, want[:, None].expand(-1, 4))


# ---- the host side of the library
def _library():
    from minsu3d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.ms3d_fps_ws_bytes.restype = ctypes.c_size_t
    return lib


def test_sizes():
    from minsu3d_amd import _lib
    lib = _library()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert lib.ms3d_fps_resident_rows() >= 1024
    assert _lib.lib().ms3d_fps_ws_bytes.restype is ctypes.c_size_t
    L = ctypes.c_long
    sizes = [lib.ms3d_fps_ws_bytes(L(v), 4) for v in (1, 2, 63, 64, 65, 1000, 8192, 8193, 100000, 400000, 2 ** 31 - 1)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    assert sizes[-1] >= 20 * (2 ** 31 - 1) > 2 ** 32              # 20 B a row in the float body, no 32-bit wrap
    assert lib.ms3d_fps_ws_bytes(L(1000), 1) <= lib.ms3d_fps_ws_bytes(L(1000), 2) <= lib.ms3d_fps_ws_bytes(L(1000), 65535)
    assert lib.ms3d_fps_ws_bytes(L(0), 4) == 0 and lib.ms3d_fps_ws_bytes(L(10), 0) == 0 and lib.ms3d_fps_ws_bytes(L(-3), 4) == 0


@pytest.mark.parametrize("entry", ["ms3d_fps_i32", "ms3d_fps_f32"])
def test_return_codes(entry):
    """every code is decided on the host before the launch, so HOST buffers stand in for the device's and nothing runs"""
    lib = _library()
    fn = getattr(lib, entry)
    V, B, M = 12, 2, 3
    data = (ctypes.c_int * (4 * V))()
    order = (ctypes.c_longlong * V)(*range(V))
    seg = (ctypes.c_int * (B + 1))(0, 5, V)
    out = (ctypes.c_longlong * (B * M))()
    need = lib.ms3d_fps_ws_bytes(ctypes.c_long(V), B)
    raw = (ctypes.c_char * (need + 64))()
    ws = (ctypes.addressof(raw) + 15) & ~15                        # 16-byte aligned
    S = ctypes.c_size_t

    def call(data=data, order=order, seg=seg, V=V, B=B, M=M, out=out, ws=ws, nbytes=need):
        return fn(data, order, seg, None, None, V, B, M, out, ctypes.c_void_p(ws), S(nbytes), None)

    assert call(V=-1) == E_UNSUPPORTED and call(B=-1) == E_UNSUPPORTED and call(B=65536) == E_UNSUPPORTED
    assert call(M=0) == E_UNSUPPORTED and call(M=-4) == E_UNSUPPORTED
    assert call(V=0) == 0 and call(B=0) == 0
    assert call(V=0, data=None, order=None, seg=None, out=None, ws=None, nbytes=0) == 0      # no pointer is looked at
    assert call(V=0, M=0) == E_UNSUPPORTED                                          # the ranges come first
    for missing in ("data", "order", "seg", "out", "ws"):
        assert call(**{missing: None}) == E_UNSUPPORTED, missing
    assert call(ws=ws + 4) == E_UNSUPPORTED                                         # not 16-byte aligned
    assert call(nbytes=need - 1) == E_WORKSPACE and call(nbytes=0) == E_WORKSPACE
