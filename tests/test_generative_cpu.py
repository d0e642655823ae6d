"""Generative transposed convolution and pruning: what can be checked without a GPU -- the exported names, the header, the
refusals, and the expectation itself: the numpy restatement of the generated coordinate set (tests/generative_ref.py, which
the GPU tests compare the engine against) is checked here against dense torch, float64, for every geometry they use."""
import os
import re

import numpy as np
import pytest
import torch

import minsu3d_amd.MinkowskiEngine as ME
from generative_ref import GEOMS, dense_support, downsample_np, expand_np, strides_for, _key
from sparse_ref import random_sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("MinkowskiGenerativeConvolutionTranspose", "MinkowskiPruning")


def test_new_names_exported():
    for name in NEW:
        assert isinstance(getattr(ME, name), type), name
    assert callable(ME.SparseTensor.coordinate_rows) and callable(ME.SparseTensor.features_at_coordinates)
    assert callable(ME.CoordinateManager.rooted)
    import minsu3d_amd.dropin.MinkowskiEngine as dropin
    for name in NEW:
        assert getattr(dropin, name) is getattr(ME, name) and name in dropin.__all__, name
    for word in NEW + ("features_at_coordinates",):
        assert word in ME.__doc__, word


def test_header_declares_new_symbols():
    """(tests/test_abi_cpu.py then proves that the cross-compiled library exports them)"""
    text = open(os.path.join(ROOT, "include", "minsu3d_hip.h")).read()
    for sym in ("ms3d_coords_expand_workspace_bytes", "ms3d_coords_expand", "ms3d_coords_prune", "ms3d_scatter_rows"):
        assert re.search(r"\b" + sym + r"\s*\(", text), sym


@pytest.mark.parametrize("kw,K", [(dict(kernel_size=2, stride=2), 8), (dict(kernel_size=3, stride=2, bias=True), 27),
                                  (dict(kernel_size=3), 27), (dict(kernel_size=5, dilation=2), 125)])
def test_constructor(kw, K):
    m = ME.MinkowskiGenerativeConvolutionTranspose(4, 8, dimension=3, **kw)
    assert tuple(m.kernel.shape) == (K, 4, 8)
    assert list(m.state_dict().keys()) == (["kernel", "bias"] if kw.get("bias") else ["kernel"])
    assert float(m.kernel.detach().abs().max()) <= 1.0 / np.sqrt(4 * K)


def test_refusals():
    gen = ME.MinkowskiGenerativeConvolutionTranspose
    with pytest.raises(NotImplementedError, match="kernel_size=3, stride=3"):
        gen(4, 8, kernel_size=3, stride=3, dimension=3)
    with pytest.raises(NotImplementedError, match="kernel_size=2, stride=1"):
        gen(4, 8, kernel_size=2, stride=1, dimension=3)
    with pytest.raises(NotImplementedError, match="dimension=2"):
        gen(4, 8, kernel_size=3, stride=2, dimension=2)
    with pytest.raises(NotImplementedError, match="no per-axis tuples"):
        gen(4, 8, kernel_size=(3, 3, 3), stride=2, dimension=3)
    # stride 2 from an odd tensor stride: refused before any backend is touched
    coords = torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 2]], dtype=torch.int32)
    for cm, ts in ((ME.CoordinateManager(coords), 1), (ME.CoordinateManager.rooted(coords * 3, 3), 3)):
        x = ME.SparseTensor(torch.randn(3, 4), coordinate_manager=cm, tensor_stride=ts)
        with pytest.raises(NotImplementedError, match=f"kernel_size=3, stride=2, dilation=1 on tensor stride {ts}"):
            gen(4, 8, kernel_size=3, stride=2, dimension=3)(x)


def test_rooted_manager_on_cpu_rows():
    coords = torch.tensor([[0, 0, 0, 0], [0, 4, 0, 0], [1, 0, 0, 8]], dtype=torch.int32)
    cm = ME.CoordinateManager.rooted(coords, 4)
    assert cm.perm is None and cm.inv is None and list(cm.coords) == [4] and cm.size(4) == 3
    assert cm.identity(4).tolist() == [[0, 1, 2]]
    order, inv, offsets, counts = cm.batch_rows(4)
    assert offsets.tolist() == [0, 2, 3] and counts.view(-1).tolist() == [2.0, 1.0]
    x = ME.SparseTensor(torch.randn(3, 4), coordinate_manager=cm, tensor_stride=4)
    assert torch.equal(x.C, coords) and x.F.shape == (3, 4)
    lin = ME.MinkowskiLinear(4, 5)
    assert torch.allclose(lin(x).F, lin.linear(x.F))
    # the existing constructor is what it was
    old = ME.CoordinateManager(coords)
    assert list(old.coords) == [1] and not hasattr(old, "root")


def test_layers_name_the_hip_backend_when_it_lacks_them():
    from minsu3d_amd import backend

    class Bare:
        pass
    coords = torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0]], dtype=torch.int32)
    x = ME.SparseTensor(torch.randn(2, 4), coordinate_manager=ME.CoordinateManager(coords))
    backend.set_backend(Bare())           # (tests/conftest.py restores the backend)
    with pytest.raises(NotImplementedError, match="HIP backend"):
        ME.MinkowskiPruning()(x, torch.tensor([True, False]))
    with pytest.raises(NotImplementedError, match="HIP backend"):
        x.coordinate_rows(coords)
    with pytest.raises(NotImplementedError, match="HIP backend"):
        ME.MinkowskiGenerativeConvolutionTranspose(4, 8, kernel_size=3, dimension=3)(x)


def test_pruning_checks_its_mask():
    from minsu3d_amd import backend

    class Stub:
        def coords_prune(self, coords, keep):
            raise AssertionError("a refused mask must not reach the backend")
    coords = torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0]], dtype=torch.int32)
    x = ME.SparseTensor(torch.randn(2, 4), coordinate_manager=ME.CoordinateManager(coords))
    backend.set_backend(Stub())
    for bad in (torch.tensor([1, 0]), torch.tensor([1.0, 0.0]), torch.tensor([True]), torch.tensor([True, False, True]),
                torch.tensor([[True, False]])):
        with pytest.raises(ValueError, match=r"bool \[2\]"):
            ME.MinkowskiPruning()(x, bad)


def test_entry_point_refuses_what_it_cannot_index():
    """host-side contract of ms3d_coords_expand, decided before anything is launched (so it runs without a GPU): more than
    2^31 - 1 candidates and K < 1 are MS3D_E_UNSUPPORTED with a workspace size of 0; no input rows is an empty set"""
    import ctypes as C
    from minsu3d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    lib.ms3d_coords_expand_workspace_bytes.restype = C.c_size_t
    assert _lib.E_UNSUPPORTED == 10002
    assert lib.ms3d_coords_expand_workspace_bytes(1 << 20, 2048) == 0            # 2^31 candidates
    assert lib.ms3d_coords_expand_workspace_bytes((1 << 20) - 1, 2048) >= 12 * 2 * ((1 << 31) - 2048)
    small = lib.ms3d_coords_expand_workspace_bytes(1000, 27)
    assert 27000 * (24 + 8) <= small <= 27000 * (48 + 8) + 8192                  # what the header states per candidate
    n = C.c_int(-1)
    null = C.c_void_p(0)
    call = lambda vin, k: lib.ms3d_coords_expand(null, vin, null, k, null, C.byref(n), null, C.c_size_t(0), null)
    assert call(1 << 20, 2048) == _lib.E_UNSUPPORTED and n.value == 0
    assert call(5, 0) == _lib.E_UNSUPPORTED
    n.value = -1
    assert call(0, 27) == 0 and n.value == 0
    keep = lib.ms3d_coords_prune(null, 0, null, null, null, null, C.byref(n), null, C.c_size_t(0), null)
    assert keep == 0 and n.value == 0


@pytest.mark.parametrize("shift", [0, -9])
@pytest.mark.parametrize("ks,stride,dil", GEOMS)
def test_expected_set_is_the_support_of_the_dense_operator(ks, stride, dil, shift):
    """pins the GPU tests' expectation: expand_np gives exactly the voxels a dense transposed convolution of the occupancy
    grid with an all-ones kernel reaches (float64, CPU), for every geometry and input tensor stride used there; the shifted
    cloud (negative coordinates) is compared after shifting the dense result by the same amount"""
    B, G = 2, 12
    rng = np.random.default_rng(7)
    fine, _ = random_sparse(rng, B=B, grid=G, n=400, C=1)
    for ts in strides_for(stride):
        coords = fine
        t = 1
        while t < ts:
            t *= 2
            coords = downsample_np(coords, t)
        want = dense_support(coords, ks, stride, dil, ts, B, G)
        moved = coords.copy()
        moved[:, 1:] += shift * ts                       # stays on the lattice of the tensor stride
        got = expand_np(moved, ks, stride, dil, ts)
        assert got.dtype == np.int32 and len(np.unique(_key(got))) == len(got)          # distinct rows
        back = got.astype(np.int64)
        back[:, 1:] -= shift * ts
        assert np.array_equal(np.sort(_key(back)), want), (ks, stride, dil, ts)
        # order: first occurrence in input-row-major, offset-minor candidate order; for one input row that is offset order
        one = expand_np(moved[:1], ks, stride, dil, ts)
        assert len(one) == ks ** 3 and tuple(one[0, 1:] - moved[0, 1:]) == ((0, 0, 0) if ks % 2 == 0 else
                                                                          (-(ks // 2) * dil * (ts // stride),) * 3)
