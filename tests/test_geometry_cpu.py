"""General sparse geometries (any kernel size / dilation, stride 1 or 2, bias, pooling): what can be checked without a GPU
-- the offset rule, the constructors and the header."""
import os
import re

import numpy as np
import pytest
import torch

import minsu3d_amd.MinkowskiEngine as ME

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _offsets_restated(ks, dilation, ts):
    i = np.arange(ks) - ((ks - 1) // 2 if ks % 2 else 0)
    return np.array([(x, y, z) for z in i for y in i for x in i], np.int32) * dilation * ts


@pytest.mark.parametrize("ks", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("dilation", [1, 2, 3])
@pytest.mark.parametrize("ts", [1, 2, 4])
def test_offset_rule(ks, dilation, ts):
    off = ME.kernel_offsets(ks, dilation, ts)
    assert off.dtype == np.int32 and off.shape == (ks ** 3, 3)
    assert np.array_equal(off, _offsets_restated(ks, dilation, ts))
    if ks % 2:
        assert np.array_equal(off[::-1], -off)          # the mirror rule a submanifold map's backward-data pass relies on


@pytest.mark.parametrize("ts", [1, 2, 4])
def test_offsets_k3_order(ts):
    """(3, 1, 1) is the order ms3d_kmap_k3 documents: k = ix + 3 iy + 9 iz <-> (ix - 1, iy - 1, iz - 1) * ts"""
    off = ME.kernel_offsets(3, 1, ts)
    for k in range(27):
        assert tuple(off[k]) == ((k % 3 - 1) * ts, ((k // 3) % 3 - 1) * ts, (k // 9 - 1) * ts)


def test_offsets_k2_order():
    """(2, 2, 1): the in-cell offsets of the k2 table, koff = dx + 2 dy + 4 dz"""
    off = ME.kernel_offsets(2, 1, 2)
    for k in range(8):
        assert tuple(off[k]) == ((k & 1) * 2, ((k >> 1) & 1) * 2, ((k >> 2) & 1) * 2)


@pytest.mark.parametrize("kw,K", [(dict(kernel_size=5), 125), (dict(kernel_size=3, stride=2), 27),
                                  (dict(kernel_size=3, dilation=2), 27), (dict(kernel_size=3, bias=True), 27),
                                  (dict(kernel_size=4, stride=2), 64)])
@pytest.mark.parametrize("cls", [ME.MinkowskiConvolution, ME.MinkowskiConvolutionTranspose])
def test_constructors(cls, kw, K):
    if cls is ME.MinkowskiConvolutionTranspose and kw.get("stride", 1) != 2:
        kw = dict(kw, stride=2)
    m = cls(4, 8, dimension=3, **kw)
    assert tuple(m.kernel.shape) == (K, 4, 8)
    bound = 1.0 / np.sqrt(4 * K)
    assert float(m.kernel.detach().abs().max()) <= bound
    if kw.get("bias"):
        assert tuple(m.bias.shape) == (1, 8) and isinstance(m.bias, torch.nn.Parameter)
        assert float(m.bias.detach().abs().max()) <= bound
        assert list(m.state_dict().keys()) == ["kernel", "bias"]
    else:
        assert m.bias is None and list(m.state_dict().keys()) == ["kernel"]


def test_bias_state_dict_round_trip():
    a = ME.MinkowskiConvolution(4, 8, kernel_size=3, bias=True, dimension=3)
    b = ME.MinkowskiConvolution(4, 8, kernel_size=3, bias=True, dimension=3)
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.bias, b.bias) and torch.equal(a.kernel, b.kernel)


@pytest.mark.parametrize("kw,word", [(dict(kernel_size=2, stride=1), "kernel_size=2, stride=1"),
                                     (dict(kernel_size=3, stride=3), "kernel_size=3, stride=3"),
                                     (dict(kernel_size=3, stride=4), "stride=4")])
def test_refused_geometries(kw, word):
    for make in (lambda: ME.MinkowskiConvolution(4, 8, dimension=3, **kw), lambda: ME.MinkowskiMaxPooling(**kw)):
        with pytest.raises(NotImplementedError) as e:
            make()
        assert word in str(e.value)


def test_refused_dimension():
    with pytest.raises(NotImplementedError, match="dimension=2"):
        ME.MinkowskiConvolution(4, 8, kernel_size=3, dimension=2)
    with pytest.raises(NotImplementedError, match="dimension=4"):
        ME.MinkowskiAvgPooling(kernel_size=2, stride=2, dimension=4)


def test_new_names_exported():
    for name in ("MinkowskiMaxPooling", "MinkowskiAvgPooling", "MinkowskiSumPooling", "MinkowskiGlobalMaxPooling",
                 "MinkowskiGlobalAvgPooling", "MinkowskiGlobalSumPooling", "MinkowskiLinear", "MinkowskiDropout"):
        assert isinstance(getattr(ME, name), type), name
    lin = ME.MinkowskiLinear(4, 3)
    assert sorted(lin.state_dict().keys()) == ["linear.bias", "linear.weight"]


def test_linear_dropout_on_cpu_rows():
    cm = ME.CoordinateManager(torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 2]], dtype=torch.int32))
    x = ME.SparseTensor(torch.randn(3, 4), coordinate_manager=cm)
    lin = ME.MinkowskiLinear(4, 5)
    assert torch.allclose(lin(x).F, lin.linear(x.F))
    drop = ME.MinkowskiDropout(0.5).eval()
    assert torch.equal(drop(x).F, x.F)


def test_header_declares_new_symbols():
    """(tests/test_abi_cpu.py then proves that the cross-compiled library exports them)"""
    text = open(os.path.join(ROOT, "include", "minsu3d_hip.h")).read()
    for sym in ("ms3d_kmap_general", "ms3d_kmap_invert", "ms3d_pool_forward", "ms3d_pool_backward",
                "ms3d_spconv_backward_weight_g", "ms3d_spconv_layer_backward_g", "ms3d_spconv_wgrad_is_bf16x3_g"):
        assert re.search(r"\b" + sym + r"\s*\(", text), sym
