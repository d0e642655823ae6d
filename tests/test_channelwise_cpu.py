"""MinkowskiChannelwiseConvolution: what can be checked without a GPU -- the export, the parameter shapes and names, the init
bound, the refused geometries, that the layer stays out of prepare_conv_weights, the header, and the host arithmetic that
sizes the backward-weight workspace (called through ctypes on the cross-compiled library: no device needed)."""
import ctypes
import math
import os
import re

import pytest
import torch

import minsu3d_amd.MinkowskiEngine as ME
from minsu3d_amd.MinkowskiEngine import modules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ms3d_chconv_forward", "ms3d_chconv_backward_weight", "ms3d_chconv_wgrad_rows_per_part", "ms3d_chconv_wgrad_parts",
           "ms3d_chconv_wgrad_ws_floats")


def test_exported_from_the_package_and_the_dropin():
    assert isinstance(ME.MinkowskiChannelwiseConvolution, type)
    import minsu3d_amd.dropin.MinkowskiEngine as dropin
    assert dropin.MinkowskiChannelwiseConvolution is ME.MinkowskiChannelwiseConvolution
    assert "MinkowskiChannelwiseConvolution" in dropin.__all__


@pytest.mark.parametrize("ks,stride", [(1, 1), (2, 2), (3, 1), (5, 1)])
@pytest.mark.parametrize("bias", [False, True])
def test_parameters(ks, stride, bias):
    C = 6
    m = ME.MinkowskiChannelwiseConvolution(C, kernel_size=ks, stride=stride, bias=bias, dimension=3)
    K = ks ** 3
    assert tuple(m.kernel.shape) == (K, C) and m.kernel.dtype == torch.float32
    bound = 1.0 / math.sqrt(C * K)
    assert float(m.kernel.detach().abs().max()) <= bound
    if bias:
        assert isinstance(m.bias, torch.nn.Parameter) and tuple(m.bias.shape) == (1, C)
        assert float(m.bias.detach().abs().max()) <= bound
        assert list(m.state_dict().keys()) == ["kernel", "bias"]
    else:
        assert m.bias is None and list(m.state_dict().keys()) == ["kernel"]


def test_state_dict_round_trip():
    a = ME.MinkowskiChannelwiseConvolution(8, kernel_size=3, bias=True, dimension=3)
    b = ME.MinkowskiChannelwiseConvolution(8, kernel_size=3, bias=True, dimension=3)
    assert not torch.equal(a.kernel, b.kernel)
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.kernel, b.kernel) and torch.equal(a.bias, b.bias)


@pytest.mark.parametrize("kw,word", [(dict(kernel_size=2, stride=1), "kernel_size=2, stride=1"),
                                     (dict(kernel_size=3, stride=3), "kernel_size=3, stride=3"),
                                     (dict(kernel_size=3, stride=4), "stride=4"),
                                     (dict(kernel_size=(3, 3, 3)), "no per-axis tuples"),
                                     (dict(kernel_size=7), "at most 254 kernel offsets")])
def test_refused_geometries(kw, word):
    """the words of test_geometry_cpu.test_refused_geometries (and of check_geometry for tuples and large kernels)"""
    with pytest.raises(NotImplementedError) as e:
        ME.MinkowskiChannelwiseConvolution(4, dimension=3, **kw)
    assert word in str(e.value)


def test_refused_dimension():
    with pytest.raises(NotImplementedError, match="dimension=2"):
        ME.MinkowskiChannelwiseConvolution(4, kernel_size=3, dimension=2)


def test_stays_out_of_prepare_conv_weights():
    """not a _ConvBase: the one-launch weight layout collects the dense-weight convolutions only and never stamps a (K, C)
    kernel.  (Parameters on the CPU: the pass lays nothing out; what it COLLECTED is on the model.)"""
    from minsu3d_amd import backend

    class Recorder:
        weight_token = 7

        def __init__(self):
            self.calls = []

        def prep_weights_multi(self, layers, **kw):
            self.calls.append(list(layers))

    dw = ME.MinkowskiChannelwiseConvolution(4, kernel_size=3, bias=True, dimension=3)
    pw = ME.MinkowskiConvolution(4, 8, kernel_size=1, dimension=3)
    assert not isinstance(dw, modules._ConvBase)
    model = torch.nn.Sequential(dw, pw)
    rec = Recorder()
    backend.set_backend(rec)               # (tests/conftest.py restores the backend)
    before = dw.kernel.detach().clone()
    with torch.no_grad():
        ME.prepare_conv_weights(model)
    assert len(rec.calls) == 1 and rec.calls[0] == []
    assert model.__dict__["_ms3d_convs"] == (pw,)
    assert not hasattr(dw.kernel, "_ms3d_wf") and "_kernel_eff" not in dw.__dict__ and "_wf_buf" not in dw.__dict__
    assert torch.equal(dw.kernel, before)


def test_header_declares_the_five_symbols():
    text = open(os.path.join(ROOT, "include", "minsu3d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ms3d_[a-z0-9_]+)\s*\(", text))
    for s in SYMBOLS:
        assert s in declared, s


def _library():
    from minsu3d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.ms3d_chconv_wgrad_ws_floats.restype = ctypes.c_size_t
    return lib


def test_workspace_arithmetic():
    lib = _library()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    r = lib.ms3d_chconv_wgrad_rows_per_part()
    assert r >= 1
    for V in (0, 1, r - 1, r, r + 1, 2 * r + 1):
        parts = lib.ms3d_chconv_wgrad_parts(V)
        assert parts == -(-V // r), (V, parts)
        for K, C in ((1, 1), (8, 3), (27, 20), (125, 64), (216, 68)):
            assert lib.ms3d_chconv_wgrad_ws_floats(V, K, C) == parts * K * C, (V, K, C)


def test_size_function_registered_beside_the_others():
    """_lib.lib() gives the size_t function its return type (a default int would truncate a large workspace)"""
    from minsu3d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    assert _lib.lib().ms3d_chconv_wgrad_ws_floats.restype is ctypes.c_size_t
    V, K, C = 2 ** 31 - 1, 216, 4096            # > 2^32 floats
    r = _lib.lib().ms3d_chconv_wgrad_rows_per_part()
    assert _lib.lib().ms3d_chconv_wgrad_ws_floats(V, K, C) == -(-V // r) * K * C
