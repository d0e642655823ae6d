"""MinkowskiInstanceNorm / MinkowskiStableInstanceNorm and the table of activation layers: what can be checked without a GPU
-- the exports, the parameter shapes, init and names, that train() and eval() differ in nothing, the refusals, the header, and
the host arithmetic of the library (slice count, workspace size) called through ctypes on the cross-compiled library."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

import minsu3d_amd.MinkowskiEngine as ME

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ms3d_inorm_slices", "ms3d_inorm_workspace_bytes", "ms3d_inorm_forward", "ms3d_inorm_backward")
NORMS = (("MinkowskiInstanceNorm", 1e-8), ("MinkowskiStableInstanceNorm", 1e-6))
ACTIVATIONS = (("MinkowskiELU", nn.ELU, dict(alpha=0.7)), ("MinkowskiLeakyReLU", nn.LeakyReLU, dict(negative_slope=0.2)),
               ("MinkowskiPReLU", nn.PReLU, dict(num_parameters=5, init=0.1)), ("MinkowskiSELU", nn.SELU, {}),
               ("MinkowskiCELU", nn.CELU, dict(alpha=1.3)), ("MinkowskiGELU", nn.GELU, {}), ("MinkowskiSiLU", nn.SiLU, {}),
               ("MinkowskiTanh", nn.Tanh, {}), ("MinkowskiSoftplus", nn.Softplus, dict(beta=2.0, threshold=5.0)),
               ("MinkowskiHardswish", nn.Hardswish, {}), ("MinkowskiHardtanh", nn.Hardtanh, dict(min_val=-0.5, max_val=0.8)),
               ("MinkowskiReLU6", nn.ReLU6, {}), ("MinkowskiSoftmax", nn.Softmax, dict(dim=1)),
               ("MinkowskiLogSoftmax", nn.LogSoftmax, dict(dim=1)))


def test_exported_from_the_package_and_the_dropin():
    import minsu3d_amd.dropin.MinkowskiEngine as dropin
    for name in [n for n, _ in NORMS] + [n for n, _, _ in ACTIVATIONS]:
        assert isinstance(getattr(ME, name), type), name
        assert getattr(dropin, name) is getattr(ME, name), name
        assert name in dropin.__all__, name
    assert issubclass(ME.MinkowskiStableInstanceNorm, ME.MinkowskiInstanceNorm)


@pytest.mark.parametrize("name,eps", NORMS)
def test_parameters(name, eps):
    m = getattr(ME, name)(6)
    assert m.num_features == 6 and m.eps == eps
    assert isinstance(m.weight, nn.Parameter) and isinstance(m.bias, nn.Parameter)
    assert tuple(m.weight.shape) == (1, 6) and tuple(m.bias.shape) == (1, 6)
    assert m.weight.dtype == torch.float32 and m.bias.dtype == torch.float32
    assert torch.equal(m.weight.detach(), torch.ones(1, 6)) and torch.equal(m.bias.detach(), torch.zeros(1, 6))
    assert list(m.state_dict().keys()) == ["weight", "bias"]
    assert list(dict(m.named_buffers()).keys()) == []          # no running statistics
    assert getattr(ME, name)(6, eps=1e-3).eps == 1e-3


@pytest.mark.parametrize("name,eps", NORMS)
def test_state_dict_round_trip(name, eps):
    a, b = getattr(ME, name)(8), getattr(ME, name)(8)
    with torch.no_grad():
        a.weight.uniform_(0.5, 1.5)
        a.bias.uniform_(-0.3, 0.3)
    assert not torch.equal(a.weight, b.weight)
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias)


class _Recorder:
    """a backend that records what the layer hands to inorm_forward and returns x itself"""

    def __init__(self):
        self.calls = []

    def inorm_forward(self, x, group, eps, weight, bias):
        self.calls.append((group.order, group.seg_start, group.seg_of_row, eps))
        B = group.seg_start.numel() - 1
        return x.clone(), x.new_zeros((B, x.size(1))), x.new_ones((B, x.size(1)))


def _cpu_tensor(C=4):
    coords = torch.tensor([[2, 0, 0, 0], [0, 1, 0, 0], [2, 0, 0, 2], [5, 1, 1, 1], [0, 0, 3, 0], [2, 2, 2, 2]], dtype=torch.int32)
    cm = ME.CoordinateManager(coords)
    return cm, ME.SparseTensor(torch.randn(coords.size(0), C), coordinate_manager=cm)


@pytest.mark.parametrize("name,eps", NORMS)
def test_train_and_eval_are_the_same_layer(name, eps):
    """no flag of the module changes with the mode and the backend is handed the same arguments in both"""
    from minsu3d_amd import backend
    m = getattr(ME, name)(4)
    rec = _Recorder()
    backend.set_backend(rec)               # (tests/conftest.py restores the backend)
    cm, x = _cpu_tensor()
    flags = []
    for mode in (True, False):
        m.train(mode)
        flags.append({k: v for k, v in vars(m).items() if not k.startswith("_") and k != "training"})
        y = m(x)
        assert y.coordinate_manager is cm and y.tensor_stride == 1 and y._pending is None
    assert flags[0] == flags[1]
    (o0, s0, r0, e0), (o1, s1, r1, e1) = rec.calls
    assert e0 == e1 == eps and torch.equal(o0, o1) and torch.equal(s0, s1) and torch.equal(r0, r1)


def test_batch_segments_follow_batch_rows():
    """batch indices 0, 2, 5 handed over interleaved: segment = the rank of the batch index; batch_rows is what it was"""
    cm, _ = _cpu_tensor()
    order, inv, offsets, counts = cm.batch_rows(1)
    seg = cm.batch_segments(1)
    assert seg.dtype == torch.int32 and seg.tolist() == [1, 0, 1, 2, 0, 1]
    assert cm.batch_segments(1) is seg                                     # cached per tensor stride
    assert order.dtype == torch.int64 and order.tolist() == [1, 4, 0, 2, 5, 3]
    assert offsets.dtype == torch.int32 and offsets.tolist() == [0, 2, 5, 6]
    assert counts.view(-1).tolist() == [2.0, 3.0, 1.0] and inv[order].tolist() == list(range(6))
    for s in range(3):
        assert (seg[order[offsets[s]:offsets[s + 1]]] == s).all()


@pytest.mark.parametrize("name,eps", NORMS)
def test_channel_mismatch_names_both_numbers(name, eps):
    _, x = _cpu_tensor(C=4)
    with pytest.raises(ValueError) as e:
        getattr(ME, name)(7)(x)
    assert "4" in str(e.value) and "7" in str(e.value) and name in str(e.value)


@pytest.mark.parametrize("name,eps", NORMS)
def test_backend_without_the_kernel_is_an_error(name, eps):
    from minsu3d_amd import backend
    from minsu3d_amd.MinkowskiEngine import functional as Fn

    class Bare:
        pass

    backend.set_backend(Bare())            # (tests/conftest.py restores the backend)
    cm, x = _cpu_tensor()
    with pytest.raises(NotImplementedError, match=r"needs the HIP backend \(ms3d_inorm_forward\)"):
        getattr(ME, name)(4)(x)
    with pytest.raises(NotImplementedError, match=r"needs the HIP backend \(ms3d_inorm_forward\)"):
        Fn.instance_norm(x.F, None, None, cm.batch_group(1), 1e-5)


@pytest.mark.parametrize("name,module,kw", ACTIVATIONS)
def test_activation_equals_its_torch_module(name, module, kw):
    _, x = _cpu_tensor(C=5)
    x = x._like(3.0 * x.F)
    layer = getattr(ME, name)(**kw)
    assert type(layer.module) is module
    want = module(**kw)(x.F)
    y = layer(x)
    assert isinstance(y, ME.SparseTensor) and y.coordinate_manager is x.coordinate_manager and y.tensor_stride == 1
    assert torch.equal(y.F, want)
    args = tuple(kw.values())              # positional arguments reach the module too
    assert torch.equal(getattr(ME, name)(*args)(x).F, want)


def test_prelu_keeps_minkowskiengine_key():
    m = ME.MinkowskiPReLU(num_parameters=3)
    assert list(m.state_dict().keys()) == ["module.weight"]
    assert list(ME.MinkowskiELU().state_dict().keys()) == []


def test_relu_and_sigmoid_are_untouched():
    from minsu3d_amd.MinkowskiEngine import modules
    assert not issubclass(ME.MinkowskiReLU, modules._NonlinearityBase)
    assert not issubclass(ME.MinkowskiSigmoid, modules._NonlinearityBase)
    assert not hasattr(ME.MinkowskiReLU(), "module")


def test_header_declares_the_symbols():
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
    return _lib


def test_slices_and_workspace_arithmetic():
    """ms3d_inorm_workspace_bytes(B, C) = 8 * 2 * B * (slices + 1) * C (include/minsu3d_hip.h), 0 for B <= 0"""
    lib = ctypes.CDLL(_library().LIB_PATH)
    lib.ms3d_inorm_workspace_bytes.restype = ctypes.c_size_t
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    S = lib.ms3d_inorm_slices()
    assert S >= 1
    for B in (-1, 0):
        assert lib.ms3d_inorm_workspace_bytes(B, 32) == 0
    for B in (1, 3, 16, 65535):
        for C in (1, 3, 4, 66, 132, 4096):
            assert lib.ms3d_inorm_workspace_bytes(B, C) == 8 * 2 * B * (S + 1) * C, (B, C)
    assert 8 * 2 * 65535 * (S + 1) * 4096 > 2 ** 32


def test_size_function_registered_beside_the_others():
    """_lib.lib() gives the size_t function its return type (a default int would truncate a large workspace)"""
    lib = _library().lib()
    assert lib.ms3d_inorm_workspace_bytes.restype is ctypes.c_size_t
    S = lib.ms3d_inorm_slices()
    B, C = 65535, 8192
    want = 8 * 2 * B * (S + 1) * C
    assert want > 2 ** 32 and lib.ms3d_inorm_workspace_bytes(B, C) == want
