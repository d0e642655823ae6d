"""Kernel-map attention (ME.kernel_attention, ME.MinkowskiKernelAttention, csrc/kattn.hip): what can be checked without a GPU
-- the exports, the parameter shapes and names, every ValueError, the geometry refusals in their existing words, the
NotImplementedError of a backend without the kernels, the header, and the host side of the library through ctypes on the
cross-compiled library: the workspace arithmetic and the argument checks, which all happen before any launch."""
import ctypes
import os
import re

import pytest
import torch

import minsu3d_amd.MinkowskiEngine as ME
from minsu3d_amd.MinkowskiEngine import modules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ms3d_kattn_forward", "ms3d_kattn_backward_q", "ms3d_kattn_backward_kv", "ms3d_kattn_rows_per_part",
           "ms3d_kattn_dbias_parts", "ms3d_kattn_dbias_ws_floats")
E_WORKSPACE, E_UNSUPPORTED = 10001, 10002          # MS3D_E_* of include/minsu3d_hip.h
MAX_D = 128                                        # the head dimension the header documents as the cap
COORDS = torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 2], [1, 1, 1, 1], [0, 0, 3, 0], [1, 2, 2, 2]], dtype=torch.int32)


def _tensors(C=8, cq=None, ts_q=1):
    cm = ME.CoordinateManager(COORDS)
    V = COORDS.size(0)
    q = ME.SparseTensor(torch.randn(V, C if cq is None else cq), coordinate_manager=cm, tensor_stride=ts_q)
    k = ME.SparseTensor(torch.randn(V, C), coordinate_manager=cm)
    v = ME.SparseTensor(torch.randn(V, C), coordinate_manager=cm)
    return q, k, v


def test_exported_from_the_package_and_the_dropin():
    import minsu3d_amd.dropin.MinkowskiEngine as dropin
    assert isinstance(ME.MinkowskiKernelAttention, type) and callable(ME.kernel_attention)
    for name in ("MinkowskiKernelAttention", "kernel_attention"):
        assert getattr(dropin, name) is getattr(ME, name), name
        assert name in dropin.__all__, name
    assert "kernel_attention" in ME.__doc__ and "MinkowskiKernelAttention" in ME.__doc__
    assert ME.__doc__.index("MinkowskiKernelAttention") < ME.__doc__.index("Not supported (each raises")


@pytest.mark.parametrize("ks,K", [(1, 1), (3, 27), (5, 125)])
def test_parameters(ks, K):
    C, H = 12, 3
    m = ME.MinkowskiKernelAttention(C, H, kernel_size=ks)
    assert isinstance(m.qkv, torch.nn.Linear) and isinstance(m.proj, torch.nn.Linear)
    assert tuple(m.qkv.weight.shape) == (3 * C, C) and tuple(m.qkv.bias.shape) == (3 * C,)
    assert tuple(m.proj.weight.shape) == (C, C) and tuple(m.proj.bias.shape) == (C,)
    assert isinstance(m.rel_bias, torch.nn.Parameter) and tuple(m.rel_bias.shape) == (K, H)
    assert m.rel_bias.dtype == torch.float32 and torch.equal(m.rel_bias.detach(), torch.zeros(K, H))
    assert sorted(m.state_dict().keys()) == sorted(["qkv.weight", "qkv.bias", "proj.weight", "proj.bias", "rel_bias"])
    assert not isinstance(m, modules._ConvBase)
    n = ME.MinkowskiKernelAttention(C, H, kernel_size=ks, qkv_bias=False, rel_pos_bias=False)
    assert n.rel_bias is None and n.qkv.bias is None
    assert sorted(n.state_dict().keys()) == sorted(["qkv.weight", "proj.weight", "proj.bias"])


def test_region_parameters_and_state_dict_round_trip():
    cross = ME.KernelGenerator(kernel_size=3, region_type=ME.RegionType.HYPER_CROSS)
    a = ME.MinkowskiKernelAttention(8, 2, kernel_generator=cross)
    assert tuple(a.rel_bias.shape) == (7, 2) and a.kernel_volume == 7
    b = ME.MinkowskiKernelAttention(8, 2, kernel_generator=cross)
    with torch.no_grad():
        a.rel_bias.uniform_(-1, 1)
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.rel_bias, b.rel_bias) and torch.equal(a.qkv.weight, b.qkv.weight)


def test_stays_out_of_prepare_conv_weights():
    from minsu3d_amd import backend

    class Recorder:
        weight_token = 7

        def __init__(self):
            self.calls = []

        def prep_weights_multi(self, layers, **kw):
            self.calls.append(list(layers))

    att = ME.MinkowskiKernelAttention(4, 2)
    pw = ME.MinkowskiConvolution(4, 8, kernel_size=1, dimension=3)
    model = torch.nn.Sequential(att, pw)
    rec = Recorder()
    backend.set_backend(rec)               # (tests/conftest.py restores the backend)
    with torch.no_grad():
        ME.prepare_conv_weights(model)
    assert model.__dict__["_ms3d_convs"] == (pw,)


def test_value_errors():
    q, k, v = _tensors(C=8)
    with pytest.raises(ValueError, match="num_heads=3"):
        ME.kernel_attention(q, k, v, 3)
    with pytest.raises(ValueError, match="num_heads=3"):
        ME.MinkowskiKernelAttention(8, 3)
    q6, _, _ = _tensors(C=8, cq=6)
    with pytest.raises(ValueError, match="same number of channels"):
        ME.kernel_attention(q6, k, v, 2)
    v6 = ME.SparseTensor(torch.randn(COORDS.size(0), 6), coordinate_manager=k.coordinate_manager)
    with pytest.raises(ValueError, match="same number of channels"):
        ME.kernel_attention(q, k, v6, 2)
    _, _, v_other = _tensors(C=8)                      # a manager of its own
    with pytest.raises(ValueError, match="same coordinate set"):
        ME.kernel_attention(q, k, v_other, 2)
    v2 = ME.SparseTensor(torch.randn(COORDS.size(0), 8), coordinate_manager=k.coordinate_manager, tensor_stride=2)
    with pytest.raises(ValueError, match="same coordinate set"):
        ME.kernel_attention(q, k, v2, 2)
    q2 = ME.SparseTensor(torch.randn(COORDS.size(0), 8), coordinate_manager=k.coordinate_manager, tensor_stride=2)
    with pytest.raises(ValueError, match="tensor stride 2"):
        ME.kernel_attention(q2, k, v, 2)               # stride 1 wants q at 1
    with pytest.raises(ValueError, match="tensor stride 1"):
        ME.kernel_attention(q, k, v, 2, kernel_size=2, stride=2)       # stride 2 wants q at 2
    for shape in ((27,), (2, 27), (26, 2), (27, 4)):
        with pytest.raises(ValueError, match=r"rel_bias must have shape \(K, num_heads\) = \(27, 2\)"):
            ME.kernel_attention(q, k, v, 2, rel_bias=torch.zeros(shape))
    cross = ME.KernelGenerator(kernel_size=3, region_type=ME.RegionType.HYPER_CROSS)
    with pytest.raises(ValueError, match=r"\(7, 2\)"):
        ME.kernel_attention(q, k, v, 2, rel_bias=torch.zeros(27, 2), kernel_generator=cross)
    with pytest.raises(ValueError, match="contradicts the kernel_generator"):
        ME.kernel_attention(q, k, v, 2, kernel_size=5, kernel_generator=cross)


@pytest.mark.parametrize("kw,word", [(dict(kernel_size=2, stride=1), "kernel_size=2, stride=1"),
                                     (dict(kernel_size=3, stride=3), "kernel_size=3, stride=3"),
                                     (dict(kernel_size=3, stride=4), "stride=4"),
                                     (dict(kernel_size=(3, 3, 3)), "no per-axis tuples"),
                                     (dict(kernel_size=7), "at most 254 kernel offsets")])
def test_refused_geometries(kw, word):
    """the words of test_geometry_cpu.test_refused_geometries (and of check_geometry for tuples and large kernels)"""
    q, k, v = _tensors()
    with pytest.raises(NotImplementedError) as e:
        ME.kernel_attention(q, k, v, 2, **kw)
    assert word in str(e.value)
    want = None
    try:
        ME.MinkowskiMaxPooling(**kw)
    except NotImplementedError as ref:
        want = str(ref)
    assert str(e.value) == want                        # word for word what the other layers say
    if "stride" not in kw:
        with pytest.raises(NotImplementedError) as e:
            ME.MinkowskiKernelAttention(8, 2, **kw)
        assert word in str(e.value)


def test_refused_dimension():
    with pytest.raises(NotImplementedError, match="dimension=2: only 3-D sparse tensors are supported"):
        ME.MinkowskiKernelAttention(8, 2, dimension=2)


def test_backend_without_the_kernels_is_an_error():
    from minsu3d_amd import backend
    from minsu3d_amd.MinkowskiEngine import functional as Fn
    V = COORDS.size(0)
    ident = torch.arange(V, dtype=torch.int32).view(1, V)

    class Bare:
        pass

    class Tables:                                      # builds the maps, has no attention kernel
        def kmap_k3(self, coords, ts):
            return torch.full((27, V), -1, dtype=torch.int32)

        def kmap_invert(self, nbr, K, vout, vin):
            return nbr.clone()

    sentence = r"kernel-map attention needs the HIP backend \(ms3d_kattn_forward\)"
    backend.set_backend(Bare())                        # (tests/conftest.py restores the backend)
    x = torch.randn(V, 8)
    with pytest.raises(NotImplementedError, match=sentence):
        Fn.kernel_attention_rows(x, x, x, None, ident, ident, V, V, 1, 2, 0.5)
    backend.set_backend(Tables())
    q, k, v = _tensors()
    with pytest.raises(NotImplementedError, match=sentence):
        ME.kernel_attention(q, k, v, 2)
    with pytest.raises(NotImplementedError, match=sentence):
        ME.MinkowskiKernelAttention(8, 2)(k)


def test_header_declares_the_six_symbols():
    text = open(os.path.join(ROOT, "include", "minsu3d_hip.h")).read()
    assert "D <= 128" in text                          # the documented cap MAX_D stands for
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
    lib.ms3d_kattn_dbias_ws_floats.restype = ctypes.c_size_t
    return lib


def test_workspace_arithmetic():
    lib = _library()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    r = lib.ms3d_kattn_rows_per_part()
    assert r >= 1
    for V in (0, 1, r - 1, r, r + 1, 2 * r + 1):
        parts = lib.ms3d_kattn_dbias_parts(V)
        assert parts == -(-V // r), (V, parts)
        for K, H in ((1, 1), (8, 3), (27, 4), (125, 8), (254, 1024)):
            assert lib.ms3d_kattn_dbias_ws_floats(V, K, H) == parts * K * H, (V, K, H)
    V, K, H = 2 ** 31 - 1, 254, 1024                   # > 2^32 floats
    assert -(-V // r) * K * H > 2 ** 32
    assert lib.ms3d_kattn_dbias_ws_floats(V, K, H) == -(-V // r) * K * H
    assert lib.ms3d_kattn_dbias_ws_floats(-5, K, H) == 0 and lib.ms3d_kattn_dbias_parts(-5) == 0


def test_size_function_registered_beside_the_others():
    """_lib.lib() gives the size_t function its return type (a default int would truncate a large workspace)"""
    from minsu3d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    assert _lib.lib().ms3d_kattn_dbias_ws_floats.restype is ctypes.c_size_t
    V, K, H = 2 ** 31 - 1, 254, 1024
    r = _lib.lib().ms3d_kattn_rows_per_part()
    assert _lib.lib().ms3d_kattn_dbias_ws_floats(V, K, H) == -(-V // r) * K * H


def _calls(lib):
    """the three entry points with every pointer NULL: (Vrows, K, H, D) -> return code.  The argument checks come before
    anything is launched or dereferenced, so no device is needed."""
    N, f = ctypes.c_void_p(0), ctypes.c_float(1.0)

    def forward(V, K, H, D):
        return lib.ms3d_kattn_forward(N, N, N, N, N, V, K, H, D, f, N, N, N)

    def backward_q(V, K, H, D):
        return lib.ms3d_kattn_backward_q(N, N, N, N, N, N, N, N, V, K, H, D, f, N, N, N, N, ctypes.c_size_t(0), N)

    def backward_kv(V, K, H, D):
        return lib.ms3d_kattn_backward_kv(N, N, N, N, N, N, N, N, N, V, K, H, D, f, N, N, N)

    return forward, backward_q, backward_kv


@pytest.mark.parametrize("K,H,D", [(0, 2, 8), (255, 2, 8), (27, 0, 8), (27, 2, 0), (27, 2, MAX_D + 1), (-1, 2, 8), (27, -3, 8)])
def test_bad_shapes_are_unsupported_before_any_launch(K, H, D):
    for call in _calls(_library()):
        assert call(100, K, H, D) == E_UNSUPPORTED
        assert call(0, K, H, D) == E_UNSUPPORTED       # the shape is refused whatever the row count


def test_no_rows_is_success_and_null_pointers_are_refused():
    for call in _calls(_library()):
        for K, H, D in ((1, 1, 1), (27, 4, 16), (254, 8, MAX_D)):
            assert call(0, K, H, D) == 0
            assert call(-7, K, H, D) == 0
            assert call(100, K, H, D) == E_UNSUPPORTED         # rows to work on and nothing to read them from


def test_short_workspace_is_refused():
    """a dbias request with too few workspace floats: MS3D_E_WORKSPACE, decided on the host (the pointers are never followed:
    they are host buffers here and no device exists)"""
    lib = _library()
    V, K, H, D = 100, 27, 2, 4
    buf = (ctypes.c_float * 16)()
    P = ctypes.cast(buf, ctypes.c_void_p)
    need = lib.ms3d_kattn_dbias_ws_floats(V, K, H)
    assert need == -(-V // lib.ms3d_kattn_rows_per_part()) * K * H > 0
    rc = lib.ms3d_kattn_backward_q(P, P, P, P, P, P, P, P, V, K, H, D, ctypes.c_float(1.0), P, P, P, P,
                                   ctypes.c_size_t(need - 1), ctypes.c_void_p(0))
    assert rc == E_WORKSPACE
