"""Per-sample voxel attention (ME.voxel_attention, ME.MinkowskiVoxelAttention, csrc/vattn.hip): what can be checked without a GPU
-- the exports, the module's parameter names and state_dict round trip, every argument check and every refusal, the
NotImplementedError for CPU tensors and for a backend without the kernels, the header, and the host side of the library through
ctypes on the cross-compiled library: the workspace size and the argument checks, which all happen before any launch."""
import ctypes
import os
import re

import pytest
import torch

import minsu3d_amd.MinkowskiEngine as ME
from minsu3d_amd.MinkowskiEngine import modules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ms3d_vattn_forward", "ms3d_vattn_backward_x", "ms3d_vattn_backward_kv", "ms3d_vattn_backward_kv_ws_floats")
E_WORKSPACE, E_UNSUPPORTED = 10001, 10002          # MS3D_E_* of include/minsu3d_hip.h
MAX_D, MAX_Q, MAX_C, MAX_B = 128, 1024, 1024, 65535        # the limits the header documents
# batch indices 0, 2 and 5 (gaps), the rows of the samples interleaved
COORDS = torch.tensor([[0, 0, 0, 0], [5, 1, 0, 0], [0, 0, 0, 2], [2, 1, 1, 1], [0, 0, 3, 0], [5, 2, 2, 2], [2, 0, 0, 1]],
                      dtype=torch.int32)
V, B = COORDS.size(0), 3


def _x(C=8, dtype=torch.float32):
    return ME.SparseTensor(torch.randn(V, C).to(dtype), coordinate_manager=ME.CoordinateManager(COORDS))


def test_exported_from_the_package_and_the_dropin():
    import minsu3d_amd.dropin.MinkowskiEngine as dropin
    assert isinstance(ME.MinkowskiVoxelAttention, type) and callable(ME.voxel_attention)
    for name in ("MinkowskiVoxelAttention", "voxel_attention"):
        assert getattr(dropin, name) is getattr(ME, name), name
        assert name in dropin.__all__, name
    doc = ME.__doc__
    assert "voxel_attention(x, keys, values" in doc and "MinkowskiVoxelAttention(embed_dim" in doc
    assert doc.index("MinkowskiQueryAttention(embed_dim") < doc.index("MinkowskiVoxelAttention(embed_dim") \
        < doc.index("Not supported (each raises")
    assert doc.count("Not supported") == 1                       # the section says "Out of scope", as the attention sections do
    assert "MultiheadAttention" in ME.voxel_attention.__doc__ and "NaN" in ME.voxel_attention.__doc__
    # the other direction now points here instead of refusing
    assert "voxel_attention" in ME.query_attention.__doc__ and "MinkowskiVoxelAttention" in ME.MinkowskiQueryAttention.__doc__
    with pytest.raises(TypeError, match="voxel_attention"):
        ME.query_attention(_x(), torch.randn(B, 4, 8), torch.randn(B, 4, 8), 2)
    with pytest.raises(TypeError, match="MinkowskiVoxelAttention"):
        ME.MinkowskiQueryAttention(8, 2)(_x(), torch.randn(B, 4, 8))


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("cq", [None, 5])
def test_parameters_and_state_dict_round_trip(cq, bias):
    E, H = 12, 3
    a = ME.MinkowskiVoxelAttention(E, H, query_channels=cq, bias=bias)
    ci = E if cq is None else cq
    assert a.query_channels == ci and a.embed_dim == E and a.num_heads == H
    for name, shape in (("q_proj", (E, E)), ("k_proj", (E, ci)), ("v_proj", (E, ci)), ("out_proj", (E, E))):
        lin = getattr(a, name)
        assert isinstance(lin, torch.nn.Linear) and tuple(lin.weight.shape) == shape, name
        assert (lin.bias is not None) == bias and (not bias or tuple(lin.bias.shape) == (E,)), name
    keys = [f"{n}.{p}" for n in ("q_proj", "k_proj", "v_proj", "out_proj") for p in (("weight", "bias") if bias else ("weight",))]
    assert sorted(a.state_dict().keys()) == sorted(keys)
    assert not isinstance(a, modules._ConvBase)
    b = ME.MinkowskiVoxelAttention(E, H, query_channels=cq, bias=bias)
    b.load_state_dict(a.state_dict())
    for key, t in a.state_dict().items():
        assert torch.equal(t, b.state_dict()[key]), key
    with pytest.raises(ValueError, match="num_heads=5"):
        ME.MinkowskiVoxelAttention(E, 5)


def test_stays_out_of_prepare_conv_weights():
    from minsu3d_amd import backend

    class Recorder:
        weight_token = 7

        def prep_weights_multi(self, layers, **kw):
            pass

    att = ME.MinkowskiVoxelAttention(4, 2)
    pw = ME.MinkowskiConvolution(4, 8, kernel_size=1, dimension=3)
    model = torch.nn.Sequential(att, pw)
    backend.set_backend(Recorder())               # (tests/conftest.py restores the backend)
    with torch.no_grad():
        ME.prepare_conv_weights(model)
    assert model.__dict__["_ms3d_convs"] == (pw,)


def test_value_errors():
    x = _x(C=8)
    k = torch.randn(B, 4, 8)
    with pytest.raises(ValueError, match="num_heads=3"):
        ME.voxel_attention(x, k, k, 3)
    for shape in ((B, 4, 6), (B, 8), (B * 4, 8), (B, 4, 8, 1)):
        with pytest.raises(ValueError, match=r"keys must have shape \[B, Q, C\] with C = 8"):
            ME.voxel_attention(x, torch.randn(shape), torch.randn(shape), 2)
    for shape in ((B, 5, 8), (B, 4, 6), (B - 1, 4, 8)):
        with pytest.raises(ValueError, match=r"keys\.shape != values\.shape"):
            ME.voxel_attention(x, k, torch.randn(shape), 2)
    for wrong in (2, 4, 6):                            # 6 = the largest batch index + 1: not the number of indices present
        with pytest.raises(ValueError) as e:
            ME.voxel_attention(x, torch.randn(wrong, 4, 8), torch.randn(wrong, 4, 8), 2)
        assert f"B = {wrong} samples" in str(e.value) and f"holds {B} batch indices" in str(e.value)
    for shape in ((V,), (4, V), (V, 5), (V - 1, 4)):
        with pytest.raises(ValueError, match=rf"attn_mask must have shape \[V, Q\] = \[{V}, 4\]"):
            ME.voxel_attention(x, k, k, 2, attn_mask=torch.zeros(shape, dtype=torch.bool))
    mod = ME.MinkowskiVoxelAttention(8, 2, query_channels=5)
    with pytest.raises(ValueError, match="the layer embed_dim=8"):
        mod(_x(C=6), torch.randn(B, 4, 5))
    with pytest.raises(ValueError, match=r"queries must have shape \[B, Q, 5\]"):
        mod(x, torch.randn(B, 4, 8))


def test_every_refusal_names_what_it_refuses():
    x = _x(C=8)
    k = torch.randn(B, 4, 8)
    with pytest.raises(TypeError, match=r"x is a SparseTensor, keys and values are dense tensors \[B, Q, C\]"):
        ME.voxel_attention(k, x, x, 2)                 # the arguments of query_attention
    with pytest.raises(TypeError, match="query_attention"):
        ME.voxel_attention(x, x, x, 2)
    with pytest.raises(TypeError, match="keys and values must be float32 tensors"):
        ME.voxel_attention(x, None, None, 2)
    with pytest.raises(TypeError, match="MinkowskiQueryAttention"):
        ME.MinkowskiVoxelAttention(8, 2)(k, x)
    with pytest.raises(NotImplementedError, match="a different Q per sample"):
        ME.voxel_attention(x, [torch.randn(3, 8), torch.randn(4, 8), torch.randn(2, 8)], k, 2)
    with pytest.raises(TypeError, match="float masks are not offered"):
        ME.voxel_attention(x, k, k, 2, attn_mask=torch.zeros(V, 4))
    with pytest.raises(ValueError, match="per-head masks are not offered"):
        ME.voxel_attention(x, k, k, 2, attn_mask=torch.zeros(2, V, 4, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="attention dropout"):
        ME.voxel_attention(x, k, k, 2, dropout=0.1)
    with pytest.raises(NotImplementedError, match="attention dropout"):
        ME.MinkowskiVoxelAttention(8, 2, dropout=0.1)
    for dtype in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match="float16 / bfloat16 are not offered"):
            ME.voxel_attention(x, k.to(dtype), k.to(dtype), 2)
        with pytest.raises(TypeError, match="float16 / bfloat16 are not offered"):
            ME.voxel_attention(_x(dtype=dtype), k, k, 2)
    with pytest.raises(NotImplementedError, match="ms3d_vattn_forward") as e:
        ME.voxel_attention(x, k, k, 2)                 # CPU tensors
    assert "CPU tensors" in str(e.value)
    with pytest.raises(NotImplementedError, match="ms3d_vattn_forward"):
        ME.MinkowskiVoxelAttention(8, 2)(x, k)


@pytest.mark.parametrize("C,H,Q,word,cap", [(MAX_D + 1, 1, 2, f"head dimension D = {MAX_D + 1}", MAX_D),
                                            (8, 2, MAX_Q + 1, f"Q = {MAX_Q + 1}", MAX_Q),
                                            (MAX_C + 8, 12, 2, f"C = num_heads \\* D = {MAX_C + 8}", MAX_C)])
def test_limits_are_named(C, H, Q, word, cap):
    k = torch.randn(B, Q, C)
    with pytest.raises(ValueError, match=word + f" is above the kernels' limit of {cap}$"):
        ME.voxel_attention(_x(C=C), k, k, H)


def test_empty_calls_return_zeros():
    x = _x(C=8)
    y = ME.voxel_attention(x, torch.randn(B, 0, 8), torch.randn(B, 0, 8), 2)           # nothing to attend to: zero
    assert isinstance(y, ME.SparseTensor) and y.coordinate_manager is x.coordinate_manager
    assert tuple(y.F.shape) == (V, 8) and y.F.dtype == torch.float32 and not y.F.any()
    e = ME.SparseTensor(torch.randn(0, 8), coordinate_manager=ME.CoordinateManager(COORDS[:0]))
    y = ME.voxel_attention(e, torch.randn(0, 4, 8), torch.randn(0, 4, 8), 2)
    assert tuple(y.F.shape) == (0, 8)
    with pytest.raises(ValueError, match="holds 0 batch indices"):
        ME.voxel_attention(e, torch.randn(1, 4, 8), torch.randn(1, 4, 8), 2)


def test_backend_without_the_kernels_is_an_error():
    from minsu3d_amd import backend
    from minsu3d_amd.MinkowskiEngine import functional as Fn

    class Bare:
        pass

    backend.set_backend(Bare())                        # (tests/conftest.py restores the backend)
    rows, k = torch.randn(V, 8), torch.randn(B, 4, 8)
    with pytest.raises(NotImplementedError, match=r"needs the HIP backend \(ms3d_vattn_forward\)"):
        Fn.voxel_attention_rows(rows, k, k, None, None, 2, 0.5)
    with pytest.raises(NotImplementedError, match="ms3d_vattn_forward"):
        ME.voxel_attention(_x(), k, k, 2)


def test_header_declares_the_symbols():
    text = open(os.path.join(ROOT, "include", "minsu3d_hip.h")).read()
    block = text[text.index("csrc/vattn.hip"):]
    assert "1 <= D <= 128, H >= 1, H * D <= 1024, 0 <= Q <= 1024, 0 <= B <= 65535" in block[:block.index("*/")]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ms3d_[a-z0-9_]+)\s*\(", text))
    for s in SYMBOLS:
        assert s in declared, s
    assert re.search(r"size_t\s+ms3d_vattn_backward_kv_ws_floats\s*\(\s*long chunks, int Q, int H, int D\s*\)", text)


def _library():
    from minsu3d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    lib.ms3d_vattn_backward_kv_ws_floats.restype = ctypes.c_size_t
    return lib


def test_size_function_registered_beside_the_others():
    """_lib.lib() gives the size_t function its return type (a default int would truncate a large workspace)"""
    from minsu3d_amd import _lib
    _library()
    assert _lib.lib().ms3d_vattn_backward_kv_ws_floats.restype is ctypes.c_size_t
    assert _lib.lib().ms3d_qattn_ws_floats.restype is ctypes.c_size_t            # (and the others keep theirs)


def test_workspace_arithmetic():
    lib = _library()
    L = ctypes.c_long
    for chunks in (0, 1, 7, 1000):
        for Q, H, D in ((1, 1, 1), (100, 8, 16), (33, 3, 5), (MAX_Q, 8, MAX_D)):
            assert lib.ms3d_vattn_backward_kv_ws_floats(L(chunks), Q, H, D) == chunks * Q * 2 * H * D, (chunks, Q, H, D)
    chunks, Q, H, D = 2 ** 24, MAX_Q, 8, MAX_D             # > 2^32 floats
    assert chunks * Q * 2 * H * D > 2 ** 32
    assert lib.ms3d_vattn_backward_kv_ws_floats(L(chunks), Q, H, D) == chunks * Q * 2 * H * D
    for empty in ((-5, Q, H, D), (3, 0, H, D), (3, Q, 0, D), (3, Q, H, 0)):
        assert lib.ms3d_vattn_backward_kv_ws_floats(L(empty[0]), *empty[1:]) == 0, empty
    # the peak-memory test's shape: 20 000 rows in chunks of the library's size, Q = 256, 8 heads of 8 channels -- the partials
    # are about a quarter of one float [V, Q] matrix
    r = lib.ms3d_qattn_rows_per_chunk()
    chunks = -(-12000 // r) + -(-8000 // r)
    assert 4 * lib.ms3d_vattn_backward_kv_ws_floats(L(chunks), 256, 8, 8) < 20000 * 256 * 4 // 3


def _calls(lib):
    """the three entry points with every pointer NULL: (V, B, Q, H, D) -> return code.  The argument checks come before anything
    is launched or dereferenced, so no device is needed."""
    N, f, L, Z = ctypes.c_void_p(0), ctypes.c_float(1.0), ctypes.c_long, ctypes.c_size_t(0)

    def forward(V, B, Q, H, D):
        return lib.ms3d_vattn_forward(N, N, N, N, N, N, L(V), B, Q, H, D, f, N, N, N)

    def backward_x(V, B, Q, H, D):
        return lib.ms3d_vattn_backward_x(N, N, N, N, N, N, N, N, N, L(V), B, Q, H, D, f, N, N, N)

    def backward_kv(V, B, Q, H, D):
        return lib.ms3d_vattn_backward_kv(N, N, N, N, N, N, N, N, N, N, N, N, N, L(V), B, 1, Q, H, D, f, N, N, N, Z, N)

    return forward, backward_x, backward_kv


@pytest.mark.parametrize("B_,Q,H,D", [(2, 4, 0, 8), (2, 4, 2, 0), (2, 4, 1, MAX_D + 1), (2, 4, 16, 128), (2, 4, 1025, 1),
                                      (2, MAX_Q + 1, 2, 8), (2, -1, 2, 8), (MAX_B + 1, 4, 2, 8), (-1, 4, 2, 8), (2, 4, -3, 8)])
def test_bad_shapes_are_unsupported_before_any_launch(B_, Q, H, D):
    for call in _calls(_library()):
        assert call(100, B_, Q, H, D) == E_UNSUPPORTED
        assert call(0, B_, Q, H, D) == E_UNSUPPORTED       # the shape is refused whatever the row count
    for call in _calls(_library()):
        assert call(-7, 2, 4, 2, 8) == E_UNSUPPORTED


def test_negative_chunk_count_is_unsupported():
    N, f, L = ctypes.c_void_p(0), ctypes.c_float(1.0), ctypes.c_long
    rc = _library().ms3d_vattn_backward_kv(N, N, N, N, N, N, N, N, N, N, N, N, N, L(100), 2, -1, 4, 2, 8, f, N, N, N,
                                           ctypes.c_size_t(0), N)
    assert rc == E_UNSUPPORTED


def test_nothing_to_do_is_success_and_null_pointers_are_refused():
    for call in _calls(_library()):
        for Q, H, D in ((1, 1, 1), (100, 8, 16), (MAX_Q, 8, MAX_D)):
            assert call(0, 2, Q, H, D) == 0
            assert call(100, 0, Q, H, D) == 0
            assert call(100, 2, 0, H, D) == 0
            assert call(100, 2, Q, H, D) == E_UNSUPPORTED      # rows to work on and nothing to read them from


def test_short_workspace_is_refused():
    """too few workspace floats: MS3D_E_WORKSPACE, decided on the host (the pointers are never followed: they are host buffers
    here and no device exists)"""
    lib = _library()
    V_, B_, chunks, Q, H, D = 100, 2, 2, 5, 2, 4
    buf = (ctypes.c_float * 16)()
    P, f, L = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_float(1.0), ctypes.c_long
    need = lib.ms3d_vattn_backward_kv_ws_floats(L(chunks), Q, H, D)
    assert need == chunks * Q * 2 * H * D > 0
    rc = lib.ms3d_vattn_backward_kv(P, P, P, P, P, P, P, P, P, P, P, P, P, L(V_), B_, chunks, Q, H, D, f, P, P, P,
                                    ctypes.c_size_t(need - 1), ctypes.c_void_p(0))
    assert rc == E_WORKSPACE
    # both outputs NULL: nothing to write is refused, not run
    rc = lib.ms3d_vattn_backward_kv(P, P, P, P, P, P, P, P, P, P, P, P, P, L(V_), B_, chunks, Q, H, D, f, ctypes.c_void_p(0),
                                    ctypes.c_void_p(0), P, ctypes.c_size_t(need), ctypes.c_void_p(0))
    assert rc == E_UNSUPPORTED
