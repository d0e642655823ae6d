"""Per-sample query attention (ME.query_attention, ME.MinkowskiQueryAttention, csrc/qattn.hip): what can be checked without a
GPU -- the exports, the module's parameter names and state_dict round trip, every argument check and every refusal, the
NotImplementedError for CPU tensors and for a backend without the kernels, the header, and the host side of the library through
ctypes on the cross-compiled library: the chunk arithmetic, the workspace sizes and the argument checks, which all happen
before any launch."""
import ctypes
import os
import re

import pytest
import torch

import minsu3d_amd.MinkowskiEngine as ME
from minsu3d_amd.MinkowskiEngine import modules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ms3d_qattn_forward", "ms3d_qattn_backward_q", "ms3d_qattn_backward_kv", "ms3d_qattn_rows_per_chunk",
           "ms3d_qattn_chunks", "ms3d_qattn_chunk_list", "ms3d_qattn_ws_floats", "ms3d_qattn_backward_ws_floats")
E_WORKSPACE, E_UNSUPPORTED = 10001, 10002          # MS3D_E_* of include/minsu3d_hip.h
MAX_D, MAX_Q, MAX_C, MAX_B = 128, 1024, 1024, 65535        # the limits the header documents
# batch indices 0, 2 and 5 (gaps), the rows of the samples interleaved
COORDS = torch.tensor([[0, 0, 0, 0], [5, 1, 0, 0], [0, 0, 0, 2], [2, 1, 1, 1], [0, 0, 3, 0], [5, 2, 2, 2], [2, 0, 0, 1]],
                      dtype=torch.int32)
V, B = COORDS.size(0), 3


def _tensors(C=8, cv=None):
    cm = ME.CoordinateManager(COORDS)
    k = ME.SparseTensor(torch.randn(V, C), coordinate_manager=cm)
    v = ME.SparseTensor(torch.randn(V, C if cv is None else cv), coordinate_manager=cm)
    return k, v


def test_exported_from_the_package_and_the_dropin():
    import minsu3d_amd.dropin.MinkowskiEngine as dropin
    assert isinstance(ME.MinkowskiQueryAttention, type) and callable(ME.query_attention)
    for name in ("MinkowskiQueryAttention", "query_attention"):
        assert getattr(dropin, name) is getattr(ME, name), name
        assert name in dropin.__all__, name
    assert "query_attention" in ME.__doc__ and "MinkowskiQueryAttention" in ME.__doc__
    assert ME.__doc__.index("MinkowskiQueryAttention") < ME.__doc__.index("Not supported (each raises")
    assert "MultiheadAttention" in ME.query_attention.__doc__ and "NaN" in ME.query_attention.__doc__


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("cin", [None, 5])
def test_parameters_and_state_dict_round_trip(cin, bias):
    E, H = 12, 3
    a = ME.MinkowskiQueryAttention(E, H, in_channels=cin, bias=bias)
    ci = E if cin is None else cin
    for name, shape in (("q_proj", (E, E)), ("k_proj", (E, ci)), ("v_proj", (E, ci)), ("out_proj", (E, E))):
        lin = getattr(a, name)
        assert isinstance(lin, torch.nn.Linear) and tuple(lin.weight.shape) == shape, name
        assert (lin.bias is not None) == bias and (not bias or tuple(lin.bias.shape) == (E,)), name
    keys = [f"{n}.{p}" for n in ("q_proj", "k_proj", "v_proj", "out_proj") for p in (("weight", "bias") if bias else ("weight",))]
    assert sorted(a.state_dict().keys()) == sorted(keys)
    assert not isinstance(a, modules._ConvBase)
    b = ME.MinkowskiQueryAttention(E, H, in_channels=cin, bias=bias)
    b.load_state_dict(a.state_dict())
    for key, t in a.state_dict().items():
        assert torch.equal(t, b.state_dict()[key]), key
    with pytest.raises(ValueError, match="num_heads=5"):
        ME.MinkowskiQueryAttention(E, 5)


def test_stays_out_of_prepare_conv_weights():
    from minsu3d_amd import backend

    class Recorder:
        weight_token = 7

        def prep_weights_multi(self, layers, **kw):
            pass

    att = ME.MinkowskiQueryAttention(4, 2)
    pw = ME.MinkowskiConvolution(4, 8, kernel_size=1, dimension=3)
    model = torch.nn.Sequential(att, pw)
    backend.set_backend(Recorder())               # (tests/conftest.py restores the backend)
    with torch.no_grad():
        ME.prepare_conv_weights(model)
    assert model.__dict__["_ms3d_convs"] == (pw,)


def test_value_errors():
    k, v = _tensors(C=8)
    q = torch.randn(B, 4, 8)
    with pytest.raises(ValueError, match="num_heads=3"):
        ME.query_attention(q, k, v, 3)
    _, v_other = _tensors(C=8)                         # a manager of its own
    with pytest.raises(ValueError, match="same coordinate set"):
        ME.query_attention(q, k, v_other, 2)
    v2 = ME.SparseTensor(torch.randn(V, 8), coordinate_manager=k.coordinate_manager, tensor_stride=2)
    with pytest.raises(ValueError, match="same coordinate set"):
        ME.query_attention(q, k, v2, 2)
    for shape in ((B, 4, 6), (B, 8), (B * 4, 8), (B, 4, 8, 1)):
        with pytest.raises(ValueError, match=r"queries must have shape \[B, Q, C\] with C = 8"):
            ME.query_attention(torch.randn(shape), k, v, 2)
    for wrong in (2, 4, 6):                            # 6 = the largest batch index + 1: not the number of indices present
        with pytest.raises(ValueError) as e:
            ME.query_attention(torch.randn(wrong, 4, 8), k, v, 2)
        assert f"B = {wrong} samples" in str(e.value) and f"holds {B} batch indices" in str(e.value)
    for shape in ((V,), (4, V), (V, 5), (V - 1, 4)):
        with pytest.raises(ValueError, match=rf"attn_mask must have shape \[V, Q\] = \[{V}, 4\]"):
            ME.query_attention(q, k, v, 2, attn_mask=torch.zeros(shape, dtype=torch.bool))


def test_every_refusal_names_what_it_refuses():
    k, v = _tensors(C=8)
    q = torch.randn(B, 4, 8)
    with pytest.raises(NotImplementedError, match="a different Q per sample"):
        ME.query_attention([torch.randn(3, 8), torch.randn(4, 8), torch.randn(2, 8)], k, v, 2)
    with pytest.raises(TypeError, match="float masks are not offered"):
        ME.query_attention(q, k, v, 2, attn_mask=torch.zeros(V, 4))
    with pytest.raises(ValueError, match="per-head masks are not offered"):
        ME.query_attention(q, k, v, 2, attn_mask=torch.zeros(2, V, 4, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="attention dropout"):
        ME.query_attention(q, k, v, 2, dropout=0.1)
    with pytest.raises(NotImplementedError, match="attention dropout"):
        ME.MinkowskiQueryAttention(8, 2, dropout=0.1)
    _, v6 = _tensors(C=8, cv=6)
    v6 = ME.SparseTensor(v6.F, coordinate_manager=k.coordinate_manager)
    with pytest.raises(ValueError, match="a value head dimension different from D"):
        ME.query_attention(q, k, v6, 2)
    for dtype in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match="float16 / bfloat16 are not offered"):
            ME.query_attention(q.to(dtype), k, v, 2)
        kh = ME.SparseTensor(k.F.to(dtype), coordinate_manager=k.coordinate_manager)
        with pytest.raises(TypeError, match="float16 / bfloat16 are not offered"):
            ME.query_attention(q, kh, kh, 2)
    with pytest.raises(TypeError, match="the reverse direction \\(voxels attending to queries\\)"):
        ME.query_attention(k, q, q, 2)
    with pytest.raises(TypeError, match="the reverse direction \\(voxels attending to queries\\)"):
        ME.MinkowskiQueryAttention(8, 2)(k, q)
    with pytest.raises(NotImplementedError, match="ms3d_qattn_forward") as e:
        ME.query_attention(q, k, v, 2)                 # CPU tensors
    assert "CPU tensors" in str(e.value)
    with pytest.raises(NotImplementedError, match="ms3d_qattn_forward"):
        ME.MinkowskiQueryAttention(8, 2)(q, k)


@pytest.mark.parametrize("C,H,Q,word", [(MAX_D + 1, 1, 2, f"head dimension D = {MAX_D + 1}"), (8, 2, MAX_Q + 1, f"Q = {MAX_Q + 1}"),
                                        (MAX_C + 8, 12, 2, f"C = num_heads \\* D = {MAX_C + 8}")])
def test_limits_are_named(C, H, Q, word):
    k, v = _tensors(C=C)
    with pytest.raises(ValueError, match=word + " is above the kernels' limit"):
        ME.query_attention(torch.randn(B, Q, C), k, v, H)


def test_empty_calls_return_empty_tensors():
    k, v = _tensors(C=8)
    out = ME.query_attention(torch.randn(B, 0, 8), k, v, 2)
    assert tuple(out.shape) == (B, 0, 8) and out.dtype == torch.float32
    cm = ME.CoordinateManager(COORDS[:0])
    e = ME.SparseTensor(torch.randn(0, 8), coordinate_manager=cm)
    out = ME.query_attention(torch.randn(0, 4, 8), e, e, 2)
    assert tuple(out.shape) == (0, 4, 8)
    with pytest.raises(ValueError, match="holds 0 batch indices"):
        ME.query_attention(torch.randn(1, 4, 8), e, e, 2)


def test_backend_without_the_kernels_is_an_error():
    from minsu3d_amd import backend
    from minsu3d_amd.MinkowskiEngine import functional as Fn

    class Bare:
        pass

    backend.set_backend(Bare())                        # (tests/conftest.py restores the backend)
    k, v = _tensors()
    x = torch.randn(V, 8)
    with pytest.raises(NotImplementedError, match=r"needs the HIP backend \(ms3d_qattn_forward\)"):
        Fn.query_attention_rows(torch.randn(B, 4, 8), x, x, None, None, 2, 0.5)
    with pytest.raises(NotImplementedError, match="ms3d_qattn_forward"):
        ME.query_attention(torch.randn(B, 4, 8), k, v, 2)


def test_header_declares_the_symbols():
    text = open(os.path.join(ROOT, "include", "minsu3d_hip.h")).read()
    assert "1 <= D <= 128, H >= 1, H * D <= 1024, 0 <= Q <= 1024, 0 <= B <= 65535" in text
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
    lib.ms3d_qattn_ws_floats.restype = ctypes.c_size_t
    lib.ms3d_qattn_backward_ws_floats.restype = ctypes.c_size_t
    lib.ms3d_qattn_chunks.restype = ctypes.c_long
    return lib


def _chunks_python(lengths, r):
    """the chunk list in plain Python: by sample ascending, then by run ascending"""
    seg, first = [], []
    for b, n in enumerate(lengths):
        first.append(len(seg))
        seg += [b] * (-(-n // r))
    return seg, first + [len(seg)]


def test_chunk_arithmetic():
    lib = _library()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    r = lib.ms3d_qattn_rows_per_chunk()
    assert r >= 1
    for lengths in ([1], [r - 1], [r], [r + 1], [2 * r + 3], [1, r - 1, r, r + 1, 2 * r + 3], [5 * r, 1, 3 * r + 1], []):
        B_ = len(lengths)
        start = [0]
        for n in lengths:
            start.append(start[-1] + n)
        seg_start = (ctypes.c_int * (B_ + 1))(*start)
        want_seg, want_first = _chunks_python(lengths, r)
        n = lib.ms3d_qattn_chunks(seg_start, B_)
        assert n == len(want_seg) == sum(-(-x // r) for x in lengths), lengths
        chunk_seg = (ctypes.c_int * max(n, 1))()
        chunk_first = (ctypes.c_int * (B_ + 1))()
        assert lib.ms3d_qattn_chunk_list(seg_start, B_, chunk_seg, chunk_first) == 0
        assert list(chunk_seg)[:n] == want_seg and list(chunk_first) == want_first, lengths
    assert lib.ms3d_qattn_chunks(None, 3) == 0 and lib.ms3d_qattn_chunks(seg_start, -1) == 0
    assert lib.ms3d_qattn_chunk_list(None, 2, chunk_seg, chunk_first) == E_UNSUPPORTED
    assert lib.ms3d_qattn_chunk_list(seg_start, MAX_B + 1, chunk_seg, chunk_first) == E_UNSUPPORTED


def test_backend_chunk_list_and_the_managers_cache():
    from minsu3d_amd.backend import get_backend
    be = get_backend()
    r = be.qattn_rows_per_chunk()
    lengths = [1, r + 1, 2 * r + 3]
    start = torch.tensor([0, 1, r + 2, 3 * r + 5], dtype=torch.int32)
    seg, first = be.qattn_chunk_list(start)
    want_seg, want_first = _chunks_python(lengths, r)
    assert seg.dtype == first.dtype == torch.int32 and seg.tolist() == want_seg and first.tolist() == want_first
    cm = ME.CoordinateManager(COORDS)
    seg, first, n = cm.batch_chunks(1)
    assert n == B and seg.tolist() == [0, 1, 2] and first.tolist() == [0, 1, 2, 3]
    assert cm.batch_chunks(1) is cm.batch_chunks(1)        # built once per coordinate set
    assert cm.caller_rows(1) is None                       # rows held in the caller's order


def test_workspace_arithmetic():
    lib = _library()
    L = ctypes.c_long
    for chunks in (0, 1, 7, 1000):
        for Q, H, D in ((1, 1, 1), (100, 8, 16), (33, 3, 5), (MAX_Q, 8, MAX_D)):
            assert lib.ms3d_qattn_ws_floats(L(chunks), Q, H, D) == chunks * Q * (H * D + 2 * H), (chunks, Q, H, D)
            assert lib.ms3d_qattn_backward_ws_floats(L(chunks), Q, H, D) == chunks * Q * (2 * H * D + H), (chunks, Q, H, D)
    chunks, Q, H, D = 2 ** 24, MAX_Q, 8, MAX_D             # > 2^32 floats
    assert chunks * Q * (H * D + 2 * H) > 2 ** 32
    assert lib.ms3d_qattn_ws_floats(L(chunks), Q, H, D) == chunks * Q * (H * D + 2 * H)
    assert lib.ms3d_qattn_ws_floats(L(-5), Q, H, D) == 0 and lib.ms3d_qattn_backward_ws_floats(L(3), 0, H, D) == 0
    # the peak-memory test's shape: one sample of 20 000 rows, Q = 256, 8 heads of 8 channels -- the documented partials are
    # under half of one float [V, Q] matrix
    r = lib.ms3d_qattn_rows_per_chunk()
    Vp, Qp = 20000, 256
    assert 4 * lib.ms3d_qattn_backward_ws_floats(L(-(-Vp // r)), Qp, 8, 8) < Vp * Qp * 4 // 2
    assert 4 * lib.ms3d_qattn_ws_floats(L(-(-Vp // r)), Qp, 8, 8) < Vp * Qp * 4 // 2


def test_size_functions_registered_beside_the_others():
    """_lib.lib() gives the size_t functions their return type (a default int would truncate a large workspace)"""
    from minsu3d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    assert _lib.lib().ms3d_qattn_ws_floats.restype is ctypes.c_size_t
    assert _lib.lib().ms3d_qattn_backward_ws_floats.restype is ctypes.c_size_t
    assert _lib.lib().ms3d_qattn_chunks.restype is ctypes.c_long


def _calls(lib):
    """the three entry points with every pointer NULL: (V, B, Q, H, D) -> return code.  The argument checks come before anything
    is launched or dereferenced, so no device is needed."""
    N, f, L, Z = ctypes.c_void_p(0), ctypes.c_float(1.0), ctypes.c_long, ctypes.c_size_t(0)

    def forward(V, B, Q, H, D):
        return lib.ms3d_qattn_forward(N, N, N, N, N, N, N, N, N, L(V), B, 1, Q, H, D, f, N, N, N, Z, N)

    def backward_q(V, B, Q, H, D):
        return lib.ms3d_qattn_backward_q(N, N, N, N, N, N, N, N, N, N, N, N, L(V), B, 1, Q, H, D, f, N, N, N, Z, N)

    def backward_kv(V, B, Q, H, D):
        return lib.ms3d_qattn_backward_kv(N, N, N, N, N, N, N, N, N, N, L(V), B, Q, H, D, f, N, N, N)

    return forward, backward_q, backward_kv


@pytest.mark.parametrize("B_,Q,H,D", [(2, 4, 0, 8), (2, 4, 2, 0), (2, 4, 1, MAX_D + 1), (2, 4, 16, 128), (2, 4, 1025, 1),
                                      (2, MAX_Q + 1, 2, 8), (2, -1, 2, 8), (MAX_B + 1, 4, 2, 8), (-1, 4, 2, 8), (2, 4, -3, 8)])
def test_bad_shapes_are_unsupported_before_any_launch(B_, Q, H, D):
    for call in _calls(_library()):
        assert call(100, B_, Q, H, D) == E_UNSUPPORTED
        assert call(0, B_, Q, H, D) == E_UNSUPPORTED       # the shape is refused whatever the row count
    for call in _calls(_library()):
        assert call(-7, 2, 4, 2, 8) == E_UNSUPPORTED


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
    need = lib.ms3d_qattn_ws_floats(L(chunks), Q, H, D)
    assert need == chunks * Q * (H * D + 2 * H) > 0
    rc = lib.ms3d_qattn_forward(P, P, P, P, P, P, P, P, P, L(V_), B_, chunks, Q, H, D, f, P, P, P, ctypes.c_size_t(need - 1),
                                ctypes.c_void_p(0))
    assert rc == E_WORKSPACE
    need = lib.ms3d_qattn_backward_ws_floats(L(chunks), Q, H, D)
    rc = lib.ms3d_qattn_backward_q(P, P, P, P, P, P, P, P, P, P, P, P, L(V_), B_, chunks, Q, H, D, f, P, P, P,
                                   ctypes.c_size_t(need - 1), ctypes.c_void_p(0))
    assert rc == E_WORKSPACE
