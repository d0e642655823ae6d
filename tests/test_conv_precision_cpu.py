"""CPU: the matmul-precision surface of the sparse convolutions (torch.set_float32_matmul_precision) -- the string ->
C ABI code mapping, the host-only geometry queries of the *_p entry points (include/minsu3d_hip.h) and the host
extension's signatures.  No GPU needed: the library loads and its geometry functions run on the host."""
import ctypes as C

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from minsu3d_amd import _lib
    L = _lib.lib()
    L.ms3d_spconv_wgrad_ws_floats.restype = C.c_size_t
    L.ms3d_spconv_wgrad_ws_floats_p.restype = C.c_size_t
    return L


def test_precision_string_maps_to_code():
    from minsu3d_amd.MinkowskiEngine import functional as Fn
    assert [Fn.precision_code(s) for s in ("highest", "high", "medium")] == [0, 1, 2]
    with pytest.raises(ValueError):
        Fn.precision_code("low")
    prev = torch.get_float32_matmul_precision()

    class Be:
        matmul_precision_aware = True
    try:
        for s, want in (("highest", 0), ("high", 1), ("medium", 2)):
            torch.set_float32_matmul_precision(s)
            assert Fn.conv_precision(Be()) == want
            assert Fn.conv_precision(object()) == 0          # a backend without bf16 kernels always runs exact
        with Fn.pass_precision(1):                           # a model forward's value beats the switch ...
            torch.set_float32_matmul_precision("medium")
            assert Fn.conv_precision(Be()) == 1
        assert Fn.conv_precision(Be()) == 2                  # ... for that pass only
    finally:
        torch.set_float32_matmul_precision(prev)


def test_geometry_functions_reject_bad_precision(lib):
    bad = 10002                                              # MS3D_E_UNSUPPORTED
    for p in (3, -1):
        assert lib.ms3d_spconv_aux_kind_p(27, 64, 64, p) == bad
        assert lib.ms3d_spconv_wgrad_pieces(200000, 27, 64, 64, 0, p) == bad
        assert lib.ms3d_spconv_wgrad_ws_floats_p(200000, 27, 64, 64, p) == 0


def test_aux_kind_and_pieces_per_precision(lib):
    # wide layers: bf16 image of 3 / 2 / 1 pieces; narrow / K = 1 layers: the precision-0 kind at every precision
    assert [lib.ms3d_spconv_aux_kind_p(27, 64, 64, p) for p in (0, 1, 2)] == [2, 3, 4]
    assert [lib.ms3d_spconv_aux_kind_p(8, 96, 48, p) for p in (0, 1, 2)] == [2, 3, 4]
    for K, ci, co in ((27, 16, 16), (27, 32, 32), (1, 64, 64), (8, 32, 64), (27, 32, 64), (27, 320, 160)):
        k0 = lib.ms3d_spconv_aux_kind(K, ci, co)
        assert k0 not in (2, 3, 4)
        assert [lib.ms3d_spconv_aux_kind_p(K, ci, co, p) for p in (0, 1, 2)] == [k0] * 3
    assert lib.ms3d_spconv_aux_kind_p(27, 64, 64, 0) == lib.ms3d_spconv_aux_kind(27, 64, 64)
    # backward-weight: the wide K = 27 layers with enough rows take the bf16 kernel, everything else the f32 kernels
    for V, K, ci, co, ol in ((200000, 27, 64, 64, 0), (50000, 27, 128, 128, 0), (200000, 27, 96, 96, 0)):
        assert lib.ms3d_spconv_wgrad_is_bf16x3(V, K, ci, co, ol) == 1
        assert [lib.ms3d_spconv_wgrad_pieces(V, K, ci, co, ol, p) for p in (0, 1, 2)] == [3, 2, 1]
    for V, K, ci, co, ol in ((200000, 27, 32, 32, 0), (2500, 27, 80, 80, 0), (200000, 8, 64, 64, 0), (200000, 27, 64, 64, 1)):
        assert lib.ms3d_spconv_wgrad_is_bf16x3(V, K, ci, co, ol) == 0
        assert [lib.ms3d_spconv_wgrad_pieces(V, K, ci, co, ol, p) for p in (0, 1, 2)] == [0, 0, 0]


def test_wgrad_workspace_upper_bound(lib):
    """fewer pieces need less workspace: the precision-0 size (what every caller allocates, and what
    ms3d_spconv_layer_ws_floats contains) bounds every precision"""
    shapes = [(V, K, ci, co) for V in (1, 31, 2500, 11700, 29999, 30000, 31000, 32000, 32512, 32513, 50000, 196000, 420000)
              for K, ci, co in ((27, 48, 48), (27, 64, 64), (27, 64, 128), (27, 96, 48), (27, 128, 128), (27, 256, 256),
                                (27, 16, 16), (8, 64, 96), (1, 16, 20))]
    n_bf = 0
    for V, K, ci, co in shapes:
        w0 = lib.ms3d_spconv_wgrad_ws_floats(V, K, ci, co)
        assert lib.ms3d_spconv_wgrad_ws_floats_p(V, K, ci, co, 0) == w0
        w1, w2 = (lib.ms3d_spconv_wgrad_ws_floats_p(V, K, ci, co, p) for p in (1, 2))
        assert 0 < w2 <= w1 <= w0, (V, K, ci, co)
        if lib.ms3d_spconv_wgrad_is_bf16x3(V, K, ci, co, 0):
            n_bf += 1
            assert w2 < w1 < w0
    assert n_bf >= 20


def test_host_extension_takes_precision():
    from minsu3d_amd import backend
    ext = backend._load_host_ext()
    if ext is None:
        pytest.skip("host extension not built")
    for name, n_args in (("conv_layer_forward", 20), ("conv_layer_backward", 30), ("res_block_forward", 24)):
        doc = getattr(ext, name).__doc__
        assert "Overloaded function" in doc, name
        assert f"arg{n_args - 1}:" in doc, (name, doc)         # the form with the trailing precision argument ...
        assert doc.count(f"arg{n_args - 2}:") == 2 and f"arg{n_args}:" not in doc    # ... beside the one without


def test_backend_signatures_take_precision():
    import inspect
    from minsu3d_amd.backend import HipBackend
    for name in ("conv_layer_forward", "conv_layer_backward", "res_block_forward", "prep_weights_multi",
                 "conv_backward_weight"):
        sig = inspect.signature(getattr(HipBackend, name))
        assert sig.parameters["precision"].default == 0, name
