"""Coordinate map keys and layers onto given coordinates: what can be checked without a GPU -- the key itself, the exported
names, the header, and every refusal that is decided before a backend is touched (a stub backend fails the test if it is
reached).  The refusals this feature must NOT lift are restated at the end."""
import os
import re

import pytest
import torch

import minsu3d_amd.MinkowskiEngine as ME

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COORDS = torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0], [0, 2, 2, 0], [1, 0, 0, 2]], dtype=torch.int32)


class Untouchable:
    """a backend no attribute of which may be asked for"""

    def __getattr__(self, name):
        raise AssertionError(f"a refused call must not reach the backend (asked for {name})")


@pytest.fixture
def x():
    from minsu3d_amd import backend
    t = ME.SparseTensor(torch.randn(4, 4), coordinate_manager=ME.CoordinateManager(COORDS))
    backend.set_backend(Untouchable())           # (tests/conftest.py restores the backend)
    return t


def coarse(ts=2):
    c = COORDS.clone()
    c[:, 1:] *= ts
    return ME.SparseTensor(torch.randn(4, 4), coordinate_manager=ME.CoordinateManager.rooted(c, ts), tensor_stride=ts)


# ------------------------------------------------------------------------------------------------ 1. the key
def test_key_equality_hash_repr():
    cm, other = ME.CoordinateManager(COORDS), ME.CoordinateManager(COORDS.clone())
    a, b, c, d = (ME.CoordinateMapKey(cm, 1), ME.CoordinateMapKey(cm, 1), ME.CoordinateMapKey(cm, 2),
                  ME.CoordinateMapKey(other, 1))
    assert a == b and hash(a) == hash(b) and not (a != b)
    assert a != c and a != d and c != d          # another stride; an EQUAL set on another manager object
    assert a != (cm, 1) and a != 1
    assert len({a, b, c, d}) == 3 and {a: "x"}[b] == "x"
    assert a.get_tensor_stride() == [1, 1, 1] and c.get_tensor_stride() == [2, 2, 2]
    assert a.get_coordinate_size() == 4
    assert a.coordinate_manager is cm and c.tensor_stride == 2
    r = repr(c)
    assert r.startswith("CoordinateMapKey(") and "[2, 2, 2]" in r and repr(a) == repr(b) and repr(a) != repr(d)


def test_tensor_key_and_get_coordinates():
    cm = ME.CoordinateManager(COORDS)
    t = ME.SparseTensor(torch.randn(4, 3), coordinate_manager=cm)
    key = t.coordinate_map_key
    assert isinstance(key, ME.CoordinateMapKey) and key == ME.CoordinateMapKey(cm, 1) and key == t.coordinate_map_key
    assert torch.equal(cm.get_coordinates(key), t.C) and torch.equal(cm.get_coordinates(1), t.C)
    with pytest.raises(ValueError, match="another coordinate manager"):
        ME.CoordinateManager(COORDS).get_coordinates(key)
    with pytest.raises(ValueError, match="tensor stride 4"):
        cm.get_coordinates(ME.CoordinateMapKey(cm, 4))
    c2 = coarse(2)
    assert c2.coordinate_map_key.get_tensor_stride() == [2, 2, 2]
    assert torch.equal(c2.coordinate_manager.get_coordinates(c2.coordinate_map_key), c2.C)


def test_constructor_on_a_key_without_a_permutation():
    """(rows held in the caller's order: no backend is needed; the Morton-sorted case runs on the GPU)"""
    cm = ME.CoordinateManager(COORDS)
    t = ME.SparseTensor(torch.randn(4, 3), coordinate_manager=cm)
    f = torch.randn(4, 5, requires_grad=True)
    for z in (ME.SparseTensor(f, coordinate_map_key=t.coordinate_map_key),
              ME.SparseTensor(f, coordinate_map_key=t.coordinate_map_key, coordinate_manager=cm),
              ME.SparseTensor(f, coordinate_map_key=t.coordinate_map_key, tensor_stride=1)):
        assert z.coordinate_manager is cm and z.tensor_stride == 1 and z.F is f and torch.equal(z.C, t.C)
        assert z.coordinate_map_key == t.coordinate_map_key
    c2 = coarse(2)
    z = ME.SparseTensor(torch.ones(4, 2), coordinate_map_key=c2.coordinate_map_key)
    assert z.tensor_stride == 2 and z.coordinate_manager is c2.coordinate_manager and torch.equal(z.C, c2.C)
    # the engine's own form keeps its meaning, default stride included
    assert ME.SparseTensor(f, coordinate_manager=cm).tensor_stride == 1
    assert ME.SparseTensor(torch.ones(4, 2), coordinate_manager=c2.coordinate_manager, tensor_stride=2).tensor_stride == 2
    assert "HELD" in ME.SparseTensor.__init__.__doc__


def test_constructor_refusals(x):
    key, cm = x.coordinate_map_key, x.coordinate_manager
    f = torch.randn(4, 4)
    with pytest.raises(ValueError, match="not the manager of coordinate_map_key"):
        ME.SparseTensor(f, coordinate_map_key=key, coordinate_manager=ME.CoordinateManager(COORDS))
    with pytest.raises(ValueError, match="4 rows"):
        ME.SparseTensor(torch.randn(3, 4), coordinate_map_key=key)
    with pytest.raises(ValueError, match="4 rows"):
        ME.SparseTensor(torch.randn(4), coordinate_map_key=key)
    with pytest.raises(ValueError, match="not both"):
        ME.SparseTensor(f, coordinates=COORDS, coordinate_map_key=key)
    with pytest.raises(ValueError, match="no coordinate set of tensor stride 2"):
        ME.SparseTensor(f, coordinate_map_key=ME.CoordinateMapKey(cm, 2))
    with pytest.raises(ValueError, match="tensor_stride=2 differs"):
        ME.SparseTensor(f, coordinate_map_key=key, tensor_stride=2)
    with pytest.raises(ValueError, match="a CoordinateMapKey"):
        ME.SparseTensor(f, coordinate_map_key=(cm, 1))


# ------------------------------------------------------------------------------------------------ 2. names
def test_new_names_exported():
    assert isinstance(ME.CoordinateMapKey, type)
    assert isinstance(ME.SparseTensor.coordinate_map_key, property)
    for name in ("get_coordinates", "target_map", "expand"):
        assert callable(getattr(ME.CoordinateManager, name)), name
    import minsu3d_amd.dropin.MinkowskiEngine as dropin
    assert dropin.CoordinateMapKey is ME.CoordinateMapKey and "CoordinateMapKey" in dropin.__all__
    for word in ("CoordinateMapKey", "coordinate_map_key", "coordinates=", "expand_coordinates", "ms3d_coords_check"):
        assert word in ME.__doc__, word
    import inspect
    sig = inspect.signature(ME.MinkowskiConvolution.forward).parameters
    assert list(sig)[:3] == ["self", "x", "residual"] and sig["coordinates"].kind is inspect.Parameter.KEYWORD_ONLY
    for cls in (ME.MinkowskiConvolutionTranspose, ME.MinkowskiChannelwiseConvolution, ME.MinkowskiMaxPooling,
                ME.MinkowskiAvgPooling, ME.MinkowskiSumPooling, ME.MinkowskiPoolingTranspose):
        assert list(inspect.signature(cls.forward).parameters)[:3] == ["self", "x", "coordinates"], cls.__name__


def test_header_declares_the_entry_point():
    """(tests/test_abi_cpu.py then proves that the cross-compiled library exports it)"""
    text = open(os.path.join(ROOT, "include", "minsu3d_hip.h")).read()
    assert re.search(r"\bint ms3d_coords_check\s*\(const int \*coords, int V, int lattice, int \*flags", text)
    for name, bit in (("MS3D_COORDS_OUT_OF_RANGE", 1), ("MS3D_COORDS_OFF_LATTICE", 2), ("MS3D_COORDS_REPEATED", 4)):
        assert re.search(rf"#define {name} {bit}\b", text), name


def test_entry_point_refuses_bad_arguments_only():
    """host-side contract of ms3d_coords_check, decided before anything is launched: V == 0 is flags 0 and MS3D_OK, a NULL
    flags pointer, a lattice below 1 and a negative V are MS3D_E_UNSUPPORTED"""
    import ctypes as C
    from minsu3d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    null, flags = C.c_void_p(0), C.c_int(-1)
    call = lambda v, lattice, f: lib.ms3d_coords_check(null, v, lattice, f, null, C.c_size_t(0), null)
    assert call(0, 1, C.byref(flags)) == 0 and flags.value == 0
    flags.value = -1
    assert call(0, 4, C.byref(flags)) == 0 and flags.value == 0
    assert call(0, 0, C.byref(flags)) == _lib.E_UNSUPPORTED
    assert call(-1, 1, C.byref(flags)) == _lib.E_UNSUPPORTED
    assert call(0, 1, null) == _lib.E_UNSUPPORTED
    assert call(5, 1, C.byref(flags)) == _lib.E_UNSUPPORTED          # rows without a coords / workspace pointer


# ------------------------------------------------------------------------------------------------ 3. refusals of the layers
def _target_layers():
    return [("conv", ME.MinkowskiConvolution(4, 8, kernel_size=3, dimension=3), True),
            ("convT", ME.MinkowskiConvolutionTranspose(4, 8, kernel_size=3, stride=1, dimension=3), False),
            ("chconv", ME.MinkowskiChannelwiseConvolution(4, kernel_size=3, dimension=3), False),
            ("max", ME.MinkowskiMaxPooling(3, dimension=3), False), ("avg", ME.MinkowskiAvgPooling(3, dimension=3), False),
            ("sum", ME.MinkowskiSumPooling(3, dimension=3), False),
            ("poolT", ME.MinkowskiPoolingTranspose(3, 1, dimension=3), False)]


def test_bad_targets_are_refused_before_a_backend(x):
    wrong_stride = coarse(2)
    for name, layer, kw_only in _target_layers():
        call = (lambda t: layer(x, coordinates=t))
        for bad in (torch.zeros((3, 3), dtype=torch.int32), torch.zeros((4,), dtype=torch.int64), torch.zeros((3, 4)),
                    torch.zeros((3, 4), dtype=torch.bool), torch.zeros((2, 3, 4), dtype=torch.int32)):
            with pytest.raises(ValueError, match=r"integer tensor \[M, 4\]"):
                call(bad)
        with pytest.raises(TypeError, match="CoordinateMapKey"):
            call([[0, 0, 0, 0]])
        for t in (wrong_stride, wrong_stride.coordinate_map_key):
            with pytest.raises(ValueError, match="tensor stride 2, the layer's output tensor stride is 1"):
                call(t)
        with pytest.raises(ValueError, match="holds no coordinate set of tensor stride 1"):
            call(ME.CoordinateMapKey(wrong_stride.coordinate_manager, 1))
        if not kw_only:          # MinkowskiEngine's second positional argument
            with pytest.raises(ValueError, match="the layer's output tensor stride is 1"):
                layer(x, wrong_stride)


def test_convolution_second_positional_stays_residual(x):
    conv = ME.MinkowskiConvolution(4, 8, kernel_size=3, dimension=3)
    key = x.coordinate_map_key
    with pytest.raises(ValueError, match="residual / skip .* coordinates="):
        conv(x, x, coordinates=key)
    with pytest.raises(ValueError, match="residual / skip .* coordinates="):
        conv(x, skip=("head", ME.SkipLink()), coordinates=key)
    with pytest.raises(TypeError):
        conv(x, None, None, key)                 # keyword only
    exp = ME.MinkowskiConvolution(4, 8, kernel_size=3, dimension=3, expand_coordinates=True)
    with pytest.raises(ValueError, match="residual / skip .* expand_coordinates=True"):
        exp(x, x)


def test_strided_targets_need_the_output_stride(x):
    for layer in (ME.MinkowskiConvolution(4, 8, kernel_size=2, stride=2, dimension=3),
                  ME.MinkowskiSumPooling(2, stride=2, dimension=3),
                  ME.MinkowskiChannelwiseConvolution(4, kernel_size=3, stride=2, dimension=3)):
        with pytest.raises(ValueError, match="tensor stride 1, the layer's output tensor stride is 2"):
            layer(x, coordinates=x)                 # the input's own set is not a stride-2 set
        with pytest.raises(ValueError, match="holds no coordinate set of tensor stride 2"):
            layer(x, coordinates=ME.CoordinateMapKey(x.coordinate_manager, 2))      # never downsampled


def test_transposed_layers_refuse_an_odd_tensor_stride_in_generates_wording(x):
    three = COORDS.clone()
    three[:, 1:] *= 3
    odd = ME.SparseTensor(torch.randn(4, 4), coordinate_manager=ME.CoordinateManager.rooted(three, 3), tensor_stride=3)
    for t, ts in ((x, 1), (odd, 3)):
        for layer in (ME.MinkowskiConvolutionTranspose(4, 8, kernel_size=2, stride=2, dimension=3),
                      ME.MinkowskiPoolingTranspose(2, 2, dimension=3)):
            with pytest.raises(NotImplementedError, match=f"kernel_size=2, stride=2, dilation=1 on tensor stride {ts}: a "
                                                          "generative stride-2 layer needs an even tensor stride"):
                layer(t, COORDS)
    for layer in (ME.MinkowskiConvolutionTranspose(4, 8, kernel_size=2, stride=2, dimension=3, expand_coordinates=True),
                  ME.MinkowskiPoolingTranspose(2, 2, dimension=3, expand_coordinates=True)):
        with pytest.raises(NotImplementedError, match="kernel_size=2, stride=2, dilation=1 on tensor stride 1"):
            layer(x)


def test_expand_coordinates_refusals(x):
    with pytest.raises(NotImplementedError, match=r"stride=2, expand_coordinates=True"):
        ME.MinkowskiConvolution(4, 8, kernel_size=3, stride=2, dimension=3, expand_coordinates=True)
    with pytest.raises(NotImplementedError, match=r"stride=2, expand_coordinates=True"):
        ME.MinkowskiConvolution(4, 8, kernel_size=2, stride=2, dimension=3, expand_coordinates=True)
    for layer in (ME.MinkowskiConvolution(4, 8, kernel_size=3, dimension=3, expand_coordinates=True),
                  ME.MinkowskiConvolutionTranspose(4, 8, kernel_size=3, stride=1, dimension=3, expand_coordinates=True),
                  ME.MinkowskiPoolingTranspose(3, 1, dimension=3, expand_coordinates=True)):
        assert layer.expand_coordinates and "expand_coordinates=True" in repr(layer)
        with pytest.raises(ValueError, match="not both"):
            layer(x, coordinates=x.coordinate_map_key)
    plain = ME.MinkowskiConvolution(4, 8, kernel_size=3, dimension=3)
    assert not plain.expand_coordinates and "expand_coordinates" not in repr(plain)
    assert list(plain.state_dict()) == ["kernel"]


def test_layers_name_the_hip_backend_when_it_lacks_the_entry_points(x):
    from minsu3d_amd import backend

    class Bare:
        pass
    backend.set_backend(Bare())
    target = COORDS[:2].clone()
    with pytest.raises(NotImplementedError, match="HIP backend"):
        ME.MinkowskiConvolution(4, 8, kernel_size=3, dimension=3)(x, coordinates=target)
    with pytest.raises(NotImplementedError, match="HIP backend"):
        ME.MinkowskiConvolution(4, 8, kernel_size=3, dimension=3, expand_coordinates=True)(x)
    with pytest.raises(NotImplementedError, match="HIP backend"):
        ME.MinkowskiSumPooling(3, dimension=3)(x, coordinates=coarse(1).coordinate_map_key)


def test_prepared_weight_image_flag_is_per_module():
    """the mirror flag prepare_conv_weights lays an image out with: static geometry, except where the module was CONSTRUCTED
    with expand_coordinates (its output set is never its input set)"""
    conv = ME.MinkowskiConvolution
    assert conv(4, 8, kernel_size=3, dimension=3)._image_mirror()
    assert conv(4, 8, kernel_size=5, dilation=2, dimension=3)._image_mirror()
    assert not conv(4, 8, kernel_size=3, dimension=3, expand_coordinates=True)._image_mirror()
    assert not conv(4, 8, kernel_size=1, dimension=3)._image_mirror()
    assert not conv(4, 8, kernel_size=3, stride=2, dimension=3)._image_mirror()
    assert not ME.MinkowskiGenerativeConvolutionTranspose(4, 8, kernel_size=3, dimension=3)._image_mirror()
    assert not ME.MinkowskiConvolutionTranspose(4, 8, kernel_size=3, stride=1, dimension=3,
                                                expand_coordinates=True)._image_mirror()
    # a call between two sets never takes a mirrored image: an unstamped alias of the parameter stands in for it
    m = conv(4, 8, kernel_size=3, dimension=3)
    m.kernel._ms3d_wf = ("stamp",)
    alias = m._kernel_two_sets()
    assert alias is not m.kernel and alias.data_ptr() == m.kernel.data_ptr() and not hasattr(alias, "_ms3d_wf")
    s2 = conv(4, 8, kernel_size=3, stride=2, dimension=3)
    assert s2._kernel_two_sets() is s2.kernel


# ------------------------------------------------------------------------------------------------ 4. what stays refused
def test_existing_refusals_unchanged(x):
    for cls in (ME.MinkowskiConvolution, ME.MinkowskiConvolutionTranspose):
        with pytest.raises(NotImplementedError, match="no per-axis tuples"):
            cls(4, 8, kernel_size=(3, 3, 3), dimension=3)
        with pytest.raises(NotImplementedError, match="strides other than 1 and 2"):
            cls(4, 8, kernel_size=3, stride=3, dimension=3)
        with pytest.raises(NotImplementedError, match="an even kernel size needs stride 2"):
            cls(4, 8, kernel_size=2, stride=1, dimension=3)
        with pytest.raises(NotImplementedError, match="dimension=2"):
            cls(4, 8, kernel_size=3, dimension=2)
    with pytest.raises(NotImplementedError, match="dimension=2"):
        ME.MinkowskiPoolingTranspose(2, 2, dimension=2)
    with pytest.raises(NotImplementedError, match="strides other than 1 and 2"):
        ME.MinkowskiMaxPooling(3, stride=4, dimension=3)
    # transposed layers WITHOUT coordinates= and without expand_coordinates on an uncached finer set
    for t in (x, coarse(2)):
        with pytest.raises(NotImplementedError, match="generating new coordinates is not supported"):
            ME.MinkowskiConvolutionTranspose(4, 8, kernel_size=2, stride=2, dimension=3)(t)
        with pytest.raises(NotImplementedError, match="cached finer coordinate set"):
            ME.MinkowskiConvolutionTranspose(4, 8, kernel_size=2, stride=2, dimension=3)(t)
        with pytest.raises(NotImplementedError, match="cached finer coordinate set"):
            ME.MinkowskiPoolingTranspose(2, 2, dimension=3)(t)
    with pytest.raises(NotImplementedError, match="generating new coordinates is not supported"):
        ME.MinkowskiConvolutionTranspose(4, 8, kernel_size=3, stride=1, dimension=3)(x)
    other = ME.SparseTensor(torch.randn(4, 4), coordinate_manager=ME.CoordinateManager(COORDS))
    with pytest.raises(ValueError, match=r"\+= across two coordinate sets"):
        y = ME.SparseTensor(torch.randn(4, 4), coordinate_manager=x.coordinate_manager)
        y += other
    with pytest.raises(NotImplementedError, match="at most 16"):
        ME.MinkowskiUnion()(*[ME.SparseTensor(torch.randn(4, 4), coordinate_manager=ME.CoordinateManager(COORDS))
                              for _ in range(17)])
