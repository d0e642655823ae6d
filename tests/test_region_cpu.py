"""Kernel regions (RegionType, KernelGenerator, `kernel_generator=`): what can be checked without a GPU -- the exported names,
the offset rules against their restatement (tests/region_ref.py), the constructors of every layer that takes a generator,
the refusals, that a HYPER_CUBE generator IS the plain layer (a recording backend: k3 is asked for, never kmap_region), the
header and the host-decided contracts of ms3d_kmap_region, and the error a backend without the entry point gives."""
import math
import os
import re

import numpy as np
import pytest
import torch

import minsu3d_amd.MinkowskiEngine as ME
from region_ref import cross_offsets, cube_offsets, custom_offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COORDS = torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0], [0, 2, 2, 0], [1, 0, 0, 2]], dtype=torch.int32)
RT = ME.RegionType
MIXED = [(0, 0, 0), (1, 0, 0), (0, 2, -1), (-1, 0, 0), (3, 3, 3)]


def cross(ks=3, **kw):
    return ME.KernelGenerator(ks, region_type=RT.HYPER_CROSS, dimension=3, **kw)


def custom(rows=MIXED, **kw):
    return ME.KernelGenerator(region_type=RT.CUSTOM, region_offsets=torch.tensor(rows, dtype=torch.int32), dimension=3, **kw)


# ------------------------------------------------------------------------------------------------ 1. names
def test_names_exported():
    import enum
    import minsu3d_amd.dropin.MinkowskiEngine as dropin
    assert issubclass(RT, enum.Enum)
    assert [(m.name, m.value) for m in RT] == [("HYPER_CUBE", 0), ("HYPER_CROSS", 1), ("CUSTOM", 2)]
    for name in ("RegionType", "KernelGenerator"):
        assert getattr(dropin, name) is getattr(ME, name) and name in dropin.__all__, name
    for word in ("RegionType", "KernelGenerator", "kernel_generator=", "HYPER_CROSS", "CUSTOM", "ms3d_kmap_region", "axis_types",
                 "not pinned"):
        assert word in ME.__doc__, word
    import inspect
    args = list(inspect.signature(ME.KernelGenerator.__init__).parameters)[1:]
    assert args == ["kernel_size", "stride", "dilation", "is_transpose", "region_type", "region_offsets", "expand_coordinates",
                    "axis_types", "dimension"]
    for cls in (ME.MinkowskiConvolution, ME.MinkowskiConvolutionTranspose, ME.MinkowskiGenerativeConvolutionTranspose,
                ME.MinkowskiChannelwiseConvolution, ME.MinkowskiMaxPooling, ME.MinkowskiAvgPooling, ME.MinkowskiSumPooling,
                ME.MinkowskiPoolingTranspose):
        assert list(inspect.signature(cls.__init__).parameters)[-1] == "kernel_generator", cls.__name__      # appended
    for name in ("kernel_map", "kernel_map_inverse", "target_map", "generate", "expand"):
        p = inspect.signature(getattr(ME.CoordinateManager, name)).parameters
        assert list(p)[-1] == "region" and p["region"].default is None, name


# ------------------------------------------------------------------------------------------------ 2. offsets
@pytest.mark.parametrize("ts", [1, 2, 4])
@pytest.mark.parametrize("dil", [1, 2, 3])
@pytest.mark.parametrize("ks", [1, 3, 5, 7])
def test_cross_offsets(ks, dil, ts):
    g = cross(ks, dilation=dil)
    got = g.offsets(ts)
    assert got.dtype == np.int32 and got.shape == (3 * (ks - 1) + 1, 3) and g.kernel_volume == got.shape[0]
    assert np.array_equal(got, cross_offsets(ks, dil, ts))
    assert (g.kernel_size, g.stride, g.dilation, g.region_type, g.region_offsets, g.dimension) == (ks, 1, dil, RT.HYPER_CROSS,
                                                                                               None, 3)
    if ks == 1:
        assert np.array_equal(got, cube_offsets(1, dil, ts))


@pytest.mark.parametrize("ts", [1, 2, 4])
def test_custom_and_cube_offsets(ts):
    for rows in (MIXED, [(1, 0, 0)], [(-1, 0, 0), (0, 0, 0), (1, 0, 0)], (cube_offsets(3, 1, 1) + [1, 0, 0]).tolist()):
        for form in (torch.tensor(rows, dtype=torch.int32), torch.tensor(rows, dtype=torch.int64), np.array(rows), rows):
            g = ME.KernelGenerator(kernel_size=9, region_type=RT.CUSTOM, region_offsets=form)
            assert np.array_equal(g.offsets(ts), custom_offsets(rows, ts)) and g.offsets(ts).dtype == np.int32
            assert g.kernel_volume == len(rows)
            assert g.region_offsets.dtype == torch.int32 and g.region_offsets.device.type == "cpu"
            assert g.region_offsets.tolist() == [list(r) for r in rows]
    for ks, dil in ((3, 1), (3, 2), (5, 1), (1, 1)):
        g = ME.KernelGenerator(ks, 1, dil, dimension=3)
        assert np.array_equal(g.offsets(ts), cube_offsets(ks, dil, ts)) and g.kernel_volume == ks ** 3
        assert np.array_equal(g.offsets(ts), ME.kernel_offsets(ks, dil, ts))
    g = ME.KernelGenerator(2, 2)
    assert np.array_equal(g.offsets(ts), cube_offsets(2, 1, ts)) and g.kernel_volume == 8 and g.region_type is RT.HYPER_CUBE


def test_generator_is_hashable_by_value():
    a, b = cross(3), cross(3)
    assert a == b and hash(a) == hash(b) and not (a != b) and len({a, b}) == 1
    assert a != cross(5) and a != cross(3, dilation=2) and a != cross(3, stride=2) and a != ME.KernelGenerator(3)
    assert custom() == custom() and hash(custom()) == hash(custom())
    assert custom() != custom(MIXED[::-1]) and custom() != custom(MIXED[:4])         # the order is part of the value
    assert custom(stride=2) != custom() and cross(3, expand_coordinates=True) != a and cross(3, is_transpose=True) != a
    assert {a: 1}[b] == 1 and a != "cross"
    assert "HYPER_CROSS" in repr(a) and "kernel_volume=7" in repr(a)
    assert a.expand_coordinates is False and a.is_transpose is False
    assert cross(3, expand_coordinates=True).expand_coordinates is True


# ------------------------------------------------------------------------------------------------ 3. constructors
CONVS = (ME.MinkowskiConvolution, ME.MinkowskiConvolutionTranspose, ME.MinkowskiGenerativeConvolutionTranspose)
POOLS = (ME.MinkowskiMaxPooling, ME.MinkowskiAvgPooling, ME.MinkowskiSumPooling)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("which", ["cross3", "cross5d2", "custom", "single"])
def test_layer_constructors(which, stride):
    g = {"cross3": lambda: cross(3, stride=stride), "cross5d2": lambda: cross(5, stride=stride, dilation=2),
         "custom": lambda: custom(stride=stride), "single": lambda: custom([(1, 0, 0)], stride=stride)}[which]()
    K = {"cross3": 7, "cross5d2": 13, "custom": 5, "single": 1}[which]
    assert g.kernel_volume == K
    cin, cout = 6, 10
    for cls in CONVS:
        torch.manual_seed(0)
        m = cls(cin, cout, kernel_generator=g, bias=True, dimension=3)
        assert tuple(m.kernel.shape) == (K, cin, cout) and tuple(m.bias.shape) == (1, cout), cls.__name__
        assert sorted(m.state_dict()) == ["bias", "kernel"]
        bound = 1.0 / math.sqrt(cin * K)
        assert float(m.kernel.detach().abs().max()) <= bound and float(m.bias.detach().abs().max()) <= bound
        big = cls(64, 64, kernel_generator=g, dimension=3)
        assert float(big.kernel.detach().abs().max()) > 0.9 / math.sqrt(64 * K) and big.bias is None
        assert (m.kernel_size, m.stride, m.dilation, m.kernel_volume) == (g.kernel_size, stride, g.dilation, K)
        assert m.region == g.region_key and m.region is not None and not m._image_mirror()
        assert g.region_type.name in m.extra_repr() and g.region_type.name in repr(m)
        assert sorted(cls(cin, cout, kernel_generator=g, dimension=3).state_dict()) == ["kernel"]
    m = ME.MinkowskiChannelwiseConvolution(cin, kernel_generator=g, bias=True, dimension=3)
    assert tuple(m.kernel.shape) == (K, cin) and tuple(m.bias.shape) == (1, cin) and sorted(m.state_dict()) == ["bias", "kernel"]
    assert float(m.kernel.detach().abs().max()) <= 1.0 / math.sqrt(cin * K) and m.kernel_volume == K and m.stride == stride
    assert g.region_type.name in m.extra_repr()
    ks = g.kernel_size if g.region_type is RT.HYPER_CROSS else 3
    for cls in POOLS:
        m = cls(ks, kernel_generator=g, dimension=3)
        assert (m.stride, m.dilation, m.region, m.kernel_volume) == (stride, g.dilation, g.region_key, K), cls.__name__
        assert g.region_type.name in m.extra_repr() and not list(m.state_dict())
    m = ME.MinkowskiPoolingTranspose(ks, stride, kernel_generator=g, dimension=3)
    assert (m.stride, m.dilation, m.region) == (stride, g.dilation, g.region_key) and g.region_type.name in m.extra_repr()


def test_expand_coordinates_is_layer_argument_or_generator_attribute():
    assert ME.MinkowskiConvolution(4, 4, kernel_generator=cross(3, expand_coordinates=True), dimension=3).expand_coordinates
    assert ME.MinkowskiConvolution(4, 4, kernel_generator=cross(3), expand_coordinates=True, dimension=3).expand_coordinates
    assert not ME.MinkowskiConvolution(4, 4, kernel_generator=cross(3), dimension=3).expand_coordinates
    assert ME.MinkowskiPoolingTranspose(3, 1, kernel_generator=cross(3, expand_coordinates=True)).expand_coordinates
    assert ME.MinkowskiConvolutionTranspose(4, 4, kernel_generator=ME.KernelGenerator(2, 2, expand_coordinates=True),
                                            dimension=3).expand_coordinates


# ------------------------------------------------------------------------------------------------ 4. a cube generator
class Recorder:
    """a backend that records which table builders are asked for; every table is a marker tensor"""
    weight_token = None

    def __init__(self, names):
        self.calls = []
        self._names = names

    def __getattr__(self, name):
        if name.startswith("__") or name not in self._names:
            raise AttributeError(name)

        def call(*a, **k):
            self.calls.append(name)
            if name == "kmap_region":
                return torch.zeros(1, dtype=torch.int32), torch.ones(1, dtype=torch.int32)
            return torch.zeros(1, dtype=torch.int32)
        return call


@pytest.mark.parametrize("geom", [(3, 1, 1), (2, 2, 1), (5, 1, 1), (1, 1, 1), (3, 2, 2), (3, 1, 2)])
def test_cube_generator_builds_the_plain_layer(geom):
    ks, stride, dil = geom
    g = ME.KernelGenerator(ks, stride, dil, region_type=RT.HYPER_CUBE, dimension=3)
    assert g.region_key is None
    layers = [(ME.MinkowskiConvolution, (5, 7)), (ME.MinkowskiConvolutionTranspose, (5, 7)),
              (ME.MinkowskiGenerativeConvolutionTranspose, (5, 7)), (ME.MinkowskiChannelwiseConvolution, (5,))]
    for cls, ch in layers:
        torch.manual_seed(3)
        a = cls(*ch, kernel_size=ks, stride=stride, dilation=dil, bias=True, dimension=3)
        torch.manual_seed(3)
        b = cls(*ch, kernel_generator=g, bias=True, dimension=3)
        torch.manual_seed(3)
        c = cls(*ch, kernel_size=ks, stride=stride, dilation=dil, kernel_generator=g, bias=True, dimension=3)
        for m in (b, c):
            assert torch.equal(a.kernel, m.kernel) and torch.equal(a.bias, m.bias), cls.__name__
            for attr in ("kernel_size", "stride", "dilation", "kernel_volume", "region"):
                assert getattr(a, attr) == getattr(m, attr), (cls.__name__, attr)
            assert a.extra_repr() == m.extra_repr() and m.region is None
            if hasattr(a, "_image_mirror"):
                assert a._image_mirror() == m._image_mirror() and a.expand_coordinates == m.expand_coordinates
    for cls in POOLS + (ME.MinkowskiPoolingTranspose,):
        a, b = cls(ks, stride, dil, dimension=3), cls(ks, stride, kernel_generator=g, dimension=3)
        assert (a.kernel_size, a.stride, a.dilation, a.region) == (b.kernel_size, b.stride, b.dilation, b.region) == (ks, stride,
                                                                                                                  dil, None)


def test_cube_generator_takes_the_k3_route_and_a_cross_the_region_entry():
    from minsu3d_amd import backend
    rec = Recorder({"kmap_k3", "kmap_region", "kmap_general", "kmap_invert"})
    backend.set_backend(rec)                     # (tests/conftest.py restores the backend)
    cm = ME.CoordinateManager(COORDS)
    conv = ME.MinkowskiConvolution(4, 4, kernel_generator=ME.KernelGenerator(3, dimension=3), dimension=3)
    spec, out_ts = conv._spec(cm, 1)
    assert rec.calls == ["kmap_k3"] and out_ts == 1 and spec.K == 27 and spec.mirror and spec.sub is None
    assert spec.nbr_fwd is cm.k3(1) and cm.kernel_map(1, 3, 1, 1)[0] is cm.k3(1)
    # the cross: one call of kmap_region gives both tables; mirror = False, sub = False
    del rec.calls[:]
    cr = ME.MinkowskiConvolution(4, 4, kernel_generator=cross(3), dimension=3)
    spec, out_ts = cr._spec(cm, 1)
    assert rec.calls == ["kmap_region"] and (spec.K, spec.mirror, spec.sub, out_ts) == (7, False, False, 1)
    assert spec.nbr_fwd is not spec.nbr_bwd
    km = cm.kernel_map(1, 3, 1, 1, region=cross(3))
    assert km[0] is spec.nbr_fwd and km[1] is spec.nbr_bwd and km[2:] == (4, 4, 7, 1, False) and rec.calls == ["kmap_region"]
    assert cm.kernel_map(1, 3, 1, 1, region=cross(3).region_key)[0] is spec.nbr_fwd            # the key names the same entry
    assert cm.kernel_map_inverse(1, 3, 1, 1, region=cross(3)) is spec.nbr_bwd and rec.calls == ["kmap_region"]
    # a CUSTOM list of 27 offsets and one of a single offset are two-set layers as well
    shifted = custom((cube_offsets(3, 1, 1) + [1, 0, 0]).tolist())
    for g, K in ((shifted, 27), (custom([(1, 0, 0)]), 1)):
        spec, _ = ME.MinkowskiConvolution(4, 4, kernel_generator=g, dimension=3)._spec(cm, 1)
        assert (spec.K, spec.mirror, spec.sub) == (K, False, False)
    assert "kmap_k3" not in rec.calls


def test_backend_without_the_entry_point():
    from minsu3d_amd import backend
    backend.set_backend(Recorder({"kmap_k3", "kmap_general", "kmap_invert"}))
    cm = ME.CoordinateManager(COORDS)
    with pytest.raises(NotImplementedError, match=r"needs the HIP backend \(ms3d_kmap_region\)"):
        cm.kernel_map(1, 3, 1, 1, region=cross(3))
    x = ME.SparseTensor(torch.randn(4, 4), coordinate_manager=cm)
    with pytest.raises(NotImplementedError, match="ms3d_kmap_region"):
        ME.MinkowskiConvolution(4, 4, kernel_generator=custom(), dimension=3)(x)
    with pytest.raises(NotImplementedError, match="ms3d_kmap_region"):
        ME.MinkowskiMaxPooling(3, kernel_generator=cross(3), dimension=3)(x)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_generator_refusals():
    KG = ME.KernelGenerator
    with pytest.raises(NotImplementedError, match="axis_types"):
        KG(3, axis_types=[0, 0, 0])
    for d in (2, 4, 0):
        with pytest.raises(NotImplementedError, match=f"dimension={d}"):
            KG(3, dimension=d)
    assert KG(3, dimension=-1).dimension == 3 and KG(3, dimension=3).dimension == 3
    for kw in (dict(kernel_size=(3, 3, 3)), dict(kernel_size=3, stride=(1, 1, 1)), dict(kernel_size=3, dilation=(1, 1, 1)),
               dict(kernel_size=(3, 3, 3), region_type=RT.HYPER_CROSS), dict(kernel_size=3, stride=[2, 2, 2],
                                                                            region_type=RT.HYPER_CROSS),
               dict(stride=(1, 1, 1), region_type=RT.CUSTOM, region_offsets=MIXED)):
        with pytest.raises(NotImplementedError, match="no per-axis tuples"):
            KG(**kw)
    for ks in (2, 4, 6):
        with pytest.raises(ValueError, match="odd kernel size"):
            KG(ks, region_type=RT.HYPER_CROSS)
        with pytest.raises(ValueError, match="odd kernel size"):
            KG(ks, stride=2, region_type=RT.HYPER_CROSS)
    for kw in (dict(kernel_size=3, stride=3), dict(kernel_size=3, stride=3, region_type=RT.HYPER_CROSS),
               dict(stride=4, region_type=RT.CUSTOM, region_offsets=MIXED)):
        with pytest.raises(NotImplementedError, match="strides other than 1 and 2"):
            KG(**kw)
    with pytest.raises(NotImplementedError, match="at most 254"):
        KG(7)                                                                     # 343 cube offsets
    with pytest.raises(NotImplementedError, match="at most 254"):
        KG(87, region_type=RT.HYPER_CROSS)                                       # 6 * 43 + 1 = 259
    assert KG(85, region_type=RT.HYPER_CROSS).kernel_volume == 253
    rows255 = [(i, 0, 0) for i in range(255)]
    with pytest.raises(NotImplementedError, match="at most 254"):
        KG(region_type=RT.CUSTOM, region_offsets=rows255)
    assert KG(region_type=RT.CUSTOM, region_offsets=rows255[:254]).kernel_volume == 254
    with pytest.raises(NotImplementedError, match="even kernel size needs stride 2"):
        KG(2)
    with pytest.raises(ValueError, match="distinct"):
        KG(region_type=RT.CUSTOM, region_offsets=[(0, 0, 0), (1, 0, 0), (0, 0, 0)])
    with pytest.raises(ValueError, match="dilation must be 1"):
        KG(dilation=2, region_type=RT.CUSTOM, region_offsets=MIXED)
    with pytest.raises(ValueError, match="needs region_offsets"):
        KG(3, region_type=RT.CUSTOM)
    for bad in (torch.zeros(3, 2, dtype=torch.int32), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(3, 3), [1, 2, 3]):
        with pytest.raises(ValueError, match=r"\[K, 3\]"):
            KG(region_type=RT.CUSTOM, region_offsets=bad)
    with pytest.raises(ValueError, match="CUSTOM"):
        KG(3, region_offsets=MIXED)


def test_layer_refusals():
    g = cross(3)
    for kw in (dict(kernel_size=5), dict(stride=2), dict(dilation=2)):
        with pytest.raises(ValueError, match="contradicts the kernel_generator"):
            ME.MinkowskiConvolution(4, 4, kernel_generator=g, dimension=3, **kw)
        with pytest.raises(ValueError, match="contradicts the kernel_generator"):
            ME.MinkowskiChannelwiseConvolution(4, kernel_generator=g, dimension=3, **kw)
    with pytest.raises(ValueError, match="kernel_size=5 contradicts"):
        ME.MinkowskiMaxPooling(5, kernel_generator=g)
    with pytest.raises(ValueError, match="stride=2 contradicts"):
        ME.MinkowskiPoolingTranspose(3, 2, kernel_generator=g)
    with pytest.raises(ValueError, match="kernel_size=3 contradicts"):
        ME.MinkowskiConvolutionTranspose(4, 4, kernel_size=3, kernel_generator=ME.KernelGenerator(2, 2), dimension=3)
    # what agrees with the generator, and the ignored kernel size of a CUSTOM region, pass
    ME.MinkowskiConvolution(4, 4, kernel_size=3, stride=1, dilation=1, kernel_generator=g, dimension=3)
    ME.MinkowskiConvolution(4, 4, kernel_size=3, kernel_generator=custom(), dimension=3)
    with pytest.raises(TypeError, match="KernelGenerator"):
        ME.MinkowskiConvolution(4, 4, kernel_generator=RT.HYPER_CROSS, dimension=3)
    # the refusals that exist, when the geometry arrives through a generator
    with pytest.raises(NotImplementedError, match="no per-axis tuples"):
        ME.MinkowskiConvolution(4, 4, kernel_generator=ME.KernelGenerator((3, 3, 3)), dimension=3)
    with pytest.raises(NotImplementedError, match="strides other than 1 and 2"):
        ME.MinkowskiConvolution(4, 4, kernel_generator=ME.KernelGenerator(3, stride=3), dimension=3)
    with pytest.raises(NotImplementedError, match="dimension=2"):
        ME.MinkowskiConvolution(4, 4, kernel_generator=ME.KernelGenerator(3, dimension=2), dimension=3)
    with pytest.raises(NotImplementedError, match="dimension=2"):
        ME.MinkowskiConvolution(4, 4, kernel_generator=g, dimension=2)
    for gen in (ME.KernelGenerator(3, 2, expand_coordinates=True), cross(3, stride=2, expand_coordinates=True),
                custom(stride=2, expand_coordinates=True)):
        with pytest.raises(NotImplementedError, match="expand_coordinates is supported at stride 1 only"):
            ME.MinkowskiConvolution(4, 4, kernel_generator=gen, dimension=3)
    with pytest.raises(NotImplementedError, match="expand_coordinates is supported at stride 1 only"):
        ME.MinkowskiConvolution(4, 4, kernel_generator=cross(3, stride=2), expand_coordinates=True, dimension=3)


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"a refused call must not reach the backend (asked for {name})")


def test_residual_and_skip_are_refused_on_region_layers():
    from minsu3d_amd import backend
    cm = ME.CoordinateManager(COORDS)
    x = ME.SparseTensor(torch.randn(4, 4), coordinate_manager=cm)
    backend.set_backend(Untouchable())
    for g in (cross(3), custom()):
        conv = ME.MinkowskiConvolution(4, 4, kernel_generator=g, dimension=3)
        with pytest.raises(ValueError, match="residual / skip"):
            conv(x, x)
        with pytest.raises(ValueError, match="residual / skip"):
            conv(x, skip=("head", None))
    with pytest.raises(NotImplementedError, match="strides other than 1 and 2"):
        cm.kernel_map(1, 3, 3, 1, region=cross(3))


# ------------------------------------------------------------------------------------------------ 6. the entry point
def test_header_declares_the_entry_point():
    """(tests/test_abi_cpu.py then proves that the cross-compiled library exports it)"""
    text = open(os.path.join(ROOT, "include", "minsu3d_hip.h")).read()
    assert re.search(r"\bint ms3d_kmap_region\s*\(const int \*coords, int V, const int \*offsets[^,]*,\s*const int \*partner[^,]*, "
                     r"int K,\s*int \*nbr_fwd[^,]*, int \*nbr_inv[^,]*, void \*workspace, size_t workspace_bytes,\s*"
                     r"ms3d_stream_t stream\);", text)
    assert "DISTINCT rows only" in text


def test_entry_point_contracts_decided_on_the_host():
    """K outside 1 .. 254 and a partner list that is not an involution are MS3D_E_UNSUPPORTED, a short workspace is
    MS3D_E_WORKSPACE, V == 0 with valid arguments returns 0: all with V = 0 and NULL device pointers, so no device is touched"""
    import ctypes as C
    from minsu3d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    lib.ms3d_coord_workspace_bytes.restype = C.c_size_t
    null, ws = C.c_void_p(0), lib.ms3d_coord_workspace_bytes(0)

    def call(partner, K=None, bytes_=ws):
        arr = (C.c_int * max(len(partner), 1))(*partner)
        return lib.ms3d_kmap_region(null, 0, null, arr, len(partner) if K is None else K, null, null, null, C.c_size_t(bytes_),
                                    null)
    cross3 = [0, 2, 1, 4, 3, 6, 5]
    assert call(cross3) == 0
    assert call([0]) == 0 and call([-1]) == 0 and call([-1, 3, -1, 1, 4]) == 0
    assert call(list(range(253, -1, -1))) == 0                                     # K = 254, fully partnered
    assert call([0], K=0) == _lib.E_UNSUPPORTED and call([0], K=-1) == _lib.E_UNSUPPORTED
    assert call([-1] * 255) == _lib.E_UNSUPPORTED                                 # K = 255
    assert call([1, 2, 0]) == _lib.E_UNSUPPORTED                                  # a cycle, not an involution
    assert call([1, -1]) == _lib.E_UNSUPPORTED                                    # partner[partner[0]] != 0
    assert call([0, 7]) == _lib.E_UNSUPPORTED and call([0, -2]) == _lib.E_UNSUPPORTED     # out of range
    assert call(cross3, bytes_=ws - 1) == 10001                                   # MS3D_E_WORKSPACE
    assert lib.ms3d_kmap_region(null, 0, null, null, 7, null, null, null, C.c_size_t(ws), null) == _lib.E_UNSUPPORTED
