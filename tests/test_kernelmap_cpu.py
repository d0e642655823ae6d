"""Kernel, stride and origin maps as index pairs: what can be checked without a GPU -- the header and the library's symbols,
the workspace arithmetic, every refusal the entry points decide on the host (called with null or short arguments: nothing is
launched), the dispatch of CoordinateManager.kernel_map on the type of its first argument, every error that is raised before a
backend is touched (a stub backend fails the test if it is reached), and the yardstick's own self-check."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import minsu3d_amd.MinkowskiEngine as ME
from minsu3d_amd import backend
from kmap_ref import pairs_np, visible_pairs
from region_ref import cube_offsets, dict_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ms3d_kmap_pairs_rows", "ms3d_kmap_pairs_workspace_bytes", "ms3d_kmap_pairs_count", "ms3d_kmap_pairs_fill")
COORDS = torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0], [0, 2, 2, 0], [1, 0, 0, 2], [3, 1, 1, 1]], dtype=torch.int32)
E_WORKSPACE, E_UNSUPPORTED = 10001, 10002


class Untouchable:
    """a backend no attribute of which may be asked for"""

    def __getattr__(self, name):
        raise AssertionError(f"a refused call must not reach the backend (asked for {name})")


def _library():
    from minsu3d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def _tensor(coords=COORDS, ts=1):
    cm = ME.CoordinateManager(coords) if ts == 1 else ME.CoordinateManager.rooted(coords, ts)
    return ME.SparseTensor(torch.randn(coords.size(0), 3), coordinate_manager=cm, tensor_stride=ts)


# ---------------------------------------------------------------- header, library, host arithmetic
def test_header_declares_and_library_exports_the_symbols():
    text = open(os.path.join(ROOT, "include", "minsu3d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ms3d_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(_library().LIB_PATH)
    for s in SYMBOLS:
        assert s in declared and hasattr(lib, s), s


def test_workspace_is_host_arithmetic_and_grows_with_the_table():
    _lib = _library()
    lib = _lib.lib()
    size = lib.ms3d_kmap_pairs_workspace_bytes
    assert size.restype is C.c_size_t
    R = lib.ms3d_kmap_pairs_rows()
    assert R >= 64 and R % 64 == 0
    runs = lambda v: -(-v // R)
    base = size(1, 1)
    assert base >= 4
    for K, V in ((1, R), (1, R + 1), (27, 100000), (254, 100000), (27, 1000000), (65535, 30000)):
        got = size(K, V)
        assert 4 * K * runs(V) + (base - 256) <= got <= 4 * K * runs(V) + base + 256, (K, V, got)
    assert size(27, 100000) < size(254, 100000) < size(254, 1000000)
    assert size(27, 0) == 0 and size(0, 10) == 0 and size(65536, 10) == 0 and size(27, -1) == 0
    assert size(65535, 65535) == 0                          # K * Vout > 2^31 - 1: refused, so nothing to size


def test_entry_points_refuse_on_the_host():
    """every refusal is decided before a pointer is read or anything is launched, so this runs without a GPU: the `device`
    pointers below are host arrays nobody may touch"""
    _lib = _library()
    lib = C.CDLL(_lib.LIB_PATH)
    lib.ms3d_kmap_pairs_workspace_bytes.restype = C.c_size_t
    null, LL, Z = C.c_void_p(0), C.c_longlong, C.c_size_t
    some = C.cast((C.c_int * 16)(), C.c_void_p)              # a non-NULL pointer
    big = Z(1 << 30)

    def count(nbr=some, K=27, vout=100, vin=100, start=some, ws=some, ws_bytes=big):
        return lib.ms3d_kmap_pairs_count(nbr, K, vout, vin, null, start, ws, ws_bytes, null)

    def fill(nbr=some, K=27, vout=100, vin=100, pairs=some, ld=LL(50), ws=some, ws_bytes=big):
        return lib.ms3d_kmap_pairs_fill(nbr, K, vout, vin, null, null, pairs, ld, ws, ws_bytes, null)

    for fn in (count, fill):
        assert fn(K=0) == E_UNSUPPORTED and fn(K=-3) == E_UNSUPPORTED and fn(K=65536) == E_UNSUPPORTED
        assert fn(vout=-1) == E_UNSUPPORTED and fn(vin=-1) == E_UNSUPPORTED
        assert fn(nbr=null) == E_UNSUPPORTED
        assert fn(K=65535, vout=65535) == E_UNSUPPORTED      # K * Vout > 2^31 - 1
        assert fn(K=2, vout=2 ** 30) == E_UNSUPPORTED
        need = lib.ms3d_kmap_pairs_workspace_bytes(27, 100)
        assert need > 0
        assert fn(ws_bytes=Z(need - 1)) == E_WORKSPACE and fn(ws_bytes=Z(0)) == E_WORKSPACE and fn(ws=null) == E_WORKSPACE
        assert fn(vout=0) == 0 and fn(vout=0, nbr=null, ws=null, ws_bytes=Z(0)) == 0      # nothing to do: nothing is read
    assert count(start=null) == E_UNSUPPORTED and count(start=null, vout=0) == E_UNSUPPORTED
    assert fill(pairs=null) == E_UNSUPPORTED and fill(ld=LL(-1)) == E_UNSUPPORTED
    assert fill(ld=LL(0)) == 0 and fill(ld=LL(0), pairs=null) == 0                         # P == 0: nothing is written


def test_hip_backend_has_the_binding_and_refuses_cpu_tensors(monkeypatch):
    from minsu3d_amd import _lib
    _library()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    hb = backend.HipBackend()
    with pytest.raises(_lib.HipLibraryError):
        hb.kmap_pairs(torch.full((27, 5), -1, dtype=torch.int32), 27, 5, 5)


# ---------------------------------------------------------------- the yardstick checks itself
def test_pairs_np_agrees_with_nonzero():
    rng = np.random.default_rng(3)
    K, vout, vin = 5, 37, 29
    nbr = np.where(rng.random((K, vout)) < 0.4, rng.integers(0, vin, (K, vout)), -1).astype(np.int32)
    nbr[2] = -1                                              # an offset without a pair between two that have some
    pairs, start = pairs_np(nbr)
    kk, oo = np.nonzero(nbr >= 0)                            # row-major: k ascending, then o ascending
    assert np.array_equal(pairs[1], oo) and np.array_equal(pairs[0], nbr[kk, oo])
    assert np.array_equal(start, np.concatenate([[0], np.cumsum((nbr >= 0).sum(1))]))
    assert start[2] == start[3] and pairs.dtype == np.int64 and start.dtype == np.int32
    # renamed: the visible table is nbr[:, out_order] with its entries sent through in_rename
    out_order, in_rename = rng.permutation(vout), rng.permutation(vin)
    pairs2, start2 = pairs_np(nbr, out_order, in_rename)
    vis = nbr[:, out_order]
    kk, oo = np.nonzero(vis >= 0)
    assert np.array_equal(pairs2[1], oo) and np.array_equal(pairs2[0], in_rename[vis[kk, oo]]) and np.array_equal(start2, start)
    # an entry >= vin counts as -1
    pairs3, start3 = pairs_np(nbr, vin=10)
    assert np.array_equal(pairs3[0], nbr[(nbr >= 0) & (nbr < 10)]) and start3[-1] == ((nbr >= 0) & (nbr < 10)).sum()
    empty, s0 = pairs_np(np.full((3, 4), -1))
    assert empty.shape == (2, 0) and s0.tolist() == [0, 0, 0, 0]


def test_visible_pairs_is_the_coordinate_equation():
    c = COORDS.numpy()
    offs = cube_offsets(3, 1, 1)
    fwd = visible_pairs(c, c, offs)
    assert sorted(fwd) == list(fwd) and 13 in fwd and np.array_equal(fwd[13], np.stack([np.arange(5), np.arange(5)]))
    for k, p in fwd.items():
        assert np.array_equal(c[p[1]][:, 1:] + offs[k], c[p[0]][:, 1:]) and np.array_equal(c[p[1]][:, 0], c[p[0]][:, 0])
    tr = visible_pairs(c, c, offs, transposed=True)
    for k, p in tr.items():
        assert np.array_equal(c[p[1]][:, 1:] - offs[k], c[p[0]][:, 1:])


# ---------------------------------------------------------------- the dispatch of kernel_map
class K3Backend:
    """the one table the engine form below asks for, from the dictionary map"""

    def kmap_k3(self, coords, ts):
        c = coords.numpy()
        return torch.from_numpy(dict_map(c, c, cube_offsets(3, 1, ts)))


def test_engine_form_goes_through_the_dispatch_unchanged():
    backend.set_backend(K3Backend())                         # (tests/conftest.py restores the backend)
    cm = ME.CoordinateManager(COORDS)
    km = cm.kernel_map(1, 3)
    assert isinstance(km, tuple) and len(km) == 7
    nbr_fwd, nbr_bwd, vin, vout, K, out_ts, mirror = km
    assert nbr_bwd is nbr_fwd and (vin, vout, K, out_ts, mirror) == (5, 5, 27, 1, True) and nbr_fwd is cm.k3(1)
    assert np.array_equal(nbr_fwd.numpy(), dict_map(COORDS.numpy(), COORDS.numpy(), cube_offsets(3, 1, 1)))
    assert cm.kernel_map(1, 3, 1, 1, region=None) is not None and cm.kernel_map(1, kernel_size=3)[0] is nbr_fwd
    assert cm.kernel_map_tables(1, 3)[0] is nbr_fwd
    ident = cm.kernel_map(1, 1)
    assert len(ident) == 7 and ident[4] == 1 and ident[0].view(-1).tolist() == [0, 1, 2, 3, 4]
    with pytest.raises(NotImplementedError, match="strides other than 1 and 2"):
        cm.kernel_map(1, 3, 3)


def test_key_form_needs_the_hip_backend():
    class Bare:
        pass
    x = _tensor()
    key = x.coordinate_map_key
    for be in (Bare(), None):                                # a backend without the kernel; the HIP backend on CPU tensors
        backend.set_backend(be)
        if be is None:
            _library()
        for call in (lambda: x.coordinate_manager.kernel_map(key, key), lambda: x.coordinate_manager.kernel_map(x, x, kernel_size=3),
                     lambda: x.coordinate_manager.kernel_map_pairs(key, key, kernel_size=5)):
            with pytest.raises(NotImplementedError, match=r"needs the HIP backend \(ms3d_kmap_pairs"):
                call()


def test_value_errors_come_before_any_backend_call():
    x = _tensor()
    c2 = COORDS.clone()
    c2[:, 1:] *= 2
    y2 = _tensor(c2, ts=2)                                   # a stride-2 set on another manager
    cm, key = x.coordinate_manager, x.coordinate_map_key
    backend.set_backend(Untouchable())
    for fn in (cm.kernel_map, cm.kernel_map_pairs):
        # the keys' strides contradict `stride`
        with pytest.raises(ValueError, match="contradict stride=2"):
            fn(key, key, stride=2, kernel_size=2)
        with pytest.raises(ValueError, match="contradict stride=1"):
            fn(x, y2)
        with pytest.raises(ValueError, match="contradict stride=2 of a transposed map"):
            fn(x, y2, stride=2, kernel_size=2, is_transpose=True)
        # a key's manager holds no such set
        with pytest.raises(ValueError, match="in_key's manager holds no coordinate set of tensor stride 4"):
            fn(ME.CoordinateMapKey(cm, 4), key)
        with pytest.raises(ValueError, match="out_key's manager holds no coordinate set of tensor stride 2"):
            fn(key, ME.CoordinateMapKey(cm, 2), stride=2, kernel_size=2)
        # a generator beside contradicting arguments
        g = ME.KernelGenerator(3, 1, 2, dimension=3)
        with pytest.raises(ValueError, match="kernel_size=5 contradicts kernel_generator"):
            fn(key, key, kernel_size=5, kernel_generator=g)
        with pytest.raises(ValueError, match="stride=2 contradicts kernel_generator"):
            fn(key, key, stride=2, kernel_generator=g)
        with pytest.raises(ValueError, match="is_transpose=True contradicts kernel_generator"):
            fn(key, key, is_transpose=True, kernel_generator=g)
        with pytest.raises(ValueError, match="region_type=.*HYPER_CROSS.* contradicts kernel_generator"):
            fn(key, key, region_type=ME.RegionType.HYPER_CROSS, kernel_generator=g)
        with pytest.raises(ValueError, match="region_offsets contradicts kernel_generator"):
            fn(key, key, region_offsets=torch.tensor([[1, 0, 0]]), kernel_generator=g)
        # the geometry refusals are the existing ones
        with pytest.raises(NotImplementedError, match="strides other than 1 and 2"):
            fn(key, key, stride=3)
        with pytest.raises(NotImplementedError, match="an even kernel size needs stride 2"):
            fn(key, key, kernel_size=2)
        with pytest.raises(NotImplementedError, match="at most 254 kernel offsets"):
            fn(key, key, kernel_size=7)
        with pytest.raises(TypeError, match="out_key: a CoordinateMapKey or a SparseTensor"):
            fn(key, 1)


def test_stride_and_stride_map_errors_and_origin_map():
    x = _tensor()
    other = _tensor(COORDS.clone())
    cm, key = x.coordinate_manager, x.coordinate_map_key
    backend.set_backend(Untouchable())
    assert cm.stride(key, 1) is key and cm.stride(x, 1) == key
    for bad in (3, 6, 0, -2, 2.0, (2, 2, 2)):
        with pytest.raises(NotImplementedError, match="strides other than 1 and 2") as e:
            cm.stride(key, bad)
        assert repr(bad) in str(e.value)
    with pytest.raises(ValueError, match="holds no coordinate set of tensor stride 8"):
        cm.stride(ME.CoordinateMapKey(cm, 8), 2)
    with pytest.raises(ValueError, match="different coordinate managers"):
        cm.stride_map(key, ME.CoordinateMapKey(other.coordinate_manager, 2))
    for fine, coarse_ts in ((1, 1), (2, 1), (1, 3), (1, 6), (4, 2)):
        with pytest.raises(ValueError, match="COARSER"):
            cm.stride_map(ME.CoordinateMapKey(cm, fine), ME.CoordinateMapKey(cm, coarse_ts))
    # origin_map is plain torch over batch_rows: batch indices 0, 0, 0, 1, 3 -> ranks 0, 0, 0, 1, 2
    om = cm.origin_map(key)
    assert list(om) == [0] and om[0].dtype == torch.int64 and om[0].tolist() == [[0, 1, 2, 3, 4], [0, 0, 0, 1, 2]]
    assert cm.origin_map(x) is om
    with pytest.raises(ValueError, match="holds no coordinate set of tensor stride 2"):
        cm.origin_map(ME.CoordinateMapKey(cm, 2))


def test_words():
    for word in ("kernel_map(in_key, out_key", "kernel_map_pairs", "stride_map", "origin_map", "ms3d_kmap_pairs_count",
                 "ms3d_kmap_pairs_fill", "not pinned", "is_pool"):
        assert word in ME.__doc__, word
    assert "Kernel, stride and origin maps" in ME.__doc__.split("Not supported")[0]
    assert "int64" in ME.CoordinateManager.kernel_map.__doc__ and "not pinned" in ME.CoordinateManager.kernel_map.__doc__
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert s in integration, s
    assert "kmap_pairs" in open(os.path.join(ROOT, "DESIGN.md")).read()
