"""SparseTensor + coordinate manager.

A SparseTensor is (features [V, C], coordinate manager, tensor stride).  Row order of the input coordinates is
preserved (the reference indexes the U-Net output with the dataset's voxel_point_map, backbone.py:40).

BatchNorm / ReLU are LAZY: `MinkowskiBatchNorm` computes the batch statistics with a HIP reduction and returns
a tensor that only records (scale, shift[, relu]); the following convolution applies them while gathering its
input rows, so `Sequential(BN, ReLU, Conv)` is one gather kernel and never materialises the normalised
activations.  Touching `.features` of such a tensor materialises it (one elementwise kernel).
"""
import enum
import functools
import os

import numpy as np
import torch

from ..backend import BatchGroup, NeighbourGroup, get_backend
from . import functional as Fn


def kernel_offsets(kernel_size, dilation=1, tensor_stride=1):
    """int32 [kernel_size^3, 3] (x, y, z) offsets of a kernel in voxel units, in the order the weights are indexed:
    k = ix + ks * iy + ks^2 * iz (x fastest).  Odd sizes are centred, (i - (ks - 1) / 2) * dilation * tensor_stride (the
    3x3x3 table's order); even sizes reach forward from the output coordinate, i * dilation * tensor_stride (the in-cell
    offsets of the k2 s2 table)."""
    ks = int(kernel_size)
    i = np.arange(ks) - ((ks - 1) // 2 if ks % 2 else 0)
    iz, iy, ix = np.meshgrid(i, i, i, indexing="ij")
    return (np.stack([ix, iy, iz], -1).reshape(-1, 3) * (int(dilation) * int(tensor_stride))).astype(np.int32)


def check_geometry(kernel_size, stride, dilation):
    """the (kernel size, stride, dilation) triples the engine builds kernel maps for; anything else raises
    NotImplementedError naming the geometry (at construction of a layer and again in kernel_map)"""
    geom = f"kernel_size={kernel_size}, stride={stride}, dilation={dilation}"
    if not all(isinstance(v, int) for v in (kernel_size, stride, dilation)) or kernel_size < 1 or dilation < 1:
        raise NotImplementedError(f"{geom}: one positive integer per argument (no per-axis tuples)")
    if stride not in (1, 2):
        raise NotImplementedError(f"{geom}: strides other than 1 and 2 are not supported")
    if stride == 1 and kernel_size % 2 == 0:
        raise NotImplementedError(f"{geom}: an even kernel size needs stride 2 (MinkowskiEngine refuses it as well)")
    if kernel_size ** 3 > 254:
        raise NotImplementedError(f"{geom}: at most 254 kernel offsets (kernel_size <= 6)")


class RegionType(enum.Enum):
    """the shape of a kernel: every cell of the cube, the axes through its centre, or a list the caller writes"""
    HYPER_CUBE = 0
    HYPER_CROSS = 1
    CUSTOM = 2


def region_offsets(region, tensor_stride=1):
    """int32 [K, 3] (x, y, z) offsets in voxel units, in weight order, of a region key (KernelGenerator.region_key):
    ("HYPER_CROSS", kernel_size, dilation): the centre first, then axis x at -h .. -1, +1 .. +h, then y, then z (h =
    (kernel_size - 1) // 2, K = 6 h + 1), each times dilation * tensor_stride; ("CUSTOM", rows): the rows in the order given,
    times tensor_stride."""
    if region[0] == "CUSTOM":
        return (np.asarray(region[1], dtype=np.int64).reshape(-1, 3) * int(tensor_stride)).astype(np.int32)
    _, kernel_size, dilation = region
    h = (kernel_size - 1) // 2
    steps = [s for s in range(-h, h + 1) if s != 0]
    rows = [(0, 0, 0)]
    for axis in range(3):
        rows += [tuple(s if a == axis else 0 for a in range(3)) for s in steps]
    return (np.asarray(rows, dtype=np.int64).reshape(-1, 3) * (int(dilation) * int(tensor_stride))).astype(np.int32)


def _region_key(region):
    """a layer's `region` argument (None, a KernelGenerator or a region key) -> None for a cube, else the hashable key"""
    if isinstance(region, KernelGenerator):
        return region.region_key
    return region


class KernelGenerator:
    """MinkowskiEngine's kernel generator: the geometry of a convolution or pooling layer as one object, handed to the layers
    as `kernel_generator=`.  Attributes: kernel_size, stride, dilation (plain ints), region_type, region_offsets (int32 CPU
    tensor [K, 3] for CUSTOM, else None), kernel_volume, expand_coordinates, is_transpose, dimension (3).  Hashable by value.
    `offsets(tensor_stride)` -> np.int32 [K, 3] in voxel units, in weight order (an engine extra):

      HYPER_CUBE   kernel_offsets(kernel_size, dilation, ts); K = kernel_size ** 3.  The plain layer: a layer handed such a
                   generator is the layer its plain arguments build.
      HYPER_CROSS  odd kernel sizes; see region_offsets.  Kernel size 1 is the cube of size 1.
      CUSTOM       region_offsets: an integer tensor or array [K, 3], 1 <= K <= 254, distinct rows (ValueError), used in the
                   order given and multiplied by the tensor stride only: dilation must be 1 (ValueError), kernel_size is
                   ignored.

    Refused at construction: axis_types, dimension other than -1 / 3, per-axis tuples, strides other than 1 and 2, more than
    254 offsets (NotImplementedError); an even cross (ValueError).  These rules are chosen here, MinkowskiEngine's as
    recalled, not pinned (see the package docstring)."""

    def __init__(self, kernel_size=-1, stride=1, dilation=1, is_transpose=False, region_type=RegionType.HYPER_CUBE,
                 region_offsets=None, expand_coordinates=False, axis_types=None, dimension=-1):
        if axis_types is not None:
            raise NotImplementedError(f"axis_types={axis_types!r}: per-axis region types are not supported")
        if isinstance(dimension, bool) or dimension not in (-1, 3):
            raise NotImplementedError(f"dimension={dimension}: only 3-D sparse tensors are supported")
        if not isinstance(region_type, RegionType):
            raise TypeError(f"region_type: a RegionType, got {region_type!r}")
        geom = f"kernel_size={kernel_size}, stride={stride}, dilation={dilation}"
        offs = None
        if region_type is RegionType.HYPER_CUBE:
            check_geometry(kernel_size, stride, dilation)
            K = kernel_size ** 3
        else:
            sized = (stride, dilation) if region_type is RegionType.CUSTOM else (kernel_size, stride, dilation)
            if not all(isinstance(v, int) for v in sized) or min(sized) < 1:
                raise NotImplementedError(f"{geom}: one positive integer per argument (no per-axis tuples)")
            if stride not in (1, 2):
                raise NotImplementedError(f"{geom}: strides other than 1 and 2 are not supported")
            if region_type is RegionType.HYPER_CROSS:
                if kernel_size % 2 == 0:
                    raise ValueError(f"{geom}: a HYPER_CROSS region needs an odd kernel size")
                K = 3 * (kernel_size - 1) + 1
            else:
                if region_offsets is None:
                    raise ValueError("region_type=CUSTOM needs region_offsets: an integer tensor or array [K, 3]")
                if dilation != 1:
                    raise ValueError(f"{geom}: a CUSTOM region carries its offsets as written; dilation must be 1")
                offs = region_offsets.detach().cpu().numpy() if torch.is_tensor(region_offsets) else np.asarray(region_offsets)
                if offs.ndim != 2 or offs.shape[1] != 3 or offs.shape[0] < 1 or offs.dtype.kind not in "iu":
                    raise ValueError(f"region_offsets: an integer tensor or array [K, 3] with K >= 1, got "
                                     f"{list(offs.shape)} {offs.dtype}")
                K = offs.shape[0]
                if not isinstance(kernel_size, int):
                    kernel_size = -1
            if K > 254:
                raise NotImplementedError(f"{geom}: a region of {K} offsets: at most 254 kernel offsets")
            if offs is not None:
                offs = np.ascontiguousarray(offs.astype(np.int32))
                if len({tuple(r) for r in offs.tolist()}) != K:
                    raise ValueError("region_offsets: the rows must be distinct (an offset occurs twice)")
        if region_offsets is not None and region_type is not RegionType.CUSTOM:
            raise ValueError(f"region_offsets needs region_type=RegionType.CUSTOM, got {region_type}")
        self.kernel_size, self.stride, self.dilation = kernel_size, stride, dilation
        self.is_transpose, self.expand_coordinates = bool(is_transpose), bool(expand_coordinates)
        self.region_type, self.dimension, self.axis_types = region_type, 3, None
        self.region_offsets = None if offs is None else torch.from_numpy(offs.copy())
        self.kernel_volume = K
        if region_type is RegionType.HYPER_CUBE or (region_type is RegionType.HYPER_CROSS and kernel_size == 1):
            self.region_key = None                      # a cube: the layers and the coordinate manager never see a region
        elif region_type is RegionType.HYPER_CROSS:
            self.region_key = ("HYPER_CROSS", kernel_size, dilation)
        else:
            self.region_key = ("CUSTOM", tuple(tuple(r) for r in offs.tolist()))

    def offsets(self, tensor_stride=1):
        """np.int32 [kernel_volume, 3]: the offsets in voxel units at that tensor stride, in weight order"""
        if self.region_key is None:
            return kernel_offsets(self.kernel_size, self.dilation, tensor_stride)
        return region_offsets(self.region_key, tensor_stride)

    def _value(self):
        return (self.region_type, self.kernel_size, self.stride, self.dilation, self.is_transpose, self.expand_coordinates,
                self.region_key)

    def __eq__(self, other):
        return isinstance(other, KernelGenerator) and other._value() == self._value()

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self._value())

    def __repr__(self):
        return (f"KernelGenerator(kernel_size={self.kernel_size}, stride={self.stride}, dilation={self.dilation}, "
                f"region_type={self.region_type}, kernel_volume={self.kernel_volume}"
                + (", is_transpose=True" if self.is_transpose else "")
                + (", expand_coordinates=True" if self.expand_coordinates else "") + ")")


class CoordinateMapKey:
    """The name of ONE coordinate set: a coordinate manager plus a tensor stride -- the pair `+`, `cat`, `slice` and `union`
    compare already.  Hashable; two keys are equal when the manager is the same object and the stride is equal.  What
    `SparseTensor.coordinate_map_key` returns, what `SparseTensor(features, coordinate_map_key=...)` and the `coordinates=`
    argument of the layers take."""
    __slots__ = ("coordinate_manager", "tensor_stride")

    def __init__(self, coordinate_manager, tensor_stride):
        self.coordinate_manager, self.tensor_stride = coordinate_manager, tensor_stride

    def __eq__(self, other):
        return (isinstance(other, CoordinateMapKey) and other.coordinate_manager is self.coordinate_manager
                and other.tensor_stride == self.tensor_stride)

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash((id(self.coordinate_manager), self.tensor_stride))

    def get_tensor_stride(self):
        return [self.tensor_stride] * 3

    def get_coordinate_size(self):
        return 4

    def __repr__(self):
        return (f"CoordinateMapKey(tensor_stride={self.get_tensor_stride()}, coordinate_size=4, "
                f"manager=0x{id(self.coordinate_manager):x})")


_COORDS_FLAG_REASONS = ((1, "a row lies outside the packable range: a coordinate outside [-16384, 16384) or a batch index outside "
                            "[0, 524288)"),
                        (2, "a coordinate is not a multiple of the output tensor stride {ts}"),
                        (4, "a coordinate occurs twice (the rows of an output set are distinct)"))
_TARGET_SETS = {}     # (id of a coordinate tensor, output tensor stride, device) -> (rooted manager, the tensor, its version)


def _target_rows(coordinates):
    """the [M, 4] integer tensor a layer's `coordinates=` may be (checked before anything touches a backend)"""
    if coordinates.dim() != 2 or coordinates.size(1) != 4 or coordinates.is_floating_point() or coordinates.is_complex() \
            or coordinates.dtype == torch.bool:
        raise ValueError(f"coordinates=: an integer tensor [M, 4] (b, x, y, z), a CoordinateMapKey or a SparseTensor, got a "
                         f"tensor {list(coordinates.shape)} {coordinates.dtype}")


def target_key(coordinates, out_ts, device):
    """The coordinate set a layer was told to write onto (`coordinates=`) -> its CoordinateMapKey.
    A CoordinateMapKey (or a SparseTensor: its key) names a set some manager holds; its stride must be the layer's output
    stride `out_ts` (ValueError otherwise), nothing else is checked.  An integer tensor [M, 4] of (b, x, y, z), any integer
    dtype, any device, is moved to `device` as int32 and becomes the only set of a manager rooted at out_ts that holds the rows
    in the given order; it is validated ONCE by ms3d_coords_check (backend.coords_check), every raised bit a ValueError naming
    it -- nothing is clipped, merged or dropped.  The manager is kept per tensor OBJECT and version (the four newest, with the
    tensor): two layers handed the same tensor land on the same manager, an in-place edit makes a new one."""
    if isinstance(coordinates, SparseTensor):
        coordinates = coordinates.coordinate_map_key
    if isinstance(coordinates, CoordinateMapKey):
        if coordinates.tensor_stride != out_ts:
            raise ValueError(f"coordinates=: the target set has tensor stride {coordinates.tensor_stride}, the layer's output "
                             f"tensor stride is {out_ts}")
        if coordinates.tensor_stride not in coordinates.coordinate_manager.coords:
            raise ValueError(f"coordinates=: the key's manager holds no coordinate set of tensor stride {out_ts}")
        return coordinates
    if not torch.is_tensor(coordinates):
        raise TypeError(f"coordinates=: an integer tensor [M, 4], a CoordinateMapKey or a SparseTensor, got "
                        f"{type(coordinates).__name__}")
    _target_rows(coordinates)
    ident = (id(coordinates), out_ts, str(device))
    hit = _TARGET_SETS.get(ident)
    if hit is None or hit[1] is not coordinates or hit[2] != coordinates._version:
        be = get_backend()
        if not hasattr(be, "coords_check"):
            raise NotImplementedError("a layer onto given coordinates needs the HIP backend (ms3d_coords_check)")
        rows = coordinates.detach().to(device=device, dtype=torch.int32).contiguous()
        if rows.numel() > 0 and rows.data_ptr() == coordinates.data_ptr():
            rows = rows.clone()          # the set must not follow a later in-place edit of the caller's tensor
        flags = be.coords_check(rows, out_ts)
        for bit, reason in _COORDS_FLAG_REASONS:
            if flags & bit:
                raise ValueError("coordinates=: " + reason.format(ts=out_ts))
        _TARGET_SETS.pop(ident, None)
        hit = _TARGET_SETS[ident] = (CoordinateManager.rooted(rows, out_ts), coordinates, coordinates._version)
        while len(_TARGET_SETS) > 4:
            _TARGET_SETS.pop(next(iter(_TARGET_SETS)))
    return CoordinateMapKey(hit[0], out_ts)


def _as_key(what, name):
    """a CoordinateMapKey, or a SparseTensor (its key) -> the CoordinateMapKey"""
    if isinstance(what, SparseTensor):
        return what.coordinate_map_key
    if not isinstance(what, CoordinateMapKey):
        raise TypeError(f"{name}: a CoordinateMapKey or a SparseTensor, got {type(what).__name__}")
    return what


def _check_region_geometry(kernel_size, stride, dilation, region):
    """check_geometry for a cube; a region (validated when its KernelGenerator was built) only has its stride checked"""
    if region is None:
        check_geometry(kernel_size, stride, dilation)
    elif stride not in (1, 2):
        raise NotImplementedError(f"region={region}, stride={stride}: strides other than 1 and 2 are not supported")


def _offsets_of(kernel_size, dilation, tensor_stride, region):
    """the offset list of a layer: kernel_offsets of a cube, region_offsets of a region key"""
    if region is None:
        return kernel_offsets(kernel_size, dilation, tensor_stride)
    return region_offsets(region, tensor_stride)


class CoordinateManager:
    """coordinates per tensor stride and kernel maps per (stride, kind), built once and shared by every
    convolution of a level and by the backward pass (ME's coordinate manager does the same caching)."""

    def __init__(self, coordinates, spatial_sort=False):
        assert coordinates.dtype == torch.int32 and coordinates.size(1) == 4
        # Engine-internal row order: voxels sorted by (batch, Morton code) so that the rows a convolution gathers
        # for neighbouring outputs are neighbours in HBM / the same XCD's L2.  `perm` maps internal row -> caller
        # row, `inv` the other way; callers never see the internal order (SparseTensor.features un-permutes).
        self.perm = self.inv = None
        if spatial_sort:
            perm = get_backend().spatial_order(coordinates.contiguous())
            if perm is not None:
                self.perm = perm
                self.inv = torch.empty_like(perm)
                self.inv[perm] = torch.arange(perm.numel(), device=perm.device)
                self.coords_external = coordinates
                coordinates = coordinates[perm]
        self.coords = {1: coordinates.contiguous()}
        self._k3 = {}
        self._k2 = {}       # fine stride -> (nbr_down [8,Vc], nbr_up [8,Vf])
        self._ident = {}
        self._kmaps = {}    # (ts, kernel_size, stride, dilation) -> kernel_map() tuple of the general geometries
        self._kinv = {}     # the same key -> inverse table (pooling backward over a submanifold map)
        self._batch_groups = {}     # ts -> BatchGroup: the rows grouped by batch index, what every per-sample op reads

    @classmethod
    def rooted(cls, coordinates, tensor_stride):
        """a manager whose FIRST coordinate set lives at `tensor_stride` (a generated or pruned set: nothing finer exists
        below it).  No Morton permutation -- the rows stay in the order they were made in, which is the order callers see.
        k3 / k2 / identity / kernel_map / kernel_map_inverse / batch_rows work from that stride upward."""
        assert coordinates.dtype == torch.int32 and coordinates.dim() == 2 and coordinates.size(1) == 4
        cm = cls.__new__(cls)
        cm.perm = cm.inv = None
        cm.root = int(tensor_stride)
        cm.coords = {cm.root: coordinates.contiguous()}
        cm._k3, cm._k2, cm._ident, cm._kmaps, cm._kinv, cm._batch_groups = {}, {}, {}, {}, {}, {}
        return cm

    def generate(self, ts, kernel_size, stride=1, dilation=1, region=None):
        """what a generative transposed convolution from tensor stride ts needs -> (manager rooted at ts // stride on the
        generated set, nbr_fwd [K, Vout], nbr_bwd [K, Vin], Vin, Vout, K, output tensor stride); built once per (ts, kernel
        size, stride, dilation), so two layers of one geometry on one input share the output manager.  The set is every
        c + offsets[k] over the input rows c and kernel_offsets(kernel_size, dilation, ts // stride), in first-occurrence
        order (backend.coords_expand); nbr_fwd[k][o] = input row at out[o] - offsets[k], nbr_bwd its inverse.  region (a
        non-cube KernelGenerator or its key): its offsets at ts // stride instead, part of the cache key."""
        kernel_size, stride, dilation, region = int(kernel_size), int(stride), int(dilation), _region_key(region)
        _check_region_geometry(kernel_size, stride, dilation, region)
        geom = f"kernel_size={kernel_size}, stride={stride}, dilation={dilation}" + (f", region={region}" if region else "")
        if ts % stride != 0:
            raise NotImplementedError(f"{geom} on tensor stride {ts}: a generative stride-2 layer needs an even tensor stride")
        cache = self.__dict__.setdefault("_generated", {})
        key = (ts, kernel_size, stride, dilation) if region is None else (ts, stride, region)
        gen = cache.get(key)
        if gen is None:
            be = get_backend()
            if not (hasattr(be, "coords_expand") and hasattr(be, "kmap_general")):
                raise NotImplementedError(f"{geom}: generating coordinates needs the HIP backend (ms3d_coords_expand)")
            out_ts = ts // stride
            offsets = _offsets_of(kernel_size, dilation, out_ts, region)
            cin = self.coords[ts]
            vin, K = cin.size(0), offsets.shape[0]
            # first occurrence counts in the order of the rows the CALLER sees (x.coordinates): on a Morton-sorted manager
            # the set is expanded from the external rows, the tables below are built over the engine's
            ext = self.coords_external if (ts == 1 and self.perm is not None) else cin
            out = be.coords_expand(ext, torch.from_numpy(offsets))
            vout = out.size(0)
            nbr_fwd = be.kmap_general(cin, out, torch.from_numpy(-offsets))
            nbr_bwd = be.kmap_invert(nbr_fwd, K, vout, vin)
            gen = cache[key] = (CoordinateManager.rooted(out, out_ts), nbr_fwd, nbr_bwd, vin, vout, K, out_ts)
        return gen

    def get_coordinates(self, key):
        """the rows of the coordinate set `key` names (a CoordinateMapKey of this manager, or a tensor stride) in the order the
        CALLER sees them: visible_coords"""
        if isinstance(key, CoordinateMapKey):
            if key.coordinate_manager is not self:
                raise ValueError("get_coordinates: the key names a set of another coordinate manager")
            key = key.tensor_stride
        if key not in self.coords:
            raise ValueError(f"get_coordinates: this manager holds no coordinate set of tensor stride {key}")
        return self.visible_coords(key)

    def target_map(self, ts, key, kernel_size, stride=1, dilation=1, transposed=False, region=None):
        """the kernel map of a layer from this manager's set of tensor stride ts ONTO the set `key` names (any manager) ->
        (nbr_fwd [K, Vout], nbr_bwd [K, Vin], Vin, Vout, K).  Both sets are taken as their managers HOLD them (a Morton-sorted
        stride-1 set through coords[1], not coords_external), like every table.  Forward layers (convolution, pooling,
        channel-wise): nbr_fwd[k][o] = input row at target[o] + kernel_offsets(kernel_size, dilation, ts)[k].  Transposed layers
        (transposed convolution, pooling transpose): nbr_fwd[k][o] = input row at target[o] - kernel_offsets(kernel_size,
        dilation, key's stride)[k] -- y[o] = sum_k x[o - off_k] W[k], the rule of generate().  nbr_bwd is the inverse table
        (the target's rows are distinct).  A target row no input reaches is a column of -1.  Built once per (ts, key, geometry,
        direction) and kept on this manager with the key (the sixteen newest).  region (a non-cube KernelGenerator or its
        key): its offsets at the same tensor stride and with the same sign, part of the cache key."""
        kernel_size, stride, dilation, region = int(kernel_size), int(stride), int(dilation), _region_key(region)
        cache = self.__dict__.setdefault("_target_maps", {})
        ident = (ts, key, kernel_size, stride, dilation, bool(transposed))
        if region is not None:
            ident = (ts, key, stride, region, bool(transposed))
        hit = cache.get(ident)
        if hit is None:
            _check_region_geometry(kernel_size, stride, dilation, region)
            be = get_backend()
            if not (hasattr(be, "kmap_general") and hasattr(be, "kmap_invert")):
                raise NotImplementedError("a layer onto given coordinates needs the HIP backend (ms3d_kmap_general)")
            out_ts = key.tensor_stride
            offsets = _offsets_of(kernel_size, dilation, out_ts if transposed else ts, region)
            if transposed:
                offsets = -offsets
            cin, out = self.coords[ts], key.coordinate_manager.coords[out_ts]
            vin, vout, K = cin.size(0), out.size(0), offsets.shape[0]
            nbr_fwd = be.kmap_general(cin, out, torch.from_numpy(offsets))
            hit = cache[ident] = (nbr_fwd, be.kmap_invert(nbr_fwd, K, vout, vin), vin, vout, K)
            while len(cache) > 16:
                cache.pop(next(iter(cache)))
        return hit

    def expand(self, ts, kernel_size, dilation=1, region=None):
        """what a stride-1 convolution with expand_coordinates=True needs -> (manager rooted at ts on every coordinate the
        kernel reaches, nbr_fwd [K, Vout], nbr_bwd [K, Vin], Vin, Vout, K): the set is every c - kernel_offsets(kernel_size,
        dilation, ts)[k] over the rows c the CALLER sees, in first-occurrence order (backend.coords_expand, as generate()), the
        tables are target_map's.  Built once per (ts, kernel size, dilation); region (a non-cube KernelGenerator or its key):
        its offsets instead, part of the cache key."""
        kernel_size, dilation, region = int(kernel_size), int(dilation), _region_key(region)
        _check_region_geometry(kernel_size, 1, dilation, region)
        cache = self.__dict__.setdefault("_expanded", {})
        ident = (ts, kernel_size, dilation) if region is None else (ts, region)
        hit = cache.get(ident)
        if hit is None:
            be = get_backend()
            if not (hasattr(be, "coords_expand") and hasattr(be, "kmap_general")):
                raise NotImplementedError(f"kernel_size={kernel_size}, dilation={dilation}: expand_coordinates needs the HIP "
                                          "backend (ms3d_coords_expand)")
            out = be.coords_expand(self.visible_coords(ts), torch.from_numpy(-_offsets_of(kernel_size, dilation, ts, region)))
            out_cm = CoordinateManager.rooted(out, ts)
            hit = cache[ident] = (out_cm,) + self.target_map(ts, CoordinateMapKey(out_cm, ts), kernel_size, 1, dilation,
                                                             region=region)
        return hit

    def visible_coords(self, ts):
        """the coordinates of tensor stride ts in the order the CALLER sees them (x.coordinates)"""
        if ts == 1 and self.inv is not None:
            return self.coords_external
        return self.coords[ts]

    def union(self, ts, others):
        """the union of this manager's coordinate set of tensor stride ts with the sets of the same stride of the managers
        `others` (at most 15) -> (manager rooted at ts on the union set, in_rows int32 [N, n]: union row -> row of operand i or
        -1, out_rows: per operand int32 [V_i] row -> union row, n); operand 0 is this manager.  The set is in first-occurrence
        order of the rows the caller sees (x.coordinates): this set's rows, then the rows of others[0] it lacks, and so on
        (backend.coords_union).  The maps name rows as the operands HOLD them: on a Morton-sorted manager at stride 1 the
        engine's permutation is composed into them, so the feature kernels gather straight from the held rows.  Built once per
        (ts, others) and kept on this manager together with the other managers (their ids cannot be reused while the entry
        lives): a + b and a * b share one output manager."""
        mans = [self] + list(others)
        if len(mans) > 16:
            raise NotImplementedError(f"a union of {len(mans)} coordinate sets: at most 16")
        cache = self.__dict__.setdefault("_unions", {})
        key = (ts,) + tuple(id(m) for m in others)
        hit = cache.get(key)
        if hit is None:
            be = get_backend()
            if not hasattr(be, "coords_union"):
                raise NotImplementedError("arithmetic across coordinate sets needs the HIP backend (ms3d_coords_union)")
            out, out_rows, in_rows = be.coords_union([m.visible_coords(ts) for m in mans])
            n = out.size(0)
            if ts == 1 and any(m.inv is not None for m in mans):
                in_rows, out_rows = in_rows.clone(), list(out_rows)
                for i, m in enumerate(mans):
                    if m.inv is not None and m.size(1) > 0:
                        if n > 0:
                            r = in_rows[i].long()
                            in_rows[i] = torch.where(r >= 0, m.inv[r.clamp(min=0)], r).to(torch.int32)
                        out_rows[i] = out_rows[i][m.perm]
            out_rows = [r.contiguous() for r in out_rows]
            hit = cache[key] = (CoordinateManager.rooted(out, ts), in_rows.contiguous(), out_rows, n, tuple(others))
        return hit[:4]

    def broadcast_map(self, ts, gcm, gts):
        """what broadcasting one row per batch index (the set of tensor stride gts of the manager gcm: what a global pooling
        returns; only its batch column is read) onto this manager's set of tensor stride ts needs -> (grow int32 [V]: per held
        row the held row of the global tensor that carries its batch index, or -1 -- such a voxel sees the zero vector; (order,
        seg_start, seg_of_g): batch_rows' grouping and the segment of every global row, the summation order of the global
        operand's gradient).  A batch index that occurs twice in the global set raises ValueError.  Built once per pair (two
        small host reads) and kept with gcm."""
        cache = self.__dict__.setdefault("_broadcasts", {})
        key = (ts, id(gcm), gts)
        hit = cache.get(key)
        if hit is None:
            gb = gcm.__dict__.setdefault("_batch_index", {}).get(gts)
            if gb is None:
                gb = gcm.coords[gts][:, 0].cpu().numpy()
                if len(np.unique(gb)) != len(gb):
                    gb = ValueError("broadcast: a batch index occurs twice in the global tensor (batch indices "
                                    f"{gb.tolist()}); it must hold one row per batch index")
                gcm._batch_index[gts] = gb
            if isinstance(gb, ValueError):
                raise gb
            group = self.batch_group(ts)
            order, offsets, present = group.order, group.seg_start, group.indices   # batch index of every segment, ascending
            dev = self.coords[ts].device
            seg = {int(b): s for s, b in enumerate(present)}
            seg_of_g = torch.tensor([seg.get(int(b), -1) for b in gb], dtype=torch.int32, device=dev)
            lut = torch.full((int(max([-1] + gb.tolist() + list(present))) + 2,), -1, dtype=torch.int32, device=dev)
            lut[torch.as_tensor(gb, device=dev).long()] = torch.arange(len(gb), dtype=torch.int32, device=dev)
            grow = lut[self.coords[ts][:, 0].long()].contiguous()
            hit = cache[key] = (grow, (order.contiguous(), offsets.contiguous(), seg_of_g), gcm)
        return hit[:2]

    def interpolation_map(self, ts, points):
        """the trilinear interpolation map of the float points [N, 4] (batch index, x, y, z in voxel units) into the
        coordinate set of tensor stride ts -> (rows int32 [8, N], weights float32 [8, N], (entry_sorted int64, seg_start int32
        [V + 1])); the rules are ms3d_interp_map's (include/minsu3d_hip.h): corner j = bx + 2 by + 4 bz, rows -1 where the set
        has no voxel.  `rows` names the rows as the engine HOLDS them (the table is built over the held set, so the Morton
        permutation of a sorted manager is in it already; `visible_rows` turns them into the rows the caller sees).  The
        grouping is the map's entries e = 8 * point + corner with a row, stably sorted by row: the fixed order in which the
        backward sums a voxel's gradients.  Built once per points tensor OBJECT and version (the way a sorted index is kept on
        its tensor) and kept on this manager with the tensor; the four newest maps are kept.  An engine extra."""
        cache = self.__dict__.setdefault("_interp", {})
        key = (ts, id(points))
        hit = cache.get(key)
        if hit is None or hit[3] is not points or hit[4] != points._version:
            be = get_backend()
            if not hasattr(be, "interp_map"):
                raise NotImplementedError("interpolation needs the HIP backend (ms3d_interp_map)")
            if points.dim() != 2 or points.size(1) != 4 or not points.is_floating_point():
                raise ValueError(f"interpolation: float coordinates [N, 4] (batch index, x, y, z), got {list(points.shape)} "
                                 f"{points.dtype}")
            coords = self.coords[ts]
            p = points.detach().to(device=coords.device, dtype=torch.float32).contiguous()
            rows, weights = be.interp_map(coords, p, ts)
            v = coords.size(0)
            flat = rows.t().reshape(-1)                                   # point-major: entry e = 8 * point + corner
            valid = torch.nonzero(flat >= 0).view(-1)
            of_row = flat[valid].long()
            entry_sorted = valid[torch.sort(of_row, stable=True).indices].contiguous()
            seg_start = torch.zeros(v + 1, dtype=torch.int32, device=rows.device)
            seg_start[1:] = torch.cumsum(torch.bincount(of_row, minlength=v), 0)
            hit = cache[key] = (rows, weights, (entry_sorted, seg_start), points, points._version)
            while len(cache) > 4:
                cache.pop(next(iter(cache)))
        return hit[:3]

    def visible_rows(self, ts, rows):
        """held row numbers (int32, -1 = none) -> the rows of .coordinates / .features the caller sees"""
        if ts == 1 and self.perm is not None and rows.numel() > 0:
            return torch.where(rows >= 0, self.perm[rows.clamp(min=0).long()], rows.long()).to(torch.int32)
        return rows

    @functools.singledispatchmethod
    def kernel_map(self, ts, kernel_size, stride=1, dilation=1, region=None):
        """Two forms, chosen by the type of the first argument (a single-dispatch method: this is its base implementation).

        kernel_map(ts, kernel_size, stride=1, dilation=1, region=None), ts a tensor stride: the ENGINE's form, the tables the
        layers consume -- kernel_map_tables, unchanged (the layers call that name, past the dispatch).

        kernel_map(in_key, out_key, stride=1, kernel_size=3, dilation=1, region_type=RegionType.HYPER_CUBE, region_offsets=None,
        is_transpose=False, is_pool=False, kernel_generator=None), the keys CoordinateMapKeys or SparseTensors (their keys):
        MinkowskiEngine's form -> dict {k: int64 [2, N_k]} of the offsets k that have at least one pair, in ascending k.
        Column (i, o) of entry k: row i of in_key's `.coordinates` feeds row o of out_key's `.coordinates` through kernel[k], rows
        as the CALLER sees them (a Morton-sorted set is renamed inside the export kernel):
          forward     C_out[o] + off_k == C_in[i], off = kernel_offsets / region_offsets at the INPUT's tensor stride
          transposed  C_out[o] - off_k == C_in[i], off at the OUTPUT's tensor stride (the rule of generate())
        so y.F = sum_k index_add(o, x.F[i] @ W[k]) is the layer, and inside an entry o ascends.  The entries are views of
        kernel_map_pairs' tensor (see there for the tables, the errors and the cache); the dict is cached with it.  int64 and
        "only the offsets that have pairs" are MinkowskiEngine's conventions as recalled, not pinned."""
        return self.kernel_map_tables(ts, kernel_size, stride, dilation, region=region)

    def _kernel_map_of_keys(self, in_key, out_key, stride=1, kernel_size=3, dilation=1, region_type=RegionType.HYPER_CUBE,
                            region_offsets=None, is_transpose=False, is_pool=False, kernel_generator=None):
        """kernel_map's implementation for a CoordinateMapKey or a SparseTensor first (registered below the classes)"""
        return self._pair_lists(in_key, out_key, stride, kernel_size, dilation, region_type, region_offsets, is_transpose,
                                is_pool, kernel_generator)[2]

    def kernel_map_pairs(self, in_key, out_key, stride=1, kernel_size=3, dilation=1, region_type=RegionType.HYPER_CUBE,
                         region_offsets=None, is_transpose=False, is_pool=False, kernel_generator=None):
        """the packed form of kernel_map(in_key, out_key, ...) -> (pairs int64 [2, P], start int32 [K + 1] on the device): row 0
        the input rows, row 1 the output rows, offset k in columns start[k] .. start[k + 1] (backend.kmap_pairs, csrc/
        kmap_pairs.hip).  An engine extra.
        The table that is exported (all of them exist already): same manager, not transposed, out stride == in stride * stride:
        kernel_map_tables(in stride, ...)[0]; same manager, transposed, in stride == out stride * stride: the inverse table of
        kernel_map_tables(out stride, ...) (kernel_map_inverse); another manager -- a `coordinates=` target, an expanded,
        generated or pruned set: target_map(in stride, out_key, ...).  The geometry is checked by KernelGenerator, so its
        refusals apply (strides other than 1 and 2, an even kernel at stride 1, more than 254 offsets: NotImplementedError).
        ValueError, before any backend is touched: the keys' tensor strides contradict `stride`; a key's manager holds no set of
        its tensor stride; kernel_generator together with an argument that is not at its default and differs from the
        generator's.  is_pool is accepted and changes nothing (pooling and convolution share their tables).  The work is done
        by in_key's manager, whichever manager was asked.  A Morton-sorted stride-1 set hands its `inv` as out_order and its
        `perm` as in_rename (int32 copies kept on the manager).  Cached on in_key's manager per (keys, geometry, direction); the
        lists onto another manager are kept with the key, the sixteen newest, as target_map keeps its tables."""
        return self._pair_lists(in_key, out_key, stride, kernel_size, dilation, region_type, region_offsets, is_transpose,
                                is_pool, kernel_generator)[:2]

    def _pair_lists(self, in_key, out_key, stride=1, kernel_size=3, dilation=1, region_type=RegionType.HYPER_CUBE,
                    region_offsets=None, is_transpose=False, is_pool=False, kernel_generator=None):
        """-> (pairs, start, dict) of kernel_map_pairs / kernel_map(in_key, out_key, ...)"""
        in_key, out_key = _as_key(in_key, "in_key"), _as_key(out_key, "out_key")
        cm, in_ts, out_ts = in_key.coordinate_manager, in_key.tensor_stride, out_key.tensor_stride
        out_cm = out_key.coordinate_manager
        for name, key in (("in_key", in_key), ("out_key", out_key)):
            if key.tensor_stride not in key.coordinate_manager.coords:
                raise ValueError(f"kernel_map: {name}'s manager holds no coordinate set of tensor stride {key.tensor_stride}")
        given = dict(kernel_size=kernel_size, stride=stride, dilation=dilation, region_type=region_type,
                     is_transpose=bool(is_transpose))
        if kernel_generator is None:
            kernel_generator = KernelGenerator(kernel_size, stride, dilation, bool(is_transpose), region_type, region_offsets)
        else:
            if not isinstance(kernel_generator, KernelGenerator):
                raise TypeError(f"kernel_generator: a KernelGenerator, got {type(kernel_generator).__name__}")
            defaults = dict(kernel_size=3, stride=1, dilation=1, region_type=RegionType.HYPER_CUBE, is_transpose=False)
            for name, value in given.items():
                if value != defaults[name] and value != getattr(kernel_generator, name):
                    raise ValueError(f"kernel_map: {name}={value!r} contradicts kernel_generator ({kernel_generator!r})")
            if region_offsets is not None:
                theirs = kernel_generator.region_offsets
                mine = torch.as_tensor(region_offsets).to(torch.int64).cpu()
                if theirs is None or theirs.shape != mine.shape or not torch.equal(theirs.to(torch.int64), mine):
                    raise ValueError(f"kernel_map: region_offsets contradicts kernel_generator ({kernel_generator!r})")
        g = kernel_generator
        transposed = g.is_transpose
        if (in_ts != out_ts * g.stride) if transposed else (out_ts != in_ts * g.stride):
            raise ValueError(f"kernel_map: tensor strides {in_ts} -> {out_ts} contradict stride={g.stride}"
                             + (" of a transposed map (in == out * stride)" if transposed else " (out == in * stride)"))
        own = out_cm is cm
        cache = cm.__dict__.setdefault("_pair_lists_own" if own else "_pair_lists_onto", {})
        ident = (in_ts, out_key, g.stride, transposed) + ((g.kernel_size, g.dilation) if g.region_key is None else (g.region_key,))
        hit = cache.get(ident)
        if hit is None:
            be = get_backend()
            if not hasattr(be, "kmap_pairs") or not cm.coords[in_ts].is_cuda:
                raise NotImplementedError("kernel_map(in_key, out_key, ...) needs the HIP backend (ms3d_kmap_pairs_count)")
            geom = (g.kernel_size, g.stride, g.dilation)
            if not own:
                nbr, _, vin, vout, K = cm.target_map(in_ts, out_key, *geom, transposed=transposed, region=g.region_key)
            elif transposed:
                _, _, vout, vin, K, _, _ = cm.kernel_map_tables(out_ts, *geom, region=g.region_key)
                nbr = cm.kernel_map_inverse(out_ts, *geom, region=g.region_key)
            else:
                nbr, _, vin, vout, K, _, _ = cm.kernel_map_tables(in_ts, *geom, region=g.region_key)
            pairs, start = be.kmap_pairs(nbr.contiguous(), K, vout, vin, out_cm._rows32("inv") if out_ts == 1 else None,
                                         cm._rows32("perm") if in_ts == 1 else None)
            s = start.tolist()
            hit = cache[ident] = (pairs, start, {k: pairs[:, s[k]:s[k + 1]] for k in range(K) if s[k + 1] > s[k]})
            while not own and len(cache) > 16:
                cache.pop(next(iter(cache)))
        return hit

    def _rows32(self, which):
        """`perm` / `inv` as int32 (what the export kernel reads), None on a manager that holds its rows in the caller's order"""
        rows = getattr(self, which)
        if rows is None:
            return None
        cache = self.__dict__.setdefault("_perm32", {})
        if which not in cache:
            cache[which] = rows.to(torch.int32).contiguous()
        return cache[which]

    def stride(self, key, stride=2):
        """CoordinateMapKey of the set at key's tensor stride * stride on key's manager, made through k2 (one stride-2 step
        per factor of two) when missing.  stride == 1 returns the key; anything but a power of two raises NotImplementedError."""
        key = _as_key(key, "key")
        cm, ts = key.coordinate_manager, key.tensor_stride
        if isinstance(stride, bool) or not isinstance(stride, int) or stride < 1 or stride & (stride - 1):
            raise NotImplementedError(f"stride={stride!r}: strides other than 1 and 2 are built from stride-2 steps, so only "
                                      "powers of two are supported")
        if ts not in cm.coords:
            raise ValueError(f"stride: the key's manager holds no coordinate set of tensor stride {ts}")
        if stride == 1:
            return key
        while stride > 1:
            cm.k2(ts)
            ts, stride = 2 * ts, stride // 2
        return CoordinateMapKey(cm, ts)

    def stride_map(self, in_key, stride_key):
        """(in_rows int64 [V_in], out_rows int64 [V_in]): every row of the finer set in_key with its parent -- the row at
        floor(c / s) * s -- in the coarser set stride_key of the SAME manager, rows as the caller sees both sets, in_rows
        ascending (an arange).  stride_key's tensor stride is in_key's times a power of two >= 2; the levels in between are
        made on the way.  From the k2 up-tables (one valid entry per column), chained across the levels; built once.  Keys of
        different managers or a coarser -> finer order: ValueError."""
        in_key, stride_key = _as_key(in_key, "in_key"), _as_key(stride_key, "stride_key")
        cm, ts, top = in_key.coordinate_manager, in_key.tensor_stride, stride_key.tensor_stride
        if stride_key.coordinate_manager is not cm:
            raise ValueError("stride_map: the two keys name sets of different coordinate managers")
        ratio = top // ts if isinstance(top, int) and isinstance(ts, int) and top % ts == 0 else 0
        if ratio < 2 or ratio & (ratio - 1):
            raise ValueError(f"stride_map: tensor strides {ts} -> {top}: the second key must name the COARSER set, at the "
                             "first one's tensor stride times a power of two >= 2")
        if ts not in cm.coords:
            raise ValueError(f"stride_map: in_key's manager holds no coordinate set of tensor stride {ts}")
        cache = cm.__dict__.setdefault("_stride_maps", {})
        hit = cache.get((ts, top))
        if hit is None:
            parent, level = None, ts
            while level < top:
                up = cm.k2(level)[1].amax(0).long()[:cm.size(level)]          # [V_level]: the one valid entry of every column
                parent = up if parent is None else up[parent]
                level *= 2
            if ts == 1 and cm.inv is not None:
                parent = parent[cm.inv]
            hit = cache[(ts, top)] = (torch.arange(parent.numel(), dtype=torch.int64, device=parent.device), parent.contiguous())
        return hit

    def origin_map(self, key):
        """{0: int64 [2, V]}: row 0 the rows of the set as the caller sees them, ascending; row 1 the row of a
        MinkowskiGlobal*Pooling output the sample of each row lands in: the rank of its batch index among the batch indices
        present (batch_segments, which is how _GlobalPoolBase orders its output rows).  Built once per set."""
        key = _as_key(key, "key")
        cm, ts = key.coordinate_manager, key.tensor_stride
        if ts not in cm.coords:
            raise ValueError(f"origin_map: the key's manager holds no coordinate set of tensor stride {ts}")
        cache = cm.__dict__.setdefault("_origin_maps", {})
        if ts not in cache:
            seg = cm.batch_group(ts).seg_of_row.long()
            if ts == 1 and cm.inv is not None:
                seg = seg[cm.inv]
            cache[ts] = {0: torch.stack([torch.arange(seg.numel(), dtype=torch.int64, device=seg.device), seg])}
        return cache[ts]

    def kernel_map_tables(self, ts, kernel_size, stride=1, dilation=1, region=None):
        """-> (nbr_fwd [K, Vout], nbr_bwd [K, Vin], Vin, Vout, K, output tensor stride, mirror) for a layer from the
        coordinate set of tensor stride ts; built once per key.  (3, 1, 1), (2, 2, 1) and (1, 1, *) are the tables of
        k3() / k2() / identity().  Stride 1 (odd kernel sizes only): the output set is the input set, the table is its own
        transpose up to k <-> K-1-k (nbr_bwd = nbr_fwd, mirror = True).  Stride 2: the output set is the stride-2 set of
        k2() whatever the kernel size, nbr_bwd is the inverse table, mirror = False.  Other strides: NotImplementedError.
        Offsets: kernel_offsets().
        region (a non-cube KernelGenerator or its key; kernel_size and dilation are then the region's own): the offsets are
        region_offsets(region, ts) and the layer works between "two sets" even at stride 1 on its own set -> (nbr_fwd [K, Vout],
        nbr_bwd = the inverse table [K, Vin], Vin, Vout, K, output tensor stride, False).  Stride 1: both tables from one pass
        of backend.kmap_region (ms3d_kmap_region); stride 2: onto the stride-2 set of k2(), kmap_general + kmap_invert."""
        kernel_size, stride, dilation, region = int(kernel_size), int(stride), int(dilation), _region_key(region)
        if region is not None:
            return self._region_map(ts, stride, region)
        if kernel_size == 1 and stride == 1:
            ident, V = self.identity(ts), self.size(ts)
            return ident, ident, V, V, 1, ts, False
        if (kernel_size, stride, dilation) == (3, 1, 1):
            nbr, V = self.k3(ts), self.size(ts)
            return nbr, nbr, V, V, 27, ts, True
        if (kernel_size, stride, dilation) == (2, 2, 1):
            down, up = self.k2(ts)
            return down, up, self.size(ts), self.size(2 * ts), 8, 2 * ts, False
        key = (ts, kernel_size, stride, dilation)
        km = self._kmaps.get(key)
        if km is None:
            check_geometry(kernel_size, stride, dilation)
            be = get_backend()
            if not hasattr(be, "kmap_general"):
                raise NotImplementedError(f"kernel_size={kernel_size}, stride={stride}, dilation={dilation}: this backend "
                                          "builds the 3x3x3, 2x2x2 stride-2 and 1x1x1 maps only")
            offsets = torch.from_numpy(kernel_offsets(kernel_size, dilation, ts))
            K, vin = offsets.size(0), self.size(ts)
            if stride == 1:
                nbr = be.kmap_general(self.coords[ts], self.coords[ts], offsets)
                km = (nbr, nbr, vin, vin, K, ts, True)
            else:
                self.k2(ts)                    # makes the stride-2 coordinate set (every strided layer lands on it)
                out = self.coords[2 * ts]
                vout = out.size(0)
                nbr = be.kmap_general(self.coords[ts], out, offsets)
                km = (nbr, be.kmap_invert(nbr, K, vout, vin), vin, vout, K, 2 * ts, False)
            self._kmaps[key] = km
        return km

    def _region_map(self, ts, stride, region):
        key = (ts, stride, region)
        km = self._kmaps.get(key)
        if km is None:
            _check_region_geometry(0, stride, 0, region)
            be = get_backend()
            offsets = region_offsets(region, ts)
            K, vin = offsets.shape[0], self.size(ts)
            if stride == 1:
                if not hasattr(be, "kmap_region"):
                    raise NotImplementedError(f"region={region} at stride 1 needs the HIP backend (ms3d_kmap_region)")
                nbr, inv = be.kmap_region(self.coords[ts], offsets)
                km = (nbr, inv, vin, vin, K, ts, False)
            else:
                if not (hasattr(be, "kmap_general") and hasattr(be, "kmap_invert")):
                    raise NotImplementedError(f"region={region} at stride 2 needs the HIP backend (ms3d_kmap_general)")
                self.k2(ts)                    # makes the stride-2 coordinate set (every strided layer lands on it)
                out = self.coords[2 * ts]
                vout = out.size(0)
                nbr = be.kmap_general(self.coords[ts], out, torch.from_numpy(offsets))
                km = (nbr, be.kmap_invert(nbr, K, vout, vin), vin, vout, K, 2 * ts, False)
            self._kmaps[key] = km
        return km

    def kernel_map_inverse(self, ts, kernel_size, stride=1, dilation=1, region=None):
        """[K, Vin] table that names, per offset, the OUTPUT row an input row feeds (what a backward gather of a pooling
        layer walks): nbr_bwd of a strided map; for a submanifold map -- whose nbr_bwd is the forward table, to be read
        with mirrored offsets -- the inverse is built (and kept) here"""
        nbr_fwd, nbr_bwd, vin, vout, K, _, mirror = self.kernel_map_tables(ts, kernel_size, stride, dilation, region=region)
        if not mirror and nbr_bwd is not nbr_fwd:
            return nbr_bwd
        key = (ts, int(kernel_size), int(stride), int(dilation))
        if key not in self._kinv:
            self._kinv[key] = get_backend().kmap_invert(nbr_fwd.contiguous(), K, vout, vin)
        return self._kinv[key]

    def batch_group(self, ts):
        """the backend.BatchGroup of the coordinate set of tensor stride ts: its rows, as they are HELD, grouped by batch index
        -- order, seg_start, seg_of_row, the held <-> caller row maps of a Morton-sorted manager, and on first use the inverse
        order, the counts, and (one host read each) the segment lengths, the batch indices present and the attention chunk
        list.  Rows are batch-contiguous already only for some inputs, so nothing relies on it.  One stable sort, once per
        tensor stride; every per-sample op reads this record, the accessors below are views onto it.  An engine extra."""
        g = self._batch_groups.get(ts)
        if g is None:
            held = ts == 1 and self.perm is not None
            g = self._batch_groups[ts] = BatchGroup(self.coords[ts][:, 0], self.perm.to(torch.int32).contiguous() if held else None,
                                                    self.inv if held else None)
        return g

    def batch_rows(self, ts):
        """-> (order int64 [V]: rows sorted by batch, stable; its inverse permutation; offsets int32 [B + 1] into `order`, one
        segment per batch index PRESENT, ascending; counts float32 [B, 1]) of batch_group(ts)"""
        return self.batch_group(ts).rows

    def batch_segments(self, ts):
        """int32 [V]: for every row of the coordinate set, as it is HELD, the index of its segment in batch_rows(ts) (the rank
        of its batch index among the batch indices present): seg_of_row of batch_group(ts)"""
        return self.batch_group(ts).seg_of_row

    def batch_chunks(self, ts):
        """the chunk list of query_attention over batch_rows(ts) -> (chunk_seg int32 [chunks]: the sample of every chunk,
        chunk_first int32 [B + 1]: the first chunk of every sample, chunks): every segment cut into runs of
        ms3d_qattn_rows_per_chunk() positions of `order`, sorted by sample, then by run (backend.qattn_chunk_list): chunks of
        batch_group(ts), one host read"""
        return self.batch_group(ts).chunks

    def batch_lengths(self, ts):
        """the number of rows of every segment of batch_rows(ts) as a tuple of Python ints: lengths of batch_group(ts), one
        host read"""
        return self.batch_group(ts).lengths

    def batch_indices(self, ts):
        """the batch indices present, ascending, as a tuple of Python ints -- the batch index of every segment of
        batch_rows(ts): indices of batch_group(ts), one host read"""
        return self.batch_group(ts).indices

    def caller_rows(self, ts):
        """int32 [V]: for every row of the set as it is HELD, the row of .coordinates / .features the caller sees it at; None
        where the two orders are the same (no Morton permutation, or a coarser set): row_map of batch_group(ts)"""
        return self.batch_group(ts).row_map

    def extent(self, ts):
        """(per-axis minimum [3], per-axis maximum [3], largest batch index) of the coordinate set as Python ints, None for an
        empty set; one small host read, once per tensor stride.  An engine extra."""
        cache = self.__dict__.setdefault("_extent", {})
        if ts not in cache:
            c = self.coords[ts]
            if c.size(0) == 0:
                cache[ts] = None
            else:
                lo, hi = c.amin(0), c.amax(0)
                v = torch.cat([lo[1:], hi[1:], hi[:1]]).tolist()
                cache[ts] = (tuple(v[0:3]), tuple(v[3:6]), v[6])
        return cache[ts]

    def dense_map(self, ts, origin, divisor, grid):
        """the map between the rows of the coordinate set of tensor stride ts, as they are HELD, and the cells of a dense grid
        (B, X, Y, Z): a row's cell index per axis is (x - origin) / divisor, its cell ((b * X + x') * Y + y') * Z + z' -> (cell_row
        int32 [B*X*Y*Z]: the row at each cell or -1; row_cell int32 [V]: the cell of each row or -1; (rows outside the grid, rows
        the divisor does not divide, rows that lost their cell to another row)) -- backend.dense_cell_map.  Built once per (ts,
        origin, divisor, grid), as kernel maps are (one host sync); the table is as large as the grid, so only the four newest
        maps are kept.  An engine extra."""
        cache = self.__dict__.setdefault("_dense_maps", {})
        key = (ts, tuple(int(v) for v in origin), int(divisor), tuple(int(v) for v in grid))
        hit = cache.get(key)
        if hit is None:
            be = get_backend()
            if not hasattr(be, "dense_cell_map"):
                raise NotImplementedError("SparseTensor.dense needs the HIP backend (ms3d_dense_cell_map)")
            hit = cache[key] = be.dense_cell_map(self.coords[ts], key[1], key[2], key[3])
            while len(cache) > 4:
                cache.pop(next(iter(cache)))
        return hit

    def decomposition(self, ts):
        """list of int64 row lists, one per batch index 0 .. B - 1 (B = largest batch index + 1; an index without rows gets an
        empty list): the rows of .coordinates / .features -- the order the CALLER sees -- of every sample, each in ascending
        row order.  From batch_rows where the rows are held in the caller's order, from one stable sort of the caller's batch
        column on a Morton-sorted manager; one host read, once per tensor stride.  An engine extra."""
        cache = self.__dict__.setdefault("_decomposition", {})
        perms = cache.get(ts)
        if perms is None:
            b = self.visible_coords(ts)[:, 0].long()
            if ts == 1 and self.perm is not None:
                sb, order = torch.sort(b, stable=True)
                present, counts = torch.unique_consecutive(sb, return_counts=True)
                present, counts = present.tolist(), counts.tolist()
            else:
                group = self.batch_group(ts)
                order, counts, present = group.order, list(group.lengths), list(group.indices)
            parts = dict(zip(present, torch.split(order, counts))) if counts else {}
            perms = cache[ts] = [parts.get(i, order[:0]) for i in range((present[-1] + 1) if present else 0)]
        return perms

    def k3(self, ts):
        if ts not in self._k3:
            self._k3[ts] = get_backend().kmap_k3(self.coords[ts], ts)
        return self._k3[ts]

    def k2(self, ts):
        """stride-2 map from tensor stride ts to 2*ts; creates the coarse coordinate set on first use"""
        if ts not in self._k2:
            be = get_backend()
            oc, parent, koff = be.downsample(self.coords[ts], ts)
            if 2 * ts not in self.coords:
                self.coords[2 * ts] = oc.contiguous()
            self._k2[ts] = be.kmap_k2(parent, koff, oc.size(0))
        return self._k2[ts]

    def prepare(self, n_levels):
        """build the coordinate sets and kernel maps of `n_levels` U-Net levels now.  Each stride-2 map needs the
        coarse voxel count on the host (one sync); done up front the syncs hit an almost empty queue, done lazily
        inside the network each one drains the convolutions queued before it and the GPU then idles while the host
        catches up."""
        ts = 1
        for lvl in range(n_levels):
            self.k3(ts)
            self.identity(ts)        # table of the 1x1 projections (ResidualBlock.downsample) of this level
            if lvl + 1 < n_levels:
                self.k2(ts)
            ts *= 2

    def identity(self, ts):
        if ts not in self._ident:
            V = self.coords[ts].size(0)
            self._ident[ts] = _iota(V, self.coords[ts].device).view(1, V)
        return self._ident[ts]

    def size(self, ts):
        return self.coords[ts].size(0)


_IOTA = {}


def _iota(n, device):
    """int32 0..n-1 as a view of one long, growing arange per device (the K = 1 tables of every level of every batch: 9
    arange launches per step otherwise)"""
    t = _IOTA.get(device)
    if t is None or t.numel() < n:
        t = _IOTA[device] = torch.arange(max(2 * n, 1 << 20), dtype=torch.int32, device=device)
        if t.is_cuda:
            # used from several streams (main, prefetch) without further ordering: complete before anybody sees it
            # (happens once, and again only when a larger batch makes it grow)
            torch.cuda.current_stream(device).synchronize()
    return t[:n]


_PREFETCHED = {}   # (data_ptr, shape) of a coordinate tensor -> (future of (manager, cuda event), the tensor itself)


def prefetch_coordinates(coordinates, n_levels, wait_current_stream=True, channels=None, point_map=None):
    """Input pipelining (not part of ME's API): build everything that depends on the COORDINATES of a batch the next
    forward will use -- engine row order, the coordinate sets and kernel maps of `n_levels` U-Net levels, their pair
    lists -- on the helper thread and a side stream, e.g. while the current step's backward pass keeps the GPU busy and
    the interpreter idle.  `SparseTensor(features, coordinates)` picks the result up when it is given the same tensor.
    wait_current_stream=False: the coordinates are known to be complete (a resident batch), the side stream need not
    wait for the work queued on the caller's stream.  channels: the channel width of every level (the pair list a
    convolution walks depends on it: 128-row tiles above 32 channels); without it the 16 / 32-channel lists are built and
    a wider level builds its own on first use.  point_map: the batch's voxel_point_map -- its stable sort (the fixed
    summation order of the voxel -> point broadcast's backward, backend.sorted_rows) is built here too."""
    if not coordinates.is_cuda or os.environ.get("MS3D_PREFETCH_COORDS", "1") == "0":
        return
    key = (coordinates.data_ptr(), tuple(coordinates.shape))
    if key in _PREFETCHED:
        return
    from ..backend import prefetch_stream, prefetch_worker as worker
    side = prefetch_stream(coordinates.device)
    if wait_current_stream:
        side.wait_stream(torch.cuda.current_stream())

    def build():
        with torch.cuda.stream(side), torch.no_grad():
            be = get_backend()
            cm = CoordinateManager(coordinates.to(torch.int32), spatial_sort=True)
            cm.prepare(n_levels)
            ts = 1
            for lvl in range(n_levels):          # the lists the convolutions of these levels will ask for
                nbr, v = cm.k3(ts), cm.size(ts)
                c = channels[lvl] if channels is not None else 16
                be.pairlist(nbr, 27, v, c, c)
                be.offsetlist(nbr, 27, v)
                if lvl + 1 < n_levels:
                    down, up = cm.k2(ts)
                    vc = cm.size(2 * ts)
                    c2 = channels[lvl + 1] if channels is not None else 16
                    be.pairlist(down, 8, vc, c, c2); be.pairlist(down, 8, vc, c2, c); be.offsetlist(down, 8, vc)
                    be.pairlist(up, 8, v, c2, c); be.pairlist(up, 8, v, c, c2); be.offsetlist(up, 8, v)
                ts *= 2
            if getattr(be, "kernel_timer", None) is not None:
                # bench.py's roofline wants the valid-pair count of every table (algorithmic bytes): counted here, on the
                # prefetch stream, instead of by two torch launches per table inside a sampled (timed) step
                for t in list(cm._k3.values()) + [x for pair in cm._k2.values() for x in pair]:
                    be.table(t).pair_count()
            if point_map is not None and point_map.is_cuda and point_map.dtype == torch.int64 and be.deterministic():
                be.sorted_rows(point_map)    # its record orders every consumer behind this stream by itself (backend.SortedIndex)
            ev = torch.cuda.Event()
            ev.record(side)
            return cm, ev

    _PREFETCHED[key] = (worker().submit(build), coordinates)
    while len(_PREFETCHED) > 2:      # prefetched but never used (end of an epoch, a skipped batch): do not pile up
        fut, coords = _PREFETCHED.pop(next(iter(_PREFETCHED)))
        # its kernels may still be reading `coords` on the side stream when the last reference goes away here
        fut.add_done_callback(lambda f, c=coords, s=side: c.record_stream(s))


def _take_prefetched(coordinates):
    pf = _PREFETCHED.pop((coordinates.data_ptr(), tuple(coordinates.shape)), None) if _PREFETCHED else None
    if pf is None or pf[1] is not coordinates:
        return None
    cm, ev = pf[0].result()
    cur = torch.cuda.current_stream()
    cur.wait_event(ev)
    # everything was allocated under the side stream and is used (and eventually freed) under this one
    tables = [t for t in list(cm._k3.values()) + [t for pair in cm._k2.values() for t in pair] if t is not None]
    held = [cm.perm, cm.inv] + list(cm.coords.values()) + tables
    ext = getattr(cm, "coords_external", None)
    if ext is not None and ext is not coordinates:
        held.append(ext)     # an int32 copy made on the side stream (the caller's coordinates had another dtype)
    table = get_backend().table
    for t in tables:
        held.extend(table(t).tensors())      # the lists (and the pair count) the prefetch derived from the table
    for t in held:
        if t is not None and t.is_cuda:
            t.record_stream(cur)
    return cm


_SORT_MIN_ROWS = int(os.environ.get("MS3D_SORT_MIN_ROWS", "100000"))


class SparseTensor:
    def __init__(self, features, coordinates=None, device=None, coordinate_manager=None, tensor_stride=None,
                 coordinate_map_key=None, _pending=None, _stats=None):
        """Three forms.  SparseTensor(features, coordinates): a new manager; the rows stay in the caller's order.
        SparseTensor(features, coordinate_map_key=key[, coordinate_manager=key's manager]): a new tensor on an EXISTING set;
        `features` are in the CALLER's order, the order of `.coordinates` of that set, and go through one gather
        (functional.PermuteRowsFn, gradients flow back) into the order a Morton-sorted manager holds them in.
        SparseTensor(features, coordinate_manager=cm, tensor_stride=ts) is the ENGINE's constructor, used by every layer:
        the rows are taken AS HELD by the manager, which on a Morton-sorted stride-1 set is not the order of `.coordinates`
        / `.features` -- pass a key to hand over rows in that order."""
        if coordinate_map_key is not None:
            key = coordinate_map_key
            if not isinstance(key, CoordinateMapKey):
                raise ValueError(f"coordinate_map_key: a CoordinateMapKey, got {type(key).__name__}")
            if coordinates is not None:
                raise ValueError("coordinate_map_key names an existing coordinate set: pass either it or coordinates=, not both")
            if coordinate_manager is not None and coordinate_manager is not key.coordinate_manager:
                raise ValueError("coordinate_manager is not the manager of coordinate_map_key")
            if tensor_stride is not None and tensor_stride != key.tensor_stride:
                raise ValueError(f"tensor_stride={tensor_stride!r} differs from the tensor stride of coordinate_map_key, "
                                 f"{key.tensor_stride}")
            coordinate_manager, tensor_stride = key.coordinate_manager, key.tensor_stride
            if tensor_stride not in coordinate_manager.coords:
                raise ValueError(f"coordinate_map_key: its manager holds no coordinate set of tensor stride {tensor_stride}")
            rows = coordinate_manager.size(tensor_stride)
            if features.dim() != 2 or features.size(0) != rows:
                raise ValueError(f"features {list(features.shape)}: the coordinate set of coordinate_map_key has {rows} rows")
            if device is not None:
                features = features.to(device)
            if tensor_stride == 1 and coordinate_manager.perm is not None:
                features = Fn.PermuteRowsFn.apply(features, coordinate_manager.perm, coordinate_manager.inv)
        elif tensor_stride is None:
            tensor_stride = 1
        if coordinate_manager is None:
            if device is not None:
                features, coordinates = features.to(device), coordinates.to(device)
            coordinate_manager = _take_prefetched(coordinates) if coordinates.is_cuda else None
            if coordinate_manager is None:
                # small tensors (the proposal grids of the score / refinement nets: tens of thousands of rows, a few MB
                # of features that live in L2 anyway) keep the caller's row order: the Morton sort, the permutation
                # and its inverse cost more than the locality buys
                coordinate_manager = CoordinateManager(coordinates.to(torch.int32),
                                                       spatial_sort=coordinates.size(0) >= _SORT_MIN_ROWS)
            if coordinate_manager.perm is not None:
                features = features[coordinate_manager.perm]
        self._F = features
        self._F_ext = None
        self.coordinate_manager = coordinate_manager
        self.tensor_stride = tensor_stride
        self._pending = _pending  # None or dict(scale, shift, relu, bn ctx) not yet applied to _F
        self._stats = _stats      # per-block (sum, sum^2) partials of _F left by the producing conv's epilogue

    # ---- ME attribute surface
    @property
    def features(self):
        """rows in the CALLER's order (the order of the coordinates the tensor was built from)"""
        self._materialize()
        inv = self.coordinate_manager.inv if self.tensor_stride == 1 else None
        if inv is None:
            return self._F
        if self._F_ext is None:
            self._F_ext = Fn.PermuteRowsFn.apply(self._F, inv, self.coordinate_manager.perm)
        return self._F_ext

    F = features

    def _raw(self):
        """materialised rows in the engine's internal order"""
        self._materialize()
        return self._F

    @property
    def coordinates(self):
        cm = self.coordinate_manager
        if self.tensor_stride == 1 and cm.inv is not None:
            return cm.coords_external
        return cm.coords[self.tensor_stride]

    C = coordinates

    @property
    def coordinate_map_key(self):
        """the CoordinateMapKey of this tensor's coordinate set: (its manager, its tensor stride)"""
        return CoordinateMapKey(self.coordinate_manager, self.tensor_stride)

    @property
    def device(self):
        return self._F.device

    def _materialize(self):
        if self._pending is not None:
            self._F = Fn.bn_act(self._F, self._pending)
            self._pending = None
            self._stats = None
            self._F_ext = None

    def _like(self, features, pending=None, tensor_stride=None, stats=None):
        return SparseTensor(features, coordinate_manager=self.coordinate_manager,
                            tensor_stride=self.tensor_stride if tensor_stride is None else tensor_stride,
                            _pending=pending, _stats=stats)

    # ---- rows by coordinate
    def coordinate_rows(self, query):
        """int32 [N]: the row of `.features` / `.coordinates` that holds each coordinate of `query` (int [N, 4]: b, x, y, z),
        -1 where the tensor has no such voxel.  A lookup in the hash table of the coordinate set (the K = 1, offset-0 kernel
        map); not part of ME's API."""
        assert query.dim() == 2 and query.size(1) == 4
        cm, ts = self.coordinate_manager, self.tensor_stride
        be = get_backend()
        if not hasattr(be, "kmap_general"):
            raise NotImplementedError("coordinate_rows needs the HIP backend (ms3d_kmap_general)")
        n = query.size(0)
        if n == 0:
            return torch.empty(0, dtype=torch.int32, device=self.device)
        q = query.to(device=self.device, dtype=torch.int32).contiguous()
        rows = be.kmap_general(cm.coords[ts], q, torch.zeros((1, 3), dtype=torch.int32)).view(-1)[:n]
        if ts == 1 and cm.perm is not None:      # the set is held in the engine's row order: name the caller's rows
            rows = torch.where(rows >= 0, cm.perm[rows.clamp(min=0).long()], rows.long()).to(torch.int32)
        return rows

    def features_at_coordinates(self, query):
        """float [N, C]: the feature row at each coordinate of `query` (int [N, 4]), zeros where the tensor has no such voxel;
        differentiable (a coordinate asked for twice sends both gradients to its row, summed in a fixed order)"""
        rows = self.coordinate_rows(query).long()
        feats = self.features
        if rows.numel() == 0:
            return feats.new_zeros((0, feats.size(1)))
        padded = torch.cat([feats, feats.new_zeros((1, feats.size(1)))])      # absent -> the zero row behind the last one
        return Fn.gather_rows(padded, torch.where(rows < 0, torch.full_like(rows, feats.size(0)), rows))

    # ---- dense tensors
    def dense(self, shape=None, min_coordinate=None, contract_stride=True):
        """-> (dense float32 [B, C, X, Y, Z], min_coordinate int32 [1, 3], tensor_stride int32 [3]; the last two on the CPU).
        dense[b, :, x', y', z'] is the feature row at the cell, exactly 0 where the tensor has no voxel.  MinkowskiEngine is
        not installed where this engine is developed; this is the specification:

        Origin.  min_coordinate=None: the per-axis minimum of the tensor's coordinates (zeros for an empty tensor); it is
        returned.  min_coordinate=0 (any int): that value on every axis.  Otherwise 3 ints: a list, or a tensor [3] / [1, 3].
        Cell index.  contract_stride=True: (c - origin) / tensor_stride per axis; an origin or a coordinate difference that is
        not a multiple of the tensor stride raises ValueError.  contract_stride=False: c - origin.
        Shape.  shape=None: B = largest batch index + 1, spatial sizes = largest cell index + 1 per axis.  Given: torch.Size or
        tuple (B, C, X, Y, Z), C checked against the features (ValueError).
        Errors.  ValueError naming how many rows lie outside the grid (a negative cell index, one >= the size, or a batch index
        >= B), and ValueError for a set that holds a coordinate twice.  More than 2^31 - 1 cells: NotImplementedError.

        The rows are read where the manager holds them (a Morton-sorted set is not un-permuted, a pending BatchNorm / ReLU is
        materialised first); the cell map is cached on the manager (CoordinateManager.dense_map).  Gradients flow to the
        features; the coordinates get none.  Every element of the result is written once by one kernel (csrc/dense.hip)."""
        cm, ts = self.coordinate_manager, self.tensor_stride
        c = self._F.size(1)
        if not isinstance(ts, int):
            raise NotImplementedError(f"dense() on tensor_stride={ts!r}: one integer tensor stride (no per-axis tuples)")
        divisor = ts if contract_stride else 1
        ext = cm.extent(ts)
        if min_coordinate is None:
            origin = ext[0] if ext is not None else (0, 0, 0)
        elif isinstance(min_coordinate, int):
            origin = (min_coordinate,) * 3
        else:
            origin = tuple(int(v) for v in torch.as_tensor(min_coordinate).reshape(-1).tolist())
            if len(origin) != 3:
                raise ValueError(f"dense(): min_coordinate must hold 3 integers, got {len(origin)}")
        if any(o % divisor for o in origin):
            raise ValueError(f"dense(): min_coordinate {list(origin)} is not a multiple of the tensor stride {ts} "
                             "(pass contract_stride=False to keep the coordinates as they are)")
        if shape is None:
            if ext is None:
                grid = (0, 0, 0, 0)
            else:
                grid = (ext[2] + 1,) + tuple(max((hi - o) // divisor + 1, 0) for hi, o in zip(ext[1], origin))
        else:
            shape = tuple(int(v) for v in shape)
            if len(shape) != 5:
                raise ValueError(f"dense(): shape must be (B, C, X, Y, Z), got {list(shape)}")
            if shape[1] != c:
                raise ValueError(f"dense(): shape {list(shape)} asks for {shape[1]} channels, the features have {c}")
            if min(shape) < 0:
                raise ValueError(f"dense(): negative size in shape {list(shape)}")
            grid = (shape[0],) + shape[2:]
        if grid[0] * grid[1] * grid[2] * grid[3] > 2 ** 31 - 1:
            raise NotImplementedError(f"dense(): a grid of {list(grid)} (B, X, Y, Z) has more than 2^31 - 1 cells")
        cell_row, row_cell, (outside, offgrid, lost) = cm.dense_map(ts, origin, divisor, grid)
        if offgrid:
            raise ValueError(f"dense(): {offgrid} rows have a coordinate whose difference to min_coordinate {list(origin)} is "
                             f"not a multiple of the tensor stride {ts}")
        if outside:
            raise ValueError(f"dense(): {outside} rows lie outside the grid {list(grid)} (B, X, Y, Z) from min_coordinate "
                             f"{list(origin)} (a negative cell index, one past the size, or a batch index >= B)")
        if lost:
            raise ValueError(f"dense(): the coordinate set holds a coordinate more than once ({lost} rows repeat another row's)")
        out = Fn.dense_scatter(self._raw(), cell_row, row_cell, (grid[0], c) + grid[1:])
        return out, torch.tensor([origin], dtype=torch.int32), torch.tensor([ts] * 3, dtype=torch.int32)

    # ---- per-sample views (plain torch over the rows the caller sees; rows of a sample keep their order)
    @property
    def decomposition_permutations(self):
        """list of int64 row lists into .features / .coordinates, one per batch index 0 .. B - 1, empty lists included"""
        return list(self.coordinate_manager.decomposition(self.tensor_stride))

    @property
    def decomposed_coordinates(self):
        """list of int32 [n_b, 3]: the coordinates of every sample without the batch column"""
        coords = self.coordinates
        return [coords[p, 1:] for p in self.decomposition_permutations]

    @property
    def decomposed_features(self):
        """list of float [n_b, C]: the feature rows of every sample (differentiable)"""
        feats = self.features
        return [feats[p] for p in self.decomposition_permutations]

    @property
    def decomposed_coordinates_and_features(self):
        return self.decomposed_coordinates, self.decomposed_features

    def _sample_rows(self, batch_index):
        perms = self.coordinate_manager.decomposition(self.tensor_stride)
        if not isinstance(batch_index, int) or not 0 <= batch_index < len(perms):
            raise ValueError(f"batch index {batch_index!r}: the tensor holds the batch indices 0 .. {len(perms) - 1}")
        return perms[batch_index]

    def coordinates_at(self, batch_index):
        """int32 [n_b, 3]: the coordinates of one sample without the batch column"""
        return self.coordinates[self._sample_rows(batch_index), 1:]

    def features_at(self, batch_index):
        """float [n_b, C]: the feature rows of one sample (differentiable)"""
        return self.features[self._sample_rows(batch_index)]

    # ---- points in, points out (TensorField)
    def slice(self, field):
        """TensorField on `field`'s points: every point gets the row of its voxel (TensorField.slice)"""
        return field.slice(self)

    def cat_slice(self, field):
        """the same with the field's own features in front (TensorField.cat_slice)"""
        return field.cat_slice(self)

    def interpolate(self, field):
        """TensorField on `field`'s points: the trilinear interpolation of this tensor's rows at the points' continuous
        coordinates, zeros for absent voxels, no renormalisation (ms3d_interp_map / ms3d_interp_forward).  Gradients flow to
        the features only; like MinkowskiEngine, the coordinates get none."""
        rows, weights, group = self.coordinate_manager.interpolation_map(self.tensor_stride, field._points())
        return field._like(Fn.interpolate(self._raw(), rows, weights, group))

    def __iadd__(self, other):      # `x += identity` (common.py:48)
        if not isinstance(other, SparseTensor):
            self._F = self._dense_op(other, torch.add)
        elif other.coordinate_manager is not self.coordinate_manager or other.tensor_stride != self.tensor_stride:
            raise ValueError("+= across two coordinate sets: an in-place operation cannot change the set of its left operand "
                             "(write a = a + b)")
        else:
            self._F = self._raw() + other._raw()
        self._stats = None
        self._F_ext = None
        return self

    def __add__(self, other):
        if not isinstance(other, SparseTensor):
            return self._like(self._dense_op(other, torch.add))
        if other.coordinate_manager is not self.coordinate_manager or other.tensor_stride != self.tensor_stride:
            return union_op(0, self, other)
        return self._like(self._raw() + other._raw())

    def __sub__(self, other):
        if not isinstance(other, SparseTensor):
            return self._like(self._dense_op(other, torch.sub))
        if other.coordinate_manager is not self.coordinate_manager or other.tensor_stride != self.tensor_stride:
            return union_op(1, self, other)
        return self._like(self._raw() - other._raw())

    def __mul__(self, other):
        if not isinstance(other, SparseTensor):
            return self._like(self._dense_op(other, torch.mul))
        if other.coordinate_manager is not self.coordinate_manager or other.tensor_stride != self.tensor_stride:
            return union_op(2, self, other)
        return self._like(self._raw() * other._raw())

    __radd__ = __add__      # scalar + tensor, scalar * tensor (a SparseTensor on the left is handled by its own method)
    __rmul__ = __mul__

    def _dense_op(self, other, fn):
        """fn(rows, other) for a Python scalar or a torch.Tensor broadcastable to [V, C].  A tensor with one row per voxel is
        in the CALLER's row order (that of .features) and is permuted into the engine's where one is held."""
        rows = self._raw()
        if torch.is_tensor(other):
            if other.dim() > 2 or (other.dim() == 2 and other.size(0) not in (1, rows.size(0))):
                raise ValueError(f"a tensor operand must broadcast to the rows [{rows.size(0)}, {rows.size(1)}], got "
                                 f"{list(other.shape)}")
            other = other.to(rows.device)
            perm = self.coordinate_manager.perm if self.tensor_stride == 1 else None
            if perm is not None and other.dim() == 2 and other.size(0) == rows.size(0) and rows.size(0) > 1:
                other = other[perm]
        elif not isinstance(other, (int, float)):
            raise TypeError(f"unsupported operand for a SparseTensor: {type(other).__name__}")
        return fn(rows, other)


# kernel_map(in_key, out_key, ...): the forms chosen by the type of the first argument (the classes exist only here)
for _cls in (CoordinateMapKey, SparseTensor):
    CoordinateManager.kernel_map.register(_cls, CoordinateManager._kernel_map_of_keys)


class SparseTensorQuantizationMode(enum.Enum):
    """what a voxel's feature is when several points fall into it (TensorField.sparse)"""
    RANDOM_SUBSAMPLE = 0        # the FIRST point of the voxel: "random" is the canonical first occurrence, as everywhere here
    UNWEIGHTED_AVERAGE = 1      # mean of the voxel's points
    UNWEIGHTED_SUM = 2          # their sum
    MAX_POOL = 4                # per-element maximum (lowest point index on ties)


_REDUCE_CODE = {SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE: 0, SparseTensorQuantizationMode.UNWEIGHTED_SUM: 1,
                SparseTensorQuantizationMode.MAX_POOL: 2}


def _check_tensor_stride(ts):
    if not isinstance(ts, int) or ts < 1 or ts & (ts - 1):
        raise NotImplementedError(f"tensor_stride={ts!r}: one positive power of two (no per-axis tuples)")
    return ts


class TensorField:
    """Features at continuous positions: `coordinates` [N, 4] (batch index first, x, y, z in voxel units, float or integer),
    `features` [N, C].  `.sparse()` voxelises, `.slice()` / `.cat_slice()` bring a SparseTensor's rows back to the points,
    `SparseTensor.interpolate(field)` reads a tensor at the points trilinearly.  The rules (floor, first-occurrence order,
    ascending-point sums) are MinkowskiEngine's as recalled, not pinned; DESIGN section 4.2 writes them down."""

    def __init__(self, features, coordinates, quantization_mode=SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE, device=None):
        if not isinstance(quantization_mode, SparseTensorQuantizationMode):
            raise NotImplementedError(f"quantization_mode={quantization_mode!r}: a SparseTensorQuantizationMode")
        if coordinates.dim() != 2 or coordinates.size(1) != 4 or features.dim() != 2 or features.size(0) != coordinates.size(0):
            raise ValueError(f"TensorField: coordinates [N, 4] and features [N, C], got {list(coordinates.shape)} and "
                             f"{list(features.shape)}")
        if device is not None:
            features, coordinates = features.to(device), coordinates.to(device)
        self._F, self._C = features, coordinates.to(features.device)
        self.quantization_mode = quantization_mode
        self._shared = {}        # caches that depend on the coordinates only; fields made by _like() share them

    @property
    def features(self):
        return self._F

    F = features

    @property
    def coordinates(self):
        return self._C

    C = coordinates

    @property
    def device(self):
        return self._F.device

    def _like(self, features):
        f = TensorField.__new__(TensorField)
        f._F, f._C, f.quantization_mode, f._shared = features, self._C, self.quantization_mode, self._shared
        return f

    def _points(self):
        """the coordinates as ONE float tensor object (an interpolation map is cached per object)"""
        if self._C.is_floating_point():
            return self._C
        p = self._shared.get("points")
        if p is None:
            p = self._shared["points"] = self._C.to(torch.float32)
        return p

    def _points32(self):
        """the coordinates as ONE contiguous float32 tensor [N, 4] (float64 points are taken to float32 once)"""
        p = self._points()
        if p.dtype == torch.float32 and p.is_contiguous():
            return p
        q = self._shared.get("points32")
        if q is None:
            q = self._shared["points32"] = p.to(torch.float32).contiguous()
        return q

    def _batch_group(self):
        """the backend.BatchGroup of the points: grouped by batch index as CoordinateManager.batch_group groups rows (a field's
        points are held in the caller's order: no row_map).  One stable sort of the batch column, once per field; fields made
        by _like() share the record."""
        g = self._shared.get("batch_group")
        if g is None:
            g = self._shared["batch_group"] = BatchGroup(self._C[:, 0])
        return g

    def _batch_indices(self):
        """the batch indices present, ascending, as a tuple of Python ints: indices of _batch_group(), one host read"""
        return self._batch_group().indices

    def _quantized(self, ts):
        """int32 [N, 4]: the voxel of every point at tensor stride ts, floor(p / ts) * ts per axis (floor, not truncation:
        -0.5 -> -ts); the batch column is taken as an integer"""
        q = self._shared.get(("q", ts))
        if q is None:
            c = self._C
            if c.is_floating_point():
                xyz = torch.floor(c[:, 1:] / ts).to(torch.int32) * ts
            else:
                xyz = torch.div(c[:, 1:], ts, rounding_mode="floor").to(torch.int32) * ts
            q = self._shared[("q", ts)] = torch.cat([c[:, :1].to(torch.int32), xyz], 1).contiguous()
        return q

    def sparse(self, tensor_stride=1, quantization_mode=None):
        """-> SparseTensor at `tensor_stride` (a power of two) on the voxels floor(p / ts) * ts, in first-occurrence order of
        the points (ms3d_sparse_quantize); its features per `quantization_mode` (default: the field's): the mean / sum of the
        voxel's points added in ascending point index, the per-element maximum, or the voxel's first point.  A field of at
        least _SORT_MIN_ROWS voxels at stride 1 gets a Morton-sorted manager like any SparseTensor.  `.inverse_mapping`
        afterwards names every point's row in the order of the result's .features / .coordinates."""
        ts = _check_tensor_stride(tensor_stride)
        mode = self.quantization_mode if quantization_mode is None else quantization_mode
        if not isinstance(mode, SparseTensorQuantizationMode):
            raise NotImplementedError(f"quantization_mode={mode!r}: a SparseTensorQuantizationMode")
        be = get_backend()
        if not hasattr(be, "sparse_quantize"):
            raise NotImplementedError("TensorField.sparse needs the HIP backend (ms3d_sparse_quantize)")
        if mode in _REDUCE_CODE and not hasattr(be, "field_reduce"):
            raise NotImplementedError("TensorField.sparse needs the HIP backend (ms3d_field_reduce)")
        q = self._quantized(ts)
        uniq, inv = be.sparse_quantize(q)
        uniq, inverse = uniq.long(), inv.long()
        coords = q[uniq]
        v = coords.size(0)
        cm = (CoordinateManager(coords, spatial_sort=v >= _SORT_MIN_ROWS) if ts == 1 else CoordinateManager.rooted(coords, ts))
        # the maps below name rows as the engine HOLDS them: the Morton permutation is composed into them once
        held = cm.inv[inverse] if cm.inv is not None else inverse
        feats = self._F if self._F.dtype == torch.float32 else self._F.float()
        if v == 0:
            y = feats.new_empty((0, feats.size(1)))
        elif mode is SparseTensorQuantizationMode.RANDOM_SUBSAMPLE:
            y = Fn.gather_rows(feats, uniq[cm.perm] if cm.perm is not None else uniq, max_dup=1)
        else:
            order = torch.sort(held, stable=True).indices.contiguous()
            seg_start = torch.zeros(v + 1, dtype=torch.int32, device=held.device)
            seg_start[1:] = torch.cumsum(torch.bincount(held, minlength=v), 0)
            y = Fn.field_reduce(feats, _REDUCE_CODE[mode], held.to(torch.int32).contiguous(), order, seg_start, v)
        self._shared["sparse"] = (cm, ts, inverse, held)
        return SparseTensor(y, coordinate_manager=cm, tensor_stride=ts)

    @property
    def inverse_mapping(self):
        """int64 [N]: point -> row of the last .sparse() (in the order of its .features / .coordinates)"""
        last = self._shared.get("sparse")
        if last is None:
            raise ValueError("TensorField.inverse_mapping: call .sparse() first")
        return last[2]

    def _rows_in(self, x):
        """int64 [N]: per point the row of x.features its voxel has at x's tensor stride, x.features.size(0) where x lacks
        the voxel; looked up once per (manager, tensor stride) through SparseTensor.coordinate_rows"""
        cache = self._shared.setdefault("rows", {})
        key = (id(x.coordinate_manager), x.tensor_stride)
        hit = cache.get(key)
        if hit is None or hit[1] is not x.coordinate_manager:
            r = x.coordinate_rows(self._quantized(_check_tensor_stride(x.tensor_stride))).long()
            n_rows = x.coordinate_manager.size(x.tensor_stride)
            hit = cache[key] = (torch.where(r < 0, torch.full_like(r, n_rows), r), x.coordinate_manager)
        return hit[0]

    def slice(self, x):
        """TensorField on these points with out[n] = x.F[row of point n's voxel].  On the tensor `.sparse()` made (same manager
        and stride) the cached inverse map is used; on any other manager or stride -- the output of a generative layer, a
        pruned tensor, a coarser level -- the rows are looked up once and a point whose voxel x lacks gets the zero row.  The
        gradient of a voxel row is the sum of its points' gradients in ascending point index."""
        if self._C.size(0) == 0:
            return self._like(x._F.new_zeros((0, x._F.size(1))))
        last = self._shared.get("sparse")
        if last is not None and x.coordinate_manager is last[0] and x.tensor_stride == last[1]:
            return self._like(Fn.gather_rows(x._raw(), last[3]))
        rows = self._rows_in(x)
        feats = x.features
        padded = torch.cat([feats, feats.new_zeros((1, feats.size(1)))])      # absent -> the zero row behind the last one
        return self._like(Fn.gather_rows(padded, rows))

    def cat_slice(self, x):
        """.slice(x) with the field's own features concatenated in front"""
        return self._like(torch.cat([self._F, self.slice(x)._F], 1))


_FPS_MAX_B = 65535                       # the limit of csrc/fps.hip
_FPS_LO, _FPS_HI = -16384, 16384         # the packable range: squared distances inside it fit unsigned 32-bit arithmetic


def _fps_torch(points, batch, lengths, M, start):
    """the rule of farthest_point_sampling as a torch expression: a loop of M steps over all samples at once.  points [V, 3]
    (int64: exact distances; float32: every operation rounded to float32) and batch [V] in the CALLER's row order, lengths:
    the rows of every sample present (ascending batch index), start: int64 [B] caller rows or None -> int64 [B, M].  A sample
    is laid out in ascending caller row and argmax returns the first of equal values, hence the lowest caller row."""
    B, L, V, dev = len(lengths), max(lengths), points.size(0), points.device
    rows = torch.sort(batch, stable=True).indices
    n = torch.tensor(lengths, dtype=torch.int64, device=dev)
    pos = torch.arange(L, device=dev)
    valid = pos[None, :] < n[:, None]
    idx = rows[((torch.cumsum(n, 0) - n)[:, None] + pos[None, :]).clamp(max=V - 1)]     # [B, L]; the padding is never chosen
    P = points[idx]
    ar = torch.arange(B, device=dev)
    at = torch.zeros(B, dtype=torch.int64, device=dev) if start is None else ((idx == start[:, None]) & valid).int().argmax(1)
    big = float("inf") if P.is_floating_point() else torch.iinfo(torch.int64).max
    nearest = torch.full((B, L), big, dtype=P.dtype, device=dev)
    out = torch.empty((B, M), dtype=torch.int64, device=dev)
    for j in range(M):
        if j:
            d = P - P[ar, at].unsqueeze(1)
            d = d * d
            nearest = torch.minimum(nearest, (d[..., 0] + d[..., 1]) + d[..., 2])
            at = torch.where(valid, nearest, -1).argmax(1)
        out[:, j] = idx[ar, at]
    return out


class _SupportSet:
    """the set a per-sample point op searches -- a SparseTensor or a TensorField as csrc/fps.hip and csrc/knn.hip take it: its
    kind, data [V, 4] as HELD (int32 coordinates / float32 points) and group, the BatchGroup of its rows.  Integer coordinates
    outside the packable range are refused here."""

    def __init__(self, x, name, what):
        self.x = x
        if isinstance(x, SparseTensor):
            cm, ts = x.coordinate_manager, x.tensor_stride
            self.kind, self.data, self.group = SparseTensor, cm.coords[ts], cm.batch_group(ts)
            if self.data.size(0):
                lo, hi, _ = cm.extent(ts)
                if min(lo) < _FPS_LO or max(hi) >= _FPS_HI:
                    raise ValueError(f"{name}: coordinates from {min(lo)} to {max(hi)} leave the packable range [{_FPS_LO}, "
                                     f"{_FPS_HI}), outside which squared distances do not fit 32 bits")
        elif isinstance(x, TensorField):
            self.kind, self.data, self.group = TensorField, x._points32(), x._batch_group()
        else:
            raise TypeError(f"{name}: {what} must be a SparseTensor or a TensorField, got {type(x).__name__}")
        self.V = self.data.size(0)

    def words(self, held, segment):
        """the rows `held` as packed queries: int32 words [n, 4] = (segment, x, y, z)"""
        w = self.data[held]
        w = w if w.dtype == torch.int32 else w.view(torch.int32)
        w[:, 0] = segment
        return w

    def caller_of_order(self):
        """the caller row of every position of `order`"""
        g = self.group
        return g.order if g.row_map is None else g.row_map[g.order].long()


def farthest_point_sampling(x, num_samples, start=None):
    """Farthest point sampling per sample (an engine extra: MinkowskiEngine has no such function) -- the seeds of a mask
    transformer's queries, the grouping stage of a point network.  x: a SparseTensor (any tensor stride its manager holds, any
    manager: plain, Morton-sorted, rooted) or a TensorField.  -> int64 [B, M], M = num_samples (a Python int >= 1), B the number
    of batch indices PRESENT; row b belongs to the b-th of them in ascending order -- the numbering of
    CoordinateManager.batch_rows, of origin_map, of the global pooling layers and of query_attention; gaps in the batch indices
    and interleaved rows are fine.  The values are rows of x.F / x.C as the caller sees them, on a Morton-sorted manager too:
    x.F[idx] is [B, M, C], ready for MinkowskiQueryAttention; x.C[idx][..., 1:] are the positions.

    The rule, all of it: pick 0 of a sample is start[b], without `start` the sample's lowest caller row; pick j is the row of the
    sample whose distance to the nearest of the picks 0 .. j-1 is largest; among equal distances the lowest caller row wins;
    rows already picked have distance 0 and take part like any other row.  So the result is a pure function of the coordinates
    -- the same bytes on every run, whatever order the manager holds its rows in.

    Distances.  SparseTensor: the exact integer dx^2 + dy^2 + dz^2 of the coordinates at the tensor's stride, in unsigned 32-bit
    arithmetic (up to 3 * 32767^2 = 3 221 028 867 over the packable range [-16384, 16384); a coordinate outside that range is a
    ValueError).  TensorField: its float32 points (float64 input is taken to float32 first), d = (dx*dx + dy*dy) + dz*dz with
    dx = p.x - c.x, every operation rounded to float32 on its own and never contracted into an FMA, the running minimum by
    fminf.  Finite coordinates are a precondition and are not checked.  Duplicate points are legal: once every remaining
    distance is 0 the rule repeats the lowest row.

    start: an int64 tensor [B] of caller rows, one inside each sample in the numbering above; a wrong shape or dtype, a row
    outside its sample or another B is a ValueError.  Checking it is one host read, made only when start is given.
    num_samples larger than the smallest sample is a ValueError naming the sample and its size (the segment lengths are read on
    the host once per coordinate set or field).  An empty tensor gives an empty [0, M] result.

    Device tensors: one launch of csrc/fps.hip, one workgroup per sample, no atomics, no waiting between workgroups; a sample of
    at most ms3d_fps_resident_rows() rows stays in registers, a larger one is swept from a workspace every pick.  The rows are
    read where the manager holds them; nothing is permuted or copied.  CPU tensors: the same rule as a torch expression, a loop
    of M steps.  The index is not differentiable: gradients reach x.F through the caller's x.F[idx] or ME.gather_rows.
    Out of scope: other metrics, feature-space sampling, a different M per sample, float16 or float64 distances, gradients
    with respect to the coordinates.  Grouping rows around the picks: knn_query(x, k, idx)."""
    name = "farthest_point_sampling"
    if isinstance(num_samples, bool) or not isinstance(num_samples, int) or num_samples < 1:
        raise ValueError(f"{name}: num_samples must be a Python int >= 1, got {num_samples!r}")
    M = num_samples
    sup = _SupportSet(x, name, "x")
    data, group, V, dev = sup.data, sup.group, sup.V, sup.data.device
    if V == 0:
        if start is not None and (not torch.is_tensor(start) or start.dtype != torch.int64 or tuple(start.shape) != (0,)):
            raise ValueError(f"{name}: start must be an int64 tensor [B] with B = 0, the samples of x")
        return torch.empty((0, M), dtype=torch.int64, device=dev)
    B, lengths = group.B, group.lengths
    small = min(range(B), key=lengths.__getitem__)
    if M > lengths[small]:
        raise ValueError(f"{name}: num_samples = {M} is larger than sample {small}, which has {lengths[small]} rows")
    if B > _FPS_MAX_B:
        raise ValueError(f"{name}: B = {B} is above the kernel's limit of {_FPS_MAX_B}")
    start_held = None
    if start is not None:
        if not torch.is_tensor(start) or start.dtype != torch.int64:
            raise ValueError(f"{name}: start must be an int64 tensor [B] of caller rows, got "
                             f"{getattr(start, 'dtype', type(start).__name__)}")
        if tuple(start.shape) != (B,):
            raise ValueError(f"{name}: start must have shape [B] = [{B}], one row per sample of x, got {list(start.shape)}")
        start = start.to(dev)
        start_held, inside = group.held_rows(start)
        if not bool(inside.all()):
            bad = int((~inside).nonzero()[0])
            raise ValueError(f"{name}: start[{bad}] = {int(start[bad])} is not a row of sample {bad}")
    if not data.is_cuda:
        batch = x.C[:, 0].long()
        points = x.C[:, 1:].long() if isinstance(x, SparseTensor) else data[:, 1:]
        return _fps_torch(points, batch, lengths, M, start)
    be = get_backend()
    if not hasattr(be, "fps"):
        raise NotImplementedError(f"{name} on device tensors needs the HIP backend (ms3d_fps_i32)")
    return be.fps(data, group, None if start_held is None else start_held.contiguous(), M)


_KNN_MAX_K = 64                          # ms3d_knn_max_k() of csrc/knn.hip
_KNN_CHUNK = 1 << 22                     # the CPU path holds at most this many (query, row) pairs at a time


def _knn_torch(points, batch, lengths, qpoints, q_counts, k, cap):
    """the rule of knn_query as a torch expression.  points [V, 3] (int64: exact distances; float32: every operation rounded
    to float32) and batch [V] in the CALLER's row order, lengths: the rows of every sample present (ascending batch index);
    qpoints [NQ, 3] the queries grouped by sample, q_counts of them for each -> (int64 [NQ, k] caller rows, int64 / float32
    [NQ, k] distances).  Per sample the queries go in chunks of at most max(1, _KNN_CHUNK // V_b), so no more than _KNN_CHUNK
    = 2^22 (query, row) pairs are held at a time; per chunk one int64 key (distance bits << 31) | caller row -- 3 221 028 867 *
    2^31 < 2^63, and the bits of a non-negative float32 are below 2^31 -- and one torch.topk over the distinct keys."""
    dev, integer, NQ = points.device, not points.is_floating_point(), qpoints.size(0)
    rows = torch.sort(batch, stable=True).indices
    idx = torch.full((NQ, k), -1, dtype=torch.int64, device=dev)
    d2 = torch.full((NQ, k), -1 if integer else float("inf"), dtype=points.dtype, device=dev)
    s = q = 0
    for n, m in zip(lengths, q_counts):
        r = rows[s:s + n]
        P = points[r]
        step, kk = max(1, _KNN_CHUNK // max(n, 1)), min(k, n)
        for c in range(q, q + m if kk else q, step):
            Q = qpoints[c:min(c + step, q + m)]
            dx, dy, dz = (Q[:, a:a + 1] - P[:, a][None, :] for a in range(3))
            d = (dx * dx + dy * dy) + dz * dz                     # three products, two sums, each rounded on its own
            bits = d if integer else d.view(torch.int32).long()
            top = torch.topk((bits << 31) | r[None, :], kk, dim=1, largest=False, sorted=True).values
            idx[c:c + Q.size(0), :kk] = top & (2 ** 31 - 1)
            top = top >> 31
            d2[c:c + Q.size(0), :kk] = top if integer else top.to(torch.int32).view(torch.float32)
        s, q = s + n, q + m
    if cap is not None:
        far = d2 > cap
        idx[far] = -1
        d2[far] = -1 if integer else float("inf")
    return idx, d2


def knn_query(x, k, queries=None, max_squared_distance=None):
    """The k nearest rows of a query's own sample (an engine extra: MinkowskiEngine has no such function) -- grouping rows
    around the picks of farthest_point_sampling, carrying features of M picks back to all V rows (three-nearest inverse
    distance unpooling), kNN graphs for vector attention.  -> (idx int64 [..., k], d2 [..., k]).

    x, the support set: a SparseTensor (any tensor stride its manager holds; a plain, Morton-sorted or rooted manager) or a
    TensorField.  k: a Python int, 1 <= k <= 64 (ms3d_knn_max_k()).  queries:
      None             every row of x queries its own sample -> [V, k]; row i answers caller row i of x.
      int64 [B, M]     caller rows of x, the form farthest_point_sampling returns: row b lies inside the b-th batch index present
                       (the numbering of batch_rows, origin_map and query_attention) -> [B, M, k].  Duplicates inside a row are
                       legal.  A row outside its sample, another B, a wrong dtype or shape is a ValueError; that check is one
                       host read, made only for this form.
      y                another tensor of the same kind as x (SparseTensor with SparseTensor -- tensor strides and managers
                       may differ -- or TensorField with TensorField): every row of y queries the sample of x with the same batch
                       index VALUE -> [V_y, k] in y's caller row order.  A batch index present in y and absent from x is a
                       ValueError naming it; samples of x without queries are fine.  Mixed kinds are a TypeError.

    The rule, all of it: for a query at position p in sample b the answer is the k rows of sample b of x with the smallest keys
    (distance to p, caller row of x), in ascending key order.  Among equal distances the lowest caller row comes first.  A query
    that is itself a row of x finds itself first, at distance 0 (nothing is excluded).  The result is a pure function of the
    coordinates: the same bytes on every run, whatever order the manager holds its rows in.  The values are rows of x.F / x.C
    as the caller sees them: x.F[idx] is [..., k, C].

    Distances are those of farthest_point_sampling.  SparseTensor: the exact integer dx^2 + dy^2 + dz^2 in unsigned 32-bit
    arithmetic over the packable range [-16384, 16384) of both sets (outside it: ValueError), returned as int64 because it
    reaches 3 * 32767^2 = 3 221 028 867.  TensorField: float32 points (float64 is taken to float32 first), d = (dx*dx + dy*dy)
    + dz*dz with dx = q.x - p.x, every operation rounded to float32 on its own, never contracted into an FMA; returned as
    float32; finite coordinates are a precondition and are not checked.

    max_squared_distance: None, or the largest distance that qualifies -- a Python int >= 0 for a SparseTensor, a Python float
    >= 0 (taken to float32) for a TensorField; the boundary is included (d2 <= cap, on the values above).  Slots for which no
    row qualifies hold idx = -1 and d2 = -1 (int64) / +inf (float32), after all the qualifying slots: mask before indexing
    (x.F[idx] with idx = -1 reads the LAST row).  Without a cap the result never contains -1.

    ValueError: k that is not an int in range; k larger than the smallest sample of x that has queries (naming the sample and
    its size -- with a cap too, one rule; the lengths are the cached batch_lengths, no new host read); a cap of the wrong type
    for the kind, or negative; more than 65535 samples.  TypeError: an unsupported x.  An empty x or empty queries give empty
    [0, k] / [B, 0, k] results.  Host reads, each cached with the coordinate set or field: the segment lengths, the batch
    indices present (the third form only) and the extent.

    Device tensors: csrc/knn.hip -- the support set is read where it is held and packed once in segment order, then one workgroup
    takes ms3d_knn_queries_per_group() queries of one sample, a thread a query, and streams the sample through LDS in tiles of
    ms3d_knn_rows_per_tile() rows; a thread's list of its k smallest 64-bit keys, (distance bits << 32) | caller row, lives in LDS; no
    atomics, no waiting between workgroups.  The queries are packed and the results put back into the caller's order by torch
    gathers.  CPU tensors: the same rule as a torch expression (_knn_torch), at most 2^22 (query, row) pairs at a time.  The
    index is not differentiable: gradients reach x.F through x.F[idx].
    Out of scope: spatial acceleration (a grid or hash walk), mixed voxel / point queries, other metrics (pooling, weighted sums
    and interpolation over the index: knn_map with neighbor_pool / neighbor_sum / knn_interpolate), a different k per query, k above 64, float16 or float64 distances, gradients with respect to the coordinates,
    the first-k-inside-the-radius order of a ball query (the cap keeps the nearest-first order)."""
    name = "knn_query"
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _KNN_MAX_K:
        raise ValueError(f"{name}: k must be a Python int with 1 <= k <= {_KNN_MAX_K}, got {k!r}")
    sup = _SupportSet(x, name, "x")
    group = sup.group
    integer = sup.kind is SparseTensor
    cap = max_squared_distance
    if cap is not None:
        if integer and (isinstance(cap, bool) or not isinstance(cap, int)):
            raise ValueError(f"{name}: max_squared_distance must be a Python int >= 0 for a SparseTensor (its distances are exact "
                             f"integers), got {cap!r}")
        if not integer and not isinstance(cap, float):
            raise ValueError(f"{name}: max_squared_distance must be a Python float >= 0 for a TensorField, got {cap!r}")
        if not cap >= 0:
            raise ValueError(f"{name}: max_squared_distance must be >= 0, got {cap!r}")
        cap = min(cap, 2 ** 32 - 1) if integer else float(np.float32(cap))       # no distance is above 2^32 - 1
    dev, B = sup.data.device, group.B
    d2_dtype = torch.int64 if integer else torch.float32
    shape, pos = None, None              # the result's leading shape; the caller's position of every packed query, or None

    if queries is None:
        if sup.V == 0:
            return torch.empty((0, k), dtype=torch.int64, device=dev), torch.empty((0, k), dtype=d2_dtype, device=dev)
        q_words, q_start, q_counts = sup.words(group.order, group.seg_of_row[group.order]), group.seg_start, group.lengths
        pos = sup.caller_of_order()
    elif torch.is_tensor(queries):
        if queries.dtype != torch.int64:
            raise ValueError(f"{name}: queries must be an int64 tensor [B, M] of caller rows of x, got {queries.dtype}")
        if queries.dim() != 2 or queries.size(0) != B:
            raise ValueError(f"{name}: queries must have shape [B, M] with B = {B}, the samples of x, got {list(queries.shape)}")
        M = queries.size(1)
        shape = (B, M)
        if B * M == 0:
            return torch.empty((B, M, k), dtype=torch.int64, device=dev), torch.empty((B, M, k), dtype=d2_dtype, device=dev)
        queries = queries.to(dev)
        held, inside = group.held_rows(queries)
        if not bool(inside.all()):                               # the one host read of this form
            b, j = (int(v) for v in (~inside).nonzero()[0])
            raise ValueError(f"{name}: queries[{b}, {j}] = {int(queries[b, j])} is not a row of sample {b}")
        q_words = sup.words(held.reshape(-1), torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(M))
        q_start, q_counts = torch.arange(B + 1, dtype=torch.int32, device=dev) * M, (M,) * B
    elif isinstance(queries, (SparseTensor, TensorField)):
        if not isinstance(queries, sup.kind):
            raise TypeError(f"{name}: mixed kinds -- x is a {sup.kind.__name__} and queries a {type(queries).__name__}; voxels "
                            "query voxels and points query points")
        qs = _SupportSet(queries, name, "queries")
        if qs.data.device != dev:
            raise ValueError(f"{name}: x is on {dev} and queries on {qs.data.device}")
        if qs.V == 0:
            return torch.empty((0, k), dtype=torch.int64, device=dev), torch.empty((0, k), dtype=d2_dtype, device=dev)
        segment_of = {bi: s for s, bi in enumerate(group.indices)}
        absent = [bi for bi in qs.group.indices if bi not in segment_of]
        if absent:
            raise ValueError(f"{name}: batch index {absent[0]} is present in queries and absent from x")
        target = [segment_of[bi] for bi in qs.group.indices]         # ascending, as both lists are
        counts = [0] * B
        for s, n in zip(target, qs.group.lengths):
            counts[s] = n
        starts = [0]
        for n in counts:
            starts.append(starts[-1] + n)
        lut = torch.tensor(target, dtype=torch.int32, device=dev)
        q_words = qs.words(qs.group.order, lut[qs.group.seg_of_row[qs.group.order].long()])
        q_start, q_counts = torch.tensor(starts, dtype=torch.int32, device=dev), tuple(counts)
        pos = qs.caller_of_order()
    else:
        raise ValueError(f"{name}: queries must be None, an int64 tensor [B, M] of caller rows of x or a {sup.kind.__name__} "
                         f"like x, got {type(queries).__name__}")

    asked = [s for s in range(B) if q_counts[s]]
    small = min(asked, key=group.lengths.__getitem__)
    if k > group.lengths[small]:
        raise ValueError(f"{name}: k = {k} is larger than sample {small}, which has {group.lengths[small]} rows")
    if B > _FPS_MAX_B:
        raise ValueError(f"{name}: B = {B} is above the kernel's limit of {_FPS_MAX_B}")

    if not sup.data.is_cuda:
        batch = x.C[:, 0].long()
        points = x.C[:, 1:].long() if integer else sup.data[:, 1:]
        qpoints = q_words[:, 1:].long() if integer else q_words.view(torch.float32)[:, 1:]
        idx, d2 = _knn_torch(points, batch, group.lengths, qpoints, q_counts, k, cap)
    else:
        be = get_backend()
        if not hasattr(be, "knn"):
            raise NotImplementedError(f"{name} on device tensors needs the HIP backend (ms3d_knn_i32)")
        idx, d2 = be.knn(sup.data, group, q_words, q_start.contiguous(), max(q_counts), k, cap)
        if integer:
            d2 = torch.where(idx < 0, -1, d2.long() & 0xffffffff)
    if pos is not None:
        idx, d2 = torch.empty_like(idx).index_copy_(0, pos, idx), torch.empty_like(d2).index_copy_(0, pos, d2)
    if shape is not None:
        idx, d2 = idx.view(*shape, k), d2.view(*shape, k)
    return idx, d2


NeighborMap = NeighbourGroup             # the public name of the record (backend.NeighbourGroup)


def _nbr_set(t):
    """what a NeighborMap remembers of a SparseTensor / TensorField: (the token its check compares, features as held -> a
    tensor of that set, its BatchGroup)"""
    if isinstance(t, SparseTensor):
        cm, ts = t.coordinate_manager, t.tensor_stride
        return (cm, ts), lambda feats: SparseTensor(feats, coordinate_manager=cm, tensor_stride=ts), cm.batch_group(ts)
    points, mode, shared = t._C, t.quantization_mode, t._shared

    def like(feats):                     # TensorField._like without keeping t's features alive
        f = TensorField.__new__(TensorField)
        f._F, f._C, f.quantization_mode, f._shared = feats, points, mode, shared
        return f
    return (shared, None), like, t._batch_group()


def knn_map(x, k, queries=None, max_squared_distance=None):
    """knn_query(x, k, queries, max_squared_distance) wrapped as a NeighborMap: the record ME.neighbor_pool, neighbor_sum,
    knn_interpolate and neighbor_attention read.  It remembers references to the position tensors of both sides (for
    NeighborMap.relative_positions(); no copies), the support set (x's coordinate set or field) and the target the results live on:
    x's own set (queries=None), y's set (a SparseTensor / TensorField y), or none -- plain [B, M, C] results -- for an int64
    [B, M] tensor of picks.  The index is translated into the rows as both sets HOLD them here, once, by torch gathers; the
    transposed table of the backward is made on first use and kept, so every layer over one graph shares it.  Arguments,
    refusals and host reads are knn_query's."""
    idx, d2 = knn_query(x, k, queries, max_squared_distance)
    support, wrap, group = _nbr_set(x)
    data = _SupportSet(x, "knn_map", "x").data               # positions as held: references, for relative_positions()
    row_map = row_held_of = None
    if queries is None:
        target, token, positions = group, support, (data, data, None)
    elif torch.is_tensor(queries):
        target, wrap, token = None, None, (None, None)
        held = queries.to(data.device).reshape(-1).clamp(0, max(group.V - 1, 0))
        positions = (data, data, held if group.held_of is None else group.held_of[held])
    else:
        token, wrap, target = _nbr_set(queries)
        positions = (data, _SupportSet(queries, "knn_map", "queries").data, None)
    if target is not None and target.row_map is not None:
        row_map, row_held_of = target.row_map, target.held_of
    return NeighbourGroup(idx, group.V, d2, held_of=group.held_of, row_map=row_map, row_held_of=row_held_of, support=support,
                          wrap=wrap, target=token, positions=positions)


def _dense_input(x, format, device):
    if not torch.is_tensor(x) or x.dim() != 5:
        nd = x.dim() if torch.is_tensor(x) else None
        raise NotImplementedError(f"to_sparse of a {nd}-D tensor (dimension={None if nd is None else nd - 2}): only 3-D sparse "
                                  "tensors are supported, the input is [B, C, X, Y, Z]")
    if format is None:
        format = "BCXXX"
    if format not in ("BCXXX", "BXXXC"):
        raise NotImplementedError(f"format={format!r}: 'BCXXX' (the default) or 'BXXXC'")
    if device is not None:
        x = x.to(device)
    if x.dtype != torch.float32:
        x = x.float()
    if format == "BXXXC":
        x = x.permute(0, 4, 1, 2, 3)      # channels-last: one contiguous copy below, then the same kernels
    return x.contiguous()


def _to_sparse(x, format, coordinates, device, keep_all):
    x = _dense_input(x, format, device)
    be = get_backend()
    if not (hasattr(be, "dense_occupancy") and hasattr(be, "dense_cell_map")):
        raise NotImplementedError("to_sparse needs the HIP backend (ms3d_dense_occupancy)")
    B, _, X, Y, Z = x.shape
    if B * X * Y * Z > 2 ** 31 - 1:
        raise NotImplementedError(f"to_sparse: a grid of {[B, X, Y, Z]} (B, X, Y, Z) has more than 2^31 - 1 cells")
    if coordinates is None:
        _, coords, cells = be.dense_occupancy(x.detach(), keep_all)
    else:
        if coordinates.dim() != 2 or coordinates.size(1) != 4 or coordinates.is_floating_point():
            raise ValueError(f"to_sparse: coordinates must be int [n, 4] (b, x, y, z), got {list(coordinates.shape)} "
                             f"{coordinates.dtype}")
        coords = coordinates.to(device=x.device, dtype=torch.int32).contiguous()
        _, cells, (outside, _, _) = be.dense_cell_map(coords, (0, 0, 0), 1, (B, X, Y, Z))
        if outside:
            raise ValueError(f"to_sparse: {outside} coordinates lie outside the dense tensor {[B, X, Y, Z]} (B, X, Y, Z)")
    cm = CoordinateManager(coords, spatial_sort=coords.size(0) >= _SORT_MIN_ROWS)
    if cm.perm is not None:                # read the rows straight into the order the manager holds them in
        cells = cells[cm.perm].contiguous()
    return SparseTensor(Fn.dense_gather(x, cells, cm.coords[1]), coordinate_manager=cm)


def to_sparse(x, format=None, coordinates=None, device=None):
    """SparseTensor (tensor stride 1, a new manager) of a dense x [B, C, X, Y, Z] (format "BCXXX", the default) or
    [B, X, Y, Z, C] ("BXXXC": permuted and copied contiguous once, then the same kernels): the cells where ANY channel is
    non-zero (NaN counts as non-zero, -0.0 does not), coordinates (b, x, y, z) with origin 0, rows in ascending (b, x, y, z)
    order -- the order of torch.nonzero on the mask, and the order the caller sees; a set of at least _SORT_MIN_ROWS rows is
    Morton-sorted internally like any SparseTensor.  coordinates (int [n, 4]): exactly those cells, in the caller's order (one
    named twice gives two equal rows); coordinates outside x raise ValueError.  Gradients flow to x (zeros at the cells not
    kept).  An input that is not 5-D raises NotImplementedError."""
    return _to_sparse(x, format, coordinates, device, False)


def to_sparse_all(x, format=None):
    """to_sparse that keeps EVERY cell of x: B * X * Y * Z rows in ascending (b, x, y, z) order"""
    return _to_sparse(x, format, None, None, True)


def union_op(op, *tensors):
    """op 0 sum (up to 16 operands), 1 subtract, 2 multiply (two) of SparseTensors on DIFFERENT coordinate sets of one tensor
    stride: the result lives on the union of the sets (CoordinateManager.union); where an operand lacks a coordinate the rule
    of csrc/setops.hip holds.  A pending BatchNorm / ReLU is materialised first."""
    first = tensors[0]
    ts, c = first.tensor_stride, first._F.size(1)
    for t in tensors[1:]:
        if t.tensor_stride != ts:
            raise ValueError(f"tensor strides {ts} and {t.tensor_stride} differ: operands of a union live on one tensor stride")
        if t._F.size(1) != c:
            raise ValueError(f"channel counts {c} and {t._F.size(1)} differ")
    if len(tensors) > 16:
        raise NotImplementedError(f"a union of {len(tensors)} tensors: at most 16")
    cm, in_rows, out_rows, n = first.coordinate_manager.union(ts, [t.coordinate_manager for t in tensors[1:]])
    y = Fn.union_combine(op, in_rows, out_rows, n, [t._raw() for t in tensors])
    return SparseTensor(y, coordinate_manager=cm, tensor_stride=ts)


def cat(*tensors):
    """ME.cat: channel concat of tensors sharing one coordinate map (common.py:93)"""
    parts = [t._stats if (t._pending is None and torch.is_tensor(t._stats) and t._stats.numel() > 0) else None
             for t in tensors]
    # every part still carries the (sum, sum of squares) partials its convolution left behind: the statistics of the
    # concatenation are the parts' statistics side by side -- the BatchNorm that follows (ResidualBlock after the
    # U-Net's skip concat) finalizes them per part instead of running a statistics pass over the 2c-wide rows
    stats = tuple(parts) if all(p is not None for p in parts) else None
    return tensors[0]._like(torch.cat([t._raw() for t in tensors], dim=1), stats=stats)
