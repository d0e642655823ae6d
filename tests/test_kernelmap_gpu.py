"""GPU: kernel, stride and origin maps as index pairs -- the export kernels (csrc/kmap_pairs.hip) against plain loops, the
maps CoordinateManager hands out against the coordinate equation on the rows the CALLER sees, and the maps against the layers
they describe.

Yardsticks (tests/kmap_ref.py): `pairs_np`, two nested Python loops over a table; `visible_pairs`, a Python dictionary over
x.C / y.C.  Tables, pair lists and row maps are compared exactly.  A convolution rebuilt in float64 from kernel_map and
index_add is held to the bound the region tests hold the same layers to against their dense yardstick: RTOL = 1e-4 of the
tensor's largest magnitude (tests/test_region_gpu.py:24, `rel_err` at :67-69).  Sum pooling and the global sum behind origin_map
run on integer-valued features and are compared with torch.equal."""
import ctypes as C

import numpy as np
import pytest
import torch

from kmap_ref import pairs_np, visible_pairs
from region_ref import cross_offsets, cube_offsets, custom_offsets
from sparse_ref import random_sparse

pytestmark = pytest.mark.gpu
RTOL = 1e-4          # tests/test_region_gpu.py:24
DEV = "cuda"
SENTINEL = -0x5A5A5A5A5A5A5A5A
GUARD = 64
CUSTOM = [(0, 0, 0), (1, 0, 0), (0, 2, -1), (-1, 0, 0), (3, 3, 3)]          # not its own mirror image (R4 of the region tests)


@pytest.fixture(scope="module")
def ME():
    import minsu3d_amd.MinkowskiEngine as me
    return me


@pytest.fixture(scope="module")
def be():
    from minsu3d_amd.backend import get_backend
    return get_backend()


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def check(name, got, want, tol):
    assert tuple(got.shape) == tuple(want.shape), (name, tuple(got.shape), tuple(want.shape))
    e = rel_err(got, want)
    print(f"{name}: rel err {e:.3e} (bound {tol:.0e})")
    assert e <= tol, (name, e)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ---------------------------------------------------------------------------------------------- 1. the entry points
def export(be, nbr, K, vout, vin, out_order=None, in_rename=None):
    """the two entry points called as a C caller would, `pairs` sized from the device count plus GUARD sentinel columns per
    row -> (pairs [2, P], start [K + 1]) after checking that no guard column was written"""
    from minsu3d_amd import _lib
    lib = be.lib
    start = torch.full((K + 1,), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.ms3d_kmap_pairs_workspace_bytes(K, vout), dtype=torch.uint8, device=DEV)
    args = (_lib.ptr(nbr), K, vout, vin, _lib.ptr(out_order))
    rc = lib.ms3d_kmap_pairs_count(*args, _lib.ptr(start), _lib.ptr(ws), C.c_size_t(ws.numel()), _lib.stream_handle())
    assert rc == 0, rc
    P = int(start[K].item())
    assert 0 <= P <= K * vout
    buf = torch.full((2, P + GUARD), SENTINEL, dtype=torch.int64, device=DEV)
    rc = lib.ms3d_kmap_pairs_fill(*args, _lib.ptr(in_rename), _lib.ptr(buf), C.c_longlong(P + GUARD), _lib.ptr(ws),
                                  C.c_size_t(ws.numel()), _lib.stream_handle())
    assert rc == 0, rc
    assert bool((buf[:, P:] == SENTINEL).all()), "a column past P was written"
    return buf[:, :P].clone(), start


def filling(rng, name, K, vout, vin):
    valid = rng.integers(0, vin, (K, vout))
    if name == "none":
        keep = np.zeros((K, vout), bool)
    elif name == "all":
        keep = np.ones((K, vout), bool)
    elif name == "one per column":
        keep = np.zeros((K, vout), bool)
        keep[rng.integers(0, K, vout), np.arange(vout)] = True
    else:
        keep = rng.random((K, vout)) < 0.3
        if name == "gap":                                   # an offset with no pair between two that have some
            if K >= 3:
                keep[K // 2] = False
                keep[K // 2 - 1, 0] = keep[K // 2 + 1, vout - 1] = True
        elif name == "ends":                                # the first and the last offset empty
            keep[0] = keep[K - 1] = False
    return np.where(keep, valid, -1).astype(np.int32)


FILLINGS = ("none", "all", "one per column", "30 %", "gap", "ends")


@pytest.mark.parametrize("fill", FILLINGS)
@pytest.mark.parametrize("K", [1, 8, 27, 254])
def test_entry_points_exact(be, K, fill):
    R = be.lib.ms3d_kmap_pairs_rows()
    assert R >= 128 and R % 64 == 0
    rng = np.random.default_rng(1000 * K + FILLINGS.index(fill))
    for vout in (1, 63, 64, 65, 255, 256, 257, R - 1, R, R + 1, 3 * R + 1):
        vin = vout + 5
        nbr_np = filling(rng, fill, K, vout, vin)
        nbr = dev(nbr_np)
        for renamed in (False, True):
            order_np = rng.permutation(vout).astype(np.int32) if renamed else None
            rename_np = rng.permutation(vin).astype(np.int32) if renamed else None
            order = None if order_np is None else dev(order_np)
            rename = None if rename_np is None else dev(rename_np)
            want_pairs, want_start = pairs_np(nbr_np, order_np, rename_np)
            pairs, start = export(be, nbr, K, vout, vin, order, rename)
            tag = (K, fill, vout, renamed)
            assert pairs.dtype == torch.int64 and start.dtype == torch.int32
            assert torch.equal(start.cpu(), torch.from_numpy(want_start)), tag
            assert torch.equal(pairs.cpu(), torch.from_numpy(want_pairs)), tag
            again, start2 = export(be, nbr, K, vout, vin, order, rename)          # the same bytes on every run
            assert torch.equal(again, pairs) and torch.equal(start2, start), tag
    if fill == "none":
        assert pairs.shape == (2, 0)


def test_entries_past_vin_are_not_followed_and_the_binding(be):
    """an entry >= Vin counts as -1 (in_rename is Vin long: following it would read past the array); the backend's binding
    returns the same lists, and an empty table gives zeros"""
    rng = np.random.default_rng(5)
    K, vout, vin = 27, 1500, 700
    nbr_np = np.where(rng.random((K, vout)) < 0.5, rng.integers(0, 2 * vin, (K, vout)), -1).astype(np.int32)
    order_np, rename_np = rng.permutation(vout).astype(np.int32), rng.permutation(vin).astype(np.int32)
    want_pairs, want_start = pairs_np(nbr_np, order_np, rename_np, vin=vin)
    assert 0 < want_start[-1] < (nbr_np >= 0).sum()
    pairs, start = export(be, dev(nbr_np), K, vout, vin, dev(order_np), dev(rename_np))
    assert torch.equal(pairs.cpu(), torch.from_numpy(want_pairs)) and torch.equal(start.cpu(), torch.from_numpy(want_start))
    p2, s2 = be.kmap_pairs(dev(nbr_np), K, vout, vin, dev(order_np), dev(rename_np))
    assert torch.equal(p2, pairs) and torch.equal(s2, start) and tuple(p2.shape) == (2, int(want_start[-1]))
    p3, s3 = be.kmap_pairs(torch.full((K, 1), -1, dtype=torch.int32, device=DEV), K, 0, vin)
    assert tuple(p3.shape) == (2, 0) and p3.dtype == torch.int64 and s3.tolist() == [0] * (K + 1)
    p4, s4 = be.kmap_pairs(dev(nbr_np), K, vout, 0)                                  # no input rows: nothing is valid
    assert tuple(p4.shape) == (2, 0) and s4.tolist() == [0] * (K + 1)


# ---------------------------------------------------------------------------------------------- 2. through the manager
def cloud(ME, rng, n=400, grid=12, C_=4):
    coords, feats = random_sparse(rng, B=2, grid=grid, n=n, C=C_)
    p = rng.permutation(n)
    return ME.SparseTensor(dev(feats[p]), coordinates=dev(coords[p]))


def at_stride(ME, x, ts, C_=4, rng=None):
    """a tensor on the set of tensor stride ts of x's manager (made through CoordinateManager.stride)"""
    if ts == x.tensor_stride:
        return x
    cm = x.coordinate_manager
    key = cm.stride(x.coordinate_map_key, ts // x.tensor_stride)
    v = cm.get_coordinates(key).size(0)
    f = torch.ones(v, C_) if rng is None else torch.from_numpy(rng.standard_normal((v, C_)).astype(np.float32))
    return ME.SparseTensor(f.to(DEV), coordinate_map_key=key)


def check_map(tag, km, x, y, offsets, transposed=False):
    """every pair satisfies the coordinate equation on x.C / y.C, the per-offset counts are the dictionary map's -- and, since
    the output row ascends inside an entry, the entries are the dictionary map's"""
    cin, cout = x.C.cpu().numpy().astype(np.int64), y.C.cpu().numpy().astype(np.int64)
    offsets = np.asarray(offsets, np.int64)
    want = visible_pairs(cin, cout, offsets, transposed)
    assert list(km) == sorted(km) and all(v.size(1) > 0 for v in km.values()), tag
    sign = -1 if transposed else 1
    for k, p in km.items():
        assert p.dtype == torch.int64 and p.dim() == 2 and p.size(0) == 2, (tag, k)
        i, o = p.cpu().numpy()
        assert np.array_equal(cout[o][:, 1:] + sign * offsets[k], cin[i][:, 1:]), (tag, k)
        assert np.array_equal(cout[o][:, 0], cin[i][:, 0]), (tag, k)
    assert {k: v.size(1) for k, v in km.items()} == {k: v.shape[1] for k, v in want.items()}, tag
    for k, p in km.items():
        assert np.array_equal(p.cpu().numpy(), want[k]), (tag, k)
    return sum(v.size(1) for v in km.values())


def target_rows(rng, natural, ts):
    """distinct rows on the lattice of tensor stride ts: rows of the natural set, shifted copies beside it, rows far away"""
    nat = natural.cpu().numpy()
    p = rng.permutation(len(nat))
    near = nat[p[:80]] + np.array([0, ts, 0, -ts], np.int32)
    far = nat[p[80:100]] + np.array([0, 2048, 0, 0], np.int32)
    rows = np.concatenate([nat[p[100:220]], near, far])
    _, first = np.unique(rows, axis=0, return_index=True)
    rows = rows[np.sort(first)]
    return rows[rng.permutation(len(rows))].astype(np.int32)


def run_geometries(ME, x0, rng, strides=(1, 2)):
    """the issue's list on one cloud -> the number of pairs seen (so that a caller can tell the maps were not empty)"""
    from minsu3d_amd.MinkowskiEngine.tensor import target_key
    cm = x0.coordinate_manager
    total = 0
    for ts in strides:
        x = at_stride(ME, x0, ts)
        up = at_stride(ME, x0, 2 * ts)
        for ks, dil in ((3, 1), (5, 1), (3, 2)):
            total += check_map(f"({ks},1,{dil}) ts{ts}", cm.kernel_map(x, x, kernel_size=ks, dilation=dil), x, x,
                               cube_offsets(ks, dil, ts))
        for ks in (2, 3):
            total += check_map(f"({ks},2,1) ts{ts}", cm.kernel_map(x, up, stride=2, kernel_size=ks), x, up, cube_offsets(ks, 1, ts))
            total += check_map(f"transposed ({ks},2,1) ts{ts}",
                               cm.kernel_map(up, x, stride=2, kernel_size=ks, is_transpose=True), up, x,
                               cube_offsets(ks, 1, ts), transposed=True)
        total += check_map(f"cross ts{ts}", cm.kernel_map(x, x, kernel_size=3, region_type=ME.RegionType.HYPER_CROSS), x, x,
                           cross_offsets(3, 1, ts))
        g = ME.KernelGenerator(region_type=ME.RegionType.CUSTOM, region_offsets=torch.tensor(CUSTOM, dtype=torch.int32), dimension=3)
        km = cm.kernel_map(x, x, kernel_generator=g)
        total += check_map(f"custom ts{ts}", km, x, x, custom_offsets(CUSTOM, ts))
        assert km is cm.kernel_map(x, x, region_type=ME.RegionType.CUSTOM, region_offsets=torch.tensor(CUSTOM))
        assert km is cm.kernel_map(x, x, is_pool=True, kernel_generator=g)
        # a `coordinates=` target on another manager
        tgt = target_rows(rng, x.C, ts)
        tkey = target_key(torch.from_numpy(tgt), ts, x.device)
        assert tkey.coordinate_manager is not cm
        y = ME.SparseTensor(torch.zeros(len(tgt), 1, device=DEV), coordinate_map_key=tkey)
        assert np.array_equal(y.C.cpu().numpy(), tgt)
        total += check_map(f"target ts{ts}", cm.kernel_map(x, tkey, kernel_size=3), x, y, cube_offsets(3, 1, ts))
        # an expand_coordinates output
        conv = ME.MinkowskiConvolution(x.F.size(1), 3, kernel_size=3, dimension=3, expand_coordinates=True).to(DEV)
        e = conv(x)
        assert e.coordinate_manager is not cm and e.C.size(0) > x.C.size(0)
        total += check_map(f"expand ts{ts}", cm.kernel_map(x, e, kernel_size=3), x, e, cube_offsets(3, 1, ts))
    return total


def test_manager_maps_in_the_callers_numbering(ME):
    rng = np.random.default_rng(17)
    x = cloud(ME, rng)
    assert x.coordinate_manager.perm is None
    assert run_geometries(ME, x, rng) > 10000


def test_manager_maps_on_a_morton_sorted_manager(ME, monkeypatch):
    """the rows a sorted manager HOLDS are not the rows of x.C: this fails if the renaming is dropped"""
    from minsu3d_amd.MinkowskiEngine import tensor as T
    monkeypatch.setattr(T, "_SORT_MIN_ROWS", 4096)
    rng = np.random.default_rng(19)
    x = cloud(ME, rng, n=4100, grid=24)
    cm = x.coordinate_manager
    assert cm.perm is not None and not torch.equal(cm.perm, torch.arange(4100, device=DEV))
    assert run_geometries(ME, x, rng, strides=(1,)) > 100000
    pairs, start = cm.kernel_map_pairs(x, x, kernel_size=3)
    held = cm.kernel_map(1, 3)[0]                            # the engine's table, rows as held
    kk, oo = torch.nonzero(held >= 0, as_tuple=True)
    assert pairs.size(1) == kk.numel() == int(start[-1])
    assert not torch.equal(pairs, torch.stack([held[kk, oo].long(), oo]))
    # ... and it is that table, renamed: (perm[entry], perm[column]) as a set of pairs per offset
    renamed = torch.stack([cm.perm[held[kk, oo].long()], cm.perm[oo]])
    s = start.tolist()
    for k in (0, 13, 26):
        a, b = pairs[:, s[k]:s[k + 1]], renamed[:, kk == k]
        assert torch.equal(a, b[:, torch.argsort(b[1])])


# ---------------------------------------------------------------------------------------------- 3. the maps are the layers
def rebuild(km, xF, W, vout, bias=None):
    x64 = xF.detach().double()
    W64 = W.detach().double().reshape(-1, x64.size(1), W.shape[-1])          # [K, Cin, Cout]
    y = torch.zeros((vout, W64.size(2)), dtype=torch.float64, device=xF.device)
    for k, (i, o) in km.items():
        y.index_add_(0, o, x64[i] @ W64[k])
    return y if bias is None else y + bias.detach().double().view(1, -1)


@pytest.mark.parametrize("C_", [5, 16])
@pytest.mark.parametrize("sorted_", [False, True])
def test_convolutions_rebuilt_from_the_maps(ME, monkeypatch, C_, sorted_):
    from minsu3d_amd.MinkowskiEngine import tensor as T
    rng = np.random.default_rng(23 + C_)
    if sorted_:
        monkeypatch.setattr(T, "_SORT_MIN_ROWS", 4096)
    x = cloud(ME, rng, n=4100 if sorted_ else 400, grid=24 if sorted_ else 12, C_=C_)
    cm = x.coordinate_manager
    assert (cm.perm is not None) == sorted_
    cout = C_ + 3
    conv = ME.MinkowskiConvolution(C_, cout, kernel_size=3, bias=True, dimension=3).to(DEV)
    y = conv(x)
    check(f"cube C{C_}", y.F, rebuild(cm.kernel_map(x, y, kernel_size=3), x.F, conv.kernel, y.F.size(0), conv.bias), RTOL)
    g = ME.KernelGenerator(3, region_type=ME.RegionType.HYPER_CROSS, dimension=3)
    cross = ME.MinkowskiConvolution(C_, cout, kernel_generator=g, bias=True, dimension=3).to(DEV)
    y = cross(x)
    check(f"cross C{C_}", y.F, rebuild(cm.kernel_map(x, y, kernel_generator=g), x.F, cross.kernel, y.F.size(0), cross.bias), RTOL)
    down = ME.MinkowskiConvolution(C_, cout, kernel_size=3, stride=2, bias=True, dimension=3).to(DEV)
    d = down(x)
    assert d.tensor_stride == 2 and d.coordinate_map_key == cm.stride(x, 2)
    check(f"stride 2 C{C_}", d.F, rebuild(cm.kernel_map(x, d, stride=2, kernel_size=3), x.F, down.kernel, d.F.size(0), down.bias),
          RTOL)
    up = ME.MinkowskiConvolutionTranspose(cout, C_, kernel_size=2, stride=2, bias=True, dimension=3).to(DEV)
    u = up(d)
    assert u.coordinate_map_key == x.coordinate_map_key
    km = cm.kernel_map(d, u, stride=2, kernel_size=2, is_transpose=True)
    check(f"transposed C{C_}", u.F, rebuild(km, d.F, up.kernel, u.F.size(0), up.bias), RTOL)


@pytest.mark.parametrize("C_", [5, 16])
def test_sum_pooling_rebuilt_from_the_maps_exactly(ME, C_):
    """integer-valued features: a sum of at most 27 small integers is exact in float32 in any order"""
    rng = np.random.default_rng(29 + C_)
    x = cloud(ME, rng, C_=C_)
    x = ME.SparseTensor(dev(rng.integers(-8, 9, (400, C_)).astype(np.float32)), coordinate_map_key=x.coordinate_map_key)
    cm = x.coordinate_manager
    for ks, stride in ((3, 1), (2, 2), (3, 2)):
        y = ME.MinkowskiSumPooling(ks, stride=stride, dimension=3)(x)
        km = cm.kernel_map(x, y, stride=stride, kernel_size=ks, is_pool=True)
        want = torch.zeros_like(y.F)
        for k, (i, o) in km.items():
            want.index_add_(0, o, x.F[i])
        assert torch.equal(y.F, want), (ks, stride)


@pytest.mark.parametrize("sorted_", [False, True])
def test_origin_map_is_the_global_pooling(ME, monkeypatch, sorted_):
    """What _GlobalPoolBase emits, checked: one row per batch index PRESENT, ascending -- so the output row of a voxel is the
    rank of its batch index, which is what origin_map names.  Integer-valued features; the global sum is computed as mean *
    count, which is exact when the sample sizes are powers of two, so they are (256 and 128 rows; 4096 and 512 on the sorted
    manager), and the batch indices 0 and 3 leave a gap."""
    from minsu3d_amd.MinkowskiEngine import tensor as T
    rng = np.random.default_rng(31)
    if sorted_:
        monkeypatch.setattr(T, "_SORT_MIN_ROWS", 4096)
    sizes = {0: 4096, 3: 512} if sorted_ else {0: 256, 3: 128}
    grid = 24 if sorted_ else 12
    rows = []
    for b, n in sizes.items():
        cells = rng.permutation(grid ** 3)[:n]
        rows.append(np.stack([np.full(n, b), cells // grid ** 2, cells // grid % grid, cells % grid], 1))
    coords = np.concatenate(rows).astype(np.int32)
    coords = coords[rng.permutation(len(coords))]
    feats = rng.integers(-8, 9, (len(coords), 6)).astype(np.float32)
    x = ME.SparseTensor(dev(feats), coordinates=dev(coords))
    cm = x.coordinate_manager
    assert (cm.perm is not None) == sorted_
    om = cm.origin_map(x.coordinate_map_key)
    assert list(om) == [0] and om[0].dtype == torch.int64 and tuple(om[0].shape) == (2, len(coords))
    rows_in, rows_out = om[0]
    assert torch.equal(rows_in, torch.arange(len(coords), device=DEV))
    assert np.array_equal(rows_out.cpu().numpy(), np.where(coords[:, 0] == 0, 0, 1))
    g = ME.MinkowskiGlobalSumPooling()(x)
    assert g.C[:, 0].tolist() == [0, 3]
    want = torch.zeros_like(g.F).index_add_(0, rows_out, x.F[rows_in])
    assert torch.equal(g.F, want)
    assert torch.equal(g.C[rows_out, 0], x.C[rows_in, 0])
    assert cm.origin_map(x) is om
    # a coarser set of the same manager
    k2 = cm.stride(x, 2)
    o2 = cm.origin_map(k2)[0]
    c2 = cm.get_coordinates(k2)
    assert torch.equal(o2[0], torch.arange(c2.size(0), device=DEV)) and torch.equal(o2[1], (c2[:, 0] == 3).long())


# ---------------------------------------------------------------------------------------------- 4. stride, stride_map
@pytest.mark.parametrize("sorted_", [False, True])
def test_stride_and_stride_map(ME, monkeypatch, sorted_):
    from minsu3d_amd.MinkowskiEngine import tensor as T
    rng = np.random.default_rng(37)
    if sorted_:
        monkeypatch.setattr(T, "_SORT_MIN_ROWS", 4096)
    x = cloud(ME, rng, n=4100 if sorted_ else 400, grid=24 if sorted_ else 12)
    cm, k1 = x.coordinate_manager, x.coordinate_map_key
    assert (cm.perm is not None) == sorted_
    assert 2 not in cm.coords and 4 not in cm.coords
    k4 = cm.stride(k1, 4)                                    # makes the levels in between
    k2 = cm.stride(k1, 2)
    assert k4.tensor_stride == 4 and k2.tensor_stride == 2 and k4 == cm.stride(k2, 2) and cm.stride(k2, 1) is k2
    assert 2 in cm.coords and 4 in cm.coords and k4.coordinate_manager is cm
    c = {1: x.C.long(), 2: cm.get_coordinates(k2).long(), 4: cm.get_coordinates(k4).long()}
    maps = {}
    for (a, ka), (b, kb) in (((1, k1), (2, k2)), ((2, k2), (4, k4)), ((1, k1), (4, k4))):
        rin, rout = maps[(a, b)] = cm.stride_map(ka, kb)
        assert rin.dtype == rout.dtype == torch.int64 and rin.shape == rout.shape == (c[a].size(0),)
        assert torch.equal(rin, torch.arange(c[a].size(0), device=DEV))
        fine, coarse = c[a][rin], c[b][rout]
        assert torch.equal(coarse[:, 0], fine[:, 0])
        assert torch.equal(coarse[:, 1:], torch.div(fine[:, 1:], b, rounding_mode="floor") * b)
        assert cm.stride_map(ka, kb) is maps[(a, b)]
    assert torch.equal(maps[(1, 4)][1], maps[(2, 4)][1][maps[(1, 2)][1]])
    # negative coordinates floor towards -infinity
    neg = ME.SparseTensor(torch.ones(3, 1, device=DEV), coordinates=torch.tensor([[0, -1, -2, -3], [0, 0, 1, -4], [0, -5, 3, 2]],
                                                                                 dtype=torch.int32, device=DEV))
    ncm = neg.coordinate_manager
    rin, rout = ncm.stride_map(neg, ncm.stride(neg, 2))
    assert ncm.get_coordinates(2)[rout, 1:].tolist() == [[-2, -2, -4], [0, 0, -4], [-6, 2, 2]]
    # stride(key, 2) twice is the key of a tensor that went through two stride-2 layers
    down = ME.MinkowskiConvolution(4, 4, kernel_size=2, stride=2, dimension=3).to(DEV)
    fresh = ME.SparseTensor(x.F, coordinates=x.C.clone())
    fcm = fresh.coordinate_manager
    twice = fcm.stride(fcm.stride(fresh.coordinate_map_key, 2), 2)
    y = down(down(fresh))
    assert y.tensor_stride == 4 and y.coordinate_map_key == twice and hash(y.coordinate_map_key) == hash(twice)
    assert torch.equal(y.C, fcm.get_coordinates(twice))
    with pytest.raises(NotImplementedError, match="stride=3"):
        cm.stride(k1, 3)
    with pytest.raises(ValueError, match="COARSER"):
        cm.stride_map(k2, k1)
    with pytest.raises(ValueError, match="different coordinate managers"):
        cm.stride_map(k1, fcm.stride(fresh, 2))


# ---------------------------------------------------------------------------------------------- 5. the dict
def test_dict_holds_views_of_the_packed_lists_and_is_cached(ME):
    rng = np.random.default_rng(41)
    x = cloud(ME, rng)
    cm = x.coordinate_manager
    far = [(0, 0, 0), (100, 0, 0), (1, 0, 0), (0, 100, 0), (0, -1, 0)]          # offsets 1 and 3 reach nothing
    g = ME.KernelGenerator(region_type=ME.RegionType.CUSTOM, region_offsets=torch.tensor(far), dimension=3)
    km = cm.kernel_map(x, x, kernel_generator=g)
    pairs, start = cm.kernel_map_pairs(x, x, kernel_generator=g)
    assert list(km) == [0, 2, 4] and start.dtype == torch.int32 and start.is_cuda and tuple(start.shape) == (6,)
    s = start.tolist()
    assert s[0] == 0 and s[1] == s[2] == 400 and s[3] == s[4] and s[5] == pairs.size(1) and pairs.dtype == torch.int64
    for k, v in km.items():
        assert v._base is pairs and v.data_ptr() == pairs[:, s[k]:].data_ptr() and torch.equal(v, pairs[:, s[k]:s[k + 1]])
    assert torch.equal(km[0], torch.arange(400, device=DEV).expand(2, 400))
    assert cm.kernel_map(x, x, kernel_generator=g) is km and cm.kernel_map(x.coordinate_map_key, x, kernel_generator=g) is km
    again = cm.kernel_map_pairs(x, x, kernel_generator=g)
    assert again[0] is pairs and again[1] is start
    assert cm.kernel_map(x, x, kernel_size=3) is not km
    assert cm.kernel_map(x, x, kernel_size=3) is cm.kernel_map(x, x)          # the defaults
    # the engine form is where it was
    assert cm.kernel_map(1, 3)[0] is cm.k3(1) and len(cm.kernel_map(1, 3)) == 7
    # the lists onto another manager are the sixteen newest
    from minsu3d_amd.MinkowskiEngine.tensor import target_key
    tgt = torch.from_numpy(target_rows(rng, x.C, 1))
    tkey = target_key(tgt, 1, x.device)
    first = cm.kernel_map(x, tkey, kernel_size=3)
    assert cm.kernel_map(x, tkey, kernel_size=3) is first
    for dil in range(2, 19):
        cm.kernel_map(x, tkey, kernel_size=3, dilation=dil)
    assert len(cm._pair_lists_onto) == 16 and cm.kernel_map(x, tkey, kernel_size=3) is not first
