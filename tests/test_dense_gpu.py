"""GPU: the crossing between sparse rows and dense [B, C, X, Y, Z] tensors (csrc/dense.hip) -- SparseTensor.dense, to_sparse,
to_sparse_all, the three modules and the backward of each.

The yardstick is never this engine: torch on the CPU (tests/dense_ref.py) -- `d = zeros(shape); d[b, :, x, y, z] = F` for dense,
`mask.nonzero()` plus advanced indexing for to_sparse, autograd through those graphs under a random upstream gradient.  These
are copies and masked zeros, so every comparison is bit-exact (torch.equal on the whole tensor, absent cells included); the one
exception is the composed network check at the end, held to the project's bar of 1e-4 of the reference's largest magnitude.

Tile of the two feature kernels: one workgroup takes 64 consecutive cells of one batch index (scatter) or 64 consecutive list
entries (gather) and 32 channels.  Hence volumes X * Y * Z of 1 / 63 / 64 / 65 / 4097 (one less, exact, one more than a run;
many runs with a ragged tail), row counts of 63 / 64 / 65 (every cell of those volumes at B = 1) and channel counts of 1 / 3 /
31 / 32 / 33 / 64 / 66."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dense_ref import dense_reference, rows_at, to_sparse_reference

pytestmark = pytest.mark.gpu
CHANNELS = [1, 3, 31, 32, 33, 64, 66]
GRIDS = [(1, 1, 1), (3, 3, 7), (4, 4, 4), (5, 13, 1), (17, 241, 1)]          # volumes 1, 63, 64, 65, 4097
OCCUPANCY = ["single", 0.1, "all"]


@pytest.fixture(scope="module")
def ME():
    import minsu3d_amd.MinkowskiEngine as me
    return me


@pytest.fixture(scope="module")
def be():
    from minsu3d_amd.backend import get_backend
    return get_backend()


def test_tile_is_what_the_shapes_assume(be):
    assert be.lib.ms3d_dense_tile_cells() == 64 and be.lib.ms3d_dense_tile_channels() == 32


# ---------------------------------------------------------------------------------------------- helpers
def cloud(rng, grid, batches, occupancy, origin=(0, 0, 0), step=1):
    """distinct int32 (b, x, y, z) rows in random order: per batch index of `batches` one cell ("single"), a share of the cells
    of the grid (at least one) or every cell ("all"), at origin + step * cell"""
    X, Y, Z = grid
    S = X * Y * Z
    rows = []
    for b in batches:
        if occupancy == "all":
            cells = np.arange(S)
        elif occupancy == "single":
            cells = rng.choice(S, size=1)
        else:
            cells = rng.choice(S, size=max(1, int(round(occupancy * S))), replace=False)
        x, rest = np.divmod(cells, Y * Z)
        y, z = np.divmod(rest, Z)
        xyz = np.stack([x, y, z], 1) * step + np.asarray(origin)
        rows.append(np.concatenate([np.full((cells.size, 1), b), xyz], 1))
    rows = np.concatenate(rows).astype(np.int32)
    return torch.from_numpy(rows[rng.permutation(rows.shape[0])].copy())


def feats_of(rng, V, C):
    return torch.from_numpy(rng.standard_normal((V, C)).astype(np.float32))


def sparse(ME, coords, feats, requires_grad=False):
    f = feats.cuda().requires_grad_(requires_grad)
    return ME.SparseTensor(f, coords.cuda()), f


BATCHES = [("B1", [0], None), ("B3 with 1 empty", [0, 2], None), ("B larger than present", [0, 1], 4)]


# ---------------------------------------------------------------------------------------------- 1. dense forward
@pytest.mark.parametrize("C", CHANNELS)
def test_dense_forward_exact(ME, C):
    rng = np.random.default_rng(C)
    for grid in GRIDS:
        for occ in OCCUPANCY:
            for tag, batches, B in BATCHES:
                coords = cloud(rng, grid, batches, occ)
                feats = feats_of(rng, coords.size(0), C)
                x, _ = sparse(ME, coords, feats)
                nb = max(batches) + 1 if B is None else B
                shape = (nb, C) + grid
                if B is None and occ == "all":
                    d, origin, stride = x.dense()                   # the extent is the grid
                else:
                    d, origin, stride = x.dense(shape=torch.Size(shape), min_coordinate=0)
                assert d.is_cuda and d.dtype == torch.float32 and tuple(d.shape) == shape, (grid, occ, tag)
                assert origin.tolist() == [[0, 0, 0]] and stride.tolist() == [1, 1, 1]
                assert torch.equal(d.cpu(), dense_reference(coords, feats, shape)), (grid, occ, tag)


def test_dense_writes_every_element_and_nothing_else(be):
    """the output lies between two guard bands inside one allocation; stale NaNs inside are overwritten, the bands untouched"""
    rng = np.random.default_rng(1)
    C, grid, B = 33, (5, 13, 1), 2
    coords = cloud(rng, grid, [0, 1], 0.1)
    feats = feats_of(rng, coords.size(0), C)
    cell_row, _, counts = be.dense_cell_map(coords.cuda(), (0, 0, 0), 1, (B,) + grid)
    assert counts == (0, 0, 0)
    want = dense_reference(coords, feats, (B, C) + grid)
    n, guard = want.numel(), 4096
    import ctypes
    from minsu3d_amd import _lib
    buf = torch.full((n + 2 * guard,), float("nan"), device="cuda")
    f = feats.cuda()
    _lib.check(be.lib.ms3d_dense_scatter(_lib.ptr(f), ctypes.c_long(f.size(0)), ctypes.c_long(C), _lib.ptr(cell_row), None, B, C,
                                         *grid, ctypes.c_void_p(buf.data_ptr() + 4 * guard), _lib.stream_handle()), "scatter")
    assert torch.equal(buf[guard:guard + n].cpu().view(want.shape), want)
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + n:]).all()


def test_scatter_row_index_and_row_stride(be):
    """the table names rows of one order, the features are held in another (row_index), inside wider rows (ld)"""
    rng = np.random.default_rng(2)
    C, grid, B = 35, (4, 4, 5), 2
    coords = cloud(rng, grid, [0, 1], 0.4)
    V = coords.size(0)
    feats = feats_of(rng, V, C)
    cell_row, _, _ = be.dense_cell_map(coords.cuda(), (0, 0, 0), 1, (B,) + grid)
    perm = torch.from_numpy(rng.permutation(V))
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(V)
    wide = torch.full((V, C + 13), float("nan"))
    wide[:, 5:5 + C] = feats[perm]                       # held row h = table row perm[h]
    held = wide.cuda()[:, 5:5 + C]
    assert not held.is_contiguous()
    d = be.dense_scatter(held, cell_row, (B, C) + grid, row_index=inv.to(torch.int32).cuda())
    assert torch.equal(d.cpu(), dense_reference(coords, feats, (B, C) + grid))


# ---------------------------------------------------------------------------------------------- 2. origins and strides
def test_negative_coordinates_and_explicit_origin(ME):
    rng = np.random.default_rng(3)
    grid, C = (6, 5, 7), 5
    coords = cloud(rng, grid, [0, 1], "all", origin=(-4, -2, -7))
    keep = torch.from_numpy(rng.random(coords.size(0)) < 0.5)
    keep[(coords[:, 1:] == torch.tensor([-4, -2, -7])).any(1)] = True          # the extent stays the grid
    keep[(coords[:, 1:] == torch.tensor([1, 2, -1])).any(1)] = True
    coords = coords[keep]
    feats = feats_of(rng, coords.size(0), C)
    x, _ = sparse(ME, coords, feats)
    d, origin, _ = x.dense()
    assert origin.tolist() == [[-4, -2, -7]] and tuple(d.shape) == (2, C) + grid
    assert torch.equal(d.cpu(), dense_reference(coords, feats, d.shape, origin=(-4, -2, -7)))
    for o in ([-6, -2, -9], torch.tensor([[-5, -3, -7]])):
        d, origin, _ = x.dense(min_coordinate=o)
        ol = tuple(torch.as_tensor(o).view(-1).tolist())
        assert origin.tolist() == [list(ol)]
        assert tuple(d.shape) == (2, C, 2 - ol[0], 3 - ol[1], -ol[2])          # the largest coordinate is (1, 2, -1)
        assert torch.equal(d.cpu(), dense_reference(coords, feats, d.shape, origin=ol))
    big = (3, C, 9, 8, 10)                                                      # a shape larger than the extent
    d, _, _ = x.dense(shape=big, min_coordinate=[-5, -2, -8])
    assert torch.equal(d.cpu(), dense_reference(coords, feats, big, origin=(-5, -2, -8)))


@pytest.mark.parametrize("levels", [1, 2])
def test_tensor_stride_2_and_4(ME, levels):
    """a tensor produced by one or two stride-2 convolutions, with the stride contracted and not"""
    rng = np.random.default_rng(4 + levels)
    coords = cloud(rng, (11, 9, 10), [0, 1], 0.3, origin=(-3, 0, 2))
    x, _ = sparse(ME, coords, feats_of(rng, coords.size(0), 4))
    c = 4
    for _ in range(levels):
        x = ME.MinkowskiConvolution(c, 2 * c, kernel_size=2, stride=2, dimension=3).cuda()(x)
        c *= 2
    ts = 2 ** levels
    assert x.tensor_stride == ts
    yc, yf = x.C.cpu(), x.F.detach().cpu()
    lo = yc[:, 1:].amin(0).tolist()
    d, origin, stride = x.dense()
    assert origin.tolist() == [lo] and stride.tolist() == [ts] * 3
    assert torch.equal(d.cpu(), dense_reference(yc, yf, d.shape, origin=lo, divisor=ts))
    assert d.shape[2] == (int(yc[:, 1].max()) - lo[0]) // ts + 1
    d1, _, stride = x.dense(contract_stride=False)
    assert stride.tolist() == [ts] * 3 and d1.shape[2] == int(yc[:, 1].max()) - lo[0] + 1
    assert torch.equal(d1.cpu(), dense_reference(yc, yf, d1.shape, origin=lo))
    o2 = [lo[0] - 2 * ts, lo[1], lo[2] - ts]
    d2, _, _ = x.dense(shape=(3, c, 12, 12, 12), min_coordinate=o2)
    assert torch.equal(d2.cpu(), dense_reference(yc, yf, d2.shape, origin=o2, divisor=ts))
    with pytest.raises(ValueError, match="not a multiple of the tensor stride"):
        x.dense(min_coordinate=[lo[0] - 1, lo[1], lo[2]])


# ---------------------------------------------------------------------------------------------- 3. rows where they are held
def test_morton_sorted_manager_and_lazy_batchnorm(ME):
    rng = np.random.default_rng(6)
    grid, C = (20, 19, 21), 16
    coords = cloud(rng, grid, [0, 1], 0.4)
    assert coords.size(0) >= 4096
    feats = feats_of(rng, coords.size(0), C)
    cm = ME.CoordinateManager(coords.cuda(), spatial_sort=True)
    assert cm.perm is not None, "the cloud is too small to be Morton-sorted"
    f = feats.cuda().requires_grad_(True)
    x = ME.SparseTensor(f[cm.perm], coordinate_manager=cm)
    assert torch.equal(x.C.cpu(), coords)
    d, _, _ = x.dense(min_coordinate=0)
    want = dense_reference(coords, feats, d.shape)
    assert torch.equal(d.cpu(), want)
    g = torch.randn(d.shape, generator=torch.Generator().manual_seed(1))
    d.backward(g.cuda())
    fr = feats.clone().requires_grad_(True)
    dense_reference(coords, fr, d.shape).backward(g)
    assert torch.equal(f.grad.cpu(), fr.grad)
    # straight out of BatchNorm + ReLU: the pending normalisation is applied by dense() itself
    lazy = ME.MinkowskiReLU()(ME.MinkowskiBatchNorm(C).cuda().train()(x))
    assert lazy._pending is not None
    dl, _, _ = lazy.dense(min_coordinate=0)
    assert lazy._pending is None
    assert torch.equal(dl.cpu(), dense_reference(coords, lazy.F.detach().cpu(), d.shape))
    assert (dl >= 0).all() and dl.max() > 0


# ---------------------------------------------------------------------------------------------- 4. backward of dense
@pytest.mark.parametrize("C", CHANNELS)
def test_dense_backward_exact(ME, C):
    rng = np.random.default_rng(40 + C)
    for grid in GRIDS:
        for occ, batches, B in ((0.5, [0, 2], 3), ("all", [0], 1)):
            coords = cloud(rng, grid, batches, occ)
            feats = feats_of(rng, coords.size(0), C)
            x, f = sparse(ME, coords, feats, requires_grad=True)
            shape = (B, C) + grid
            d, _, _ = x.dense(shape=shape, min_coordinate=0)
            g = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
            d.backward(g.cuda())
            fr = feats.clone().requires_grad_(True)
            dense_reference(coords, fr, shape).backward(g)
            assert torch.equal(f.grad.cpu(), fr.grad), (grid, occ)


# ---------------------------------------------------------------------------------------------- 5. to_sparse
def volume(rng, shape, share=0.3):
    x = rng.standard_normal(shape).astype(np.float32)
    keep = rng.random((shape[0], 1) + tuple(shape[2:])) < share
    return torch.from_numpy(x * keep)


@pytest.mark.parametrize("C", CHANNELS)
def test_to_sparse_exact(ME, C):
    rng = np.random.default_rng(50 + C)
    for grid in GRIDS:
        for B, share in ((1, 1.1), (3, 0.3)):
            v = volume(rng, (B, C) + grid, share)
            if B == 3:
                v[1] = 0                                   # a batch index without cells
            xe = v.cuda().requires_grad_(True)
            s = ME.to_sparse(xe)
            wc, wf = to_sparse_reference(v)
            assert s.tensor_stride == 1 and s.C.dtype == torch.int32
            assert torch.equal(s.C.cpu(), wc) and torch.equal(s.F.detach().cpu(), wf), (grid, B)
            g = torch.from_numpy(rng.standard_normal(tuple(wf.shape)).astype(np.float32))
            s.F.backward(g.cuda())
            xr = v.clone().requires_grad_(True)
            to_sparse_reference(xr)[1].backward(g)
            assert torch.equal(xe.grad.cpu(), xr.grad), (grid, B)


def test_to_sparse_edge_cells_formats_and_modules(ME):
    rng = np.random.default_rng(7)
    v = volume(rng, (2, 33, 5, 13, 1), 0.2)
    v[1, :, 4, 12, 0] = 0
    v[1, 32, 4, 12, 0] = 7.0                                # only the LAST channel is non-zero
    v[0, :, 0, 0, 0] = 0
    v[0, 5, 0, 0, 0] = float("nan")                         # NaN counts as non-zero
    v[0, :, 2, 2, 0] = 0
    v[0, 1::2, 2, 2, 0] = -0.0                              # -0.0 only: dropped
    wc, wf = to_sparse_reference(v)
    rows = {tuple(r) for r in wc.tolist()}
    assert (1, 4, 12, 0) in rows and (0, 0, 0, 0) in rows and (0, 2, 2, 0) not in rows
    s = ME.to_sparse(v.cuda())
    assert torch.equal(s.C.cpu(), wc) and torch.equal(s.F.cpu().view(torch.int32), wf.view(torch.int32))      # bits: NaN, -0.0
    s2 = ME.MinkowskiToSparseTensor()(v.cuda())
    assert torch.equal(s2.C.cpu(), wc) and torch.equal(s2.F.cpu().view(torch.int32), wf.view(torch.int32))
    assert torch.equal(ME.MinkowskiToFeature()(s2).cpu().view(torch.int32), wf.view(torch.int32))
    cl = ME.to_sparse(v.permute(0, 2, 3, 4, 1).contiguous().cuda(), format="BXXXC")
    assert torch.equal(cl.C.cpu(), wc) and torch.equal(cl.F.cpu().view(torch.int32), wf.view(torch.int32))
    dev = ME.to_sparse(v, device="cuda")
    assert dev.F.is_cuda and torch.equal(dev.C.cpu(), wc)
    z = ME.to_sparse(torch.zeros(2, 3, 4, 4, 4).cuda())
    assert tuple(z.C.shape) == (0, 4) and tuple(z.F.shape) == (0, 3)
    a = ME.to_sparse_all(v.cuda())
    every = torch.ones(2, 5, 13, 1).nonzero().int()
    assert torch.equal(a.C.cpu(), every) and torch.equal(a.F.cpu().view(torch.int32), rows_at(v, every).view(torch.int32))
    a2 = ME.MinkowskiToSparseTensor(remove_zeros=False)(v.cuda())
    assert torch.equal(a2.C.cpu(), every)


def test_to_sparse_with_coordinates(ME):
    """exactly the named cells in the caller's order.  A cell named twice: two equal rows, and its gradient is the sum of the
    two -- one float32 addition, so bit-exact against float64 autograd rounded to float32.  A cell named three times is summed
    in ascending row order from zero (the engine's stated order): exact against that float32 loop, and within the two roundings
    of a three-term sum, 2 * 2^-24 * sum |g|, of float64."""
    rng = np.random.default_rng(8)
    C, grid = 35, (4, 4, 5)
    v = volume(rng, (2, C) + grid, 0.5)
    cells = rng.permutation(2 * 4 * 4 * 5)[:66]
    b, rest = np.divmod(cells, 80)
    x, rest = np.divmod(rest, 20)
    y, z = np.divmod(rest, 5)
    coords = torch.from_numpy(np.stack([b, x, y, z], 1).astype(np.int32))       # 66 distinct cells in random order
    coords = torch.cat([coords, coords[[3, 63, 20, 64]]])                       # four named twice, across the 64-entry tile edge
    n = coords.size(0)
    xe = v.cuda().requires_grad_(True)
    s = ME.to_sparse(xe, coordinates=coords.cuda())
    assert torch.equal(s.C.cpu(), coords) and torch.equal(s.F.detach().cpu(), rows_at(v, coords))
    assert torch.equal(s.F[3], s.F[66]) and torch.equal(s.F[64], s.F[69])
    g = torch.from_numpy(rng.standard_normal((n, C)).astype(np.float32))
    s.F.backward(g.cuda())
    x64 = v.double().requires_grad_(True)
    rows_at(x64, coords).backward(g.double())
    assert torch.equal(xe.grad.cpu(), x64.grad.float())

    thrice = torch.cat([coords, coords[[3, 5]]])                                # cell 3 three times, cell 5 twice
    n = thrice.size(0)
    xe = v.cuda().requires_grad_(True)
    s = ME.to_sparse(xe, coordinates=thrice.cuda())
    assert torch.equal(s.F.detach().cpu(), rows_at(v, thrice))
    g = torch.from_numpy(rng.standard_normal((n, C)).astype(np.float32))
    s.F.backward(g.cuda())
    ordered, mag = torch.zeros(v.shape), torch.zeros(v.shape, dtype=torch.float64)
    for r in range(n):
        b, x, y, z = thrice[r].tolist()
        ordered[b, :, x, y, z] += g[r]
        mag[b, :, x, y, z] += g[r].double().abs()
    assert torch.equal(xe.grad.cpu(), ordered)
    x64 = v.double().requires_grad_(True)
    rows_at(x64, thrice).backward(g.double())
    excess = ((xe.grad.cpu().double() - x64.grad).abs() - 2 * 2.0 ** -24 * mag).max().item()
    print(f"a cell named three times: |float32 ordered sum - float64| - 2 * 2^-24 * sum|g| at most {excess:.3e}")
    assert excess <= 0

    for bad in ([[2, 0, 0, 0]], [[0, 4, 0, 0]], [[0, 0, 0, -1]], [[-1, 0, 0, 0]]):
        with pytest.raises(ValueError, match="1 coordinates lie outside"):
            ME.to_sparse(v.cuda(), coordinates=torch.tensor(bad))
    s3 = ME.MinkowskiToSparseTensor(coordinates=coords[:5].cuda())(v.cuda())
    assert torch.equal(s3.F.cpu(), rows_at(v, coords[:5]))


# ---------------------------------------------------------------------------------------------- 6. round trips
def test_round_trips(ME):
    rng = np.random.default_rng(9)
    grid, C = (9, 7, 11), 6
    coords = cloud(rng, grid, [0, 2], 0.3, origin=(-3, 4, 0))
    feats = feats_of(rng, coords.size(0), C)
    feats[::7] = 0                                          # rows that are all zero do not come back
    x, _ = sparse(ME, coords, feats)
    d, origin, _ = x.dense()
    back = ME.to_sparse(d)
    nz = (feats != 0).any(1)
    want_c = coords[nz].clone()
    want_c[:, 1:] -= origin.view(1, 3)
    key = lambda c: ((c[:, 0].long() * 64 + c[:, 1]) * 64 + c[:, 2]) * 64 + c[:, 3]
    order = torch.argsort(key(want_c))
    assert torch.equal(back.C.cpu(), want_c[order]) and torch.equal(back.F.cpu(), feats[nz][order])
    v = volume(rng, (2, 5, 6, 5, 7), 0.4)
    rt = ME.to_sparse_all(v.cuda()).dense(shape=v.shape, min_coordinate=0)[0]
    assert torch.equal(rt.cpu(), v)
    assert torch.equal(ME.MinkowskiToDenseTensor(v.shape)(ME.to_sparse_all(v.cuda())).cpu(), v)


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_manager_usable(ME):
    rng = np.random.default_rng(10)
    grid, C = (4, 4, 5), 3
    coords = cloud(rng, grid, [0, 1], 0.5)
    feats = feats_of(rng, coords.size(0), C)
    x, _ = sparse(ME, coords, feats)
    n_out = int((coords[:, 1] >= 3).sum())
    with pytest.raises(ValueError, match=f"^dense\\(\\): {n_out} rows lie outside"):
        x.dense(shape=(2, C, 3, 4, 5), min_coordinate=0)
    n_b = int((coords[:, 0] >= 1).sum())
    with pytest.raises(ValueError, match=f"^dense\\(\\): {n_b} rows lie outside"):
        x.dense(shape=(1, C) + grid, min_coordinate=0)
    d, _, _ = x.dense(shape=(2, C) + grid, min_coordinate=0)
    assert torch.equal(d.cpu(), dense_reference(coords, feats, d.shape))
    twice = torch.cat([coords, coords[2:4]])
    y = ME.SparseTensor(feats_of(rng, twice.size(0), C).cuda(), coordinate_manager=ME.CoordinateManager(twice.cuda()))
    with pytest.raises(ValueError, match="more than once \\(2 rows"):
        y.dense(shape=(2, C) + grid, min_coordinate=0)
    with pytest.raises(ValueError, match="more than once \\(2 rows"):
        y.dense(shape=(2, C) + grid, min_coordinate=0)                       # the cached map refuses again
    d, _, _ = x.dense(shape=(2, C) + grid, min_coordinate=0)
    assert torch.equal(d.cpu(), dense_reference(coords, feats, d.shape))


# ---------------------------------------------------------------------------------------------- 8. reproducibility
def test_same_bytes_on_every_run(ME):
    rng = np.random.default_rng(11)
    grid, C = (17, 241, 1), 33
    coords = cloud(rng, grid, [0, 2], 0.3)
    feats = feats_of(rng, coords.size(0), C)
    g = torch.from_numpy(rng.standard_normal((3, C) + grid).astype(np.float32)).cuda()
    v = volume(rng, (2, C) + grid, 0.3).cuda()
    picks = torch.from_numpy(np.stack([rng.integers(0, 2, 300), rng.integers(0, 17, 300), rng.integers(0, 241, 300),
                                       np.zeros(300, np.int64)], 1).astype(np.int32)).cuda()      # cells named many times
    runs = []
    for _ in range(2):
        x, f = sparse(ME, coords, feats, requires_grad=True)
        d, _, _ = x.dense(shape=(3, C) + grid, min_coordinate=0)
        d.backward(g)
        xe = v.clone().requires_grad_(True)
        s = ME.to_sparse(xe)
        gs = torch.from_numpy(np.random.default_rng(5).standard_normal(tuple(s.F.shape)).astype(np.float32)).cuda()
        s.F.backward(gs)
        xp = v.clone().requires_grad_(True)
        p = ME.to_sparse(xp, coordinates=picks)
        p.F.backward(gs[:300] if gs.size(0) >= 300 else torch.ones_like(p.F))
        runs.append([d.detach(), f.grad, s.C, s.F.detach(), xe.grad, p.F.detach(), xp.grad])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32) if a.is_floating_point() else a, b.view(torch.int32) if b.is_floating_point() else b)


# ---------------------------------------------------------------------------------------------- 9. composed
def test_completion_step_against_dense_float64(ME):
    """MinkowskiToSparseTensor -> MinkowskiConvolution(k = 3, stride 2: the generative stride-2 layer behind it needs an even
    tensor stride) -> MinkowskiGenerativeConvolutionTranspose(k = 2, s = 2) -> MinkowskiToDenseTensor(shape) against dense
    float64 conv3d / conv_transpose3d on the CPU, masked as the sparse layers mask: zero cells of the input stay out (and get
    no gradient), a coarse cell exists where one of its 2^3 children does.  Forward, d input, d both kernels: <= 1e-4 of the
    reference's largest magnitude."""
    rng = np.random.default_rng(12)
    B, cin, cmid, cout, grid = 2, 8, 16, 8, (10, 8, 12)
    v = volume(rng, (B, cin) + grid, 0.35)
    v[0, :, 0, 0, 0] = torch.from_numpy(rng.standard_normal(cin).astype(np.float32))     # the output's minimum is the origin
    v[1, :, 9, 7, 11] = torch.from_numpy(rng.standard_normal(cin).astype(np.float32))    # ... and its extent the whole grid
    conv = ME.MinkowskiConvolution(cin, cmid, kernel_size=3, stride=2, dimension=3).cuda().train()
    gen = ME.MinkowskiGenerativeConvolutionTranspose(cmid, cout, kernel_size=2, stride=2, dimension=3).cuda().train()
    shape = (B, cout) + grid
    xe = v.cuda().requires_grad_(True)
    out = ME.MinkowskiToDenseTensor(shape)(gen(conv(ME.MinkowskiToSparseTensor()(xe))))
    assert tuple(out.shape) == shape
    g = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    out.backward(g.cuda())

    x64 = v.double().requires_grad_(True)
    w1 = conv.kernel.detach().cpu().double().requires_grad_(True)          # [27, cin, cmid], k = ix + 3 iy + 9 iz
    w2 = gen.kernel.detach().cpu().double().requires_grad_(True)           # [8, cmid, cout], k = ix + 2 iy + 4 iz
    m0 = (v != 0).any(1, keepdim=True).double()
    m1 = F.max_pool3d(m0, 2, 2)
    mid = F.conv3d(x64 * m0, w1.view(3, 3, 3, cin, cmid).permute(4, 3, 2, 1, 0), stride=2, padding=1) * m1
    ref = F.conv_transpose3d(mid, w2.view(2, 2, 2, cmid, cout).permute(3, 4, 2, 1, 0), stride=2)
    ref.backward(g.double())

    def check(name, got, want):
        e = ((got.detach().cpu().double() - want.detach()).abs().max() / want.detach().abs().max()).item()
        print(f"{name}: rel err {e:.3e} (bound 1e-04)")
        assert e <= 1e-4, (name, e)
    check("forward", out, ref)
    check("d input", xe.grad, x64.grad)
    check("d conv kernel", conv.kernel.grad, w1.grad)
    check("d generative kernel", gen.kernel.grad, w2.grad)
    assert (xe.grad.cpu()[(m0 == 0).expand_as(v)] == 0).all()
