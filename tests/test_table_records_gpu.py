"""GPU: the records that hold what is derived from a tensor (backend.TABLES: the pair lists, offset list, density verdict and
pair count of a neighbour table; backend.SORTS: the stable sort of a row index) -- which list a layer gets, that a copy or a
table written in place gets lists of its own, that a prefetch's lists are the ones the layers walk, and that a gather's
backward over a queued sort equals the one over a fresh sort bit for bit.

Every table is the same K = 27 table at the smallest row count from 29 990 up at which the library wants pair lists."""
import ctypes as C

import pytest
import torch

from test_fwd_routes_gpu import build_pairlist, make_table
from test_sparse_gpu import surface_coords

pytestmark = pytest.mark.gpu

K = 27


@pytest.fixture(scope="module")
def be():
    from minsu3d_amd.backend import HipBackend
    b = HipBackend()
    b.lib.ms3d_kmap_pairlist_capacity_rows.restype = C.c_size_t
    return b


@pytest.fixture(scope="module")
def V(be):
    return next(v for v in range(29_990, 31_000) if be.lib.ms3d_kmap_pairlist_wanted(K, v) == 1)


@pytest.fixture(scope="module")
def base(be, V):
    """the table every test starts from; tests that fill or write a table take a clone (a tensor of its own: no record yet)"""
    nbr, _ = make_table(be, V, K, seed=7)
    return nbr


def rows_of(be, pl):
    from minsu3d_amd import _lib
    return be.lib.ms3d_kmap_pairlist_rows_of(_lib.ptr(pl[0]))


def header(tile_start, V, rows):
    """every int of a list's header that the build writes: the tiles + 1 batch offsets and the 257 part starts, then -- behind
    the ints that pad the pick list to 16 bytes, which nobody writes (the buffers are torch.empty) -- the pick list itself"""
    tiles = (V + rows - 1) // rows
    picks = (tiles + 258 + 3) & ~3
    assert tile_start.numel() == picks + 4 * tiles
    return torch.cat([tile_start[:tiles + 258], tile_start[picks:]])


def test_pair_lists_default_settings(be, base, V, monkeypatch):
    monkeypatch.delenv("MS3D_PL_NARROW", raising=False)
    nbr = base.clone()
    for cin, cout in ((16, 16), (32, 32), (64, 32)):
        pl = be.pairlist(nbr, K, V, cin, cout)
        assert be.pairlist(nbr, K, V, cin, cout) is pl
        tile_start, entries = pl
        assert torch.is_tensor(tile_start) and torch.is_tensor(entries) and pl[0] is tile_start and pl[1] is entries
        assert pl.rows == be.lib.ms3d_spconv_pairlist_rows(V, K, cin, cout)
        assert pl.rows == rows_of(be, pl)
    ol = be.offsetlist(nbr, K, V)
    assert be.offsetlist(nbr, K, V) is ol and be.table(nbr).offsetlist is ol


def test_narrow_lists(be, base, V, monkeypatch):
    monkeypatch.setenv("MS3D_PL_NARROW", "2")
    nbr = base.clone()
    narrow = be.pairlist(nbr, K, V, 32, 32)
    assert narrow.rows == 32 and rows_of(be, narrow) == 32
    wide = be.pairlist(nbr, K, V, 16, 16)
    assert wide is not narrow and wide.rows == 64 and rows_of(be, wide) == 64
    rec = be.table(nbr)
    assert rec.pairlists[32] is narrow and rec.pairlists[64] is wide and rec.dense is True


def test_a_copy_gets_lists_of_its_own(be, base, V, monkeypatch):
    monkeypatch.delenv("MS3D_PL_NARROW", raising=False)
    pl = be.pairlist(base, K, V, 16, 16)
    copy = base.clone()
    assert be.table(copy) is not be.table(base) and be.table(copy).tensors() == []
    pl2 = be.pairlist(copy, K, V, 16, 16)
    assert pl2 is not pl and pl2[0] is not pl[0] and pl2.rows == pl.rows == 64
    assert torch.equal(header(pl2[0], V, 64), header(pl[0], V, 64))
    used = 2 * 16 * int(pl[0][(V + 63) // 64])
    assert 0 < used <= pl[1].numel()
    assert torch.equal(pl2[1].view(-1)[:used], pl[1].view(-1)[:used])
    assert be.pairlist(base, K, V, 16, 16) is pl


def test_an_in_place_write_voids_the_lists(be, base, V, monkeypatch):
    monkeypatch.delenv("MS3D_PL_NARROW", raising=False)
    nbr = base.clone()
    pl = be.pairlist(nbr, K, V, 16, 16)
    ol = be.offsetlist(nbr, K, V)
    nbr[0, :64] = -1
    pl2 = be.pairlist(nbr, K, V, 16, 16)
    assert pl2 is not pl and pl2.rows == 64 and be.offsetlist(nbr, K, V) is not ol
    want_start, _ = build_pairlist(be, nbr, K, V, 64)
    assert torch.equal(header(pl2[0], V, 64), header(want_start, V, 64))


def test_prefetched_lists_are_the_ones_the_layers_walk(be, V, monkeypatch):
    import numpy as np
    from minsu3d_amd import backend
    import minsu3d_amd.MinkowskiEngine as ME
    for k in ("MS3D_PL_NARROW", "MS3D_PREFETCH_COORDS"):
        monkeypatch.delenv(k, raising=False)
    prev = backend.set_backend(be)
    try:
        rng = np.random.default_rng(11)
        c = surface_coords(rng, 2, 5 * V, int((V / 1.5) ** 0.5) + 10)
        assert c.shape[0] >= V
        coords = torch.from_numpy(np.ascontiguousarray(c[:V])).cuda()
        g = torch.Generator(device="cuda").manual_seed(11)
        feats = torch.randn(V, 16, device="cuda", generator=g, requires_grad=True)
        ME.prefetch_coordinates(coords, 2)
        x = ME.SparseTensor(feats, coords)
        cm = x.coordinate_manager
        assert cm.size(1) == V
        rec = be.table(cm.k3(1))
        pl, ol = rec.pairlists[64], rec.offsetlist          # built by the prefetch: no layer has run yet
        assert pl.rows == 64 and ol is not None and ol[0] is not None
        conv = ME.MinkowskiConvolution(16, 16, kernel_size=3, dimension=3).cuda()
        y = conv(x)
        y.F.sum().backward()
        torch.cuda.synchronize()
        assert feats.grad is not None and bool(torch.isfinite(feats.grad).all())
        assert be.table(cm.k3(1)) is rec and rec.pairlists == {64: pl} and rec.pairlists[64] is pl and rec.offsetlist is ol
        assert be.pairlist(cm.k3(1), K, V, 16, 16) is pl and be.offsetlist(cm.k3(1), K, V) is ol
        held = rec.tensors()
        assert len(held) >= 4 and all(t.is_cuda for t in held)
        down, up = cm.k2(1)
        for t in (down, up):
            assert all(h.is_cuda for h in be.table(t).tensors())
    finally:
        backend.set_backend(prev)


def test_gather_backward_over_a_queued_sort(be, monkeypatch):
    from minsu3d_amd import backend
    from minsu3d_amd.MinkowskiEngine.functional import GatherRowsFn
    monkeypatch.delenv("MS3D_DETERMINISTIC", raising=False)
    prev = backend.set_backend(be)
    try:
        n, m, C_ = 9_000, 70_000, 16
        assert m > GatherRowsFn.PRESORT_MIN_ROWS and be.deterministic()
        g = torch.Generator(device="cuda").manual_seed(5)
        idx = torch.randint(0, n, (m,), device="cuda", generator=g)
        x = torch.randn(n, C_, device="cuda", generator=g, requires_grad=True)
        dy = torch.randn(m, C_, device="cuda", generator=g)

        def step():
            x.grad = None
            y = GatherRowsFn.apply(x, idx)
            assert torch.equal(y, x.detach()[idx])
            handle = y.grad_fn.sorted
            y.backward(dy)
            return handle, x.grad.clone()

        first = GatherRowsFn.apply(x, idx)                  # queues the sort; nobody has waited for it yet
        h0 = first.grad_fn.sorted
        assert isinstance(h0, backend.SortedIndex) and backend.SORTS.get(idx) is h0
        h1, g1 = step()
        assert h1 is h0                                     # a second forward over the same index reuses the queued record
        assert torch.equal(g1, be.scatter_add_rows(dy, idx.clone(), n))
        first.backward(dy)
        assert torch.equal(x.grad, g1 + g1)                 # accumulated onto g1; the same record, now finished, the same bytes
        idx[0] = idx[1]
        h3, g3 = step()
        assert h3 is not h1 and backend.SORTS.get(idx) is h3
        assert torch.equal(g3, be.scatter_add_rows(dy, idx.clone(), n))
        torch.cuda.synchronize()
    finally:
        backend.set_backend(prev)
