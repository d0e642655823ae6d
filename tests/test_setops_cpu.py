"""Arithmetic across coordinate sets (MinkowskiUnion, SparseTensor + - *, the MinkowskiBroadcast family): what can be checked
without a GPU -- the exported names, the header, the host-decided contracts of the entry points, the refusals, the same-set
path, and the expectation itself: the numpy restatements of tests/setops_ref.py, which the GPU tests compare the engine
against, are checked here against dense float64 torch."""
import os
import re

import numpy as np
import pytest
import torch

import minsu3d_amd.MinkowskiEngine as ME
import setops_ref as R
from sparse_ref import densify, random_sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("MinkowskiUnion", "MinkowskiBroadcastAddition", "MinkowskiBroadcastMultiplication", "MinkowskiBroadcastConcatenation",
       "MinkowskiBroadcast", "MinkowskiSigmoid")
SYMBOLS = ("ms3d_coords_union_workspace_bytes", "ms3d_coords_union", "ms3d_union_combine", "ms3d_union_combine_backward",
           "ms3d_broadcast_forward", "ms3d_broadcast_reduce_workspace_bytes", "ms3d_broadcast_reduce")
EPS = float(np.finfo(np.float32).eps)


def overlapping_sets(rng, n_sets=2, B=2, grid=8, n=120, C=5):
    """n_sets sets cut from one pool of distinct coordinates (sparse_ref.random_sparse) as overlapping windows, each shuffled:
    every neighbouring pair has rows in common, rows only in the first and rows only in the second"""
    pool, _ = random_sparse(rng, B=B, grid=grid, n=n * (n_sets + 1) // 2, C=1)
    sets, feats = [], []
    for i in range(n_sets):
        c = pool[i * n // 2:i * n // 2 + n].copy()
        rng.shuffle(c)
        sets.append(c)
        feats.append(rng.standard_normal((len(c), C)).astype(np.float32))
    return sets, feats


def test_new_names_exported():
    for name in NEW:
        assert isinstance(getattr(ME, name), type), name
    for op in ("__add__", "__sub__", "__mul__", "__radd__", "__rmul__", "__iadd__"):
        assert callable(getattr(ME.SparseTensor, op)), op
    assert callable(ME.CoordinateManager.union)
    import minsu3d_amd.dropin.MinkowskiEngine as dropin
    for name in NEW:
        assert getattr(dropin, name) is getattr(ME, name) and name in dropin.__all__, name
    for word in NEW:
        assert word in ME.__doc__, word
    unsupported = ME.__doc__.split("Not supported")[1]
    assert "MinkowskiUnion" not in unsupported and "MinkowskiBroadcast" not in unsupported


def test_header_declares_new_symbols():
    """(tests/test_abi_cpu.py then proves that the cross-compiled library exports them)"""
    text = open(os.path.join(ROOT, "include", "minsu3d_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b" + sym + r"\s*\(", text), sym


def test_entry_points_decide_their_contracts_on_the_host():
    """N = 0, N = 17, a null set list: MS3D_E_UNSUPPORTED; all sets empty: the empty set -- decided before anything is
    launched, so this runs without a GPU"""
    import ctypes as C
    from minsu3d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    lib.ms3d_coords_union_workspace_bytes.restype = C.c_size_t
    lib.ms3d_broadcast_reduce_workspace_bytes.restype = C.c_size_t
    null = C.c_void_p(0)
    n = C.c_int(-1)

    def union(start, n_sets):
        arr = (C.c_int * len(start))(*start) if start is not None else null
        return lib.ms3d_coords_union(null, arr, n_sets, null, null, null, C.byref(n), null, C.c_size_t(0), null)
    assert union([0], 0) == _lib.E_UNSUPPORTED and n.value == 0
    assert union([0] * 18, 17) == _lib.E_UNSUPPORTED
    assert union(None, 2) == _lib.E_UNSUPPORTED
    assert union([0, 5, 3], 2) == _lib.E_UNSUPPORTED                       # descending offsets
    n.value = -1
    assert union([0, 0, 0, 0], 3) == 0 and n.value == 0                    # every set empty: nothing is launched
    n.value = -1
    assert union([0] * 17, 16) == 0 and n.value == 0
    # workspace: what the header states per row (a table of 32 .. 64 bytes plus 12 bytes)
    small = lib.ms3d_coords_union_workspace_bytes(100000)
    assert 100000 * (32 + 12) <= small <= 100000 * (64 + 12) + 16384
    assert lib.ms3d_coords_union_workspace_bytes(1 << 30) == 0
    assert lib.ms3d_broadcast_reduce_workspace_bytes(3, 32) == 64 * 3 * 32 * 4
    # the feature kernels: operand counts and modes that do not exist, and empty outputs
    ptrs = (C.c_void_p * 2)(0, 0)
    comb = lambda op, n_sets, n_out: lib.ms3d_union_combine(op, ptrs, n_sets, null, n_out, 4, null, null)
    assert comb(0, 0, 10) == _lib.E_UNSUPPORTED and comb(0, 17, 10) == _lib.E_UNSUPPORTED
    assert comb(1, 3, 10) == _lib.E_UNSUPPORTED and comb(3, 2, 10) == _lib.E_UNSUPPORTED
    assert comb(0, 2, 0) == 0 and comb(2, 2, 0) == 0
    assert lib.ms3d_union_combine_backward(2, 0, null, null, 0, null, null, 4, null, null) == _lib.E_UNSUPPORTED
    assert lib.ms3d_union_combine_backward(0, 0, null, null, 0, null, null, 4, null, null) == 0
    bc = lambda mode, v, c, cg: lib.ms3d_broadcast_forward(mode, ptrs, null, null, v, c, cg, null, null)
    assert bc(4, 10, 4, 4) == _lib.E_UNSUPPORTED and bc(0, 10, 4, 8) == _lib.E_UNSUPPORTED
    assert bc(0, 0, 4, 4) == 0 and bc(2, 0, 4, 8) == 0 and bc(3, 0, 0, 8) == 0


def _tensor(coords, feats, ts=1):
    coords = torch.as_tensor(coords)
    cm = ME.CoordinateManager(coords) if ts == 1 else ME.CoordinateManager.rooted(coords, ts)
    return ME.SparseTensor(torch.as_tensor(feats), coordinate_manager=cm, tensor_stride=ts)


def test_refusals():
    from minsu3d_amd import backend

    class Stub:
        def coords_union(self, sets):
            raise AssertionError("a refused union must not reach the backend")

        def broadcast(self, *a):
            raise AssertionError("a refused broadcast must not reach the backend")
    backend.set_backend(Stub())           # (tests/conftest.py restores the backend)
    c = np.array([[0, 0, 0, 0], [0, 2, 0, 0], [1, 0, 0, 4]], np.int32)
    a = _tensor(c, np.ones((3, 4), np.float32))
    b2 = _tensor(c * 2, np.ones((3, 4), np.float32), ts=2)
    wide = _tensor(c[:2], np.ones((2, 6), np.float32))
    other = _tensor(c[::-1].copy(), np.ones((3, 4), np.float32))
    for fn in (lambda: ME.MinkowskiUnion()(a, b2), lambda: a + b2, lambda: a * b2):
        with pytest.raises(ValueError, match=r"tensor strides 1 and 2"):
            fn()
    for fn in (lambda: ME.MinkowskiUnion()(a, wide), lambda: a - wide):
        with pytest.raises(ValueError, match=r"channel counts 4 and 6"):
            fn()
    with pytest.raises(NotImplementedError, match="17"):
        ME.MinkowskiUnion()(*([a] + [_tensor(c, np.ones((3, 4), np.float32)) for _ in range(16)]))
    before = a.F.clone()
    with pytest.raises(ValueError, match="in-place"):
        a += other
    assert torch.equal(a.F, before)
    # broadcast: a batch index that occurs twice in the global tensor; channel mismatch of add / multiply
    twice = ME.SparseTensor(torch.ones(3, 4), coordinates=torch.tensor([[0, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]],
                                                                       dtype=torch.int32))
    for layer in (ME.MinkowskiBroadcastAddition, ME.MinkowskiBroadcastMultiplication, ME.MinkowskiBroadcastConcatenation,
                  ME.MinkowskiBroadcast):
        with pytest.raises(ValueError, match="occurs twice"):
            layer()(a, twice)
    glob = ME.SparseTensor(torch.ones(2, 6), coordinates=torch.tensor([[0, 0, 0, 0], [1, 0, 0, 0]], dtype=torch.int32))
    for layer in (ME.MinkowskiBroadcastAddition, ME.MinkowskiBroadcastMultiplication):
        with pytest.raises(ValueError, match=r"channel counts 4 and 6"):
            layer()(a, glob)


def test_layers_name_the_hip_backend_when_it_lacks_them():
    from minsu3d_amd import backend

    class Bare:
        pass
    c = np.array([[0, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 2]], np.int32)
    a = _tensor(c, np.ones((3, 4), np.float32))
    b = _tensor(c[1:], np.ones((2, 4), np.float32))
    glob = ME.SparseTensor(torch.ones(2, 4), coordinates=torch.tensor([[0, 0, 0, 0], [1, 0, 0, 0]], dtype=torch.int32))
    backend.set_backend(Bare())
    for fn in (lambda: ME.MinkowskiUnion()(a, b), lambda: a + b, lambda: a - b, lambda: a * b):
        with pytest.raises(NotImplementedError, match="HIP backend"):
            fn()
    for layer in (ME.MinkowskiBroadcastAddition, ME.MinkowskiBroadcastMultiplication, ME.MinkowskiBroadcastConcatenation,
                  ME.MinkowskiBroadcast):
        with pytest.raises(NotImplementedError, match="HIP backend"):
            layer()(a, glob)


def test_same_set_operators_on_cpu_rows():
    """two tensors on one manager and stride take the row-by-row path (no backend): a + b is a.F + b.F as it always was"""
    rng = np.random.default_rng(3)
    coords, fa = random_sparse(rng, n=50, C=4)
    a = _tensor(coords, fa)
    b = a._like(torch.as_tensor(rng.standard_normal((50, 4)).astype(np.float32)))
    assert torch.equal((a + b).F, a.F + b.F) and (a + b).coordinate_manager is a.coordinate_manager
    assert torch.equal((a - b).F, a.F - b.F) and torch.equal((a * b).F, a.F * b.F)
    assert torch.equal(ME.MinkowskiUnion()(a, b, a).F, a.F + b.F + a.F)
    one = ME.MinkowskiUnion()(a)
    assert torch.equal(one.F, a.F) and torch.equal(one.C, a.C)
    # scalars and tensors that broadcast to the rows
    row = torch.arange(4.0)
    assert torch.equal((a + 2).F, a.F + 2) and torch.equal((2 + a).F, a.F + 2) and torch.equal((3.0 * a).F, a.F * 3)
    assert torch.equal((a * row).F, a.F * row) and torch.equal((a - row.view(1, 4)).F, a.F - row)
    assert torch.equal((a + b.F).F, a.F + b.F)
    with pytest.raises(ValueError, match="broadcast"):
        a + torch.ones(7, 4)
    c = a._like(a.F.clone())
    c += b
    assert torch.equal(c.F, a.F + b.F)
    assert torch.equal(ME.MinkowskiSigmoid()(a).F, torch.sigmoid(a.F))


@pytest.mark.parametrize("n_sets", [2, 3, 5])
def test_union_np_is_the_support_of_the_dense_sum(n_sets):
    """pins the GPU tests' expectation: the union set is exactly the support of the sum of the dense occupancy grids, the
    order is set 0's rows, then the new rows of every further set in their order, and both maps invert each other"""
    B, G = 2, 8
    rng = np.random.default_rng(11 + n_sets)
    sets, _ = overlapping_sets(rng, n_sets, B=B, grid=G)
    for i in range(n_sets - 1):
        ka, kb = set(R.key(sets[i]).tolist()), set(R.key(sets[i + 1]).tolist())
        assert len(ka & kb) > 0 and len(ka - kb) > 0 and len(kb - ka) > 0
    out, out_rows, in_row = R.union_np(sets)
    occ = sum(densify(c, np.ones((len(c), 1), np.float32), B, G).double() for c in sets)
    want = torch.nonzero(occ[:, 0] > 0).numpy()
    assert out.dtype == np.int32 and len(np.unique(R.key(out))) == len(out)
    assert np.array_equal(np.sort(R.key(out)), np.sort(R.key(want)))
    # order
    assert np.array_equal(out[:len(sets[0])], sets[0])
    at, seen = len(sets[0]), set(R.key(sets[0]).tolist())
    for c in sets[1:]:
        new = [r for r, k in enumerate(R.key(c).tolist()) if k not in seen]
        assert np.array_equal(out[at:at + len(new)], c[new])
        at += len(new)
        seen |= set(R.key(c).tolist())
    assert at == len(out)
    # maps
    for i, c in enumerate(sets):
        assert np.array_equal(out[out_rows[i]], c)
        assert np.array_equal(in_row[i, out_rows[i]], np.arange(len(c)))
        assert (in_row[i] >= 0).sum() == len(c)
    # an empty set and a set equal to another change nothing but the maps
    out2, rows2, in2 = R.union_np([sets[0], np.zeros((0, 4), np.int32), sets[0][::-1].copy()] + sets[1:])
    assert np.array_equal(out2, out) and len(rows2[1]) == 0 and (in2[1] == -1).all()
    assert np.array_equal(in2[2, :len(sets[0])], np.arange(len(sets[0]))[::-1])


@pytest.mark.parametrize("op", [R.SUM, R.SUB, R.MUL])
def test_combine_np_is_the_dense_expression(op):
    """the combined features equal the dense sum, difference, or the product with the rule for a coordinate one operand
    lacks (zero-filled result receives a, then fn(out, b) at b's rows), float64; bar: a few float32 roundings"""
    B, G = 2, 8
    rng = np.random.default_rng(21 + op)
    sets, feats = overlapping_sets(rng, 3 if op == R.SUM else 2, B=B, grid=G)
    out, out_rows, in_row = R.union_np(sets)
    got = R.combine_np(op, feats, in_row)
    dense = [densify(c, f, B, G).double() for c, f in zip(sets, feats)]
    occ = [densify(c, np.ones((len(c), 1), np.float32), B, G).double() > 0 for c in sets]
    if op == R.SUM:
        d = sum(dense)
    elif op == R.SUB:
        d = dense[0] - dense[1]
    else:
        d = torch.where(occ[1], dense[0] * dense[1], dense[0])
    o = torch.as_tensor(out).long()
    want = d[o[:, 0], :, o[:, 1], o[:, 2], o[:, 3]].numpy()
    assert got.dtype == np.float32
    assert np.abs(got - want).max() <= 4 * EPS * np.abs(want).max()
    only_b = (in_row[0] < 0) & (in_row[1] >= 0)
    only_a = (in_row[0] >= 0) & (in_row[1] < 0)
    assert only_a.any() and only_b.any() and ((in_row[0] >= 0) & (in_row[1] >= 0)).any()
    if op == R.SUB:
        assert np.array_equal(got[only_b], -feats[1][in_row[1, only_b]])
    if op == R.MUL:
        assert np.array_equal(got[only_a], feats[0][in_row[0, only_a]]) and not got[only_b].any()
    # gradients of the restatement against autograd on the same expression (float64)
    leaves = [torch.tensor(f, dtype=torch.float64, requires_grad=True) for f in feats]
    pad = [torch.cat([l, l.new_zeros(1, l.size(1))]) for l in leaves]
    rows = [torch.as_tensor(np.where(r < 0, len(f), r)).long() for r, f in zip(in_row, feats)]
    if op == R.SUM:
        y = sum(p[r] for p, r in zip(pad, rows))
    elif op == R.SUB:
        y = pad[0][rows[0]] - pad[1][rows[1]]
    else:
        has_b = torch.as_tensor(in_row[1] >= 0).view(-1, 1)
        y = torch.where(has_b, pad[0][rows[0]] * pad[1][rows[1]], pad[0][rows[0]])
    dout = rng.standard_normal(got.shape).astype(np.float32)
    y.backward(torch.as_tensor(dout).double())
    for i in range(len(feats)):
        other = dict(other=feats[1 - i], other_row=in_row[1 - i]) if op == R.MUL else {}
        g = R.combine_backward_np(op, i, dout, out_rows[i], **other)
        want_g = leaves[i].grad.numpy()
        assert g.dtype == np.float32 and np.abs(g - want_g).max() <= 4 * EPS * max(np.abs(want_g).max(), 1.0)


@pytest.mark.parametrize("mode", [R.ADD, R.MULTIPLY, R.CAT, R.COPY])
def test_broadcast_np_is_the_dense_per_batch_expression(mode):
    B, G, C = 3, 6, 5
    rng = np.random.default_rng(31 + mode)
    coords, x = random_sparse(rng, B=B, grid=G, n=150, C=C)
    g_batch = np.array([2, 0], np.int32)                      # batch 1 has no global row: its voxels see the zero vector
    cg = C if mode in (R.ADD, R.MULTIPLY) else 3
    g = rng.standard_normal((2, cg)).astype(np.float32)
    grow = R.grow_np(coords[:, 0], g_batch)
    assert (grow == -1).any() and (grow == 0).any() and (grow == 1).any()
    got = R.broadcast_np(mode, x, g, grow)
    gd = torch.zeros(B, cg, 1, 1, 1, dtype=torch.float64)
    gd[torch.as_tensor(g_batch).long(), :, 0, 0, 0] = torch.as_tensor(g).double()
    xd = densify(coords, x, B, G).double()
    if mode == R.ADD:
        d = xd + gd
    elif mode == R.MULTIPLY:
        d = xd * gd
    elif mode == R.CAT:
        d = torch.cat([xd, gd.expand(B, cg, G, G, G)], 1)
    else:
        d = gd.expand(B, cg, G, G, G)
    o = torch.as_tensor(coords).long()
    want = d[o[:, 0], :, o[:, 1], o[:, 2], o[:, 3]].numpy()
    assert got.dtype == np.float32 and np.abs(got - want).max() <= 2 * EPS * np.abs(want).max()
    # the global operand's gradient: per batch the sum over its voxels
    dout = rng.standard_normal(got.shape).astype(np.float32)
    gl = torch.tensor(g, dtype=torch.float64, requires_grad=True)
    xl = torch.tensor(x, dtype=torch.float64)
    gr = torch.cat([gl, gl.new_zeros(1, cg)])[torch.as_tensor(np.where(grow < 0, 2, grow)).long()]
    y = {R.ADD: lambda: xl + gr, R.MULTIPLY: lambda: xl * gr, R.CAT: lambda: torch.cat([xl, gr], 1), R.COPY: lambda: gr}[mode]()
    y.backward(torch.as_tensor(dout).double())
    dg = R.broadcast_dg_np(mode, dout, x, grow, 2, C)
    assert np.abs(dg - gl.grad.numpy()).max() <= 1e-12 * np.abs(dg).max()


class NumpyBackend:
    """the backend methods the new layers call, served by the restatements on CPU tensors: lets the engine's own plumbing
    (cached unions, composed maps, the autograd functions, the broadcast maps) run without a GPU"""

    def coords_union(self, sets):
        out, rows, in_row = R.union_np([c.numpy() for c in sets])
        return torch.from_numpy(out), [torch.from_numpy(r) for r in rows], torch.from_numpy(in_row)

    def union_combine(self, op, feats, in_row, n_out):
        return torch.from_numpy(R.combine_np(op, [f.detach().numpy() for f in feats], in_row.numpy()))

    def union_combine_backward(self, op, which, dout, out_row, other=None, other_row=None):
        return torch.from_numpy(R.combine_backward_np(op, which, dout.numpy(), out_row.numpy(),
                                                      None if other is None else other.detach().numpy(),
                                                      None if other_row is None else other_row.numpy()))

    def broadcast(self, mode, x, g, grow):
        return torch.from_numpy(R.broadcast_np(mode, None if x is None else x.detach().numpy(), g.detach().numpy(),
                                               grow.numpy()))

    def broadcast_reduce(self, dout, col_off, c, x, order, seg_start, seg_of_g):
        d = dout[:, col_off:col_off + c].double()
        if x is not None:
            d = d * x.detach().double()
        dg = torch.zeros((seg_of_g.numel(), c), dtype=torch.float64)
        for j, s in enumerate(seg_of_g.tolist()):
            if s >= 0:
                dg[j] = d[order[int(seg_start[s]):int(seg_start[s + 1])]].sum(0)
        return dg.float()


def test_engine_plumbing_over_a_numpy_backend():
    from minsu3d_amd import backend
    backend.set_backend(NumpyBackend())
    rng = np.random.default_rng(55)
    sets, feats = overlapping_sets(rng, 3, B=3, grid=8, n=90, C=4)
    leaves = [torch.tensor(f, requires_grad=True) for f in feats]
    a, b, c = [_tensor(s, l) for s, l in zip(sets, leaves)]
    want_c, want_rows, want_in = R.union_np(sets)
    y = ME.MinkowskiUnion()(a, b, c)
    assert np.array_equal(y.C.numpy(), want_c) and y.tensor_stride == 1
    assert np.array_equal(y.F.detach().numpy(), R.combine_np(R.SUM, feats, want_in))
    p, q = a * b, a + b
    assert p.coordinate_manager is q.coordinate_manager and p.coordinate_manager is not y.coordinate_manager
    assert torch.equal((p + q).F, p.F + q.F) and (p + q).coordinate_manager is p.coordinate_manager
    _, _, in2 = R.union_np(sets[:2])
    assert np.array_equal(p.F.detach().numpy(), R.combine_np(R.MUL, feats[:2], in2))
    dout = rng.standard_normal(tuple(p.F.shape)).astype(np.float32)
    p.F.backward(torch.from_numpy(dout))
    rows2 = R.union_np(sets[:2])[1]
    for i in range(2):
        g = R.combine_backward_np(R.MUL, i, dout, rows2[i], feats[1 - i], in2[1 - i])
        assert np.array_equal(leaves[i].grad.numpy(), g)
    # broadcast over what a global pooling returns, every mode, with the gradients of both operands
    xb = sets[0][:, 0]
    g_batch = np.array([2, 0], np.int32)
    grow = R.grow_np(xb, g_batch)
    gc = np.zeros((2, 4), np.int32)
    gc[:, 0] = g_batch
    layers = {R.ADD: ME.MinkowskiBroadcastAddition, R.MULTIPLY: ME.MinkowskiBroadcastMultiplication,
              R.CAT: ME.MinkowskiBroadcastConcatenation, R.COPY: ME.MinkowskiBroadcast}
    for mode, layer in layers.items():
        cg = 4 if mode in (R.ADD, R.MULTIPLY) else 3
        gl = torch.tensor(rng.standard_normal((2, cg)).astype(np.float32), requires_grad=True)
        xl = torch.tensor(feats[0], requires_grad=True)
        x = _tensor(sets[0], xl)
        out = layer()(x, ME.SparseTensor(gl, coordinates=torch.from_numpy(gc)))
        assert out.coordinate_manager is x.coordinate_manager
        assert np.array_equal(out.F.detach().numpy(), R.broadcast_np(mode, feats[0], gl.detach().numpy(), grow))
        d = rng.standard_normal(tuple(out.F.shape)).astype(np.float32)
        out.F.backward(torch.from_numpy(d))
        dg = R.broadcast_dg_np(mode, d, feats[0], grow, 2, 4)
        assert np.abs(gl.grad.numpy() - dg).max() <= 1e-5 * np.abs(dg).max()
        if mode == R.COPY:
            assert xl.grad is None
        else:
            want = d[:, :4] if mode != R.MULTIPLY else d * R.broadcast_np(R.COPY, None, gl.detach().numpy(), grow)
            assert np.array_equal(xl.grad.numpy(), want)
