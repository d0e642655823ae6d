"""CPU: ME.neighbor_attention's torch path, its refusals, NeighborMap.relative_positions, the record's target check and
MinkowskiNeighborAttention, against tests/nattn_ref.py (float64 torch, plain gathers, autograd) and numpy loops."""
import numpy as np
import pytest
import torch

from fps_ref import random_voxels
from nattn_ref import check, run_ref


@pytest.fixture(scope="module")
def ME():
    import minsu3d_amd.MinkowskiEngine as me
    return me


def random_index(N, k, V, seed, invalid=0.2):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, V, size=(N, k))
    idx[rng.random((N, k)) < invalid] = -1
    return torch.from_numpy(idx)


def engine(ME, fq, fk, fv, nmap, H, bias, g, scale=None):
    q, k, v = (f.clone().requires_grad_() for f in (fq, fk, fv))
    b = None if bias is None else bias.clone().requires_grad_()
    out = ME.neighbor_attention(q, k, v, nmap, H, bias=b, scale=scale)
    (out * g).sum().backward()
    return dict(out=out.detach(), dq=q.grad, dk=k.grad, dv=v.grad, db=None if b is None else b.grad)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.float64, 1e-12)])
@pytest.mark.parametrize("H,D,k", [(1, 1, 1), (3, 3, 5), (4, 4, 16), (1, 70, 3)])
def test_cpu_path_against_the_reference(ME, dtype, tol, H, D, k):
    N, V, C = 37, 23, H * D
    g = torch.Generator().manual_seed(100 * H + D + k)
    idx = random_index(N, k, V, seed=k)
    idx[5] = -1                                        # a query without a valid slot
    nmap = ME.NeighborMap.from_index(idx, V)
    fq, fk, fv, go = (torch.randn(n, C, generator=g, dtype=dtype) for n in (N, V, V, N))
    bias = torch.randn(N, k, H, generator=g, dtype=dtype)
    bias[idx < 0] = float("nan")                      # the bias of an invalid slot is never read
    for b in (None, bias):
        got = engine(ME, fq, fk, fv, nmap, H, b, go)
        want = run_ref(fq, fk, fv, idx, H, None if b is None else torch.nan_to_num(b), go)
        for name in ("out", "dq", "dk", "dv") + (("db",) if b is not None else ()):
            assert got[name].dtype == dtype
            check(f"cpu {dtype} H{H} D{D} k{k} {name}", got[name].reshape(want[name].shape), want[name], tol)
        assert not got["out"][5].any() and not got["dq"][5].any()
        if b is not None:
            assert not got["db"][idx < 0].any()
    got = engine(ME, fq, fk, fv, nmap, H, None, go, scale=0.37)
    check("cpu scale out", got["out"], run_ref(fq, fk, fv, idx, H, None, go, scale=0.37)["out"], tol)


def test_single_valid_slot_is_a_copy(ME):
    V, N, C = 11, 40, 12
    rng = np.random.default_rng(0)
    idx = np.full((N, 4), -1, np.int64)
    pick = rng.integers(0, V, N)
    idx[np.arange(N), rng.integers(0, 4, N)] = pick
    nmap = ME.NeighborMap.from_index(torch.from_numpy(idx), V)
    q, k, v = torch.randn(N, C), torch.randn(V, C), torch.randn(V, C)
    assert torch.equal(ME.neighbor_attention(q, k, v, nmap, 3, bias=torch.randn(N, 4, 3)), v[torch.from_numpy(pick)])


def test_refusals(ME):
    name = "neighbor_attention"
    V, N, k, C = 9, 7, 3, 12
    nmap = ME.NeighborMap.from_index(random_index(N, k, V, seed=0), V)
    q, kk, v = torch.randn(N, C), torch.randn(V, C), torch.randn(V, C)
    with pytest.raises(ValueError, match=name):
        ME.neighbor_attention(q, kk, v, nmap, 5)                                   # C % num_heads
    with pytest.raises(ValueError, match=name):
        ME.neighbor_attention(q, kk, v, nmap, 0)
    wide = ME.NeighborMap.from_index(random_index(2, 2, 3, seed=1), 3)
    with pytest.raises(ValueError, match=name + ".*128"):
        ME.neighbor_attention(torch.randn(2, 129), torch.randn(3, 129), torch.randn(3, 129), wide, 1)
    with pytest.raises(ValueError, match="254"):
        ME.NeighborMap.from_index(random_index(2, 255, 3, seed=1), 3)
    for bad in (torch.randn(N, k), torch.randn(N, k, 2), torch.randn(N, k, 4).double(), torch.zeros(N, k, 4, dtype=torch.int64)):
        with pytest.raises(ValueError, match=name + ": bias"):
            ME.neighbor_attention(q, kk, v, nmap, 4, bias=bad)
    for half in (torch.float16, torch.bfloat16):
        with pytest.raises(NotImplementedError, match=name):
            ME.neighbor_attention(q.to(half), kk.to(half), v.to(half), nmap, 4)
        with pytest.raises(NotImplementedError, match=name):
            ME.neighbor_attention(q.to(half), kk, v, nmap, 4)
    with pytest.raises(ValueError, match=name):
        ME.neighbor_attention(q, kk, torch.randn(V, C + 4), nmap, 4)               # another C
    with pytest.raises(ValueError, match=name):
        ME.neighbor_attention(q[:-1], kk, v, nmap, 4)                              # another row count of q
    with pytest.raises(ValueError):
        ME.neighbor_attention(q, kk[:-1], v[:-1], nmap, 4)                         # another support
    with pytest.raises(TypeError, match=name):
        ME.neighbor_attention(q, kk, v, "no map", 4)
    # mixed k / v sets and kinds
    c = random_voxels([30, 25], seed=2, side=6)
    cm = ME.CoordinateManager(torch.from_numpy(c))
    other = ME.CoordinateManager(torch.from_numpy(c))
    x = ME.SparseTensor(torch.randn(55, C), coordinate_manager=cm)
    z = ME.SparseTensor(torch.randn(55, C), coordinate_manager=other)
    own = ME.knn_map(x, 3)
    with pytest.raises(ValueError, match=name):
        ME.neighbor_attention(x, x, z, own, 4)
    with pytest.raises(ValueError, match=name):
        ME.neighbor_attention(x, x, x.F, own, 4)
    with pytest.raises(ValueError, match="another set"):
        ME.neighbor_attention(z, x, x, own, 4)                                     # q on another set
    with pytest.raises(ValueError, match="another set"):
        ME.neighbor_attention(x.F, x, x, own, 4)                                   # a plain q for a map whose target is a set
    out = ME.neighbor_attention(x, x, x, own, 4)
    assert out.coordinate_manager is cm and tuple(out.F.shape) == (55, C)


def test_the_records_target_check(ME):
    from minsu3d_amd.backend import NeighbourGroup
    idx = random_index(6, 2, 5, seed=3)
    legacy = NeighbourGroup(idx, 5)                    # the keyword's default: not checked, any identity passes
    assert legacy.target is NeighbourGroup.UNCHECKED
    legacy.check_target((object(), 1), 6, idx.device)
    legacy.check_target((None, None), 6, idx.device)
    with pytest.raises(ValueError, match="6 queries"):
        legacy.check_target((None, None), 5, idx.device)
    token = object()
    named = NeighbourGroup(idx, 5, target=(token, 2))
    named.check_target((token, 2), 6, idx.device)
    for other in ((token, 1), (object(), 2), (None, None)):
        with pytest.raises(ValueError, match="another set"):
            named.check_target(other, 6, idx.device)
    plain = ME.NeighborMap.from_index(idx, 5)
    assert plain.target == (None, None)
    c = random_voxels([20, 20], seed=4, side=5)
    x = ME.SparseTensor(torch.randn(40, 4), coordinate_manager=ME.CoordinateManager(torch.from_numpy(c)))
    y = ME.SparseTensor(torch.randn(13, 4), coordinates=torch.from_numpy(random_voxels([6, 7], seed=5, side=5)))
    assert ME.knn_map(x, 2).target == (x.coordinate_manager, x.tensor_stride)
    assert ME.knn_map(x, 2, y).target == (y.coordinate_manager, y.tensor_stride)
    assert ME.knn_map(x, 2, ME.farthest_point_sampling(x, 3)).target == (None, None)
    # the three forms end to end: q on the target, k / v on the support
    out = ME.neighbor_attention(y, x, x, ME.knn_map(x, 2, y), 2)
    assert out.coordinate_manager is y.coordinate_manager and tuple(out.F.shape) == (13, 4)
    picks = ME.farthest_point_sampling(x, 3)
    out = ME.neighbor_attention(torch.randn(2, 3, 4), x, x, ME.knn_map(x, 2, picks), 2)
    assert torch.is_tensor(out) and tuple(out.shape) == (2, 3, 4)


def relpos_loop(sup, tgt, idx):
    """numpy loop: sup [V, 3], tgt [N, 3] positions in caller order, idx [N, k] caller rows -> float32 [N, k, 3]"""
    out = np.zeros(idx.shape + (3,), np.float32)
    for n in range(idx.shape[0]):
        for j in range(idx.shape[1]):
            if idx[n, j] >= 0:
                out[n, j] = sup[idx[n, j]].astype(np.float32) - tgt[n].astype(np.float32)
    return out


def test_relative_positions(ME):
    c = random_voxels([60, 45], seed=6, side=8)
    x = ME.SparseTensor(torch.zeros(105, 1), coordinate_manager=ME.CoordinateManager(torch.from_numpy(c)))
    own = ME.knn_map(x, 4)
    rel = own.relative_positions()
    assert rel.dtype == torch.float32 and tuple(rel.shape) == (105, 4, 3) and not rel.requires_grad
    assert np.array_equal(rel.numpy(), relpos_loop(c[:, 1:], c[:, 1:], own.idx.numpy()))
    assert own.relative_positions() is rel                                        # made once and kept
    # a y target on another manager, capped: -1 slots are zeros
    qc = random_voxels([20, 31], seed=7, side=8)
    y = ME.SparseTensor(torch.zeros(51, 1), coordinates=torch.from_numpy(qc))
    capped = ME.knn_map(x, 5, y, max_squared_distance=3)
    assert int((capped.idx < 0).sum()) > 0 and int((capped.idx >= 0).sum()) > 0
    rel = capped.relative_positions()
    assert tuple(rel.shape) == (51, 5, 3)
    assert np.array_equal(rel.numpy(), relpos_loop(c[:, 1:], y.C.numpy()[:, 1:], capped.idx.numpy()))
    assert not rel[capped.idx < 0].any()
    # picks
    picks = ME.farthest_point_sampling(x, 6)
    at = ME.knn_map(x, 3, picks)
    rel = at.relative_positions()
    assert tuple(rel.shape) == (2, 6, 3, 3)
    want = relpos_loop(c[:, 1:], c[picks.reshape(-1).numpy(), 1:], at.idx.reshape(-1, 3).numpy())
    assert np.array_equal(rel.reshape(-1, 3, 3).numpy(), want)
    # points
    rng = np.random.default_rng(8)
    p = np.concatenate([rng.integers(0, 2, (80, 1)), rng.random((80, 3)) * 4], 1).astype(np.float32)
    f = ME.TensorField(torch.zeros(80, 1), torch.from_numpy(p))
    pm = ME.knn_map(f, 3)
    assert np.array_equal(pm.relative_positions().numpy(), relpos_loop(p[:, 1:], p[:, 1:], pm.idx.numpy()))
    with pytest.raises(ValueError, match="from_index"):
        ME.NeighborMap.from_index(random_index(4, 2, 5, seed=0), 5).relative_positions()


def test_module(ME):
    torch.manual_seed(0)
    c = random_voxels([50, 40], seed=9, side=6)
    feats = torch.randn(90, 8)
    x = ME.SparseTensor(feats, coordinate_manager=ME.CoordinateManager(torch.from_numpy(c)))
    with_pos = ME.MinkowskiNeighborAttention(8, 2, k=5)
    assert sorted(with_pos.state_dict()) == ["pos.0.bias", "pos.0.weight", "pos.2.bias", "pos.2.weight", "proj.bias",
                                             "proj.weight", "qkv.bias", "qkv.weight"]
    assert not with_pos.pos[2].weight.any() and not with_pos.pos[2].bias.any()
    without = ME.MinkowskiNeighborAttention(8, 2, k=5, pos_bias=False)
    assert sorted(without.state_dict()) == ["proj.bias", "proj.weight", "qkv.bias", "qkv.weight"]
    assert sorted(ME.MinkowskiNeighborAttention(8, 2, qkv_bias=False, pos_bias=False).state_dict()) == \
        ["proj.bias", "proj.weight", "qkv.weight"]
    without.load_state_dict({n: t for n, t in with_pos.state_dict().items() if not n.startswith("pos.")})
    a, b = with_pos(x), without(x)
    assert a.coordinate_manager is x.coordinate_manager and tuple(a.F.shape) == (90, 8)
    assert torch.equal(a.F, b.F)                       # the zero-initialised position layer: plain attention
    shared = ME.knn_map(x, 3)
    assert torch.equal(with_pos(x, shared).F, without(x, nmap=shared).F) and not torch.equal(with_pos(x, shared).F, a.F)
    a.F.sum().backward()
    assert with_pos.pos[2].weight.grad is not None and with_pos.pos[2].bias.grad.abs().sum() >= 0
    for bad in (dict(num_heads=3), dict(num_heads=0), dict(num_heads=2, k=0)):
        with pytest.raises(ValueError, match="MinkowskiNeighborAttention"):
            ME.MinkowskiNeighborAttention(8, **bad)
    p = torch.cat([torch.randint(0, 2, (70, 1)).float(), torch.rand(70, 3) * 3], 1)
    f = ME.TensorField(torch.randn(70, 8), p)
    out = with_pos(f)
    assert isinstance(out, ME.TensorField) and tuple(out.F.shape) == (70, 8)
