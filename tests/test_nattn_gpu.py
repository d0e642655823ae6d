"""GPU: multi-head attention over a neighbour index (ME.neighbor_attention, MinkowskiNeighborAttention; csrc/nattn.hip).

The yardstick is tests/nattn_ref.py: float64 torch on the CPU over caller-order rows, plain gathers, a masked softmax, autograd
for every gradient.  The bound is the project's bar, RTOL = 1e-4 of the reference tensor's largest magnitude, for out, dq, dk,
dv and dbias alike (a plain float32 restatement of the formulas stays within 4.6e-6 of float64, so the bar leaves a factor of
twenty).  Every engine step runs twice and must give the same bytes.  The largest error seen per tensor is printed when the
module ends."""
import ctypes as C

import numpy as np
import pytest
import torch

from fps_ref import random_voxels
from nattn_ref import RTOL, WORST, check, run_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
HEADS = [(1, 1), (3, 3), (2, 8), (4, 4), (1, 32), (8, 16), (2, 48), (1, 128), (1, 70)]   # test_kattn_gpu's list plus (1, 70)
THREADS = 256            # NATTN_THREADS of csrc/nattn.hip: "constexpr int NATTN_THREADS = 256;"
E_WORKSPACE, E_UNSUPPORTED = 10001, 10002


@pytest.fixture(scope="module")
def ME():
    import minsu3d_amd.MinkowskiEngine as me
    return me


@pytest.fixture(scope="module")
def be():
    from minsu3d_amd.backend import get_backend
    return get_backend()


@pytest.fixture(scope="module")
def T(be):
    t = be.nbr_chunk_entries()
    assert t >= 64
    return t


def group_of(D):
    """attn_core.h group_of(D, VEC) with VEC = 4 when D % 4 == 0 (aligned rows), else 1"""
    n = D // 4 if D % 4 == 0 else D
    g = 1
    while g < n and g < 64:
        g *= 2
    return g


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def random_index(N, k, V, seed, invalid=0.2):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, V, size=(N, k))
    idx[rng.random((N, k)) < invalid] = -1
    return torch.from_numpy(idx)


def ident(t):
    return t


def rows_of(t):
    t = t if torch.is_tensor(t) else t.F
    return t.reshape(-1, t.size(-1))


def engine(ME, fq, fk, fv, nmap, H, bias, g, make_q=ident, make_kv=ident, needs=(True, True, True, True), scale=None):
    """ME.neighbor_attention on caller-order device features, run twice with the same bytes -> dict of out and the gradients
    asked for, in caller order; fq may be [..., C], bias [..., k, H]"""
    def step():
        q, k, v = (f.clone().requires_grad_(n) for f, n in zip((fq, fk, fv), needs))
        b = None if bias is None else bias.clone().requires_grad_(needs[3])
        out = ME.neighbor_attention(make_q(q), make_kv(k), make_kv(v), nmap, H, bias=b, scale=scale)
        out = out if torch.is_tensor(out) else out.F
        assert out.dtype == torch.float32 and tuple(out.shape) == tuple(fq.shape)
        if out.requires_grad:
            (out * g).sum().backward()
        return out.detach(), q.grad, k.grad, v.grad, None if b is None else b.grad
    first, second = step(), step()
    for u, v in zip(first, second):
        assert (u is None and v is None) or same_bytes(u, v)
    return dict(zip(("out", "dq", "dk", "dv", "db"), first))


def parity(ME, tag, fq, fk, fv, nmap, H, bias, g, **kw):
    """engine against the reference on the map's caller-order index, all five tensors -> (got, want)"""
    got = engine(ME, fq, fk, fv, nmap, H, bias, g, **kw)
    ref_bias = None if bias is None else torch.nan_to_num(bias)
    want = run_ref(rows_of(fq), fk, fv, nmap.idx, H, ref_bias, rows_of(g), kw.get("scale"))
    for name in ("out", "dq", "dk", "dv") + (("db",) if bias is not None else ()):
        check(f"{tag} {name}", got[name].reshape(want[name].shape), want[name], RTOL)
    if bias is not None:
        assert not got["db"].reshape(want["db"].shape).cpu()[nmap.idx.reshape(-1, nmap.k).cpu() < 0].any()
    return got, want


def draw(N, V, C, k, H, seed, idx=None, bias="normal"):
    """float32 device q [N, C], k, v [V, C], dout [N, C] and a bias [N, k, H] that is NaN where idx < 0 (never read)"""
    g = torch.Generator().manual_seed(seed)
    fq, fk, fv, go = (torch.randn(n, C, generator=g).to(DEV) for n in (N, V, V, N))
    if bias is None:
        return fq, fk, fv, None, go
    b = torch.randn(N, k, H, generator=g) if bias == "normal" else torch.randint(-100, 101, (N, k, H), generator=g).float()
    if idx is not None:
        b[idx.reshape(N, k).cpu() < 0] = float("nan")
    return fq, fk, fv, b.to(DEV), go


@pytest.mark.parametrize("bias", [None, "normal"])
@pytest.mark.parametrize("H,D", HEADS)
def test_lane_layout(ME, H, D, bias):
    N, V, k = 70, 37, 5
    idx = random_index(N, k, V, seed=100 * H + D)
    nmap = ME.NeighborMap.from_index(idx.to(DEV), V)
    fq, fk, fv, b, go = draw(N, V, H * D, k, H, seed=H + D, idx=idx, bias=bias)
    parity(ME, f"lanes H{H} D{D} {bias}", fq, fk, fv, nmap, H, b, go)


@pytest.mark.parametrize("H,D", [(2, 8), (1, 70)])
def test_rows_that_are_not_16_byte_aligned(ME, H, D):
    """D % 4 == 0 but the rows start 4 bytes off: the scalar path, within the bar of the same reference"""
    N, V, k, Cc = 33, 21, 4, H * D
    idx = random_index(N, k, V, seed=D)
    nmap = ME.NeighborMap.from_index(idx.to(DEV), V)
    fq, fk, fv, b, go = draw(N, V, Cc, k, H, seed=D, idx=idx)

    def off(t):
        o = torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(t.shape)
        assert o.data_ptr() % 16 == 4
        return o
    parity(ME, f"misaligned H{H} D{D}", fq, fk, fv, nmap, H, b, go, make_q=off, make_kv=off)


@pytest.mark.parametrize("H,D", [(2, 8), (3, 3)])
@pytest.mark.parametrize("k", [1, 3, 4, 5, 16, 17, 254])
def test_slot_loop(ME, k, H, D):
    N, V = (8, 300) if k == 254 else (45, 31)
    idx = random_index(N, k, V, seed=k)
    nmap = ME.NeighborMap.from_index(idx.to(DEV), V)
    fq, fk, fv, b, go = draw(N, V, H * D, k, H, seed=k, idx=idx)
    parity(ME, f"slots k{k} H{H} D{D}", fq, fk, fv, nmap, H, b, go)


@pytest.mark.parametrize("where", ["first", "middle", "last", "all"])
def test_invalid_slots(ME, where):
    N, V, k, H, D = 50, 19, 6, 2, 8
    idx = random_index(N, k, V, seed=1, invalid=0.0)
    cut = {"first": slice(0, 2), "middle": slice(2, 4), "last": slice(4, 6), "all": slice(0, 6)}[where]
    idx[::2, cut] = -1
    nmap = ME.NeighborMap.from_index(idx.to(DEV), V)
    fq, fk, fv, b, go = draw(N, V, H * D, k, H, seed=2, idx=idx)
    got, _ = parity(ME, f"invalid {where}", fq, fk, fv, nmap, H, b, go)
    if where == "all":                                 # exact zeros, no gradient given or received
        assert not got["out"][::2].any() and not got["dq"][::2].any() and not got["db"][::2].any()
        every = ME.NeighborMap.from_index(torch.full((N, k), -1, device=DEV), V)
        got = engine(ME, fq, fk, fv, every, H, b, go)
        assert not any(got[n].any() for n in ("out", "dq", "dk", "dv", "db"))


def test_capped_knn_map(ME):
    c, q = random_voxels([120, 80], seed=5, side=12), random_voxels([60, 45], seed=6, side=12)
    cm = ME.CoordinateManager(torch.from_numpy(c).to(DEV))
    ycm = ME.CoordinateManager(torch.from_numpy(q).to(DEV))
    x0 = ME.SparseTensor(torch.zeros(200, 1, device=DEV), coordinate_manager=cm)
    y0 = ME.SparseTensor(torch.zeros(105, 1, device=DEV), coordinate_manager=ycm)
    capped = ME.knn_map(x0, 4, y0, max_squared_distance=3)
    kept = capped.valid.cpu()
    assert int((kept == 0).sum()) >= 1 and int(((kept > 0) & (kept < 4)).sum()) >= 1 and int((kept == 4).sum()) >= 1
    H, D = 3, 3
    fq, fk, fv, b, go = draw(105, 200, H * D, 4, H, seed=3, idx=capped.idx)
    got, _ = parity(ME, "capped", fq, fk, fv, capped, H, b, go,
                    make_q=lambda t: ME.SparseTensor(t, coordinate_manager=ycm),
                    make_kv=lambda t: ME.SparseTensor(t, coordinate_manager=cm))
    assert not got["out"].cpu()[kept == 0].any()
    rel = capped.relative_positions()
    assert rel.is_cuda and tuple(rel.shape) == (105, 4, 3) and not rel[capped.idx < 0].any()
    at = capped.idx.clamp(min=0)
    want = torch.where((capped.idx >= 0)[..., None], (x0.C[at][..., 1:] - y0.C[:, None, 1:]).float(), torch.zeros((), device=DEV))
    assert torch.equal(rel, want)


@pytest.mark.parametrize("D", [1, 32, 128, 70])
def test_block_edge(ME, D):
    """N * H (H = 1) at THREADS / G - 1, THREADS / G and THREADS / G + 1 items: the last block short by one, full, and one over"""
    per = THREADS // group_of(D)
    V, k = 23, 3
    for i, N in enumerate((per - 1, per, per + 1)):
        idx = random_index(N, k, V, seed=D + i)
        nmap = ME.NeighborMap.from_index(idx.to(DEV), V)
        fq, fk, fv, b, go = draw(N, V, D, k, 1, seed=i, idx=idx)
        parity(ME, f"edge D{D} N{N}", fq, fk, fv, nmap, 1, b, go)
    # the support side: V * H at the same edges
    for i, V in enumerate((per - 1, per, per + 1)):
        idx = random_index(40, k, V, seed=D + 10 + i)
        nmap = ME.NeighborMap.from_index(idx.to(DEV), V)
        fq, fk, fv, b, go = draw(40, V, D, k, 1, seed=i, idx=idx)
        parity(ME, f"edge D{D} V{V}", fq, fk, fv, nmap, 1, b, go)


@pytest.mark.parametrize("H,D", [(2, 8), (3, 3)])
def test_transposed_table(ME, T, H, D):
    """support rows named by 0, 1, T - 1, T, T + 1, 2 T and 2 T + 1 entries, rows 0 and V - 1 among them"""
    degs = [2 * T + 1, 1, T, 0, T - 1, 2 * T, T + 1]
    V, k = len(degs), 2
    E = sum(degs)
    N = (E + k - 1) // k + 3
    rng = np.random.default_rng(D)
    flat = np.full(N * k, -1, np.int64)
    flat[rng.permutation(N * k)[:E]] = np.concatenate([np.full(d, v) for v, d in enumerate(degs)])
    idx = torch.from_numpy(flat.reshape(N, k))
    nmap = ME.NeighborMap.from_index(idx.to(DEV), V)
    seg = nmap.seg_start.cpu().numpy()
    assert list(seg[1:] - seg[:-1]) == degs and nmap.n_chunks == sum(-(-d // T) for d in degs if d > T)
    fq, fk, fv, b, go = draw(N, V, H * D, k, H, seed=D, idx=idx)
    got, _ = parity(ME, f"table H{H} D{D}", fq, fk, fv, nmap, H, b, go)
    assert not got["dk"][3].any() and not got["dv"][3].any()          # the row no entry names: exact zeros
    assert got["dk"][0].any() and got["dv"][V - 1].any()


def _feats_of(coords, Cc, seed):
    """float32 [V, C]: a function of the coordinates alone (float64 on the host, rounded once)"""
    w = np.random.default_rng(seed).standard_normal((4, Cc))
    return torch.from_numpy(np.sin(coords.cpu().numpy().astype(np.float64) @ w + 0.3).astype(np.float32)).to(DEV)


def test_held_order(ME):
    """the same voxels on a plain and on a Morton-sorted manager (a manager sorts from 4096 rows on): self-attention and a y
    target on another manager, all five tensors torch.equal in the caller's order"""
    c = random_voxels([1500, 1400, 1300], seed=12, side=16)
    yc = random_voxels([1450, 1350, 1400], seed=13, side=16)
    H, D, k = 2, 8, 4
    Cc = H * D
    ct, yt = torch.from_numpy(c), torch.from_numpy(yc)
    results = []
    for sort in (False, True):
        cm = ME.CoordinateManager(ct.to(DEV), spatial_sort=sort)
        ycm = ME.CoordinateManager(yt.to(DEV), spatial_sort=sort)
        assert (cm.perm is not None) == sort and (ycm.perm is not None) == sort
        x0 = ME.SparseTensor(torch.zeros(c.shape[0], 1, device=DEV), coordinate_manager=cm)
        y0 = ME.SparseTensor(torch.zeros(yc.shape[0], 1, device=DEV), coordinate_manager=ycm)
        own, cross = ME.knn_map(x0, k), ME.knn_map(x0, k, y0, max_squared_distance=1)
        assert int((cross.idx < 0).sum()) > 0
        if sort:
            assert own.row_perm is not None and cross.row_perm is not None
        fk, fv = _feats_of(ct, Cc, 1), _feats_of(ct, Cc, 2)
        key, ykey = ME.CoordinateMapKey(cm, 1), ME.CoordinateMapKey(ycm, 1)            # (a key: features in the caller's order)
        kv = lambda t: ME.SparseTensor(t, coordinate_map_key=key)                      # noqa: E731
        for nmap, qc, mq in ((own, ct, kv), (cross, yt, lambda t: ME.SparseTensor(t, coordinate_map_key=ykey))):
            fq, go = _feats_of(qc, Cc, 3), _feats_of(qc, Cc, 4)
            bias = torch.sin(nmap.relative_positions().sum(-1, keepdim=True) * torch.tensor([0.7, 1.3], device=DEV))
            got = engine(ME, fq, fk, fv, nmap, H, bias, go, make_q=mq, make_kv=kv)
            results.append([got[n].cpu() for n in ("out", "dq", "dk", "dv", "db")])
            if not sort:
                want = run_ref(fq, fk, fv, nmap.idx, H, bias, go)
                for n, t in zip(("out", "dq", "dk", "dv", "db"), results[-1]):
                    check(f"held order {n}", t.reshape(want[n].shape), want[n], RTOL)
    for plain, held in zip(results[:2], results[2:]):
        for u, v in zip(plain, held):
            assert torch.equal(u, v)


def test_exact_cases(ME):
    V, N, Cc, H = 50, 257, 24, 3
    rng = np.random.default_rng(9)
    idx = np.full((N, 5), -1, np.int64)
    pick = rng.integers(0, V, N)
    idx[np.arange(N), rng.integers(0, 5, N)] = pick
    nmap = ME.NeighborMap.from_index(torch.from_numpy(idx).to(DEV), V)
    fq, fk, fv, b, _ = draw(N, V, Cc, 5, H, seed=1, idx=torch.from_numpy(idx))
    out = ME.neighbor_attention(fq, fk, fv, nmap, H, bias=b)
    assert same_bytes(out, fv[torch.from_numpy(pick).to(DEV)])            # a single valid slot: that v row bit for bit
    # q = 0, bias = 0: the average of the valid rows
    idx = random_index(N, 7, V, seed=2)
    nmap = ME.NeighborMap.from_index(idx.to(DEV), V)
    fv = torch.randn(V, Cc, device=DEV)
    out = ME.neighbor_attention(torch.zeros(N, Cc, device=DEV), fk, fv, nmap, H, bias=torch.zeros(N, 7, H, device=DEV))
    check("uniform attention is the average", out, ME.neighbor_pool(fv, nmap, "avg"), 1e-6)


@pytest.mark.parametrize("H,D", [(2, 8), (3, 3), (1, 128)])
def test_large_biases_stay_finite(ME, H, D):
    N, V, k = 40, 30, 6
    idx = random_index(N, k, V, seed=3)
    nmap = ME.NeighborMap.from_index(idx.to(DEV), V)
    fq, fk, fv, b, go = draw(N, V, H * D, k, H, seed=D, idx=idx, bias="big")
    assert float(torch.nan_to_num(b).abs().max()) == 100.0
    got, _ = parity(ME, f"big bias H{H} D{D}", fq, fk, fv, nmap, H, b, go)
    assert all(bool(torch.isfinite(t).all()) for t in got.values())


def test_cross_check_against_kernel_attention(ME):
    """the 3 x 3 x 3 kernel map of a block as an index [V, 27] with -1 holes, rel_bias broadcast to [V, 27, H]"""
    V, H, D, K = 150, 2, 8, 27
    cc = np.arange(V)
    coords = np.stack([np.zeros(V, np.int64), cc // 36, (cc // 6) % 6, cc % 6], 1).astype(np.int32)
    cm = ME.CoordinateManager(torch.from_numpy(coords).to(DEV))
    key = ME.CoordinateMapKey(cm, 1)
    idx = torch.full((V, K), -1, dtype=torch.int64)
    for kk, pairs in cm.kernel_map(key, key, kernel_size=3).items():
        idx[pairs[1].cpu(), kk] = pairs[0].cpu()
    assert int((idx < 0).sum()) > 0
    nmap = ME.NeighborMap.from_index(idx.to(DEV), V)
    g = torch.Generator().manual_seed(5)
    fq, fk, fv, go = (torch.randn(V, H * D, generator=g).to(DEV) for _ in range(4))
    rel = torch.randn(K, H, generator=g).to(DEV)
    got = engine(ME, fq, fk, fv, nmap, H, rel[None].expand(V, K, H).contiguous(), go)
    q, k, v = (f.clone().requires_grad_() for f in (fq, fk, fv))
    rb = rel.clone().requires_grad_()
    y = ME.kernel_attention(*(ME.SparseTensor(t, coordinate_map_key=key) for t in (q, k, v)), H, rel_bias=rb, kernel_size=3)
    (y.F * go).sum().backward()
    for name, mine, theirs in (("out", got["out"], y.F.detach()), ("dq", got["dq"], q.grad), ("dk", got["dk"], k.grad),
                               ("dv", got["dv"], v.grad)):
        check(f"kernel_attention {name}", mine, theirs, 1e-6)
    check("kernel_attention drel_bias", got["db"].sum(0), rb.grad, 1e-4)


@pytest.mark.parametrize("needs", [(True, False, False, False), (False, False, False, True), (True, False, False, True),
                                   (False, True, True, False), (False, True, False, False), (False, False, True, False),
                                   (True, True, False, True), (False, False, False, False)])
def test_frozen_inputs(ME, needs):
    N, V, k, H, D = 60, 25, 5, 2, 8
    idx = random_index(N, k, V, seed=4)
    fq, fk, fv, b, go = draw(N, V, H * D, k, H, seed=4, idx=idx)
    full = engine(ME, fq, fk, fv, ME.NeighborMap.from_index(idx.to(DEV), V), H, b, go)
    nmap = ME.NeighborMap.from_index(idx.to(DEV), V)
    got = engine(ME, fq, fk, fv, nmap, H, b, go, needs=needs)
    assert same_bytes(got["out"], full["out"])
    for name, need in zip(("dq", "dk", "dv", "db"), needs):
        assert (got[name] is None) if not need else same_bytes(got[name], full[name]), name
    if not (needs[1] or needs[2]):
        assert "table" not in nmap.__dict__ and "chunks" not in nmap.__dict__
    else:
        assert "table" in nmap.__dict__


@pytest.mark.parametrize("kind", ["voxels", "points"])
def test_the_three_query_forms(ME, kind):
    H, D = 2, 8
    Cc = H * D
    rng = np.random.default_rng(13)
    if kind == "voxels":
        c, qc = random_voxels([300, 200], seed=1, side=10), random_voxels([130, 127], seed=2, side=10)
        cm, ycm = (ME.CoordinateManager(torch.from_numpy(a).to(DEV)) for a in (c, qc))
        mk, mq = (lambda t: ME.SparseTensor(t, coordinate_manager=cm)), (lambda t: ME.SparseTensor(t, coordinate_manager=ycm))
    else:
        c = np.concatenate([rng.integers(0, 2, (500, 1)), rng.random((500, 3)) * 6], 1).astype(np.float32)
        qc = np.concatenate([rng.integers(0, 2, (257, 1)), rng.random((257, 3)) * 6], 1).astype(np.float32)
        # (fields made by _like share the record of their points: one set for the map's check)
        mk = ME.TensorField(torch.zeros(500, 1, device=DEV), torch.from_numpy(c).to(DEV))._like
        mq = ME.TensorField(torch.zeros(257, 1, device=DEV), torch.from_numpy(qc).to(DEV))._like
    V, NQ = c.shape[0], qc.shape[0]
    x0, y0 = mk(torch.zeros(V, 1, device=DEV)), mq(torch.zeros(NQ, 1, device=DEV))
    picks = ME.farthest_point_sampling(x0, 7)
    for tag, nmap, make_q, lead in (("own", ME.knn_map(x0, 5), mk, (V,)), ("picks", ME.knn_map(x0, 4, picks), ident, (2, 7)),
                                    ("y", ME.knn_map(x0, 3, y0), mq, (NQ,))):
        g = torch.Generator().manual_seed(len(tag))
        fq, go = (torch.randn(*lead, Cc, generator=g).to(DEV) for _ in range(2))
        fk, fv = (torch.randn(V, Cc, generator=g).to(DEV) for _ in range(2))
        bias = torch.tanh(nmap.relative_positions()[..., :2].contiguous())             # [..., k, H = 2]
        parity(ME, f"{kind} {tag}", fq, fk, fv, nmap, H, bias, go, make_q=make_q, make_kv=mk)
        out = ME.neighbor_attention(make_q(fq), mk(fk), mk(fv), nmap, H)
        if tag == "picks":
            assert torch.is_tensor(out) and tuple(out.shape) == (2, 7, Cc)
        else:
            assert type(out) is type(x0)


def test_module_against_the_reference(ME):
    torch.manual_seed(0)
    c = random_voxels([260, 240], seed=15, side=10)
    cm = ME.CoordinateManager(torch.from_numpy(c).to(DEV))
    Cc, H, k = 16, 4, 6
    feats = torch.randn(c.shape[0], Cc, device=DEV)
    layer = ME.MinkowskiNeighborAttention(Cc, H, k=k, pos_hidden=8).to(DEV)
    with torch.no_grad():
        layer.pos[2].weight.normal_(0, 0.5)
        layer.pos[2].bias.normal_(0, 0.5)
    go = torch.randn(c.shape[0], Cc, device=DEV)
    names = [n for n, _ in layer.named_parameters()]

    def step():
        layer.zero_grad()
        leaf = feats.clone().requires_grad_()
        out = layer(ME.SparseTensor(leaf, coordinate_manager=cm))
        assert out.coordinate_manager is cm
        (out.F * go).sum().backward()
        return [out.F.detach(), leaf.grad] + [p.grad.clone() for p in layer.parameters()]
    first, second = step(), step()
    assert all(same_bytes(u, v) for u, v in zip(first, second))
    # the module restated with the reference function, float64 on the CPU
    from nattn_ref import nattn_ref
    nmap = ME.knn_map(ME.SparseTensor(feats, coordinate_manager=cm), k)
    P = {n: p.detach().double().cpu().requires_grad_() for n, p in layer.named_parameters()}
    f64 = feats.double().cpu().requires_grad_()
    q, kk, v = (f64 @ P["qkv.weight"].t() + P["qkv.bias"]).split(Cc, dim=1)
    rel = nmap.relative_positions().double().cpu()
    bias = torch.relu(rel @ P["pos.0.weight"].t() + P["pos.0.bias"]) @ P["pos.2.weight"].t() + P["pos.2.bias"]
    want = nattn_ref(q, kk, v, nmap.idx.cpu(), H, bias) @ P["proj.weight"].t() + P["proj.bias"]
    (want * go.double().cpu()).sum().backward()
    check("module out", first[0], want.detach(), RTOL)
    check("module dx", first[1], f64.grad, RTOL)
    for n, got in zip(names, first[2:]):
        if n == "pos.2.bias":
            # A shift of every slot's score leaves a softmax unchanged, so this gradient, the sum of dbias over all entries of a
            # head, is zero in exact arithmetic: the reference holds float64 rounding noise and has no magnitude to scale the
            # bar by.  It is the same sum as pos.2.weight's gradient with the hidden activations replaced by ones, so the bar
            # is taken from that tensor's largest magnitude.
            scale = float(P["pos.2.weight"].grad.abs().max())
            assert float(P[n].grad.abs().max()) <= 1e-12 * scale
            print(f"module d{n}: largest magnitude {float(got.abs().max()):.3e} (bound {RTOL * scale:.3e})")
            assert float(got.abs().max()) <= RTOL * scale
            continue
        check(f"module d{n}", got, P[n].grad, RTOL)


def test_refusals_on_the_device(ME, monkeypatch):
    V, N, k, H = 9, 7, 3, 4
    nmap = ME.NeighborMap.from_index(random_index(N, k, V, seed=0).to(DEV), V)
    q, kk, v = (torch.randn(n, 12, device=DEV) for n in (N, V, V))
    with pytest.raises(ValueError, match="neighbor_attention: bias"):
        ME.neighbor_attention(q, kk, v, nmap, H, bias=torch.randn(N, k, H))              # another device
    with pytest.raises(NotImplementedError, match="neighbor_attention"):
        ME.neighbor_attention(q.double(), kk.double(), v.double(), nmap, H)            # float64 rows on the device
    with pytest.raises(NotImplementedError, match="neighbor_attention"):
        ME.neighbor_attention(q.half(), kk.half(), v.half(), nmap, H)
    from minsu3d_amd.MinkowskiEngine import functional as Fn

    class Old:
        nbr_pool_forward = None
    monkeypatch.setattr(Fn, "get_backend", lambda: Old())
    with pytest.raises(NotImplementedError, match="ms3d_nattn_forward"):
        ME.neighbor_attention(q, kk, v, nmap, H)


def test_empty_sets_keep_the_inputs_in_the_graph(ME):
    for N, V in ((0, 5), (4, 0)):
        nmap = ME.NeighborMap.from_index(torch.full((N, 3), -1, dtype=torch.int64, device=DEV), V)
        q, kk, v = (torch.randn(n, 8, device=DEV, requires_grad=True) for n in (N, V, V))
        b = torch.randn(N, 3, 2, device=DEV, requires_grad=True)
        out = ME.neighbor_attention(q, kk, v, nmap, 2, bias=b)
        assert tuple(out.shape) == (N, 8) and not out.any()
        out.sum().backward()
        assert all(t.grad is not None and tuple(t.grad.shape) == tuple(t.shape) and not t.grad.any() for t in (q, kk, v, b))


class _Abi:
    """the three calls through backend.lib with every pointer one small device buffer (no call below reaches a launch)"""

    def __init__(self, be):
        self.lib = be.lib
        self.buf = torch.zeros(1024, dtype=torch.float32, device=DEV)
        self.p = C.c_void_p(self.buf.data_ptr())

    def args(self, **over):
        a = dict(V=5, N=4, k=3, H=2, D=8, n_chunks=0, ws_bytes=0, ws=None, null=())
        a.update(over)
        return a

    def ptr(self, a, name):
        return C.c_void_p(0) if name in a["null"] else self.p

    def forward(self, **over):
        a = self.args(**over)
        p = lambda n: self.ptr(a, n)                                                   # noqa: E731
        return self.lib.ms3d_nattn_forward(p("q"), p("k"), p("v"), p("bias"), p("idx"), C.c_long(a["V"]), C.c_long(a["N"]),
                                           a["k"], a["H"], a["D"], C.c_float(1.0), p("out"), p("lse"), C.c_void_p(0))

    def backward_q(self, **over):
        a = self.args(**over)
        p = lambda n: self.ptr(a, n)                                                   # noqa: E731
        return self.lib.ms3d_nattn_backward_q(p("q"), p("k"), p("v"), p("bias"), p("idx"), p("out"), p("lse"), p("dout"),
                                              C.c_long(a["V"]), C.c_long(a["N"]), a["k"], a["H"], a["D"], C.c_float(1.0),
                                              p("dq"), p("dbias"), p("delta"), C.c_void_p(0))

    def backward_kv(self, **over):
        a = self.args(**over)
        p = lambda n: self.ptr(a, n)                                                   # noqa: E731
        ws = C.c_void_p(0) if a["ws"] is None else C.c_void_p(a["ws"])
        return self.lib.ms3d_nattn_backward_kv(p("q"), p("k"), p("v"), p("bias"), p("out"), p("lse"), p("delta"), p("dout"),
                                               p("entry_sorted"), p("seg_start"), p("chunk_start"), C.c_long(a["n_chunks"]),
                                               C.c_long(a["V"]), C.c_long(a["N"]), a["k"], a["H"], a["D"], C.c_float(1.0),
                                               p("dk"), p("dv"), ws, C.c_size_t(a["ws_bytes"]), C.c_void_p(0))


def test_c_abi(be):
    abi = _Abi(be)
    every = ("q", "k", "v", "bias", "idx", "out", "lse", "dout", "dq", "dbias", "delta", "entry_sorted", "seg_start",
             "chunk_start", "dk", "dv")
    calls = (abi.forward, abi.backward_q, abi.backward_kv)
    shapes = [dict(k=0), dict(k=255), dict(H=0), dict(D=0), dict(D=129), dict(H=2 ** 30, D=4), dict(k=254, H=2 ** 24, D=1),
              dict(V=-1), dict(N=-1)]
    for call in calls:
        for bad in shapes:
            assert call(**bad) == E_UNSUPPORTED, (call.__name__, bad)
            assert call(null=every, **bad) == E_UNSUPPORTED                 # the shape is refused before any pointer is looked at
        assert call(N=0, null=every) == 0 and call(V=0, null=every) == 0      # nothing to do: no pointer is looked at
    # 2^48 blocks: refused, not wrapped (the grid of the kv pass follows V)
    assert abi.forward(N=2 ** 31 - 1, k=1, H=2 ** 20, D=128) == E_UNSUPPORTED
    assert abi.backward_q(N=2 ** 31 - 1, k=1, H=2 ** 20, D=128) == E_UNSUPPORTED
    assert abi.backward_kv(V=2 ** 31 - 1, k=1, H=2 ** 20, D=128) == E_UNSUPPORTED
    for name in ("q", "k", "v", "idx", "out", "lse"):
        assert abi.forward(null=(name,)) == E_UNSUPPORTED, name
    for name in ("q", "k", "v", "idx", "out", "lse", "dout", "delta"):
        assert abi.backward_q(null=(name,)) == E_UNSUPPORTED, name
    for name in ("q", "k", "v", "out", "lse", "delta", "dout", "entry_sorted", "seg_start", "chunk_start"):
        assert abi.backward_kv(null=(name,)) == E_UNSUPPORTED, name
    assert abi.backward_kv(null=("dk", "dv")) == E_UNSUPPORTED
    lib = be.lib
    assert lib.ms3d_nattn_ws_bytes(C.c_long(3), 16) == 3 * 2 * 16 * 4 and lib.ms3d_nattn_ws_bytes(C.c_long(0), 16) == 0
    base = abi.buf.data_ptr()
    assert abi.backward_kv(n_chunks=3, ws=base, ws_bytes=3 * 2 * 16 * 4 - 1) == E_WORKSPACE          # a short workspace
    assert abi.backward_kv(n_chunks=3, ws=base + 4, ws_bytes=1 << 20) == E_UNSUPPORTED                # a misaligned one
    assert abi.backward_kv(n_chunks=3, ws=None, ws_bytes=1 << 20) == E_UNSUPPORTED
    assert abi.backward_kv(n_chunks=-1) == E_UNSUPPORTED


@pytest.fixture(scope="module", autouse=True)
def report_the_largest_errors():
    """after the module's last test: the largest error seen per tensor (every one was asserted where it was measured)"""
    yield
    print("\nlargest error seen against float64, relative to the reference tensor's largest magnitude: " +
          ", ".join(f"{n} {WORST[n]:.2e}" for n in ("out", "dq", "dk", "dv", "db") if n in WORST))
