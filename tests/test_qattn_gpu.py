"""GPU: per-sample query attention (ME.query_attention, ME.MinkowskiQueryAttention; csrc/qattn.hip) -- forward, dqueries, dk, dv.

The yardstick is tests/qattn_ref.py: float64 torch on the CPU over the caller-order coordinates, features and mask, never this
engine's arithmetic.  Bound: the project's bar, 1e-4 of the reference tensor's largest magnitude, for out, dq, dk and dv alike
(a plain float32 restatement of the formulas stays within 6e-6 of the float64 reference on every tensor up to 20 000 rows per
sample and logits of +-96, so the bar leaves more than a factor of ten; the inputs here keep |logit| <= about 100).  Segment
lengths sit at the edges of the library's chunk (1, R - 1, R, R + 1, 2R + 3), batch indices have gaps, the rows of the samples
are interleaved; the helpers are this file's own."""
import itertools

import numpy as np
import pytest
import torch

from qattn_ref import qattn_ref

pytestmark = pytest.mark.gpu
RTOL = 1e-4

QATTN_THREADS = 256        # constexpr int QATTN_THREADS of minsu3d_amd/csrc/qattn.hip: threads of every workgroup
HEADS = [(1, 1), (3, 5), (4, 16), (8, 16), (2, 128), (1, 32)]
QUERIES = [1, 2, 31, 32, 33, 63, 64, 65, 100]


@pytest.fixture(scope="module")
def ME():
    import minsu3d_amd.MinkowskiEngine as me
    return me


@pytest.fixture(scope="module")
def R():
    from minsu3d_amd.backend import get_backend
    rows = int(get_backend().lib.ms3d_qattn_rows_per_chunk())
    assert rows >= 2
    return rows


def items_per_tile(D):
    """(query, head) items of a workgroup: 256 / G with G the lanes of a group -- attn_core.h group_of(D, 4) when D % 4 == 0 (the
    16-byte route: the test tensors are allocations of their own, so aligned), group_of(D, 1) otherwise"""
    n = D // 4 if D % 4 == 0 else D
    g = 1
    while g < n and g < 64:
        g *= 2
    return QATTN_THREADS // g


# ---------------------------------------------------------------------------------------------- helpers (own copies)
def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def check(name, got, want, tol=RTOL):
    assert tuple(got.shape) == tuple(want.shape), (name, tuple(got.shape), tuple(want.shape))
    assert bool(torch.isfinite(got).all()), name
    e = rel_err(got, want)
    print(f"{name}: rel err {e:.3e} (bound {tol:.0e})")
    assert e <= tol, (name, e)


SORT_MIN_ROWS = 4096       # CoordinateManager(spatial_sort=True) keeps the caller's order below this many rows


def cloud(rng, lengths, indices, sortable=False):
    """sum(lengths) distinct (b, x, y, z) rows: lengths[j] voxels of batch index indices[j], the rows of the samples interleaved
    by one random permutation.  sortable: one more sample of SORT_MIN_ROWS rows behind the others (three batch indices on), so
    that a manager asked to Morton-sort the set does"""
    if sortable:
        lengths, indices = list(lengths) + [SORT_MIN_ROWS], list(indices) + [max(indices) + 3]
    rows = []
    for n, b in zip(lengths, indices):
        G = int(np.ceil(n ** (1 / 3))) + 2
        cells = rng.choice(G ** 3, size=n, replace=False)
        x, rest = np.divmod(cells, G * G)
        y, z = np.divmod(rest, G)
        rows.append(np.stack([np.full(n, b), x, y, z], 1))
    c = np.concatenate(rows).astype(np.int32)
    return c[rng.permutation(c.shape[0])]


def draw(rng, coords, Q, C):
    V, B = coords.shape[0], len(set(coords[:, 0].tolist()))
    fq, g = (rng.standard_normal((B, Q, C)).astype(np.float32) for _ in range(2))
    fk, fv = (rng.standard_normal((V, C)).astype(np.float32) for _ in range(2))
    return fq, fk, fv, g


def engine(ME, coords, H, fq, fk, fv, g, mask=None, sort=False, needs=(True, True, True), scale=None):
    """ME.query_attention on caller-order features and mask -> out and the gradients asked for (dk, dv in caller order)"""
    c = torch.from_numpy(np.ascontiguousarray(coords)).cuda()
    cm = ME.CoordinateManager(c, spatial_sort=sort)
    assert (cm.perm is not None) == sort
    key = ME.CoordinateMapKey(cm, 1)
    tq, tk, tv = (torch.from_numpy(f).cuda().requires_grad_(n) for f, n in zip((fq, fk, fv), needs))
    k, v = ME.SparseTensor(tk, coordinate_map_key=key), ME.SparseTensor(tv, coordinate_map_key=key)
    m = None if mask is None else torch.from_numpy(mask).cuda()
    out = ME.query_attention(tq, k, v, H, attn_mask=m, scale=scale)
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(fq.shape)
    assert out.requires_grad == any(needs)
    if out.requires_grad:
        (out * torch.from_numpy(g).cuda()).sum().backward()
    return dict(out=out.detach(), dq=tq.grad, dk=tk.grad, dv=tv.grad)


def reference(coords, H, fq, fk, fv, g, mask=None, scale=None):
    q, k, v = (torch.from_numpy(f).double().requires_grad_(True) for f in (fq, fk, fv))
    m = None if mask is None else torch.from_numpy(mask)
    out = qattn_ref(q, k, v, torch.from_numpy(coords), H, m, scale)
    (out * torch.from_numpy(g).double()).sum().backward()
    return dict(out=out.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def compare(tag, got, want):
    for name in ("out", "dq", "dk", "dv"):
        check(f"{tag} {name}", got[name], want[name])


def sample_of_row(coords):
    """for every caller row the rank of its batch index among the indices present"""
    present = sorted(set(coords[:, 0].tolist()))
    return np.array([present.index(b) for b in coords[:, 0].tolist()])


# ---------------------------------------------------------------------------------------------- 1. segments, heads, routes
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("H,D", HEADS)
def test_segment_lengths_and_heads(ME, R, H, D, sort):
    """every segment length at the chunk's edges in one batch, batch indices with gaps, rows interleaved, a random half mask
    that depends on the caller's row -- on a manager that keeps the caller's order and on a Morton-sorted one"""
    rng = np.random.default_rng(100 * H + D)
    coords = cloud(rng, [1, R - 1, R, R + 1, 2 * R + 3], [0, 2, 5, 6, 9], sortable=sort)
    Q = 33
    data = draw(rng, coords, Q, H * D)
    mask = rng.random((coords.shape[0], Q)) < 0.5
    compare(f"segments H{H} D{D} sort={sort}", engine(ME, coords, H, *data, mask=mask, sort=sort),
            reference(coords, H, *data, mask=mask))


def test_gapped_batch_indices_without_a_mask(ME, R):
    rng = np.random.default_rng(7)
    for sort in (False, True):
        coords = cloud(rng, [R + 1, 1, 37], [0, 2, 5], sortable=sort)
        data = draw(rng, coords, 5, 12)
        compare(f"indices 0,2,5 sort={sort}", engine(ME, coords, 3, *data, sort=sort), reference(coords, 3, *data))


def test_unaligned_rows_take_the_scalar_route(ME, R):
    """D % 4 == 0 with k's rows 4 bytes off a 16-byte boundary (a view into a larger buffer): the scalar route"""
    rng = np.random.default_rng(8)
    coords = cloud(rng, [R + 1, 9], [1, 4])
    H, D, Q = 2, 8, 7
    fq, fk, fv, g = draw(rng, coords, Q, H * D)
    V = coords.shape[0]
    cm = ME.CoordinateManager(torch.from_numpy(coords).cuda())
    buf = torch.zeros(V * H * D + 1, device="cuda")
    tk = buf[1:].view(V, H * D)
    tk.copy_(torch.from_numpy(fk))
    assert tk.data_ptr() % 16 == 4
    tk.requires_grad_(True)
    tq, tv = (torch.from_numpy(f).cuda().requires_grad_(True) for f in (fq, fv))
    key = ME.CoordinateMapKey(cm, 1)
    out = ME.query_attention(tq, ME.SparseTensor(tk, coordinate_map_key=key), ME.SparseTensor(tv, coordinate_map_key=key), H)
    (out * torch.from_numpy(g).cuda()).sum().backward()
    compare("unaligned k", dict(out=out.detach(), dq=tq.grad, dk=tk.grad, dv=tv.grad), reference(coords, H, fq, fk, fv, g))


# ---------------------------------------------------------------------------------------------- 2. query counts
def _query_cases():
    cases = [(Q, 1, 32) for Q in QUERIES]                 # 32 items per tile at (1, 32): 31, 32, 33 are its edges
    for H, D in ((4, 16), (1, 1)):                        # 64 and 256 items per tile: 16 and 256 queries
        t = items_per_tile(D) // H
        cases += [(Q, H, D) for Q in (t - 1, t, t + 1)]
    return cases


@pytest.mark.parametrize("Q,H,D", _query_cases())
def test_query_counts(ME, R, Q, H, D):
    assert items_per_tile(32) == 32 and items_per_tile(16) == 64 and items_per_tile(1) == 256
    rng = np.random.default_rng(Q + 1000 * D)
    coords = cloud(rng, [R + 1, 1, 37], [0, 2, 5])
    data = draw(rng, coords, Q, H * D)
    mask = rng.random((coords.shape[0], Q)) < 0.5
    compare(f"Q{Q} H{H} D{D}", engine(ME, coords, H, *data, mask=mask), reference(coords, H, *data, mask=mask))


# ---------------------------------------------------------------------------------------------- 3. masks
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("kind", ["none", "half", "query_blocked", "voxel_blocked", "sample_blocked"])
def test_masks(ME, R, kind, sort):
    rng = np.random.default_rng(11)
    coords = cloud(rng, [R + 5, 40, 2 * R + 3], [0, 2, 5], sortable=sort)
    V, Q, H, D = coords.shape[0], 6, 4, 16
    seg = sample_of_row(coords)
    data = draw(rng, coords, Q, H * D)
    mask = None
    if kind == "half":
        mask = rng.random((V, Q)) < 0.5
    elif kind == "query_blocked":                       # query 3 of the last sample (two chunks and a tail), nowhere else
        mask = rng.random((V, Q)) < 0.2
        mask[seg != 2, 3] = False
        mask[seg == 2, 3] = True
    elif kind == "voxel_blocked":                       # one voxel of the first sample, for every query
        mask = np.zeros((V, Q), bool)
        mask[np.nonzero(seg == 0)[0][17]] = True
    elif kind == "sample_blocked":
        mask = rng.random((V, Q)) < 0.3
        mask[seg == 1] = True
    got, want = engine(ME, coords, H, *data, mask=mask, sort=sort), reference(coords, H, *data, mask=mask)
    compare(f"mask {kind} sort={sort}", got, want)
    if kind == "query_blocked":                         # nothing to attend to: zero, to the bit, and no gradient
        assert not got["out"][2, 3].any() and not got["dq"][2, 3].any()
        assert got["out"][2, 2].any() and got["out"][1, 3].any()
    if kind == "voxel_blocked":
        i = np.nonzero(seg == 0)[0][17]
        assert not got["dk"][i].any() and not got["dv"][i].any()
    if kind == "sample_blocked":
        assert not got["out"][1].any() and not got["dq"][1].any()
        rows = torch.from_numpy(np.nonzero(seg == 1)[0]).cuda()
        assert not got["dk"][rows].any() and not got["dv"][rows].any()


# ---------------------------------------------------------------------------------------------- 4. large logits
@pytest.mark.parametrize("H,D", [(4, 16), (3, 5)])
def test_large_logits_stay_finite(ME, R, H, D):
    """k scaled so that the largest |logit| is 100: exp of a raw score overflows float32, the subtracted maximum does not"""
    rng = np.random.default_rng(13)
    coords = cloud(rng, [R + 1, 60], [0, 3])
    fq, fk, fv, g = draw(rng, coords, 9, H * D)
    seg = sample_of_row(coords)
    top = 0.0
    for b in range(2):
        s = np.einsum("qhd,ihd->qih", fq[b].reshape(9, H, D).astype(np.float64), fk[seg == b].reshape(-1, H, D).astype(np.float64))
        top = max(top, np.abs(s).max() * D ** -0.5)
    fk = (fk * (100.0 / top)).astype(np.float32)
    got, want = engine(ME, coords, H, fq, fk, fv, g), reference(coords, H, fq, fk, fv, g)
    for t in got.values():
        assert bool(torch.isfinite(t).all())
    compare(f"logits +-100 H{H} D{D}", got, want)


# ---------------------------------------------------------------------------------------------- 5. frozen inputs, bytes
@pytest.fixture(scope="module")
def byte_case(ME, R):
    rng = np.random.default_rng(17)
    coords = cloud(rng, [R + 1, 1, 2 * R + 3], [0, 2, 5], sortable=True)
    H, D, Q = 4, 16, 10
    data = draw(rng, coords, Q, H * D)
    mask = rng.random((coords.shape[0], Q)) < 0.5
    full = engine(ME, coords, H, *data, mask=mask, sort=True)
    return coords, H, data, mask, full


def test_same_bytes_on_every_run(ME, byte_case):
    coords, H, data, mask, full = byte_case
    again = engine(ME, coords, H, *data, mask=mask, sort=True)
    for name in ("out", "dq", "dk", "dv"):
        assert torch.equal(again[name], full[name]), name


@pytest.mark.parametrize("needs", [n for n in itertools.product([True, False], repeat=3) if n != (True, True, True)])
def test_frozen_inputs(ME, byte_case, needs):
    coords, H, data, mask, full = byte_case
    got = engine(ME, coords, H, *data, mask=mask, sort=True, needs=needs)
    assert torch.equal(got["out"], full["out"])
    for name, need in zip(("dq", "dk", "dv"), needs):
        if need:
            assert torch.equal(got[name], full[name]), name
        else:
            assert got[name] is None, name


# ---------------------------------------------------------------------------------------------- 6. the module
def test_module_against_float64_linears(ME, R):
    rng = np.random.default_rng(19)
    coords = cloud(rng, [R + 1, 30], [1, 4])
    V, Q, E, Cin, H = coords.shape[0], 7, 32, 20, 4
    torch.manual_seed(0)
    mod = ME.MinkowskiQueryAttention(E, H, in_channels=Cin).cuda()
    fq = rng.standard_normal((2, Q, E)).astype(np.float32)
    fx = rng.standard_normal((V, Cin)).astype(np.float32)
    g = rng.standard_normal((2, Q, E)).astype(np.float32)
    mask = rng.random((V, Q)) < 0.5
    tq, tx = (torch.from_numpy(f).cuda().requires_grad_(True) for f in (fq, fx))
    x = ME.SparseTensor(tx, torch.from_numpy(coords).cuda())
    out = mod(tq, x, attn_mask=torch.from_numpy(mask).cuda())
    (out * torch.from_numpy(g).cuda()).sum().backward()

    w = {n: p.detach().double().cpu().requires_grad_(True) for n, p in mod.named_parameters()}
    lin = lambda t, n: t @ w[n + ".weight"].t() + w[n + ".bias"]
    q64, x64 = (torch.from_numpy(f).double().requires_grad_(True) for f in (fq, fx))
    k64 = lin(x64, "k_proj")
    k64.retain_grad()
    ref = lin(qattn_ref(lin(q64, "q_proj"), k64, lin(x64, "v_proj"), torch.from_numpy(coords), H, torch.from_numpy(mask)),
              "out_proj")
    (ref * torch.from_numpy(g).double()).sum().backward()
    check("module out", out, ref)
    check("module dqueries", tq.grad, q64.grad)
    check("module dx", tx.grad, x64.grad)
    for n, p in mod.named_parameters():
        if n == "k_proj.bias":
            continue
        check(f"module d{n}", p.grad, w[n].grad)
    # k_proj.bias moves every logit of a (query, head) by the same amount, which a softmax does not see: its gradient, the
    # column sum of the dk rows, is identically zero (1e-16 in float64), so an error relative to it says nothing.  It is held
    # against what the sum is made of: 1e-4 of the largest column sum of |dk|.
    made_of = k64.grad.abs().sum(0).max().item()
    e = (mod.k_proj.bias.grad.double().cpu() - w["k_proj.bias"].grad).abs().max().item() / made_of
    print(f"module dk_proj.bias: err {e:.3e} of the largest column sum of |dk| (bound {RTOL:.0e})")
    assert e <= RTOL


# ---------------------------------------------------------------------------------------------- 7. peak memory
def test_peak_memory_stays_below_one_score_matrix(ME):
    """V = 20 000, Q = 256, 8 heads of 8 channels: what forward + backward allocate above the inputs and the outputs (out, dq,
    dk, dv) stays below V * Q * 4 bytes, ONE float [V, Q] matrix -- the torch composition needs one per head"""
    rng = np.random.default_rng(23)
    coords = cloud(rng, [12000, 8000], [0, 1])
    V, Q, H, D = 20000, 256, 8, 8
    C = H * D
    fq, fk, fv, g = draw(rng, coords, Q, C)
    mask = rng.random((V, Q)) < 0.5
    cm = ME.CoordinateManager(torch.from_numpy(coords).cuda())
    key = ME.CoordinateMapKey(cm, 1)
    tq, tk, tv = (torch.from_numpy(f).cuda().requires_grad_(True) for f in (fq, fk, fv))
    tg, tm = torch.from_numpy(g).cuda(), torch.from_numpy(mask).cuda()
    k, v = ME.SparseTensor(tk, coordinate_map_key=key), ME.SparseTensor(tv, coordinate_map_key=key)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = ME.query_attention(tq, k, v, H, attn_mask=tm)
    out.backward(tg)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    outputs = sum(t.numel() * 4 for t in (out, tq.grad, tk.grad, tv.grad))
    print(f"peak above the inputs {peak / 2 ** 20:.2f} MiB, outputs {outputs / 2 ** 20:.2f} MiB, "
          f"one [V, Q] float matrix {V * Q * 4 / 2 ** 20:.2f} MiB")
    assert peak - outputs < V * Q * 4
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(tk.grad).all())
