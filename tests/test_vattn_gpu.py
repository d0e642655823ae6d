"""GPU: per-sample voxel attention (ME.voxel_attention, ME.MinkowskiVoxelAttention; csrc/vattn.hip) -- forward, dx, dkeys, dvalues.

The yardstick is tests/vattn_ref.py: float64 torch on the CPU over the caller-order coordinates, features and mask, never this
engine's arithmetic.  Bound: the project's bar, 1e-4 of the reference tensor's largest magnitude, for out, dx, dkeys and dvalues
alike (a plain float32 restatement of the formulas stays within 2.7e-6 of the float64 reference on every tensor up to 20 000
rows per sample and logits of +-100, so the bar leaves more than a factor of thirty).  Segment lengths sit at the edges of the
library's chunk (1, R - 1, R, R + 1, 2R + 3), batch indices have gaps, the rows of the samples are interleaved; the helpers are
this file's own."""
import itertools

import numpy as np
import pytest
import torch

from qattn_ref import qattn_ref
from vattn_ref import vattn_ref

pytestmark = pytest.mark.gpu
RTOL = 1e-4

THREADS = 256              # threads of every workgroup of minsu3d_amd/csrc/vattn.hip (SATTN_THREADS of attn_core.h)
HEADS = [(1, 1), (3, 5), (4, 16), (8, 16), (2, 128), (1, 32)]
NAMES = ("out", "dx", "dk", "dv")


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
    """items of a workgroup: 256 / G with G the lanes of a group -- attn_core.h group_of(D, 4) when D % 4 == 0 (the 16-byte
    route: the test tensors are allocations of their own, so aligned), group_of(D, 1) otherwise"""
    n = D // 4 if D % 4 == 0 else D
    g = 1
    while g < n and g < 64:
        g *= 2
    return THREADS // g


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
    """x, keys, values and the gradient of out"""
    V, B = coords.shape[0], len(set(coords[:, 0].tolist()))
    fx, g = (rng.standard_normal((V, C)).astype(np.float32) for _ in range(2))
    fk, fv = (rng.standard_normal((B, Q, C)).astype(np.float32) for _ in range(2))
    return fx, fk, fv, g


def engine(ME, coords, H, fx, fk, fv, g, mask=None, sort=False, needs=(True, True, True), scale=None):
    """ME.voxel_attention on caller-order features and mask -> out and dx in caller order, and the gradients asked for"""
    c = torch.from_numpy(np.ascontiguousarray(coords)).cuda()
    cm = ME.CoordinateManager(c, spatial_sort=sort)
    assert (cm.perm is not None) == sort
    tx, tk, tv = (torch.from_numpy(f).cuda().requires_grad_(n) for f, n in zip((fx, fk, fv), needs))
    x = ME.SparseTensor(tx, coordinate_map_key=ME.CoordinateMapKey(cm, 1))
    m = None if mask is None else torch.from_numpy(mask).cuda()
    y = ME.voxel_attention(x, tk, tv, H, attn_mask=m, scale=scale)
    assert isinstance(y, ME.SparseTensor) and y.coordinate_manager is cm and y.tensor_stride == x.tensor_stride
    out = y.F
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(fx.shape)
    assert out.requires_grad == any(needs)
    if out.requires_grad:
        (out * torch.from_numpy(g).cuda()).sum().backward()
    return dict(out=out.detach(), dx=tx.grad, dk=tk.grad, dv=tv.grad)


def reference(coords, H, fx, fk, fv, g, mask=None, scale=None):
    x, k, v = (torch.from_numpy(f).double().requires_grad_(True) for f in (fx, fk, fv))
    m = None if mask is None else torch.from_numpy(mask)
    out = vattn_ref(x, k, v, torch.from_numpy(coords), H, m, scale)
    (out * torch.from_numpy(g).double()).sum().backward()
    return dict(out=out.detach(), dx=x.grad, dk=k.grad, dv=v.grad)


def compare(tag, got, want):
    for name in NAMES:
        check(f"{tag} {name}", got[name], want[name])


def sample_of_row(coords):
    """for every caller row the rank of its batch index among the indices present"""
    present = sorted(set(coords[:, 0].tolist()))
    return np.array([present.index(b) for b in coords[:, 0].tolist()])


# ---------------------------------------------------------------------------------------------- 1. segments, heads
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


# ---------------------------------------------------------------------------------------------- 2. query counts
def _query_cases():
    """the four-at-a-time loop at (1, 32); the item tiles of the kv sweep: Q * H around one tile of t = 256 / G items -- Q * H
    moves in steps of H, so the nearest counts are (t / H - 1, t / H, t / H + 1) * H; and the limit Q = 1024"""
    cases = [(Q, 1, 32) for Q in (1, 2, 3, 4, 5, 7, 8, 9)]
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


def test_query_count_at_the_limit(ME):
    rng = np.random.default_rng(29)
    coords = cloud(rng, [23, 17], [0, 3])
    Q, H, D = 1024, 1, 4
    data = draw(rng, coords, Q, H * D)
    mask = rng.random((coords.shape[0], Q)) < 0.5
    compare("Q1024 H1 D4", engine(ME, coords, H, *data, mask=mask), reference(coords, H, *data, mask=mask))


# ---------------------------------------------------------------------------------------------- 3. row-item tile edges
def _row_cases():
    """V * H around n tiles of t = 256 / G (held row, head) items of forward and backward_x: exactly n t - 1, n t, n t + 1 at
    (1, 32); at (4, 16) V * H moves in steps of 4, so the rows are n t / 4 - 1, n t / 4, n t / 4 + 1"""
    cases = []
    for H, D, n in ((1, 32, 3), (4, 16, 3)):
        rows = n * items_per_tile(D) // H
        cases += [(V, H, D) for V in (rows - 1, rows, rows + 1)]
    return cases


@pytest.mark.parametrize("V,H,D", _row_cases())
def test_row_item_tile_edges(ME, V, H, D):
    rng = np.random.default_rng(V + 1000 * D)
    coords = cloud(rng, [V - 30, 30], [1, 2])
    assert coords.shape[0] == V
    data = draw(rng, coords, 6, H * D)
    mask = rng.random((V, 6)) < 0.5
    compare(f"V{V} H{H} D{D}", engine(ME, coords, H, *data, mask=mask), reference(coords, H, *data, mask=mask))


# ---------------------------------------------------------------------------------------------- 4. unaligned rows
@pytest.mark.parametrize("which", ["x", "keys"])
def test_unaligned_rows_take_the_scalar_route(ME, R, which):
    """D % 4 == 0 with the rows of x (or of keys) 4 bytes off a 16-byte boundary (a view into a larger buffer): the scalar route"""
    rng = np.random.default_rng(8)
    coords = cloud(rng, [R + 1, 9], [1, 4])
    H, D, Q = 2, 8, 7
    fx, fk, fv, g = draw(rng, coords, Q, H * D)
    src = dict(x=fx, keys=fk)[which]
    buf = torch.zeros(src.size + 1, device="cuda")
    off = buf[1:].view(src.shape)
    off.copy_(torch.from_numpy(src))
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    off.requires_grad_(True)
    tx, tk, tv = (off if which == n else torch.from_numpy(f).cuda().requires_grad_(True)
                  for n, f in (("x", fx), ("keys", fk), ("values", fv)))
    cm = ME.CoordinateManager(torch.from_numpy(coords).cuda())
    y = ME.voxel_attention(ME.SparseTensor(tx, coordinate_map_key=ME.CoordinateMapKey(cm, 1)), tk, tv, H)
    (y.F * torch.from_numpy(g).cuda()).sum().backward()
    compare(f"unaligned {which}", dict(out=y.F.detach(), dx=tx.grad, dk=tk.grad, dv=tv.grad),
            reference(coords, H, fx, fk, fv, g))


# ---------------------------------------------------------------------------------------------- 5. masks
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("kind", ["none", "half", "voxel_blocked", "query_blocked", "sample_blocked"])
def test_masks(ME, R, kind, sort):
    rng = np.random.default_rng(11)
    coords = cloud(rng, [R + 5, 40, 2 * R + 3], [0, 2, 5], sortable=sort)
    V, Q, H, D = coords.shape[0], 6, 4, 16
    seg = sample_of_row(coords)
    data = draw(rng, coords, Q, H * D)
    mask = None
    if kind == "half":
        mask = rng.random((V, Q)) < 0.5
    elif kind == "voxel_blocked":                       # one voxel of the first sample, for every query
        mask = rng.random((V, Q)) < 0.2
        i = np.nonzero(seg == 0)[0][17]
        mask[i] = True
    elif kind == "query_blocked":                       # query 3 of the last sample (two chunks and a tail), nowhere else
        mask = rng.random((V, Q)) < 0.2
        mask[seg != 2, 3] = False
        mask[seg == 2, 3] = True
    elif kind == "sample_blocked":
        mask = rng.random((V, Q)) < 0.3
        mask[seg == 1] = True
    got, want = engine(ME, coords, H, *data, mask=mask, sort=sort), reference(coords, H, *data, mask=mask)
    compare(f"mask {kind} sort={sort}", got, want)
    if kind == "voxel_blocked":                         # nothing to attend to: zero, to the bit, and no gradient
        assert not got["out"][i].any() and not got["dx"][i].any()
        assert got["out"][i - 1].any() and got["out"][i + 1].any() and got["dx"][i - 1].any() and got["dx"][i + 1].any()
    if kind == "query_blocked":
        assert not got["dk"][2, 3].any() and not got["dv"][2, 3].any()
        for b in (0, 1):
            assert got["dk"][b, 3].any() and got["dv"][b, 3].any()
        assert got["dk"][2, 2].any() and got["dv"][2, 2].any()
    if kind == "sample_blocked":
        rows = torch.from_numpy(np.nonzero(seg == 1)[0]).cuda()
        assert not got["out"][rows].any() and not got["dx"][rows].any()
        assert not got["dk"][1].any() and not got["dv"][1].any()
        assert got["dk"][0].any() and got["dv"][2].any()


# ---------------------------------------------------------------------------------------------- 6. large logits
@pytest.mark.parametrize("H,D", [(4, 16), (3, 5)])
def test_large_logits_stay_finite(ME, R, H, D):
    """keys scaled so that the largest |logit| is 100: exp of a raw score overflows float32, the subtracted maximum does not"""
    rng = np.random.default_rng(13)
    coords = cloud(rng, [R + 1, 60], [0, 3])
    fx, fk, fv, g = draw(rng, coords, 9, H * D)
    seg = sample_of_row(coords)
    top = 0.0
    for b in range(2):
        s = np.einsum("ihd,qhd->iqh", fx[seg == b].reshape(-1, H, D).astype(np.float64), fk[b].reshape(9, H, D).astype(np.float64))
        top = max(top, np.abs(s).max() * D ** -0.5)
    fk = (fk * (100.0 / top)).astype(np.float32)
    got, want = engine(ME, coords, H, fx, fk, fv, g), reference(coords, H, fx, fk, fv, g)
    for t in got.values():
        assert bool(torch.isfinite(t).all())
    compare(f"logits +-100 H{H} D{D}", got, want)


# ---------------------------------------------------------------------------------------------- 7. frozen inputs, bytes
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
    for name in NAMES:
        assert torch.equal(again[name], full[name]), name


@pytest.mark.parametrize("needs", [n for n in itertools.product([True, False], repeat=3) if n != (True, True, True)])
def test_frozen_inputs(ME, byte_case, needs):
    coords, H, data, mask, full = byte_case
    got = engine(ME, coords, H, *data, mask=mask, sort=True, needs=needs)
    assert torch.equal(got["out"], full["out"])
    for name, need in zip(("dx", "dk", "dv"), needs):
        if need:
            assert torch.equal(got[name], full[name]), name
        else:
            assert got[name] is None, name


# ---------------------------------------------------------------------------------------------- 8. the modules
def test_module_against_float64_linears(ME, R):
    rng = np.random.default_rng(19)
    coords = cloud(rng, [R + 1, 30], [1, 4])
    V, Q, E, Cq, H = coords.shape[0], 7, 32, 20, 4
    torch.manual_seed(0)
    mod = ME.MinkowskiVoxelAttention(E, H, query_channels=Cq).cuda()
    fx = rng.standard_normal((V, E)).astype(np.float32)
    fq = rng.standard_normal((2, Q, Cq)).astype(np.float32)
    g = rng.standard_normal((V, E)).astype(np.float32)
    mask = rng.random((V, Q)) < 0.5
    tx, tq = (torch.from_numpy(f).cuda().requires_grad_(True) for f in (fx, fq))
    x = ME.SparseTensor(tx, torch.from_numpy(coords).cuda())
    y = mod(x, tq, attn_mask=torch.from_numpy(mask).cuda())
    assert isinstance(y, ME.SparseTensor) and y.coordinate_manager is x.coordinate_manager
    out = y.F
    (out * torch.from_numpy(g).cuda()).sum().backward()

    w = {n: p.detach().double().cpu().requires_grad_(True) for n, p in mod.named_parameters()}
    lin = lambda t, n: t @ w[n + ".weight"].t() + w[n + ".bias"]
    x64, q64 = (torch.from_numpy(f).double().requires_grad_(True) for f in (fx, fq))
    k64 = lin(q64, "k_proj")
    k64.retain_grad()
    ref = lin(vattn_ref(lin(x64, "q_proj"), k64, lin(q64, "v_proj"), torch.from_numpy(coords), H, torch.from_numpy(mask)),
              "out_proj")
    (ref * torch.from_numpy(g).double()).sum().backward()
    check("module out", out, ref)
    check("module dx", tx.grad, x64.grad)
    check("module dqueries", tq.grad, q64.grad)
    for n, p in mod.named_parameters():
        if n == "k_proj.bias":
            continue
        check(f"module d{n}", p.grad, w[n].grad)
    # k_proj.bias moves every logit of a (row, head) by the same amount, which a softmax does not see: its gradient, the
    # column sum of the dkeys rows over B * Q, is identically zero (1e-16 in float64), so an error relative to it says nothing
    # (tests/test_qattn_gpu.py).  It is held against what the sum is made of: 1e-4 of the largest column sum of |dkeys|.
    made_of = k64.grad.abs().sum((0, 1)).max().item()
    e = (mod.k_proj.bias.grad.double().cpu() - w["k_proj.bias"].grad).abs().max().item() / made_of
    print(f"module dk_proj.bias: err {e:.3e} of the largest column sum of |dkeys| (bound {RTOL:.0e})")
    assert e <= RTOL


@pytest.mark.parametrize("sort", [False, True])
def test_two_way_step_on_one_manager_and_one_mask(ME, R, sort):
    """query_attention, then voxel_attention of the same voxels over the refined queries: one manager, one mask, one chunk list"""
    rng = np.random.default_rng(31)
    coords = cloud(rng, [R + 1, 30, 2 * R + 3], [1, 4, 6], sortable=sort)
    V, B, Q, H, D = coords.shape[0], 4 if sort else 3, 9, 4, 8
    C = H * D
    fq = rng.standard_normal((B, Q, C)).astype(np.float32)
    fx, g = (rng.standard_normal((V, C)).astype(np.float32) for _ in range(2))
    mask = rng.random((V, Q)) < 0.5
    cm = ME.CoordinateManager(torch.from_numpy(coords).cuda(), spatial_sort=sort)
    assert (cm.perm is not None) == sort
    tq, tx = (torch.from_numpy(f).cuda().requires_grad_(True) for f in (fq, fx))
    x = ME.SparseTensor(tx, coordinate_map_key=ME.CoordinateMapKey(cm, 1))
    tm = torch.from_numpy(mask).cuda()
    chunks = cm.batch_chunks(1)
    refined = ME.query_attention(tq, x, x, H, attn_mask=tm)
    y = ME.voxel_attention(x, refined, refined, H, attn_mask=tm)
    assert cm.batch_chunks(1) is chunks                        # no second chunk list
    (y.F * torch.from_numpy(g).cuda()).sum().backward()

    q64, x64 = (torch.from_numpy(f).double().requires_grad_(True) for f in (fq, fx))
    c, m = torch.from_numpy(coords), torch.from_numpy(mask)
    r64 = qattn_ref(q64, x64, x64, c, H, m)
    ref = vattn_ref(x64, r64, r64, c, H, m)
    (ref * torch.from_numpy(g).double()).sum().backward()
    check(f"two-way sort={sort} refined", refined, r64)
    check(f"two-way sort={sort} out", y.F, ref)
    check(f"two-way sort={sort} dqueries", tq.grad, q64.grad)
    check(f"two-way sort={sort} dx", tx.grad, x64.grad)


# ---------------------------------------------------------------------------------------------- 9. peak memory
def test_peak_memory_stays_below_one_score_matrix(ME):
    """V = 20 000, Q = 256, 8 heads of 8 channels: what forward + backward allocate above the inputs and the outputs (out, dx,
    dkeys, dvalues) stays below V * Q * 4 bytes, ONE float [V, Q] matrix -- the torch composition needs one per head.  By the
    formulas: 40 chunks * 256 * 2 * 64 floats = 5.2 MB of partials and 1.3 MB of lse / delta, against 20.5 MB"""
    rng = np.random.default_rng(23)
    coords = cloud(rng, [12000, 8000], [0, 1])
    V, Q, H, D = 20000, 256, 8, 8
    fx, fk, fv, g = draw(rng, coords, Q, H * D)
    mask = rng.random((V, Q)) < 0.5
    cm = ME.CoordinateManager(torch.from_numpy(coords).cuda())
    tx, tk, tv = (torch.from_numpy(f).cuda().requires_grad_(True) for f in (fx, fk, fv))
    tg, tm = torch.from_numpy(g).cuda(), torch.from_numpy(mask).cuda()
    x = ME.SparseTensor(tx, coordinate_map_key=ME.CoordinateMapKey(cm, 1))
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = ME.voxel_attention(x, tk, tv, H, attn_mask=tm).F
    out.backward(tg)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    outputs = sum(t.numel() * 4 for t in (out, tx.grad, tk.grad, tv.grad))
    print(f"peak above the inputs {peak / 2 ** 20:.2f} MiB, outputs {outputs / 2 ** 20:.2f} MiB, "
          f"one [V, Q] float matrix {V * Q * 4 / 2 ** 20:.2f} MiB")
    assert peak - outputs < V * Q * 4
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(tk.grad).all())
