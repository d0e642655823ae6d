"""GPU: kernel-map attention (ME.kernel_attention, ME.MinkowskiKernelAttention; csrc/kattn.hip) -- forward, dq, dk, dv and the
two-stage rel_bias gradient.

The yardstick is tests/kattn_ref.py: float64 torch on the CPU over the caller-order features and the index pairs of
CoordinateManager.kernel_map(in_key, out_key, ...), never this engine's arithmetic.  Bound: the project's bar, 1e-4 of the
reference tensor's largest magnitude, for out, dq, dk, dv and dbias alike (a plain float32 restatement of the formulas stays
within 7e-6 of the float64 reference on every tensor, integer biases up to +-120 included, so the bar leaves more than a
factor of ten).  Grids are at most 16^3 per sample; the helpers are this file's own."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kattn_ref import kattn_ref

pytestmark = pytest.mark.gpu
RTOL = 1e-4

# ---- the kernels' constants, each stated once (the line it mirrors in minsu3d_amd/csrc/kattn.hip)
KATTN_THREADS = 256        # constexpr int KATTN_THREADS: threads of a forward / backward_kv workgroup
ROWS_PER_PART = 64         # constexpr int KATTN_ROWS_PER_PART (checked against ms3d_kattn_rows_per_part() below)

GEOMS = {"k3": dict(kernel_size=3, stride=1, dilation=1), "k3d2": dict(kernel_size=3, stride=1, dilation=2),
         "k5": dict(kernel_size=5, stride=1, dilation=1), "k2s2": dict(kernel_size=2, stride=2, dilation=1),
         "k3s2": dict(kernel_size=3, stride=2, dilation=1), "cross3": "cross", "custom": "custom"}
HEADS = [(1, 1), (3, 3), (2, 8), (4, 4), (1, 32), (8, 16), (2, 48), (1, 128)]
CUSTOM_OFFSETS = [(1, 0, 0), (0, -1, 1), (2, 1, 0), (-1, -1, -1), (0, 0, 3)]       # no zero offset: some rows reach nothing


@pytest.fixture(scope="module")
def ME():
    import minsu3d_amd.MinkowskiEngine as me
    return me


@pytest.fixture(scope="module")
def r():
    from minsu3d_amd.backend import get_backend
    rows = int(get_backend().lib.ms3d_kattn_rows_per_part())
    assert rows == ROWS_PER_PART
    return rows


def group_lanes(D):
    """lanes of a (row, head) group on the 16-byte path (D % 4 == 0): attn_core.h group_of(D, 4)"""
    g = 1
    while g < D // 4:
        g *= 2
    return g


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


def cloud(rng, B, G, n):
    """n distinct (b, x, y, z) rows of a B x G^3 grid in random order"""
    cells = rng.choice(B * G ** 3, size=n, replace=False)
    b, rest = np.divmod(cells, G ** 3)
    x, rest = np.divmod(rest, G * G)
    y, z = np.divmod(rest, G)
    return np.stack([b, x, y, z], 1).astype(np.int32)


def block(V):
    """the first V cells of a 6 x 6 x 6 block in raster order: a fully occupied neighbourhood wherever the block has one"""
    c = np.arange(V)
    return np.stack([np.zeros(V, np.int64), c // 36, (c // 6) % 6, c % 6], 1).astype(np.int32)


def isolated(V):
    """V voxels at even coordinates of a 16^3 grid: no two are neighbours, only the centre offset is present"""
    c = np.arange(V)
    return np.stack([np.zeros(V, np.int64), 2 * (c // 64), 2 * ((c // 8) % 8), 2 * (c % 8)], 1).astype(np.int32)


def geometry(ME, name):
    """-> (keyword arguments of kernel_attention and of kernel_map alike, K, stride)"""
    g = GEOMS[name] if isinstance(name, str) else name
    if g == "cross":
        gen = ME.KernelGenerator(kernel_size=3, region_type=ME.RegionType.HYPER_CROSS)
        return dict(kernel_generator=gen), 7, 1
    if g == "custom":
        gen = ME.KernelGenerator(region_type=ME.RegionType.CUSTOM, region_offsets=np.array(CUSTOM_OFFSETS, np.int32))
        return dict(kernel_generator=gen), len(CUSTOM_OFFSETS), 1
    if isinstance(g, dict) and "kernel_generator" in g:
        return g, g["kernel_generator"].kernel_volume, g["kernel_generator"].stride
    return dict(g), g["kernel_size"] ** 3, g["stride"]


def manager(ME, coords, sort=False):
    c = torch.from_numpy(np.ascontiguousarray(coords)).cuda()
    cm = ME.CoordinateManager(c, spatial_sort=sort)
    assert (cm.perm is not None) == sort
    return cm


def engine(ME, key, q_key, geom, H, fq, fk, fv, bias, g, needs=(True, True, True, True), scale=None):
    """ME.kernel_attention on caller-order features -> out and the gradients asked for, all in caller order"""
    nq, nk, nv, nb = needs
    tq, tk, tv = (torch.from_numpy(f).cuda().requires_grad_(n) for f, n in ((fq, nq), (fk, nk), (fv, nv)))
    tb = None if bias is None else torch.from_numpy(bias).cuda().requires_grad_(nb)
    q = ME.SparseTensor(tq, coordinate_map_key=q_key)
    k, v = ME.SparseTensor(tk, coordinate_map_key=key), ME.SparseTensor(tv, coordinate_map_key=key)
    y = ME.kernel_attention(q, k, v, H, rel_bias=tb, scale=scale, **geom)
    assert y.coordinate_manager is q_key.coordinate_manager and y.tensor_stride == q_key.tensor_stride
    out = y.F
    assert out.dtype == torch.float32
    if out.requires_grad:
        (out * torch.from_numpy(g).cuda()).sum().backward()
    return dict(out=out.detach(), dq=tq.grad, dk=tk.grad, dv=tv.grad, db=None if tb is None else tb.grad)


def reference(pairs, K, H, fq, fk, fv, bias, g, scale=None):
    q, k, v = (torch.from_numpy(f).double().requires_grad_(True) for f in (fq, fk, fv))
    b = None if bias is None else torch.from_numpy(bias).double().requires_grad_(True)
    out = kattn_ref(q, k, v, pairs, K, H, b, scale)
    (out * torch.from_numpy(g).double()).sum().backward()
    return dict(out=out.detach(), dq=q.grad, dk=k.grad, dv=v.grad, db=None if b is None else b.grad)


def draw(rng, vq, vk, C, K, H, bias):
    """bias: None, "normal" or "big" (integers in [-120, 120]: exp of a raw score is inf in float32)"""
    fq, fk, fv, g = (rng.standard_normal((n, C)).astype(np.float32) for n in (vq, vk, vk, vq))
    b = None
    if bias == "normal":
        b = rng.standard_normal((K, H)).astype(np.float32)
    elif bias == "big":
        b = rng.integers(-120, 121, (K, H)).astype(np.float32)
    return fq, fk, fv, b, g


def run_case(ME, cm, geom_name, H, D, bias, seed=0, q_key=None, tag=None):
    """parity of forward and all gradients on `cm` (k, v on its stride-1 set; q on q_key, default the layer's own output set)
    -> (engine results, reference results, pairs)"""
    geom, K, stride = geometry(ME, geom_name)
    key = ME.CoordinateMapKey(cm, 1)
    q_key = cm.stride(key, stride) if q_key is None else q_key
    pairs = cm.kernel_map(key, q_key, **geom)
    vq, vk = q_key.coordinate_manager.size(q_key.tensor_stride), cm.size(1)
    rng = np.random.default_rng(1000 * H + D + seed)
    data = draw(rng, vq, vk, H * D, K, H, bias)
    got = engine(ME, key, q_key, geom, H, *data)
    want = reference(pairs, K, H, *data)
    tag = tag or f"{geom_name} H{H} D{D} {bias}"
    for name in ("out", "dq", "dk", "dv") + (("db",) if bias else ()):
        check(f"{tag} {name}", got[name], want[name])
    return got, want, pairs


def empty_rows(pairs, vq):
    seen = torch.zeros(vq, dtype=torch.bool)
    for io in pairs.values():
        seen[io[1].cpu()] = True
    return ~seen


# ---------------------------------------------------------------------------------------------- 1. parity over the reach
@pytest.fixture(scope="module")
def sweep_cm(ME):
    return manager(ME, cloud(np.random.default_rng(3), 2, 10, 300))


@pytest.mark.parametrize("bias", [None, "normal"])
@pytest.mark.parametrize("H,D", HEADS)
@pytest.mark.parametrize("geom_name", list(GEOMS))
def test_parity_sweep(ME, sweep_cm, geom_name, H, D, bias):
    got, want, pairs = run_case(ME, sweep_cm, geom_name, H, D, bias)
    vq = got["out"].size(0)
    if geom_name in ("k2s2", "k3s2"):
        assert vq != sweep_cm.size(1)
    if geom_name == "custom":
        none = empty_rows(pairs, vq)
        assert 10 < int(none.sum()) < vq                 # rows without any input, and rows with
        assert not got["out"][none.cuda()].any() and not got["dq"][none.cuda()].any()
        assert not want["out"][none].any() and not want["dq"][none].any()


# ---------------------------------------------------------------------------------------------- 2. row-count edges
@pytest.mark.parametrize("shape", ["block", "isolated"])
@pytest.mark.parametrize("which", ["1", "2", "r-1", "r", "r+1", "2r+1"])
def test_row_count_edges(ME, r, which, shape):
    """(H, D) = (2, 8): a group is 2 lanes, a forward / backward_kv workgroup takes KATTN_THREADS / 2 = 128 (row, head) items =
    64 rows, a wave 16 rows, a backward_q workgroup one part of r rows: 1, 2, r - 1, r + 1 and 2r + 1 are multiples of none"""
    V = {"1": 1, "2": 2, "r-1": r - 1, "r": r, "r+1": r + 1, "2r+1": 2 * r + 1}[which]
    H, D = 2, 8
    rows_per_workgroup = KATTN_THREADS // group_lanes(D) // H
    assert rows_per_workgroup == 64 and (2 * r + 1) % rows_per_workgroup != 0 and (r + 1) % 16 != 0
    coords = block(V) if shape == "block" else isolated(V)
    got, _, pairs = run_case(ME, manager(ME, coords), "k3", H, D, "normal", seed=V, tag=f"{shape} V{V}")
    n_pairs = sum(io.size(1) for io in pairs.values())
    if shape == "isolated":
        assert n_pairs == V and list(pairs) == [13]
    elif V >= 2 * r + 1:
        assert max(torch.bincount(torch.cat([io[1] for io in pairs.values()])).tolist()) == 27    # every input present


# ---------------------------------------------------------------------------------------------- 3. exact cases
@pytest.mark.parametrize("case", ["kernel_size=1", "isolated k3"])
@pytest.mark.parametrize("H,D", [(2, 8), (3, 3)])
def test_one_input_is_a_copy_bit_for_bit(ME, case, H, D):
    """a single present input: p = 1 exactly, so out is v and dv is dout to the bit (both access paths)"""
    V = 130
    coords, geom_name = (cloud(np.random.default_rng(5), 1, 8, V), dict(kernel_size=1, stride=1, dilation=1)) \
        if case == "kernel_size=1" else (isolated(V), "k3")
    cm = manager(ME, coords)
    geom, K, _ = geometry(ME, geom_name)
    key = ME.CoordinateMapKey(cm, 1)
    fq, fk, fv, b, g = draw(np.random.default_rng(7), V, V, H * D, K, H, "normal")
    got = engine(ME, key, key, geom, H, fq, fk, fv, b, g)
    assert torch.equal(got["out"].cpu(), torch.from_numpy(fv))
    assert torch.equal(got["dv"].cpu(), torch.from_numpy(g))
    want = reference(cm.kernel_map(key, key, **geom), K, H, fq, fk, fv, b, g)
    for name in ("dq", "dk", "db"):                     # (zero: ds = p <dout, v - out> and out is v)
        assert float(got[name].abs().max()) <= 1e-4 * float(want["dv"].abs().max()), name


def test_254_custom_offsets(ME):
    offs = np.array([(x, y, z) for z in range(-3, 3) for y in range(-3, 4) for x in range(-3, 4)], np.int32)[:254]
    gen = ME.KernelGenerator(region_type=ME.RegionType.CUSTOM, region_offsets=offs)
    assert gen.kernel_volume == 254
    cm = manager(ME, cloud(np.random.default_rng(11), 1, 10, 200))
    run_case(ME, cm, dict(kernel_generator=gen), 2, 8, "normal", tag="K254")


# ---------------------------------------------------------------------------------------------- 4. no overflow
@pytest.mark.parametrize("H,D", [(2, 8), (3, 3), (1, 128)])
def test_large_biases_do_not_overflow(ME, sweep_cm, H, D):
    got, _, _ = run_case(ME, sweep_cm, "k3", H, D, "big", seed=9)
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), name


# ---------------------------------------------------------------------------------------------- 5. row order
@pytest.fixture(scope="module")
def sorted_cm(ME):
    """4200 rows: the engine Morton-sorts from 4096 rows on, so the manager holds another order than the caller's"""
    cm = manager(ME, cloud(np.random.default_rng(13), 2, 16, 4200), sort=True)
    assert not torch.equal(cm.perm, torch.arange(4200, device="cuda"))
    return cm


@pytest.mark.parametrize("geom_name", ["k3", "k2s2"])
def test_callers_order_on_a_sorted_manager(ME, sorted_cm, geom_name):
    run_case(ME, sorted_cm, geom_name, 4, 4, "normal", seed=21)


@pytest.mark.parametrize("which", ["plain", "sorted"])
def test_q_on_another_manager(ME, sweep_cm, sorted_cm, which):
    """q on a set of its own (target_map): rows of the cloud, rows beside it and rows far from any input"""
    cm = sweep_cm if which == "plain" else sorted_cm
    rng = np.random.default_rng(23)
    nat = cm.get_coordinates(1).cpu().numpy()
    p = rng.permutation(len(nat))
    rows = np.concatenate([nat[p[:120]], nat[p[120:200]] + np.array([0, 1, 0, -1], np.int32),
                           nat[p[200:220]] + np.array([0, 2048, 0, 0], np.int32)])
    _, first = np.unique(rows, axis=0, return_index=True)
    rows = rows[np.sort(first)]
    rows = rows[rng.permutation(len(rows))].astype(np.int32)
    cmq = ME.CoordinateManager.rooted(torch.from_numpy(rows).cuda(), 1)
    got, _, pairs = run_case(ME, cm, "k3", 2, 8, "normal", seed=25, q_key=ME.CoordinateMapKey(cmq, 1), tag=f"onto {which}")
    none = empty_rows(pairs, len(rows))
    assert int(none.sum()) >= 20 and not got["out"][none.cuda()].any()


# ---------------------------------------------------------------------------------------------- 6. the module
@pytest.mark.parametrize("after_bn", [False, True])
def test_module_against_the_float64_restatement(ME, sweep_cm, after_bn):
    C, H = 16, 4
    cm, V = sweep_cm, sweep_cm.size(1)
    key = ME.CoordinateMapKey(cm, 1)
    torch.manual_seed(31)
    att = ME.MinkowskiKernelAttention(C, H, kernel_size=3).cuda()
    bn = ME.MinkowskiBatchNorm(C).cuda()
    with torch.no_grad():
        att.rel_bias.normal_()
        bn.bn.weight.uniform_(0.5, 1.5)
        bn.bn.bias.uniform_(-0.5, 0.5)
    rng = np.random.default_rng(33)
    fx = rng.standard_normal((V, C)).astype(np.float32)              # unit-variance rows
    g = rng.standard_normal((V, C)).astype(np.float32)
    tx = torch.from_numpy(fx).cuda().requires_grad_(True)
    x = ME.SparseTensor(tx, coordinate_map_key=key)
    if after_bn:
        x = bn(x)
        assert x._pending is not None                                  # the normalisation is still pending in front of the block
    y = att(x)
    assert y.coordinate_manager is cm and y.tensor_stride == 1
    (y.F * torch.from_numpy(g).cuda()).sum().backward()

    names = ["qkv.weight", "qkv.bias", "proj.weight", "proj.bias", "rel_bias"]
    params = dict(att.named_parameters())
    assert sorted(params) == sorted(names)
    p64 = {n: params[n].detach().double().cpu().requires_grad_(True) for n in names}
    x64 = torch.from_numpy(fx).double().requires_grad_(True)
    h = x64
    if after_bn:
        w64, b64 = (t.detach().double().cpu().requires_grad_(True) for t in (bn.bn.weight, bn.bn.bias))
        h = F.batch_norm(h, None, None, w64, b64, training=True, eps=bn.bn.eps)
    q, k, v = F.linear(h, p64["qkv.weight"], p64["qkv.bias"]).split(C, dim=1)
    pairs = cm.kernel_map(key, key, kernel_size=3)
    want = F.linear(kattn_ref(q, k, v, pairs, 27, H, p64["rel_bias"]), p64["proj.weight"], p64["proj.bias"])
    (want * torch.from_numpy(g).double()).sum().backward()
    tag = "module after bn" if after_bn else "module"
    check(f"{tag} forward", y.F, want.detach())
    check(f"{tag} dx", tx.grad, x64.grad)
    for n in names:
        check(f"{tag} d {n}", params[n].grad, p64[n].grad)
    if after_bn:
        check(f"{tag} d bn.weight", bn.bn.weight.grad, w64.grad)
        check(f"{tag} d bn.bias", bn.bn.bias.grad, b64.grad)


# ---------------------------------------------------------------------------------------------- 7. same bytes
def test_same_bytes_on_every_run(ME, r):
    V, H, D = 2 * r + 1, 2, 8
    cm = manager(ME, block(V))
    geom, K, _ = geometry(ME, "k3")
    key = ME.CoordinateMapKey(cm, 1)
    data = draw(np.random.default_rng(41), V, V, H * D, K, H, "normal")
    a = engine(ME, key, key, geom, H, *data)
    b = engine(ME, key, key, geom, H, *data)
    other = torch.randn(3_000_017, device="cuda")                      # an unrelated allocation in between
    c = engine(ME, key, key, geom, H, *data)
    del other
    for name in ("out", "dq", "dk", "dv", "db"):
        assert torch.equal(a[name], b[name]) and torch.equal(a[name], c[name]), name


# ---------------------------------------------------------------------------------------------- 8. frozen inputs
@pytest.mark.parametrize("q_and_bias", [True, False])
@pytest.mark.parametrize("k_and_v", [True, False])
def test_frozen_inputs(ME, sweep_cm, q_and_bias, k_and_v):
    H, D = 4, 4
    geom, K, _ = geometry(ME, "k3")
    key = ME.CoordinateMapKey(sweep_cm, 1)
    V = sweep_cm.size(1)
    data = draw(np.random.default_rng(43), V, V, H * D, K, H, "normal")
    full = engine(ME, key, key, geom, H, *data)
    got = engine(ME, key, key, geom, H, *data, needs=(q_and_bias, k_and_v, k_and_v, q_and_bias))
    assert torch.equal(got["out"], full["out"])
    for name, asked in (("dq", q_and_bias), ("db", q_and_bias), ("dk", k_and_v), ("dv", k_and_v)):
        if asked:
            assert torch.equal(got[name], full[name]), name
        else:
            assert got[name] is None, name
