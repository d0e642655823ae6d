"""GPU: arithmetic across coordinate sets -- ms3d_coords_union, the combine / broadcast kernels of csrc/setops.hip and the
layers over them (MinkowskiUnion, SparseTensor + - *, the MinkowskiBroadcast family).

Yardsticks: coordinates and maps bit for bit against tests/setops_ref.py (pinned against dense torch in test_setops_cpu.py);
forward values and the gather / single-product gradients EXACT against its float32 restatements (every element is a fixed
chain of at most N IEEE additions or one multiplication); the long sum of the global operand's gradient and the two composed
networks against float64 at the project's bar, 1e-4 of the largest magnitude of the float64 result (test_geometry_gpu.RTOL).

The tests print the worst dg error of ms3d_broadcast_reduce and the times of the size case; no run on an MI355X has been
recorded yet (DESIGN 4.2 says so).
"""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import setops_ref as R
from generative_ref import expand_np
from sparse_ref import random_sparse
from test_geometry_gpu import RTOL, check, dense_conv, dense_weight, densify64, manager_at, read_dense, rel_err

pytestmark = pytest.mark.gpu
CHANNELS = [1, 6, 16, 33, 64]


@pytest.fixture(scope="module")
def ME():
    import minsu3d_amd.MinkowskiEngine as me
    return me


@pytest.fixture(scope="module")
def be():
    from minsu3d_amd.backend import get_backend
    return get_backend()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def make_sets(rng, n_sets, n=300, B=3, grid=12, shift=0, ts=1):
    """overlapping windows of one pool of distinct coordinates, each shuffled: neighbouring sets share rows and each has rows
    of its own; coordinates are multiples of ts, moved by `shift` cells (negative coordinates)"""
    pool, _ = random_sparse(rng, B=B, grid=grid, n=n * (n_sets + 1) // 2, C=1)
    pool = pool.copy()
    pool[:, 1:] = (pool[:, 1:] + shift) * ts
    sets = []
    for i in range(n_sets):
        c = pool[i * n // 2:i * n // 2 + n].copy()
        rng.shuffle(c)
        sets.append(c)
    return sets


def big_cloud(rng, n, B=2, grid=160):
    c = np.unique(np.concatenate([rng.integers(0, B, (n + n // 4, 1)), rng.integers(0, grid, (n + n // 4, 3))], 1)
                  .astype(np.int32), axis=0)
    assert len(c) >= n
    rng.shuffle(c)
    return c[:n]


# ---------------------------------------------------------------------------------------------- 1. coordinates
@pytest.mark.parametrize("ts", [1, 2, 4])
@pytest.mark.parametrize("n_sets", [2, 3, 5])
def test_coords_union_exact(be, n_sets, ts):
    rng = np.random.default_rng(100 + 10 * n_sets + ts)
    sets = make_sets(rng, n_sets, shift=-5, ts=ts)
    assert min(c[:, 1:].min() for c in sets) < 0 and len(np.unique(np.concatenate(sets)[:, 0])) == 3
    # + an empty set in the middle and a set equal to set 0 (other row order) at the end
    variants = [sets, sets[:1] + [np.zeros((0, 4), np.int32)] + sets[1:-1] + [sets[0][::-1].copy()]]
    for v in variants:
        want, want_rows, want_in = R.union_np(v)
        out, out_rows, in_row = be.coords_union([dev(c) for c in v])
        assert out.dtype == torch.int32 and np.array_equal(host(out), want)
        assert np.array_equal(host(in_row), want_in)
        for got, w in zip(out_rows, want_rows):
            assert got.dtype == torch.int32 and np.array_equal(host(got), w)
        again = be.coords_union([dev(c) for c in v])
        assert torch.equal(again[0], out) and torch.equal(again[2], in_row)
        assert all(torch.equal(a, b) for a, b in zip(again[1], out_rows))
    empty = be.coords_union([dev(np.zeros((0, 4), np.int32))] * 2)
    assert tuple(empty[0].shape) == (0, 4) and tuple(empty[2].shape) == (2, 0)


def test_coords_union_refuses_repeats_and_range(be):
    from minsu3d_amd import _lib
    rng = np.random.default_rng(5)
    a, b = make_sets(rng, 2)
    _, _, in_row = R.union_np([a, b])
    common = np.nonzero((in_row[0] >= 0) & (in_row[1] >= 0))[0]
    only_b = np.nonzero((in_row[0] < 0) & (in_row[1] >= 0))[0]
    for u in (common[0], only_b[0]):                          # a row of set 1 again inside set 1: one that set 0 holds too (the
        twice = np.concatenate([b, b[in_row[1, u]][None]])    # slot's winner is then a row of set 0), and one only set 1 holds
        with pytest.raises(_lib.HipLibraryError, match=str(_lib.E_UNSUPPORTED)):
            be.coords_union([dev(a), dev(twice)])
    with pytest.raises(_lib.HipLibraryError, match=str(_lib.E_UNSUPPORTED)):
        be.coords_union([dev(np.concatenate([a[3:4], a])), dev(b)])
    for bad in ([0, 16384, 0, 0], [0, 0, -16385, 0], [1 << 19, 0, 0, 0], [-1, 0, 0, 0]):
        far = b.copy()
        far[11] = bad
        with pytest.raises(_lib.HipLibraryError, match=str(_lib.E_UNSUPPORTED)):
            be.coords_union([dev(a), dev(far)])
    edge = b.copy()
    edge[11] = [(1 << 19) - 1, 16383, -16384, 0]              # the corners of the packable range are legal
    out, _, _ = be.coords_union([dev(a), dev(edge)])
    assert np.array_equal(host(out), R.union_np([a, edge])[0])
    with pytest.raises(_lib.HipLibraryError, match=str(_lib.E_UNSUPPORTED)):
        be.coords_union([dev(a)] * 17)
    # the same coordinate in two DIFFERENT sets is what a union is for
    out, _, _ = be.coords_union([dev(a), dev(a)])
    assert np.array_equal(host(out), a)


def test_union_on_a_morton_sorted_manager(ME):
    """>= 100 000 rows at tensor stride 1: the engine holds the rows Morton-sorted; the union is taken over the rows the caller
    sees and the maps carry the permutation (no pass that un-permutes all rows)"""
    rng = np.random.default_rng(9)
    pool = big_cloud(rng, 180000)
    ca, cb = pool[:120000], np.ascontiguousarray(pool[60000:][::-1])
    fa = rng.standard_normal((len(ca), 16)).astype(np.float32)
    fb = rng.standard_normal((len(cb), 16)).astype(np.float32)
    la, lb = dev(fa).requires_grad_(True), dev(fb).requires_grad_(True)
    a = ME.SparseTensor(la, coordinates=dev(ca))
    b = ME.SparseTensor(lb, coordinates=dev(cb))
    for t in (a, b):
        assert t.coordinate_manager.perm is not None, "the case needs a Morton-sorted manager"
    want, want_rows, want_in = R.union_np([ca, cb])
    y = a + b
    assert y.tensor_stride == 1 and y.coordinate_manager is not a.coordinate_manager
    assert np.array_equal(host(y.C), want)
    cm, in_rows, out_rows, n = a.coordinate_manager.union(1, [b.coordinate_manager])
    assert cm is y.coordinate_manager and n == len(want)
    for i, t in enumerate((a, b)):
        perm = host(t.coordinate_manager.perm)
        held = host(in_rows[i])
        assert np.array_equal(np.where(held >= 0, perm[np.maximum(held, 0)], -1), want_in[i])
        assert np.array_equal(host(out_rows[i]), want_rows[i][perm])
    assert np.array_equal(host(y.F), R.combine_np(R.SUM, [fa, fb], want_in))
    p = a * b
    assert p.coordinate_manager is y.coordinate_manager           # one union per pair of managers
    assert np.array_equal(host(p.F), R.combine_np(R.MUL, [fa, fb], want_in))
    z = y + p                                                     # same set now: rows add up one to one
    assert z.coordinate_manager is y.coordinate_manager and torch.equal(z.F, y.F + p.F)
    dout = rng.standard_normal((len(want), 16)).astype(np.float32)
    (p.F * dev(dout)).sum().backward()
    for i, leaf in enumerate((la, lb)):                           # the leaves are in the caller's row order
        g = R.combine_backward_np(R.MUL, i, dout, want_rows[i], (fb, fa)[i], want_in[1 - i])
        assert np.array_equal(host(leaf.grad), g)
    # a [V, C] tensor operand is in the caller's row order
    assert torch.equal((a + dev(fa)).F, a.F + dev(fa))


# ---------------------------------------------------------------------------------------------- 2. values and gradients
def _tensors(ME, sets, feats, ts=1):
    out = []
    for c, f in zip(sets, feats):
        cm = ME.CoordinateManager(dev(c)) if ts == 1 else ME.CoordinateManager.rooted(dev(c), ts)
        out.append(ME.SparseTensor(dev(f).requires_grad_(True), coordinate_manager=cm, tensor_stride=ts))
    return out


@pytest.mark.parametrize("C", CHANNELS)
def test_combine_values_and_gradients_exact(ME, C):
    rng = np.random.default_rng(40 + C)
    for op, n_sets, ts in ((R.SUM, 2, 1), (R.SUM, 5, 2), (R.SUB, 2, 1), (R.MUL, 2, 4)):
        sets = make_sets(rng, n_sets, shift=-3, ts=ts)
        if n_sets == 5:
            sets[2] = np.zeros((0, 4), np.int32)                  # a pruned-away operand
        feats = [rng.standard_normal((len(c), C)).astype(np.float32) for c in sets]
        want_c, want_rows, want_in = R.union_np(sets)
        ts_ = _tensors(ME, sets, feats, ts)
        if op == R.SUM:
            y = ME.MinkowskiUnion()(*ts_)
            if n_sets == 2:
                assert torch.equal((ts_[0] + ts_[1]).F, y.F)
        else:
            y = ts_[0] - ts_[1] if op == R.SUB else ts_[0] * ts_[1]
        assert y.tensor_stride == ts and np.array_equal(host(y.C), want_c)
        want = R.combine_np(op, feats, want_in)
        assert np.array_equal(host(y.F), want), (op, C)
        dout = rng.standard_normal(want.shape).astype(np.float32)
        y.F.backward(dev(dout))
        grads = []
        for i, t in enumerate(ts_):
            other = dict(other=feats[1 - i], other_row=want_in[1 - i]) if op == R.MUL else {}
            g = R.combine_backward_np(op, i, dout, want_rows[i], **other)
            if len(sets[i]) == 0:
                assert t._F.grad is None or t._F.grad.numel() == 0
                continue
            assert np.array_equal(host(t._F.grad), g), (op, C, i)
            grads.append(t._F.grad.clone())
        # reproducibility: the same operands again, forward and backward
        ts2 = _tensors(ME, sets, feats, ts)
        y2 = ME.MinkowskiUnion()(*ts2) if op == R.SUM else (ts2[0] - ts2[1] if op == R.SUB else ts2[0] * ts2[1])
        assert torch.equal(y2.F, y.F)
        y2.F.backward(dev(dout))
        assert all(torch.equal(a, b) for a, b in zip(grads, [t._F.grad for t in ts2 if t._F.grad is not None
                                                             and t._F.grad.numel()]))


def test_union_of_one_and_of_a_pending_batchnorm(ME):
    rng = np.random.default_rng(3)
    sets = make_sets(rng, 2)
    feats = [rng.standard_normal((len(c), 8)).astype(np.float32) for c in sets]
    a, b = _tensors(ME, sets, feats)
    one = ME.MinkowskiUnion()(a)
    assert torch.equal(one.F, a.F) and torch.equal(one.C, a.C)
    bn = ME.MinkowskiBatchNorm(8).cuda().train()
    an = ME.MinkowskiReLU()(bn(a))
    assert an._pending is not None
    y = an + b                                                    # the pending BatchNorm + ReLU is materialised first
    _, _, want_in = R.union_np(sets)
    assert np.array_equal(host(y.F), R.combine_np(R.SUM, [host(an.F), feats[1]], want_in))


LAYERS = {R.ADD: "MinkowskiBroadcastAddition", R.MULTIPLY: "MinkowskiBroadcastMultiplication",
          R.CAT: "MinkowskiBroadcastConcatenation", R.COPY: "MinkowskiBroadcast"}
_DG_WORST = {}


@pytest.mark.parametrize("C", CHANNELS)
def test_broadcast_values_and_gradients(ME, C):
    rng = np.random.default_rng(60 + C)
    V, B = 20000, 4
    coords = big_cloud(rng, V, B=B, grid=40)
    x = rng.standard_normal((V, C)).astype(np.float32)
    g_batch = np.array([3, 0, 2], np.int32)                       # batch 1 has no global row; rows not in batch order
    grow = R.grow_np(coords[:, 0], g_batch)
    assert (grow == -1).any()
    gc = np.zeros((3, 4), np.int32)
    gc[:, 0] = g_batch
    for mode in (R.ADD, R.MULTIPLY, R.CAT, R.COPY):
        cg = C if mode in (R.ADD, R.MULTIPLY) else (C + 3 if C % 4 else 8)
        g = rng.standard_normal((3, cg)).astype(np.float32)
        res = []
        for rep in range(2):
            xt = ME.SparseTensor(dev(x).requires_grad_(True), coordinate_manager=ME.CoordinateManager(dev(coords)))
            gt = ME.SparseTensor(dev(g).requires_grad_(True), coordinates=dev(gc))
            y = getattr(ME, LAYERS[mode])()(xt, gt)
            assert y.coordinate_manager is xt.coordinate_manager and y.tensor_stride == 1
            want = R.broadcast_np(mode, x, g, grow)
            assert np.array_equal(host(y.F), want), (mode, C)
            dout = np.random.default_rng(7).standard_normal(want.shape).astype(np.float32)
            y.F.backward(dev(dout))
            if mode == R.ADD:
                assert np.array_equal(host(xt._F.grad), dout)
            elif mode == R.CAT:
                assert np.array_equal(host(xt._F.grad), dout[:, :C])
            elif mode == R.MULTIPLY:
                assert np.array_equal(host(xt._F.grad), dout * R.broadcast_np(R.COPY, None, g, grow))
            else:
                assert xt._F.grad is None
            dg = R.broadcast_dg_np(mode, dout, x, grow, 3, C)
            e = np.abs(host(gt._F.grad).astype(np.float64) - dg).max() / np.abs(dg).max()
            _DG_WORST[(mode, C)] = e
            print(f"broadcast mode {mode} C={C} Cg={cg}: dg rel err {e:.3e} (bound {RTOL:.0e})")
            assert e <= RTOL, (mode, C, e)
            res.append((y.F.clone(), gt._F.grad.clone(), None if xt._F.grad is None else xt._F.grad.clone()))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        assert res[0][2] is None or torch.equal(res[0][2], res[1][2])
    print(f"broadcast dg worst rel err so far: {max(_DG_WORST.values()):.3e}")


def test_broadcast_takes_what_global_pooling_returns(ME):
    """the map is cached per (set of x, set of x_glob); a voxel-less batch of x_glob and stride-2 inputs work"""
    rng = np.random.default_rng(77)
    fine, _ = random_sparse(rng, B=3, grid=12, n=500, C=1)
    cm = manager_at(ME, fine, 2)
    c2 = host(cm.coords[2])
    x = rng.standard_normal((len(c2), 8)).astype(np.float32)
    xt = ME.SparseTensor(dev(x).requires_grad_(True), coordinate_manager=cm, tensor_stride=2)
    pooled = ME.MinkowskiGlobalAvgPooling()(xt)
    y = ME.MinkowskiBroadcastMultiplication()(xt, pooled)
    assert y.tensor_stride == 2 and y.coordinate_manager is cm
    mean = np.stack([x[c2[:, 0] == b].astype(np.float64).mean(0) for b in range(3)])
    want = x.astype(np.float64) * mean[c2[:, 0]]
    assert np.abs(host(y.F) - want).max() <= RTOL * np.abs(want).max()
    m1 = cm.broadcast_map(2, pooled.coordinate_manager, 1)
    assert m1[0] is cm.broadcast_map(2, pooled.coordinate_manager, 1)[0]


# ---------------------------------------------------------------------------------------------- 3. composition
def _se_block(ME, C, seed):
    torch.manual_seed(seed)
    net = torch.nn.ModuleDict(dict(
        conv1=ME.MinkowskiConvolution(C, C, kernel_size=3, dimension=3), bn=ME.MinkowskiBatchNorm(C),
        conv2=ME.MinkowskiConvolution(C, C, kernel_size=3, dimension=3), pool=ME.MinkowskiGlobalAvgPooling(),
        fc=ME.MinkowskiLinear(C, C), gate=ME.MinkowskiSigmoid(), scale=ME.MinkowskiBroadcastMultiplication())).cuda().train()
    with torch.no_grad():
        net["bn"].bn.weight.uniform_(0.5, 1.5)
        net["bn"].bn.bias.uniform_(-0.3, 0.3)
    return net


def _se_forward(net, x):
    y = net["conv2"](net["bn"](net["conv1"](x)))
    return net["scale"](y, net["gate"](net["fc"](net["pool"](y)))) + x


def test_squeeze_and_excitation_block_against_dense(ME):
    """conv -> BatchNorm -> conv -> global average pool -> linear -> sigmoid -> broadcast-multiply -> + skip, no ReLU on the
    sparse rows (a flipped ReLU mask moves a gradient by whole terms); float64 dense torch, every gradient"""
    B, G, C = 2, 10, 16
    rng = np.random.default_rng(201)
    coords, feats = random_sparse(rng, B=B, grid=G, n=500, C=C)
    net = _se_block(ME, C, 1)
    xf = dev(feats).requires_grad_(True)
    out = _se_forward(net, ME.SparseTensor(xf, coordinate_manager=ME.CoordinateManager(dev(coords))))
    p64 = {n: p.detach().double().cpu().requires_grad_(True) for n, p in net.named_parameters()}
    x64 = torch.from_numpy(feats).double().requires_grad_(True)
    h = dense_conv(coords, x64, p64["conv1.kernel"], None, 3, 1, 1, 1, coords, B, G)
    h = F.batch_norm(h, None, None, p64["bn.bn.weight"], p64["bn.bn.bias"], True, 0.1, 1e-5)
    h = dense_conv(coords, h, p64["conv2.kernel"], None, 3, 1, 1, 1, coords, B, G)
    b = torch.from_numpy(coords[:, 0]).long()
    onehot = F.one_hot(b, B).double()
    pooled = (onehot.t() @ h) / onehot.sum(0).view(-1, 1)
    gate = torch.sigmoid(pooled @ p64["fc.linear.weight"].t() + p64["fc.linear.bias"])
    want = h * gate[b] + x64
    check("SE block forward", out.F, want, RTOL)
    g = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    out.F.backward(dev(g))
    want.backward(torch.from_numpy(g).double())
    check("SE block input gradient", xf.grad, x64.grad, RTOL)
    for n, p in net.named_parameters():
        check(f"SE block d {n}", p.grad, p64[n].grad.view(p.grad.shape), RTOL)


def _decoder(ME, C, seed):
    torch.manual_seed(seed)
    return torch.nn.ModuleDict(dict(
        up=ME.MinkowskiGenerativeConvolutionTranspose(C, C, kernel_size=2, stride=2, dimension=3),
        conv=ME.MinkowskiConvolution(C, C, kernel_size=3, dimension=3))).cuda().train()


def _decoder_forward(ME, net, x, e, mask):
    s = net["up"](x) + e
    kept = ME.MinkowskiPruning()(s, mask)
    return s, kept, net["conv"](kept)


def _decoder_inputs(ME, rng, C, B=2, G=12):
    fine, _ = random_sparse(rng, B=B, grid=G, n=300, C=1)
    cm = manager_at(ME, fine, 2)
    c2 = host(cm.coords[2])
    enc, fe = random_sparse(rng, B=B, grid=G, n=400, C=C)
    fx = rng.standard_normal((len(c2), C)).astype(np.float32)
    return cm, c2, fx, enc, fe


def test_decoder_step_against_dense(ME):
    """generative transposed convolution + an encoder tensor on another manager -> pruning -> k3 convolution"""
    B, G, C = 2, 12, 16
    rng = np.random.default_rng(301)
    cm, c2, fx, enc, fe = _decoder_inputs(ME, rng, C, B, G)
    net = _decoder(ME, C, 2)
    xf, ef = dev(fx).requires_grad_(True), dev(fe).requires_grad_(True)
    x = ME.SparseTensor(xf, coordinate_manager=cm, tensor_stride=2)
    e = ME.SparseTensor(ef, coordinates=dev(enc))
    gen_c = expand_np(c2, 2, 2, 1, 2)
    union_c, _, in_row = R.union_np([gen_c, enc])
    assert ((in_row[0] >= 0) & (in_row[1] >= 0)).any() and (in_row[0] < 0).any() and (in_row[1] < 0).any()
    mask = rng.random(len(union_c)) < 0.7
    s, kept, out = _decoder_forward(ME, net, x, e, dev(mask))
    assert np.array_equal(host(s.C), union_c) and np.array_equal(host(kept.C), union_c[mask])
    W_up = net["up"].kernel.detach().double().cpu().requires_grad_(True)
    W_c = net["conv"].kernel.detach().double().cpu().requires_grad_(True)
    x64 = torch.from_numpy(fx).double().requires_grad_(True)
    e64 = torch.from_numpy(fe).double().requires_grad_(True)
    up = F.conv_transpose3d(densify64(c2, x64, B, G // 2, 2), dense_weight(W_up, 2).transpose(0, 1), stride=2)
    assert up.shape[-1] == G
    total = up + densify64(enc, e64, B, G, 1)
    s64 = read_dense(total, union_c, 1)
    check("decoder sum on the union", s.F, s64, RTOL)
    kc = union_c[mask]
    want = dense_conv(kc, s64[torch.from_numpy(mask)], W_c, None, 3, 1, 1, 1, kc, B, G)
    check("decoder forward", out.F, want, RTOL)
    g = rng.standard_normal(tuple(want.shape)).astype(np.float32)
    out.F.backward(dev(g))
    want.backward(torch.from_numpy(g).double())
    check("decoder d x", xf.grad, x64.grad, RTOL)
    check("decoder d encoder", ef.grad, e64.grad, RTOL)
    check("decoder d up.kernel", net["up"].kernel.grad, W_up.grad, RTOL)
    check("decoder d conv.kernel", net["conv"].kernel.grad, W_c.grad, RTOL)


def test_one_training_step_twice_gives_identical_bytes(ME):
    """the decoder step followed by the squeeze-and-excitation block, one SGD step, run twice from the same seeds"""
    C = 16

    def run():
        rng = np.random.default_rng(401)
        cm, c2, fx, enc, fe = _decoder_inputs(ME, rng, C)
        dec, se = _decoder(ME, C, 5), _se_block(ME, C, 6)
        params = list(dec.parameters()) + list(se.parameters())
        opt = torch.optim.SGD(params, lr=0.1)
        x = ME.SparseTensor(dev(fx), coordinate_manager=cm, tensor_stride=2)
        e = ME.SparseTensor(dev(fe), coordinates=dev(enc))
        s = dec["up"](x) + e
        mask = torch.from_numpy(np.random.default_rng(1).random(s.F.size(0)) < 0.7).cuda()
        _, _, h = _decoder_forward(ME, dec, x, e, mask)
        out = _se_forward(se, h)
        loss = (out.F ** 2).mean()
        loss.backward()
        grads = [p.grad.clone() for p in params]
        opt.step()
        return [loss.detach().clone()] + grads + [p.detach().clone() for p in params]
    first, second = run(), run()
    assert len(first) == len(second) and all(torch.equal(a, b) for a, b in zip(first, second))


# ---------------------------------------------------------------------------------------------- 4. one size case
# ------------------------------------------------------------------------------------------------ the scalar route
def off_by_one_float(a):
    """the same values in storage that starts one float behind a 16-byte boundary (a slice of a larger buffer)"""
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    t = buf[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert buf.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 4 and t.is_contiguous() and t.contiguous().data_ptr() == t.data_ptr()
    return t


def same_bits(a, b):
    a, b = host(a), host(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


def test_misaligned_rows_take_the_scalar_route(ME, be):
    """C = 8 would take four floats per lane (130 rows: 260 threads, two blocks); operands one float off the alignment take
    one, and give the same bytes: the union of two sets under all three operations and the broadcast add / multiply / copy,
    forward and backward"""
    rng = np.random.default_rng(130)
    V, C = 130, 8
    o = np.arange(V)
    held = [o % 3 != 0, (o % 2 == 0) | (o % 3 == 0)]              # every union row has an operand; both absences occur
    in_row = np.full((2, V), -1, np.int32)
    out_rows = []
    for i in range(2):
        rows = rng.permutation(np.nonzero(held[i])[0]).astype(np.int32)       # set row -> union row
        in_row[i, rows] = np.arange(rows.size, dtype=np.int32)
        out_rows.append(rows)
    feats = [rng.standard_normal((r.size, C)).astype(np.float32) for r in out_rows]
    dout = rng.standard_normal((V, C)).astype(np.float32)
    for op in (R.SUM, R.SUB, R.MUL):
        a = be.union_combine(op, [dev(f) for f in feats], dev(in_row), V)
        b = be.union_combine(op, [off_by_one_float(f) for f in feats], dev(in_row), V)
        assert np.array_equal(host(a), R.combine_np(op, feats, in_row)), op
        assert same_bits(a, b), op
        for which in (0, 1):
            other = (feats[1 - which], in_row[1 - which]) if op == R.MUL else None
            a = be.union_combine_backward(op, which, dev(dout), dev(out_rows[which]),
                                          *(() if other is None else (dev(other[0]), dev(other[1]))))
            b = be.union_combine_backward(op, which, off_by_one_float(dout), dev(out_rows[which]),
                                          *(() if other is None else (off_by_one_float(other[0]), dev(other[1]))))
            want = R.combine_backward_np(op, which, dout, out_rows[which], *(() if other is None else other))
            assert np.array_equal(host(a), want), (op, which)
            assert same_bits(a, b), (op, which)

    coords = big_cloud(rng, V, B=3, grid=12)
    g_batch = np.array([2, 0], np.int32)                           # batch 1 has no global row
    gc = np.zeros((2, 4), np.int32)
    gc[:, 0] = g_batch
    xt = ME.SparseTensor(dev(np.zeros((V, 1), np.float32)), coordinate_manager=ME.CoordinateManager(dev(coords)))
    gt = ME.SparseTensor(dev(np.zeros((2, 1), np.float32)), coordinates=dev(gc))
    grow, red = xt.coordinate_manager.broadcast_map(1, gt.coordinate_manager, 1)
    assert (host(grow) == -1).any() and (host(grow) == 0).any() and (host(grow) == 1).any()      # (per row as it is held)
    x = rng.standard_normal((V, C)).astype(np.float32)
    g = rng.standard_normal((2, C)).astype(np.float32)
    for mode in (R.ADD, R.MULTIPLY, R.COPY):
        xa, xb = (None, None) if mode == R.COPY else (dev(x), off_by_one_float(x))
        a = be.broadcast(mode, xa, dev(g), grow)
        b = be.broadcast(mode, xb, off_by_one_float(g), grow)
        assert np.array_equal(host(a), R.broadcast_np(mode, x, g, host(grow))), mode
        assert same_bits(a, b), mode
        xa, xb = (dev(x), off_by_one_float(x)) if mode == R.MULTIPLY else (None, None)
        a = be.broadcast_reduce(dev(dout), 0, C, xa, *red)
        b = be.broadcast_reduce(off_by_one_float(dout), 0, C, xb, *red)
        dg = R.broadcast_dg_np(mode, dout, x, host(grow), 2, C)
        assert np.abs(host(a).astype(np.float64) - dg).max() / np.abs(dg).max() <= RTOL, mode
        assert same_bits(a, b), mode
        if mode == R.MULTIPLY:                                     # the gradient of x: the same kernel on dout
            assert same_bits(be.broadcast(mode, dev(dout), dev(g), grow),
                             be.broadcast(mode, off_by_one_float(dout), off_by_one_float(g), grow))


def test_concatenate_of_3_and_4_channels_reduces_by_the_scalar_route(ME):
    """x of 3 channels in front of g of 4: the gradient of g is read from dout at leading dimension 7, column offset 3,
    neither a multiple of four, so the reduction takes one float per lane"""
    rng = np.random.default_rng(7)
    V, Cx, Cg = 130, 3, 4
    coords = big_cloud(rng, V, B=3, grid=12)
    g_batch = np.array([2, 0], np.int32)
    gc = np.zeros((2, 4), np.int32)
    gc[:, 0] = g_batch
    grow = R.grow_np(coords[:, 0], g_batch)
    x = rng.standard_normal((V, Cx)).astype(np.float32)
    g = rng.standard_normal((2, Cg)).astype(np.float32)
    xt = ME.SparseTensor(dev(x).requires_grad_(True), coordinate_manager=ME.CoordinateManager(dev(coords)))
    gt = ME.SparseTensor(dev(g).requires_grad_(True), coordinates=dev(gc))
    y = ME.MinkowskiBroadcastConcatenation()(xt, gt)
    want = R.broadcast_np(R.CAT, x, g, grow)
    assert want.shape == (V, Cx + Cg) and np.array_equal(host(y.F), want)
    dout = rng.standard_normal(want.shape).astype(np.float32)
    y.F.backward(dev(dout))
    assert np.array_equal(host(xt._F.grad), dout[:, :Cx])
    dg = R.broadcast_dg_np(R.CAT, dout, x, grow, 2, Cx)
    e = np.abs(host(gt._F.grad).astype(np.float64) - dg).max() / np.abs(dg).max()
    print(f"concatenate 3 + 4: dg rel err {e:.3e} (bound {RTOL:.0e})")
    assert e <= RTOL, e


def _ms(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def test_size_case_200k_rows(ME, be):
    """two sets of 200 000 rows with half in common, C = 32: milliseconds of the HIP path beside a torch-composed formulation of
    the same results (cat + unique(dim=0, return_inverse) + index_add_; g[batch] * x with autograd), interleaved in this
    process.  Nothing is asserted about the times (none was fixed in advance); the values are compared."""
    rng = np.random.default_rng(11)
    C = 32
    pool = big_cloud(rng, 300000)
    ca, cb = pool[:200000], np.ascontiguousarray(pool[100000:][::-1])
    fa = rng.standard_normal((len(ca), C)).astype(np.float32)
    fb = rng.standard_normal((len(cb), C)).astype(np.float32)
    da, db, dfa, dfb = dev(ca), dev(cb), dev(fa), dev(fb)
    out, out_rows, in_row = be.coords_union([da, db])
    n = out.size(0)
    assert n == 300000
    dout = dev(rng.standard_normal((n, C)).astype(np.float32))
    y = be.union_combine(0, [dfa, dfb], in_row, n)
    allc, allf = torch.cat([da, db]), torch.cat([dfa, dfb])
    uq, inverse = torch.unique(allc, dim=0, return_inverse=True)
    yt = torch.zeros((uq.size(0), C), device="cuda").index_add_(0, inverse, allf)
    # the same set and the same sums (torch's rows are sorted, the engine's in first-occurrence order)
    back = torch.empty(n, dtype=torch.long, device="cuda")
    back[inverse[:len(ca)]] = out_rows[0].long()
    back[inverse[len(ca):]] = out_rows[1].long()
    assert uq.size(0) == n and torch.equal(out[back], uq) and torch.equal(y[back], yt)

    def torch_union():
        u, inv = torch.unique(torch.cat([da, db]), dim=0, return_inverse=True)
        return u, inv
    rows = []
    for _ in range(2):                                            # interleaved, two rounds; the second is reported
        rows = [("coords_union (2 x 200k rows -> 300k)", _ms(lambda: be.coords_union([da, db]), reps=10),
                 _ms(torch_union, reps=10), "cat + unique(dim=0, return_inverse)"),
                ("combine forward (sum, C=32)", _ms(lambda: be.union_combine(0, [dfa, dfb], in_row, n)),
                 _ms(lambda: torch.zeros((n, C), device="cuda").index_add_(0, inverse, torch.cat([dfa, dfb]))),
                 "cat + index_add_"),
                ("combine backward (both operands)",
                 _ms(lambda: (be.union_combine_backward(0, 0, dout, out_rows[0]), be.union_combine_backward(0, 1, dout, out_rows[1]))),
                 _ms(lambda: dout[back][inverse]), "gather through the inverse")]
    # broadcast multiply, forward and backward
    gb = np.array([0, 1], np.int32)
    g = dev(rng.standard_normal((2, C)).astype(np.float32)).requires_grad_(True)
    xt = ME.SparseTensor(dfa.clone().requires_grad_(True), coordinate_manager=ME.CoordinateManager(da, spatial_sort=True))
    assert xt.coordinate_manager.perm is not None
    gc = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    gc[:, 0] = dev(gb)
    gt = ME.SparseTensor(g, coordinates=gc)
    layer = ME.MinkowskiBroadcastMultiplication()
    d2 = dev(rng.standard_normal((len(ca), C)).astype(np.float32))
    batch = xt.coordinate_manager.coords[1][:, 0].long()            # the engine's row order, as xt._F
    xe = xt._F.detach().clone().requires_grad_(True)
    ge = g.detach().clone().requires_grad_(True)

    def hip_fwd_bwd():
        xt._F.grad = g.grad = None
        layer(xt, gt)._F.backward(d2)

    def torch_fwd_bwd():
        xe.grad = ge.grad = None
        (ge[batch] * xe).backward(d2)
    hip_fwd_bwd(); torch_fwd_bwd()
    assert torch.equal(xt._F.grad, xe.grad)
    e = rel_err(g.grad, ge.grad.double())
    dg64 = R.broadcast_dg_np(R.MULTIPLY, host(d2), host(xe), host(batch).astype(np.int32), 2, C)
    e64 = np.abs(host(g.grad).astype(np.float64) - dg64).max() / np.abs(dg64).max()
    print(f"broadcast multiply dg, 200k rows C=32: rel err {e64:.3e} vs float64 (bound {RTOL:.0e}); {e:.3e} vs torch float32")
    assert e64 <= RTOL
    for _ in range(2):
        bc = [("broadcast multiply forward", _ms(lambda: layer(xt, gt)), _ms(lambda: ge[batch] * xe), "g[batch] * x"),
              ("broadcast multiply forward + backward", _ms(hip_fwd_bwd), _ms(torch_fwd_bwd), "autograd")]
    V = len(ca)
    model = {"coords_union (2 x 200k rows -> 300k)": 2 * V * 16 + n * 16 + 2 * V * 4 + 2 * n * 4,
             "combine forward (sum, C=32)": (2 * V + n) * C * 4 + 2 * n * 4,
             "combine backward (both operands)": (2 * V + 2 * V) * C * 4 + 2 * V * 4,
             "broadcast multiply forward": 2 * V * C * 4 + V * 4,
             "broadcast multiply forward + backward": (2 + 2 + 2) * V * C * 4 + 2 * V * 4 + V * 8}
    print("setops size case: operation | HIP ms | torch ms | torch formulation | algorithmic MB")
    for name, hip_ms, torch_ms, what in rows + bc:
        print(f"setops | {name} | {hip_ms:.3f} | {torch_ms:.3f} | {what} | {model[name] / 1e6:.1f}")
