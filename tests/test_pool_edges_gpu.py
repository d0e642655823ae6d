"""GPU parity of the pooling kernels (csrc/pool.hip) through HipBackend.pool_forward / pool_backward on hand-built
offset-major tables (nbr [K, Vout], inverse [K, Vin], -1 = absent) against a float64 reference written here: the tie rule
of the maximum (lowest k, strict >) and its backward, output rows without any input, channel counts on both lane layouts
(C % 4 == 0: four floats per lane; otherwise one) crossed with row counts at the 256-thread block edge, the limits of K,
and the one-float-per-lane route taken by C % 4 == 0 when the rows are not 16-byte aligned.

Bounds.  Maximum: exact.  Sum and average: the kernel adds the n present inputs one after the other in float32 and the
average divides once, n roundings of relative size 2^-24 each on partial sums that never exceed sum |inputs|, so per
element |got - want| <= (n + 1) * 2^-24 * sum |inputs| (divided by n for the average); the same holds for the backward
gathers with the terms dout[o] (sum) and dout[o] / count[o] (average: one rounding in the division, then the adds)."""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
MAX, AVG, SUM = 0, 1, 2
U = 2.0 ** -24


@pytest.fixture(scope="module")
def be():
    from minsu3d_amd.backend import HipBackend
    return HipBackend()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tables(K, Vout, Vin, rng, present=0.6, empty=()):
    """per offset k a random partial one-to-one assignment of output rows to input rows; `empty`: output rows without
    any input.  -> (nbr [K, Vout], inverse [K, Vin]) int32"""
    nbr = np.full((K, Vout), -1, np.int32)
    m = min(Vout, Vin)
    for k in range(K):
        outs, ins = rng.permutation(Vout)[:m], rng.permutation(Vin)[:m]
        keep = rng.random(m) < present
        nbr[k, outs[keep]] = ins[keep]
    nbr[:, list(empty)] = -1
    inv = np.full((K, Vin), -1, np.int32)
    k, o = np.nonzero(nbr >= 0)
    inv[k, nbr[k, o]] = o
    assert (inv >= 0).sum() == (nbr >= 0).sum()                       # one-to-one per offset: nothing was overwritten
    return nbr, inv


def ref_forward(mode, x, nbr):
    """-> (out float64 [Vout, C], arg uint8 [Vout, C] (max), count int32 [Vout], sum |inputs| [Vout, C])"""
    on = (nbr >= 0)[:, :, None]
    vals = x.astype(np.float64)[np.clip(nbr, 0, None)]                # [K, Vout, C]
    n = (nbr >= 0).sum(0).astype(np.int32)
    mag = (np.abs(vals) * on).sum(0)
    arg = None
    if mode == MAX:
        v = np.where(on, vals, -np.inf)
        arg = np.where(n[:, None] > 0, v.argmax(0), 255).astype(np.uint8)       # argmax: the FIRST maximum = lowest k
        out = np.where(n[:, None] > 0, v.max(0), 0.0)
    else:
        out = (vals * on).sum(0)
        if mode == AVG:
            out = out / np.maximum(n, 1)[:, None]
            mag = mag / np.maximum(n, 1)[:, None]
    return out, arg, n, mag


def ref_backward(mode, dout, inv, arg, count):
    """-> (din float64 [Vin, C], number of terms [Vin], sum |terms| [Vin, C])"""
    K = inv.shape[0]
    on = (inv >= 0)[:, :, None]
    o = np.clip(inv, 0, None)
    terms = dout.astype(np.float64)[o]                                # [K, Vin, C]
    if mode == MAX:
        terms = terms * (arg[o] == np.arange(K)[:, None, None])
    elif mode == AVG:
        terms = terms / np.maximum(count, 1)[o][:, :, None]
    terms = terms * on
    return terms.sum(0), (inv >= 0).sum(0), np.abs(terms).sum(0)


def same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.int32), want.view(np.int32))


def check_mode(be, mode, x, dout, nbr, inv, tag, x_dev=None, dout_dev=None):
    """forward and backward of one mode against the reference; -> the kernel's (out, arg, count, din) as numpy"""
    K, Vout = nbr.shape
    Vin = inv.shape[1]
    out, arg, count = be.pool_forward(mode, dev(x) if x_dev is None else x_dev, dev(nbr), Vout, K)
    want, warg, n, mag = ref_forward(mode, x, nbr)
    out_h = out.cpu().numpy()
    assert (arg is not None) == (mode == MAX) and (count is not None) == (mode == AVG), tag
    if mode == MAX:
        assert same_bits(out_h, want.astype(np.float32)), tag + " forward"
        assert np.array_equal(arg.cpu().numpy(), warg), tag + " arg"
    else:
        assert np.all(np.abs(out_h - want) <= (n[:, None] + 1) * U * mag), (tag + " forward", np.abs(out_h - want).max())
        if mode == AVG:
            assert np.array_equal(count.cpu().numpy(), n), tag + " count"
    assert not out_h[n == 0].any(), tag + " empty rows"
    din = be.pool_backward(mode, dev(dout) if dout_dev is None else dout_dev, dev(inv), Vin, K, arg, count)
    wdin, m, tmag = ref_backward(mode, dout, inv, warg, n)
    din_h = din.cpu().numpy()
    assert din_h.shape == wdin.shape and din_h.dtype == np.float32
    assert np.all(np.abs(din_h - wdin) <= (m[:, None] + 1) * U * tmag), (tag + " backward", np.abs(din_h - wdin).max())
    assert not din_h[m == 0].any(), tag + " inputs that feed nothing"
    return out_h, None if arg is None else arg.cpu().numpy(), None if count is None else count.cpu().numpy(), din_h


# ---------------------------------------------------------------------------------------------- ties
def tie_case(C_):
    rng = np.random.default_rng(C_)
    K, Vout, Vin = 8, 70, 66
    nbr, inv = tables(K, Vout, Vin, rng, present=0.7, empty=(0, 13, 69))
    x = rng.integers(-1, 2, (Vin, C_)).astype(np.float32)
    dout = rng.integers(-8, 9, (Vout, C_)).astype(np.float32)           # integers: the backward sums are exact
    return x, dout, nbr, inv


def tie_properties(x, nbr):
    want, warg, n, _ = ref_forward(MAX, x, nbr)
    vals = np.where((nbr >= 0)[:, :, None], x[np.clip(nbr, 0, None)].astype(np.float64), -np.inf)
    winners = (vals == vals.max(0)).sum(0)[n > 0]
    assert (winners > 1).mean() > 0.5                                   # most maxima tie
    k = np.arange(nbr.shape[0])[:, None, None]
    lowest = np.where(vals == vals.max(0), k, 999).min(0)
    assert np.array_equal(lowest[n > 0], warg[n > 0]) and (warg[n == 0] == 255).all() and (n == 0).sum() >= 3
    return warg, n


@gpu
@pytest.mark.parametrize("C_", [3, 8])
def test_ties_go_to_the_lowest_offset(be, C_):
    """inputs from {-1, 0, 1}: values exact, arg = the lowest present k attaining the maximum, and the backward routes
    every output gradient to exactly that input (integer gradients: bit for bit)"""
    x, dout, nbr, inv = tie_case(C_)
    warg, n = tie_properties(x, nbr)
    out, arg, _, din = check_mode(be, MAX, x, dout, nbr, inv, "ties C=%d" % C_)
    assert (arg[n == 0] == 255).all() and not out[n == 0].any()
    wdin, _, _ = ref_backward(MAX, dout, inv, warg, n)
    assert same_bits(din + 0.0, wdin.astype(np.float32) + 0.0)          # + 0.0: -0.0 and 0.0 are the same gradient
    assert din.astype(np.float64).sum() == dout[n > 0].astype(np.float64).sum()        # each gradient arrives exactly once


# ---------------------------------------------------------------------------------------------- empty rows
@gpu
@pytest.mark.parametrize("C_", [5, 8])
def test_output_rows_without_input(be, C_):
    rng = np.random.default_rng(20 + C_)
    K, Vout, Vin = 8, 65, 65
    empty = (0, 1, 31, 64)
    nbr, inv = tables(K, Vout, Vin, rng, empty=empty)
    x = rng.standard_normal((Vin, C_)).astype(np.float32)
    dout = rng.standard_normal((Vout, C_)).astype(np.float32)
    dout[list(empty)] = 1e30                                            # would show in din if the backward read them
    for mode in (MAX, AVG, SUM):
        out, arg, count, din = check_mode(be, mode, x, dout, nbr, inv, "empty rows mode %d C=%d" % (mode, C_))
        assert not out[list(empty)].any() and float(np.abs(din).max()) < 1e3
        if mode == MAX:
            assert (arg[list(empty)] == 255).all()
        if mode == AVG:
            assert (count[list(empty)] == 0).all()


# ---------------------------------------------------------------------------------------------- channel and row edges
VIN_OF = {1: 1, 63: 65, 64: 64, 65: 63, 257: 256}


@gpu
@pytest.mark.parametrize("Vout", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("C_", [1, 3, 4, 64, 68])
def test_channel_and_row_edges(be, C_, Vout):
    """C = 4, 64, 68: four floats per lane (1, 16, 17 lanes per row); C = 1, 3: one.  Vout * lanes-per-row around 256
    (C = 4 at 257 rows, C = 1 at 257, C = 64 at 16 rows per block), a single row, and as many input rows for the backward"""
    rng = np.random.default_rng(1000 * C_ + Vout)
    Vin = VIN_OF[Vout]
    x = rng.standard_normal((Vin, C_)).astype(np.float32)
    dout = rng.standard_normal((Vout, C_)).astype(np.float32)
    for K in (1, 8, 27):
        nbr, inv = tables(K, Vout, Vin, rng, present=0.8)
        for mode in (MAX, AVG, SUM):
            check_mode(be, mode, x, dout, nbr, inv, "C=%d Vout=%d K=%d mode %d" % (C_, Vout, K, mode))


# ---------------------------------------------------------------------------------------------- limits of K
@gpu
def test_limits_of_k(be):
    """arg is a byte and 255 means no input: K = 254 is the last one served, its last offset (253) can win"""
    from minsu3d_amd import _lib
    rng = np.random.default_rng(7)
    Vout = Vin = 5
    x = rng.standard_normal((Vin, 4)).astype(np.float32)
    dout = rng.standard_normal((Vout, 4)).astype(np.float32)
    nbr, inv = tables(254, Vout, Vin, rng, present=0.1)
    nbr[:, 2] = -1
    nbr[253, :] = -1
    nbr[253, 2] = 3                                                     # row 2: only the last offset is present
    inv[:, :] = -1
    k, o = np.nonzero(nbr >= 0)
    inv[k, nbr[k, o]] = o
    for mode in (MAX, AVG, SUM):
        _, arg, _, _ = check_mode(be, mode, x, dout, nbr, inv, "K=254 mode %d" % mode)
        if mode == MAX:
            assert (arg[2] == 253).all()
    big = np.full((255, Vout), -1, np.int32)
    for mode in (MAX, AVG, SUM):
        with pytest.raises(_lib.HipLibraryError, match="ms3d_pool_forward failed with code %d" % _lib.E_UNSUPPORTED):
            be.pool_forward(mode, dev(x), dev(big), Vout, 255)
        arg = torch.zeros((Vout, 4), dtype=torch.uint8, device="cuda")
        count = torch.ones(Vout, dtype=torch.int32, device="cuda")
        with pytest.raises(_lib.HipLibraryError, match="ms3d_pool_backward failed with code %d" % _lib.E_UNSUPPORTED):
            be.pool_backward(mode, dev(dout), dev(big), Vin, 255, arg, count)


# ---------------------------------------------------------------------------------------------- misaligned rows
def off_by_one_float(a):
    """the same values in storage that starts one float behind a 16-byte boundary (a slice of a larger buffer)"""
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    t = buf[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert buf.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 4 and t.is_contiguous() and t.contiguous().data_ptr() == t.data_ptr()
    return t


@gpu
def test_misaligned_rows_take_the_scalar_route(be):
    """C = 8 would take four floats per lane; input and upstream gradient one float off the alignment take one, and give
    the same bytes in all three modes and both directions"""
    rng = np.random.default_rng(8)
    K, Vout, Vin, C_ = 8, 65, 63, 8
    nbr, inv = tables(K, Vout, Vin, rng, empty=(5,))
    x = rng.standard_normal((Vin, C_)).astype(np.float32)
    dout = rng.standard_normal((Vout, C_)).astype(np.float32)
    for mode in (MAX, AVG, SUM):
        a = check_mode(be, mode, x, dout, nbr, inv, "aligned mode %d" % mode)
        b = check_mode(be, mode, x, dout, nbr, inv, "misaligned mode %d" % mode, off_by_one_float(x), off_by_one_float(dout))
        assert same_bits(a[0], b[0]) and same_bits(a[3], b[3])
        for i in (1, 2):
            assert (a[i] is None and b[i] is None) or np.array_equal(a[i], b[i])


# ---------------------------------------------------------------------------------------------- the builders, on the CPU
def test_crafted_tables_are_what_they_claim():
    for C_ in (3, 8):
        x, dout, nbr, inv = tie_case(C_)
        warg, n = tie_properties(x, nbr)
        wdin, m, _ = ref_backward(MAX, dout, inv, warg, n)
        assert wdin.sum() == dout[n > 0].astype(np.float64).sum() and np.array_equal(wdin, np.round(wdin))
    nbr, inv = tables(27, 257, 256, np.random.default_rng(0), present=0.8)
    k, i = np.nonzero(inv >= 0)
    assert np.array_equal(nbr[k, inv[k, i]], i)
    # the reference's sum and average against a plain loop
    x = np.random.default_rng(1).standard_normal((256, 3)).astype(np.float32)
    for mode in (AVG, SUM):
        out, _, n, _ = ref_forward(mode, x, nbr)
        for o in (0, 100, 256):
            rows = [x[nbr[k, o]].astype(np.float64) for k in range(27) if nbr[k, o] >= 0]
            want = sum(rows) / (len(rows) if mode == AVG else 1)
            assert len(rows) == n[o] and np.allclose(out[o], want, rtol=1e-14, atol=0)
