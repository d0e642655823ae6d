"""GPU parity of the segment reductions (csrc/segment_ops.hip) and the IoU family (csrc/iou.hip) at the places a kernel
goes wrong: every channel route, segment lengths on the tile and unroll edges, proposal counts past every grid cap,
the tiled IoU histogram, ties across lanes / waves / thread stripes, signed zeros, infinities and NaN, and the backward
passes with empty proposals kept.  Inputs: tests/segment_cases.py; expectation: the serial oracle (validated against a
numpy transcription in tests/test_oracle_grouping.py).  Everything is compared bit for bit."""
import numpy as np
import pytest
import torch

import segment_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from minsu3d_amd.backend import HipBackend
    return HipBackend()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(got, want, what):
    """f32 outputs by bit pattern (NaN payloads and the sign of zero count), integers as they are"""
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g = got.view(np.int32) if got.dtype == np.float32 else got
    w = want.view(np.int32) if want.dtype == np.float32 else want
    bad = np.argwhere(g != w)
    assert bad.shape[0] == 0, "%s: %d of %d differ, first at %s: got %r (0x%08x) want %r (0x%08x)" % (
        what, bad.shape[0], g.size, tuple(bad[0]), got[tuple(bad[0])], int(g[tuple(bad[0])]) & 0xffffffff,
        want[tuple(bad[0])], int(w[tuple(bad[0])]) & 0xffffffff)


def check_forward(be, oracle, x, off, what, x_min=None):
    """the five forward operators on rows x; sec_min reads x_min where the guard rows must hold another sentinel"""
    xd, od = dev(x), dev(off)
    same_bits(be.sec_mean(xd, od), oracle.sec_mean(x, off), what + " sec_mean")
    same_bits(be.sec_max(xd, od), oracle.sec_max(x, off), what + " sec_max")
    xm = x if x_min is None else x_min
    same_bits(be.sec_min(dev(xm), od), oracle.sec_min(xm, off), what + " sec_min")
    out, mi = be.roipool_fp(xd, od)
    wout, wmi = oracle.roipool_fp(x, off)
    same_bits(out, wout, what + " roipool_fp")
    same_bits(mi, wmi, what + " roipool_fp argmax")
    same_bits(be.global_avg_pool_fp(xd, od), oracle.global_avg_pool_fp(x, off), what + " global_avg_pool_fp")
    return wmi


ALL_C = [1, 2, 3, 4, 8, 16, 19, 32, 64, 65, 100, 128]


@pytest.mark.parametrize("start", [0, 7])
@pytest.mark.parametrize("values", ["random", "special"])
@pytest.mark.parametrize("C_", ALL_C)
def test_forward_routes_at_edge_lengths(be, oracle, C_, values, start):
    """C = 1, 2, 4: seg_extreme_kernel's power-of-two path; 8 .. 64: the block kernel (C = 64: no in-wave shuffle,
    rstep = 1); 65, 100, 128: seg_serial_sum_kernel's second channel stage (cw = 1, 36, 64); segment lengths on every
    tile / unroll edge of the route (segment_cases.edge_offsets); random rows, and rows with duplicated extrema far apart
    and adjacent, a constant segment, signed zeros, infinities and NaN (segment_cases.special_values).  start = 7:
    offsets[0] = 7, and the rows in front of the first and behind the last segment would win the extremum (and turn the
    sums infinite) if a kernel read them."""
    rng = np.random.default_rng(100 * C_ + start)
    off = sc.edge_offsets(C_)
    x = rng.standard_normal((int(off[-1]), C_)).astype(np.float32)
    where = {}
    if values == "special":
        x, where = sc.special_values(x, off, rng)
    x_min = None
    if start:
        x_min, _ = sc.shifted(x, off, front=start, sentinel=-np.inf)
        x, off = sc.shifted(x, off, front=start, sentinel=np.inf)
    wmi = check_forward(be, oracle, x, off, "C=%d %s start=%d" % (C_, values, start), x_min)
    if where:
        assert (wmi[where["all_nan"]] == -1).all() and (wmi[where["all_neg_inf"]] == -1).all()
        assert (wmi[where["constant"]] == off[where["constant"]]).all()


@pytest.mark.parametrize("values", ["random", "constant"])
@pytest.mark.parametrize("C_", [3, 4, 16, 19, 64])
def test_forward_grid_stride(be, oracle, C_, values):
    """16421 proposals of 0 to 4 rows: the wave kernels' grid-stride loops (4096 blocks x 4 waves) and the block
    kernel's (4096 blocks, __syncthreads inside the loop) run a second iteration; with one constant value everywhere
    every argmax must be its segment's first row"""
    off = sc.many_short_offsets(sc.MANY_SHORT_P)
    S = int(off[-1])
    if values == "constant":
        x = np.full((S, C_), np.float32(0.37))
    else:
        x = np.random.default_rng(C_).standard_normal((S, C_)).astype(np.float32)
    wmi = check_forward(be, oracle, x, off, "C=%d %s many short" % (C_, values))
    if values == "constant":
        first = np.where(np.diff(off) > 0, off[:-1], -1).astype(np.int32)
        assert np.array_equal(wmi, np.repeat(first[:, None], C_, 1))


def _backward_offsets(kind):
    if kind == "many_short":
        off = sc.many_short_offsets(sc.MANY_SHORT_P) + 7
        return off.astype(np.int32), int(off[-1]) + 9
    lens = [0, 0, 0, 5, 1, 0, 0, 70, 0, 300, 2, 0, 0, 0, 0, 64, 65, 0, 0]      # empty runs: front, middle, end
    off = (7 + np.concatenate([[0], np.cumsum(lens)])).astype(np.int32)        # offsets[0] = 7
    return off, int(off[-1]) + 9                                               # sum_npoint > offsets[P]


@pytest.mark.parametrize("kind", ["empty_runs", "many_short"])
@pytest.mark.parametrize("C_", [3, 16, 19])
def test_backward_with_empty_proposals(be, C_, kind):
    """roipool_bp with the forward's own argmax (-1 for the empty proposals: skipped, roipool_bp_kernel's am < 0),
    global_avg_pool_bp through the backend (bisection over runs of equal offsets, offsets[0] != 0, rows behind
    offsets[P]) and ms3d_global_avg_pool_bp (one wave per proposal; 16421 proposals: its grid-stride loop).  Every
    d_feats element receives at most one addend, so the expectation is exact; rows outside every proposal are +0.0."""
    off, S = _backward_offsets(kind)
    P = off.size - 1
    rng = np.random.default_rng(C_ + P)
    x = rng.standard_normal((S, C_)).astype(np.float32)
    g = rng.standard_normal((P, C_)).astype(np.float32)
    g[g == 0] = 1.0
    lens = np.diff(off)
    od, gd = dev(off), dev(g)
    # roipool: forward argmax (checked), then the scatter
    out, mi = be.roipool_fp(dev(x), od)
    want_mi = np.full((P, C_), -1, np.int32)
    for p in np.flatnonzero(lens):
        want_mi[p] = off[p] + x[off[p]:off[p + 1]].argmax(0)                   # numpy's argmax takes the first maximum
    same_bits(mi, want_mi, "argmax")
    assert (want_mi[lens == 0] == -1).all() and (lens == 0).sum() >= 10
    want = np.zeros((S, C_), np.float32)
    pp, cc = np.nonzero(want_mi >= 0)
    np.add.at(want, (want_mi[pp, cc], cc), g[pp, cc])
    same_bits(be.roipool_bp(gd, od, mi, S), want, "roipool_bp")
    # average pool
    want = np.zeros((S, C_), np.float32)
    for p in np.flatnonzero(lens):
        want[off[p]:off[p + 1]] = g[p] / np.float32(lens[p])
    assert not want[:7].any() and not want[off[-1]:].any()
    same_bits(be.global_avg_pool_bp(gd, od, S), want, "global_avg_pool_bp (rows kernel)")
    from minsu3d_amd import _lib
    d_feats = torch.zeros((S, C_), dtype=torch.float32, device="cuda")
    _lib.check(be.lib.ms3d_global_avg_pool_bp(P, C_, _lib.ptr(d_feats), _lib.ptr(od), _lib.ptr(gd), _lib.stream_handle()),
               "ms3d_global_avg_pool_bp")
    same_bits(d_feats, want, "ms3d_global_avg_pool_bp (wave kernel)")


def _check_iou_family(be, oracle, I, off, N, seed):
    pidx, inst, pn, sig = sc.iou_inputs(I, off, N, seed)
    assert (sig == np.float32(0.5)).any() and (sig == np.nextafter(np.float32(0.5), np.float32(1))).any()
    args = (dev(pidx), dev(off), dev(inst), dev(pn))
    iou = be.get_iou(*args)
    want = oracle.get_iou(pidx, off, inst, pn)
    same_bits(iou, want, "get_iou")
    same_bits(be.get_mask_iou_on_cluster(*args), oracle.get_mask_iou_on_cluster(pidx, off, inst, pn), "on_cluster")
    same_bits(be.get_mask_iou_on_pred(*args, dev(sig)), oracle.get_mask_iou_on_pred(pidx, off, inst, pn, sig), "on_pred")
    return pidx, inst, iou, want


@pytest.mark.parametrize("I", [12288, 12289, 20000, 32767])
def test_iou_tiled_histogram(be, oracle, I):
    """I > MAX_LDS_BINS: several histogram passes per proposal, the on-pred total recomputed in each; I = 12288 is the
    last single-pass size.  Proposals of 0, 1, 300, 5000, ... points; every larger one holds the labels 0, 12287, 12288
    (the first bin of the second pass) and I - 1."""
    off = sc.sizes_to_offsets(sc.TILED_IOU_SIZES)
    _, _, _, want = _check_iou_family(be, oracle, I, off, 40000, I)
    assert want[3, I - 1] > 0 and want[3, min(I - 1, sc.MAX_LDS_BINS)] > 0 and want[3, 0] > 0


def test_iou_and_mask_label_grid_stride(be, oracle):
    """8201 proposals of 0 to 3 points: iou_kernel's and mask_label_kernel's grid-stride loops run a second iteration"""
    I, P = 37, sc.IOU_GRID_CAP + 9
    lens = np.random.default_rng(P).integers(0, 4, P)
    off = sc.sizes_to_offsets(lens)
    pidx, inst, iou, _ = _check_iou_family(be, oracle, I, off, 5000, 3)
    cls = np.random.default_rng(4).integers(-1, 18, I).astype(np.int16)
    for thr in (0.0, 0.05):
        ml, mlm = be.get_mask_label(dev(pidx), dev(off), dev(inst), dev(cls), iou, -1, thr)
        wml, wmlm = oracle.get_mask_label(pidx, off, inst, cls, iou.cpu().numpy(), -1, thr)
        same_bits(ml, wml, "mask_label thr=%g" % thr)
        same_bits(mlm, wmlm, "mask_label_mask thr=%g" % thr)
        assert wmlm.all() or thr > 0                                           # 0 >= 0: every proposal is written


@pytest.mark.parametrize("case", sc.mask_label_cases(), ids=lambda c: c["name"])
def test_mask_label_crafted_ties(be, oracle, case):
    """equal maxima in another wave, another thread stripe, a later stripe of a lower thread (the smaller index wins),
    an ignored first maximum, every class ignored, the best exactly at the threshold and one ulp below it"""
    pidx, off, inst = sc.mask_label_points(case)
    iou, cls, thr = case["iou"], case["inst_cls"], float(case["thr"])
    ml, mlm = be.get_mask_label(dev(pidx), dev(off), dev(inst), dev(cls), dev(iou), sc.IGNORED, thr)
    wml, wmlm = oracle.get_mask_label(pidx, off, inst, cls, iou, sc.IGNORED, thr)
    cml, cmlm = sc.mask_label_expected(case)
    assert np.array_equal(wml, cml) and np.array_equal(wmlm, cmlm)
    same_bits(ml, wml, case["name"] + " mask_label")
    same_bits(mlm, wmlm, case["name"] + " mask_label_mask")
