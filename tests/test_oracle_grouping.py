"""CPU: the plain-C oracle against the golden vectors produced by the REFERENCE's own code
(tests/golden/make_golden.py) and, when oracle/_ref is present, against the reference live."""
import glob
import os

import numpy as np
import pytest

from segment_cases import (edge_offsets, mask_label_cases, mask_label_expected, mask_label_points, shifted,
                           special_values)


def _cases(golden_dir):
    return sorted(glob.glob(os.path.join(golden_dir, "bfs_case*.npz")))


def test_golden_files_present(golden_dir):
    assert len(_cases(golden_dir)) >= 6 and os.path.exists(os.path.join(golden_dir, "bfs_kat.npz"))


def test_bfs_kat(oracle, golden_dir):
    g = np.load(os.path.join(golden_dir, "bfs_kat.npz"))
    a, b = oracle.pg_bfs_cluster(g["sem"], g["ball_idx"], g["start_len"], int(g["threshold"]))
    assert np.array_equal(a, g["pg_idxs"]) and np.array_equal(b, g["pg_offsets"])


@pytest.mark.parametrize("ci", range(6))
def test_oracle_vs_golden(oracle, golden_dir, ci):
    g = np.load(os.path.join(golden_dir, f"bfs_case{ci}.npz"))
    # ball query (oracle, canonical form) reproduces the graph the reference BFS consumed
    idx, sl = oracle.ballquery_batch_p(g["xyz"], g["batch_idxs"], g["batch_offsets"], float(g["radius"]))
    assert np.array_equal(idx, g["ball_idx"]) and np.array_equal(sl, g["start_len"])
    a, b = oracle.pg_bfs_cluster(g["sem"], idx, sl, int(g["threshold"]))
    assert np.array_equal(a, g["pg_idxs"]) and np.array_equal(b, g["pg_offsets"])
    for k, cid in enumerate(g["sg_class_ids"]):
        a, b = oracle.sg_bfs_cluster(g["sg_mean"], idx, sl, float(g["sg_threshold"]), int(cid))
        assert np.array_equal(a, g[f"sg{k}_idxs"]) and np.array_equal(b, g[f"sg{k}_offsets"])
    a, b = oracle.hierarchical_aggregation(g["sem"], g["xyz"], idx, sl, g["batch_idxs"], False, g["point_num_avg"],
                                           g["radius_avg"])
    assert np.array_equal(a, g["hais_idxs"]) and np.array_equal(b, g["hais_offsets"])


def test_oracle_vs_reference_live(oracle):
    if oracle.ref() is None:
        pytest.skip("oracle/_ref not built (no /root/reference here)")
    rng = np.random.default_rng(7)
    for trial in range(4):
        n = 2000
        xyz = (rng.random((n, 3)) * np.array([0.5, 0.5, 0.05])).astype(np.float32)
        b = np.zeros(n, np.uint8); bo = np.array([0, n], np.int32)
        idx, sl = oracle.ballquery_batch_p(xyz, b, bo, 0.02 + 0.01 * trial)
        sem = rng.integers(0, 3, n).astype(np.int16)
        for thr in (1, 7, 50):
            r0 = oracle.pg_bfs_cluster(sem, idx, sl, thr)
            r1 = oracle.pg_bfs_cluster(sem, idx, sl, thr, use_ref=True)
            assert np.array_equal(r0[0], r1[0]) and np.array_equal(r0[1], r1[1])
        pna = np.array([30, 100, 300], np.float32); ra = np.array([0.05, 0.1, 0.2], np.float32)
        r0 = oracle.hierarchical_aggregation(sem, xyz, idx, sl, b, False, pna, ra)
        r1 = oracle.hierarchical_aggregation(sem, xyz, idx, sl, b, False, pna, ra, use_ref=True)
        assert np.array_equal(r0[0], r1[0]) and np.array_equal(r0[1], r1[1])


@pytest.mark.parametrize("set_aggr", [False, True])
def test_hais_raw_lists_are_consistent_with_the_merged_result(oracle, golden_dir, set_aggr):
    """parts=True (the lists hierarchical_aggregation.cpp:133-175 leaves in the caller's tensors): merged the way the
    wrapper merges them they are the oracle's merged result -- which the golden case pins for point aggregation --
    and every primary's post list starts with the primary itself"""
    g = np.load(os.path.join(golden_dir, "bfs_case1.npz"))
    args = (g["sem"], g["xyz"], g["ball_idx"], g["start_len"], g["batch_idxs"], set_aggr, g["point_num_avg"], g["radius_avg"])
    parts = oracle.hierarchical_aggregation(*args, parts=True)
    merged = oracle.hierarchical_aggregation(*args)
    ki, ko = parts["kept"][:2]
    pi, po = parts["post" if set_aggr else "primary"][:2]
    pi = pi.copy(); pi[:, 0] += len(ko) - 1
    assert np.array_equal(np.concatenate([ki, pi]), merged[0].reshape(-1, 2))
    assert np.array_equal(np.concatenate([ko, po[1:] + ko[-1]]), merged[1])
    if not set_aggr:
        assert np.array_equal(merged[0], g["hais_idxs"]) and parts["post"][0].shape[0] == 0
    else:
        raw_i, raw_o = parts["primary"][:2]
        for c in range(len(raw_o) - 1):
            m = raw_o[c + 1] - raw_o[c]
            assert np.array_equal(parts["post"][0][po[c]:po[c] + m, 1], raw_i[raw_o[c]:raw_o[c + 1], 1])
    fi, fo, fc = parts["fragment"]
    assert set(map(tuple, ki[:, 1:])) <= set(map(tuple, fi[:, 1:])) and fc.shape == (len(fo) - 1, 5)


def test_ballquery_brute_force_numpy(oracle):
    """independent check of the oracle's ball query against a numpy f64-free restatement"""
    rng = np.random.default_rng(3)
    n = 700
    xyz = (rng.random((n, 3)) * 0.3).astype(np.float32)
    b = np.sort(rng.integers(0, 3, n)).astype(np.uint8)
    bo = np.concatenate([[0], np.cumsum(np.bincount(b, minlength=3))]).astype(np.int32)
    r = np.float32(0.04)
    idx, sl = oracle.ballquery_batch_p(xyz, b, bo, float(r))
    for i in range(0, n, 37):
        d = xyz[i] - xyz
        d2 = np.float32(d[:, 0] * d[:, 0])
        # fmaf chain emulated in float64 then rounded once per fma (exact for these magnitudes)
        d2 = (d[:, 1].astype(np.float64) * d[:, 1] + d2).astype(np.float32)
        d2 = (d[:, 2].astype(np.float64) * d[:, 2] + d2).astype(np.float32)
        want = np.nonzero((d2 < r * r) & (b == b[i]))[0]
        got = idx[sl[i, 0]:sl[i, 0] + sl[i, 1]]
        assert np.array_equal(got, want[:1000])


def test_segment_ops_small(oracle):
    rng = np.random.default_rng(5)
    S, C = 200, 5
    x = rng.standard_normal((S, C)).astype(np.float32)
    off = np.array([0, 3, 3, 50, 200], np.int32)
    m = oracle.sec_mean(x, off)
    for p in range(4):
        seg = x[off[p]:off[p + 1]]
        if len(seg):
            acc = np.zeros(C, np.float32)
            for row in seg:
                acc = acc + row / np.float32(len(seg))
            assert np.array_equal(m[p], acc)
    mx, am = oracle.roipool_fp(x, off)
    assert np.array_equal(mx[2], x[3:50].max(0)) and np.array_equal(am[2], 3 + x[3:50].argmax(0))
    assert np.all(am[1] == -1) and np.all(np.isneginf(mx[1]))
    assert np.array_equal(oracle.sec_min(x, off)[3], x[50:200].min(0))


def test_iou_small(oracle):
    prop_idx = np.array([0, 1, 2, 3, 4, 5, 6], np.int32)
    prop_off = np.array([0, 4, 7], np.int32)
    inst = np.array([0, 0, 1, -1, 1, 1, 1, 0], np.int16)
    pn = np.array([3, 4], np.int32)
    iou = oracle.get_iou(prop_idx, prop_off, inst, pn)
    want = np.array([[2 / (4 + 3 - 2 + 1e-5), 1 / (4 + 4 - 1 + 1e-5)], [0 / (3 + 3 + 1e-5), 3 / (3 + 4 - 3 + 1e-5)]])
    assert np.allclose(iou, want.astype(np.float32), rtol=0, atol=1e-7)
    ml, mlm = oracle.get_mask_label(prop_idx, prop_off, inst, np.array([5, -1], np.int16), iou, -1, 0.3)
    assert mlm.tolist() == [True] * 4 + [False] * 3 and ml.tolist() == [True, True, False, False, False, False, False]


# ------------------------------------------------------------------ the oracle on the edge / special-value inputs
# (tests/segment_cases.py) against a transcription of the reference's serial loops in np.float32, compared by bit
# pattern: the expectation tests/test_segment_edges_gpu.py holds the HIP kernels to is validated here, without a GPU

def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _serial_segment_ops(x, off):
    """sec_mean.cu:12-79 and roipool.cu:12-80 row by row: the mean divides before adding, the average pool sums and
    then divides, min / max compare strictly so the first extremum (and never a NaN) wins"""
    P, C = len(off) - 1, x.shape[1]
    out = {k: np.zeros((P, C), np.float32) for k in ("mean", "min", "max", "avg")}
    out["argmax"] = np.zeros((P, C), np.int32)
    with np.errstate(all="ignore"):
        for p in range(P):
            s, e = int(off[p]), int(off[p + 1])
            count = np.float32(e - s)
            mean = np.zeros(C, np.float32); total = np.zeros(C, np.float32)
            lo = np.full(C, np.inf, np.float32); hi = np.full(C, -np.inf, np.float32); am = np.full(C, -1, np.int32)
            for i in range(s, e):
                row = x[i]
                mean = mean + row / count
                total = total + row
                lt = row < lo
                lo = np.where(lt, row, lo)
                gt = row > hi
                hi = np.where(gt, row, hi); am = np.where(gt, np.int32(i), am)
            out["mean"][p], out["min"][p], out["max"][p], out["argmax"][p] = mean, lo, hi, am
            out["avg"][p] = total / count
    return out


@pytest.mark.parametrize("C_", [3, 4, 19, 65])
@pytest.mark.parametrize("start", [0, 7])
def test_segment_ops_edges_and_special_values_vs_serial_numpy(oracle, C_, start):
    rng = np.random.default_rng(50 + C_)
    off = edge_offsets(C_)
    if C_ == 65:                                          # the reduced set: one tile of the 1-channel stage
        lens = np.diff(off)
        off = np.concatenate([[0], np.cumsum(lens[lens <= 2100])]).astype(np.int32)
    x, where = special_values(rng.standard_normal((int(off[-1]), C_)).astype(np.float32), off, rng)
    if start:
        x, off = shifted(x, off, front=start)
    want = _serial_segment_ops(x, off)
    lens = np.diff(off)
    # the inputs hold what they claim: an argmax of -1 exactly for the empty, all-NaN and all--inf segments
    none = (lens == 0)
    none[[where["all_nan"], where["all_neg_inf"]]] = True
    assert np.array_equal((want["argmax"] < 0).all(1), none) and np.array_equal((want["argmax"] < 0).any(1), none)
    assert np.array_equal(want["argmax"][where["constant"]], np.full(C_, off[where["constant"]]))
    assert np.isnan(want["avg"][where["inf"]]).all() and np.isnan(want["mean"][where["some_nan"]]).all()
    assert set(np.unique(_bits(want["max"][where["zeros"]]))) == {0, -2 ** 31}      # both zeros come first somewhere
    assert np.array_equal(_bits(oracle.sec_mean(x, off)), _bits(want["mean"]))
    assert np.array_equal(_bits(oracle.sec_min(x, off)), _bits(want["min"]))
    assert np.array_equal(_bits(oracle.sec_max(x, off)), _bits(want["max"]))
    mx, am = oracle.roipool_fp(x, off)
    assert np.array_equal(_bits(mx), _bits(want["max"])) and np.array_equal(am, want["argmax"])
    assert np.array_equal(_bits(oracle.global_avg_pool_fp(x, off)), _bits(want["avg"]))
    # backward of the average: every row of proposal p receives g[p] / n, rows outside every proposal stay +0.0
    g = rng.standard_normal((len(off) - 1, C_)).astype(np.float32)
    S = x.shape[0]
    d = np.zeros((S, C_), np.float32)
    for p in range(len(off) - 1):
        if lens[p]:
            d[off[p]:off[p + 1]] = g[p] / np.float32(lens[p])
    assert np.array_equal(_bits(oracle.global_avg_pool_bp(g, off, S)), _bits(d))


@pytest.mark.parametrize("case", mask_label_cases(), ids=lambda c: c["name"])
def test_mask_label_crafted_ties_vs_serial_python(oracle, case):
    pidx, off, inst = mask_label_points(case)
    iou, cls, thr, I = case["iou"], case["inst_cls"], case["thr"], case["I"]
    ml = np.zeros(pidx.size, bool); mlm = np.zeros(pidx.size, bool)
    for p in range(iou.shape[0]):                         # cal_iou_and_masklabel.cu:84-103
        max_iou, max_ind = np.float32(0), 0
        for k in range(I):
            if iou[p, k] > max_iou and cls[k] != -1:
                max_iou, max_ind = iou[p, k], k
        assert max_ind == case["want"][p] or not case["written"][p]
        if max_iou >= thr:
            for i in range(off[p], off[p + 1]):
                if inst[pidx[i]] == max_ind:
                    ml[i] = True
                mlm[i] = True
    wml, wmlm = mask_label_expected(case)
    assert np.array_equal(ml, wml) and np.array_equal(mlm, wmlm)       # the rows are what they were crafted to be
    got = oracle.get_mask_label(pidx, off, inst, cls, iou, -1, float(thr))
    assert np.array_equal(got[0], ml) and np.array_equal(got[1], mlm)
