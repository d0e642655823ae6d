"""GPU parity of the instance post-processing kernels (csrc/postprocess.hip) at their edges, bit for bit against the
dense-mask restatement oracle.postprocess_oracle (plain numpy): pair counts on the 256-thread block edge, a point's run of
pairs across a block boundary, P = 1 and S = 0; greedy NMS past the 1024 threads of its one workgroup, IoU exactly equal
to the threshold (strict >), a suppression chain, proposals of size 0 (0 / 0 compares false).  The count matrices of the
NMS cases are built directly: symmetric, inter[a, b] <= min(n_a, n_b).  The builders check themselves on the CPU."""
import numpy as np
import pytest
import torch

from oracle import postprocess_oracle as PO

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from minsu3d_amd.backend import HipBackend
    return HipBackend()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------- cross intersection
def random_pairs(S, P, rng):
    """S unique (cluster, point) pairs sorted by point"""
    npts = max(2 * S // P, 3)
    key = np.sort(rng.choice(P * npts, S, replace=False))            # key = point * P + cluster
    pt, cl = key // P, key % P
    assert pt.size == S and np.all(np.diff(pt) >= 0) and np.unique(key).size == S
    return pt.astype(np.int32), cl.astype(np.int32)


def straddling_run(rng):
    """236 single-pair points, then ONE point in 40 proposals (positions 236..275: threads 236..255 of block 0 walk into
    block 1's pairs), then 50 more single-pair points"""
    P = 48
    pt = np.concatenate([np.arange(236), np.full(40, 236), 237 + np.arange(50)]).astype(np.int32)
    cl = np.concatenate([rng.integers(0, P, 236), np.arange(40), rng.integers(0, P, 50)]).astype(np.int32)
    run = np.where(pt == 236)[0]
    assert run[0] == 236 and run[-1] == 275 and run[0] // 256 != run[-1] // 256 and pt.size == 326
    return pt, cl, P


def check_cross(be, pt, cl, P):
    want = PO.cross_intersection(pt, cl, P)
    got = be.proposal_cross_intersection(dev(pt), dev(cl), P)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    return want


@gpu
@pytest.mark.parametrize("S", [1, 255, 256, 257, 513])
def test_cross_intersection_at_block_edges(be, S):
    pt, cl = random_pairs(S, 7, np.random.default_rng(S))
    want = check_cross(be, pt, cl, 7)
    assert int(np.trace(want)) == S


@gpu
def test_cross_intersection_run_across_a_block_boundary(be):
    pt, cl, P = straddling_run(np.random.default_rng(40))
    want = check_cross(be, pt, cl, P)
    assert want[:40, :40].min() >= 1 and want[40:, :40].max() == 0


@gpu
def test_cross_intersection_one_proposal_and_no_pairs(be):
    want = check_cross(be, np.arange(300, dtype=np.int32), np.zeros(300, np.int32), 1)
    assert want.tolist() == [[300]]
    want = check_cross(be, np.zeros(0, np.int32), np.zeros(0, np.int32), 5)
    assert want.shape == (5, 5) and not want.any()


# ---------------------------------------------------------------------------------------------- greedy NMS
def valid_counts(inter):
    n = np.diag(inter)
    assert inter.dtype == np.int32 and np.array_equal(inter, inter.T) and inter.min() >= 0
    assert np.all(inter <= np.minimum(n[:, None], n[None, :]))
    return inter


def set_pair(inter, a, b, x):
    inter[a, b] = inter[b, a] = x


def counts(P, regime, rng):
    """-> (inter, order, threshold 0.3).  none: every IoU <= 5 / 95; first: order[0] shares 90 of 100 points with every
    other proposal (IoU 0.82), the others share nothing; random: sparse random overlaps of any size up to the smaller
    proposal, and for P > 1024 a run of heavy overlaps (59 of 60 points) between neighbours over the last indices, from
    the pair (1023, 1024) on, so that what is decided about the indices >= 1024 shows in the result"""
    order = rng.permutation(P)
    if regime == "none":
        inter = rng.integers(0, 6, (P, P)).astype(np.int32)
        inter = np.minimum(inter, inter.T)
        np.fill_diagonal(inter, rng.integers(50, 101, P))
    elif regime == "first":
        inter = np.zeros((P, P), np.int32)
        np.fill_diagonal(inter, 100)
        inter[order[0], :] = inter[:, order[0]] = 90
        inter[order[0], order[0]] = 100
    else:
        n = rng.integers(20, 101, P).astype(np.int32)
        n[1023:] = 60
        if P > 1024:                                     # 1023 walks in front of 1024: its row decides about index 1024
            i, j = np.where(order == 1023)[0][0], np.where(order == 1024)[0][0]
            order[min(i, j)], order[max(i, j)] = 1023, 1024
        inter = np.zeros((P, P), np.int32)
        a, b = rng.integers(0, P, 4 * P), rng.integers(0, P, 4 * P)
        x = (rng.random(4 * P) * (np.minimum(n[a], n[b]) + 1)).astype(np.int32)
        inter[a, b] = x
        inter = np.triu(inter, 1)
        inter = inter + inter.T
        np.fill_diagonal(inter, n)
        for j in range(max(1024, P - 40), P):
            inter[j - 1, :], inter[:, j - 1], inter[j - 1, j - 1] = 0, 0, 60
        for j in range(max(1024, P - 40), P):
            set_pair(inter, j - 1, j, 59)                 # IoU 59 / 61
    return valid_counts(inter), order, 0.3


def nms_properties(P, regime, order, want):
    if regime == "none":
        assert np.array_equal(want, order)
    elif regime == "first":
        assert want.tolist() == [order[0]]
    elif P >= 1023:
        assert 1 < want.size < P
        if P > 1024:
            assert np.setdiff1d(np.arange(1024, P), want).size > 0        # something at an index >= 1024 was suppressed


def check_nms(be, inter, order, thr):
    with np.errstate(invalid="ignore"):
        want = PO.nms_from_counts(inter, order, thr)
    got = be.nms_greedy(dev(inter), dev(order), float(thr))
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (got.cpu().numpy()[:10], want[:10])
    return want


@gpu
@pytest.mark.parametrize("regime", ["none", "first", "random"])
@pytest.mark.parametrize("P", [1, 2, 1023, 1024, 1025, 2500])
def test_nms_at_the_workgroup_edge(be, P, regime):
    inter, order, thr = counts(P, regime, np.random.default_rng(P))
    nms_properties(P, regime, order, check_nms(be, inter, order, thr))


def embed(P, base, block):
    """the small crafted matrix `block` at indices base.. of a P x P matrix of otherwise disjoint proposals of size 50"""
    inter = np.zeros((P, P), np.int32)
    np.fill_diagonal(inter, 50)
    k = block.shape[0]
    inter[base:base + k, base:base + k] = block
    return valid_counts(inter)


TIES = [(1, 2, 3, 0.25), (2, 3, 3, 0.5)]


def tie_block(x, na, nb):
    assert np.float32(x) / (np.float32(na) + np.float32(nb) - np.float32(x)) in (np.float32(0.25), np.float32(0.5))
    return np.array([[na, x], [x, nb]], np.int32)


@gpu
@pytest.mark.parametrize("P,base", [(2, 0), (1030, 1026)])
@pytest.mark.parametrize("x,na,nb,thr", TIES)
def test_nms_iou_equal_to_the_threshold_does_not_suppress(be, P, base, x, na, nb, thr):
    assert np.float32(x) / (np.float32(na) + np.float32(nb) - np.float32(x)) == np.float32(thr)
    inter = embed(P, base, tie_block(x, na, nb))
    for first, second in ((base, base + 1), (base + 1, base)):
        order = np.concatenate([[first, second], np.setdiff1d(np.arange(P), [first, second])])
        want = check_nms(be, inter, order, thr)
        assert want.size == P                                               # strict >: the tie keeps both
        below = float(np.nextafter(np.float32(thr), np.float32(0)))
        want = check_nms(be, inter, order, below)
        assert want.size == P - 1 and second not in want                    # one float32 lower: suppressed


CHAIN = np.array([[10, 8, 6], [8, 10, 8], [6, 8, 10]], np.int32)     # A = 0..9, B = 2..11, C = 4..13 as point sets


@gpu
@pytest.mark.parametrize("P,base", [(3, 0), (1030, 1025)])
def test_nms_chain(be, P, base):
    """A suppresses B (8/12), B would suppress C (8/12) but is gone, A does not suppress C (6/14 < 0.5): C survives"""
    inter = embed(P, base, CHAIN)
    order = np.concatenate([base + np.arange(3), np.setdiff1d(np.arange(P), base + np.arange(3))])
    want = check_nms(be, inter, order, 0.5)
    assert want[:2].tolist() == [base, base + 2] and base + 1 not in want and want.size == P - 1
    # walked from the other end the chain is C -> B, and A survives
    want = check_nms(be, inter, np.concatenate([order[:3][::-1], order[3:]]), 0.5)
    assert want[:2].tolist() == [base + 2, base] and base + 1 not in want


@gpu
@pytest.mark.parametrize("P,base", [(4, 0), (1030, 1024)])
@pytest.mark.parametrize("thr", [0.3, -1.0])
def test_nms_proposals_of_size_zero(be, P, base, thr):
    """two proposals of size 0 among proposals of size 50: as the pivot IoU = 0 / n_b = 0, as a candidate 0 / n_a = 0,
    against each other 0 / 0 = NaN, which compares false.  At threshold -1 every IoU of 0 suppresses and only NaN does not:
    with an empty proposal first, the other empty one is the only further survivor"""
    inter = embed(P, base, np.zeros((2, 2), np.int32))
    rest = np.setdiff1d(np.arange(P), [base, base + 1])
    for order in (np.concatenate([[base], rest, [base + 1]]), np.concatenate([rest[:1], [base, base + 1], rest[1:]])):
        want = check_nms(be, inter, order, thr)
        if thr > 0:
            assert np.array_equal(want, order)
        elif order[0] == base:
            assert want.tolist() == [base, base + 1]
        else:
            assert want.tolist() == [order[0]]


# ---------------------------------------------------------------------------------------------- the builders, on the CPU
def test_crafted_inputs_are_what_they_claim():
    rng = np.random.default_rng(0)
    for S in (1, 255, 256, 257, 513):
        random_pairs(S, 7, rng)
    pt, cl, P = straddling_run(rng)
    assert PO.cross_intersection(pt, cl, P)[:40, :40].min() >= 1
    for P in (1, 2, 1023, 1024, 1025, 2500):
        for regime in ("none", "first", "random"):
            inter, order, thr = counts(P, regime, np.random.default_rng(P))
            assert sorted(order.tolist()) == list(range(P))
            nms_properties(P, regime, order, PO.nms_from_counts(inter, order, thr))
    for x, na, nb, thr in TIES:
        inter = embed(5, 2, tie_block(x, na, nb))
        order = np.array([2, 3, 0, 1, 4])
        assert PO.nms_from_counts(inter, order, thr).size == 5
        assert PO.nms_from_counts(inter, order, float(np.nextafter(np.float32(thr), np.float32(0)))).tolist() == [2, 0, 1, 4]
    assert PO.nms_from_counts(embed(3, 0, CHAIN), np.arange(3), 0.5).tolist() == [0, 2]
    with np.errstate(invalid="ignore"):
        assert PO.nms_from_counts(embed(4, 0, np.zeros((2, 2), np.int32)), np.array([0, 2, 3, 1]), -1.0).tolist() == [0, 1]
